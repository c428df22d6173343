"""pna_pyg_conv_train_fwd_f32 / pna_pyg_conv_train_bwd_f32 through ctypes (PNAConv's training forward and backward as one C call each:
models/pytorch_geometric/pna.py:120-159) against pyg_train_cases' float64 step at tower_train_cases.check_step's bars, the PyG
statistics in the saved aggregate, the packed image, bitwise repeatability, the DGL entry's bits around a PyG call, E == 0 and the
argument checks.  The cases are the smallest shapes at which each mechanism can go wrong (pyg_train_cases.CASES)."""
import ctypes
import math

import pytest
import torch

import pyg_train_cases as C
from pna_amd import _lib
from pyg_train_run import Run

pytestmark = pytest.mark.gpu

_runs = {}


def _run(name, dev):
    if name not in _runs:
        _runs[name] = Run(C.case(name), dev, repeat=2)
    return _runs[name]


@pytest.mark.parametrize("name", list(C.CASES))
def test_step_against_float64(cuda_device, name):
    r = _run(name, cuda_device)
    C.check_step(r.ref, r.out, r.gx, r.grads, r.ge)


@pytest.mark.parametrize("name", list(C.CASES))
def test_a_second_call_gives_identical_bits(cuda_device, name):
    first, second = _run(name, cuda_device).history
    assert first.keys() == second.keys()
    for k in first:
        assert torch.equal(first[k], second[k]), k


@pytest.mark.parametrize("name", ["v17_t5", "v33_div_edge1", "var_neg", "v33_edge64", "no_edges"])
def test_saved_aggregate_follows_the_pyg_rules(cuda_device, name):
    """A row without in-edges: std = sqrtf(1e-5f) exactly, every other block 0.  var is E[m0^2] - E[m0]^2 NOT clamped: within the fp32
    floor of float64, and on the destination fed three equal messages (var_neg) some entries are negative."""
    r = _run(name, cuda_device)
    V, T, Fi, A = r.meta["N"], r.T, r.Fi, r.A
    csr = r.g.csr
    rowptr, col = csr.rowptr.cpu().long(), csr.col.cpu().long()
    deg = rowptr[1:] - rowptr[:-1]
    assert int((deg == 0).sum()) >= C.ISOLATED
    got = r.a.cpu().reshape(V, T, A, Fi)
    empty_std = torch.sqrt(torch.tensor(1e-5, dtype=torch.float32))
    for i, n in enumerate(r.meta["aggregators"]):
        blk = got[deg == 0][:, :, i]
        assert bool((blk == (empty_std if n == "std" else 0.0)).all()), n
    if "var" in r.meta["aggregators"]:
        i = r.meta["aggregators"].index("var")
        TFi = T * Fi
        dst = torch.repeat_interleave(torch.arange(V), deg)
        m0 = r.x_cat[:, :TFi].double().cpu()[col]
        if r.ed:
            m0 = m0 + r.plan.x_edge(r.saved).double().cpu()
        D = deg.clamp(min=1).double()[:, None]
        s0 = torch.zeros(V, TFi, dtype=torch.float64).index_add_(0, dst, m0)
        q0 = torch.zeros(V, TFi, dtype=torch.float64).index_add_(0, dst, m0 * m0)
        var = q0 / D - (s0 / D) ** 2
        g = got[:, :, i].reshape(V, TFi).double()
        assert bool(((g - var).abs() <= 4e-6 * (q0 / D) + 1e-12).all())         # E[x^2] - E[x]^2 in fp32: absolute error ~ eps E[x^2]
        if name == "var_neg":
            assert deg[0] == 3 and bool((g[0] < 0).any()), g[0].min().item()    # the DGL rule would have clamped these to 0


@pytest.mark.parametrize("name", ["v33_div_edge1", "v17_t5"])
def test_packed_image_is_the_fold(cuda_device, name):
    r = _run(name, cuda_device)
    _, _, sd, _ = C.case(name)
    T, Fi, ed = r.T, r.Fi, r.ed
    ldw = 2 * Fi + ed
    img = r.history[0]["packed"].cpu()
    for t in range(T):
        W, b = sd[f"pre_nns.{t}.0.weight"].double(), sd[f"pre_nns.{t}.0.bias"].double()
        want, wb = torch.cat([W[:, Fi:2 * Fi], W[:, :Fi]], dim=1), b
        if ed:
            We = W[:, 2 * Fi:]
            want = torch.cat([want, We @ sd["edge_encoder.weight"].double()], dim=1)
            wb = b + We @ sd["edge_encoder.bias"].double()
        assert torch.equal(img[t * Fi * ldw:(t + 1) * Fi * ldw].view(Fi, ldw), want.float())      # float64 chains rounded once
        assert torch.equal(img[T * Fi * ldw + t * Fi:T * Fi * ldw + (t + 1) * Fi], wb.float())


def test_the_dgl_entry_gives_the_same_bits_before_and_after(cuda_device):
    """pna_tower_aggr_train_* on a standard case, a PyG call in between: the new modes leak nowhere."""
    import tower_aggr_train_cases as TC
    from tower_aggr_train_run import Run as TowerRun
    name = TC.KERNEL_CASES[0]
    before = TowerRun(TC.case(name), cuda_device).history[0]
    Run(C.case("v33_div_edge1"), cuda_device)
    after = TowerRun(TC.case(name), cuda_device).history[0]
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k], after[k]), k


@pytest.mark.parametrize("name", ["no_edges", "no_edges_edge"])
def test_a_batch_without_edges_succeeds(cuda_device, name):
    r = _run(name, cuda_device)
    assert r.g.csr.col.numel() == 0
    assert all(bool(torch.isfinite(v).all()) for k, v in r.history[0].items() if k.startswith("grad") or k == "out")
    Fi = r.Fi
    for t in range(r.T):
        assert bool((r.grads[f"pre_nns.{t}.0.weight"] == 0).all())             # nothing flows through a message
    if r.ed:
        assert bool((r.grads["edge_encoder.weight"] == 0).all()) and r.ge.shape[0] == 0
    assert math.isclose(float(r.a.max()), 1e-5 ** 0.5, rel_tol=1e-6)           # only the std blocks are non-zero


def _refused(case, dev, tweak):
    r = Run(case, dev, tweak=tweak, expect=-1)
    assert bool(torch.isnan(r.out).all()) and bool(torch.isnan(r.gx).all()) and bool(torch.isnan(r.z).all())
    assert all(bool(torch.isnan(v).all()) for v in r.grads.values())


def test_calls_outside_the_scope_are_refused(cuda_device):
    L = _lib.lib()
    L.pna_last_error.restype = ctypes.c_char_p
    plain, edge = C.case("sum_only"), C.case("v33_div_edge1")
    dummy = torch.zeros(64, device=cuda_device)

    def base_field(**kw):
        return lambda which, base, q, blk, y: [setattr(base, k, v) for k, v in kw.items()]

    def y_field(**kw):
        return lambda which, base, q, blk, y: [setattr(y, k, v) for k, v in kw.items()]

    def with_drop(which, base, q, blk, y):
        d = _lib.PnaTowerDropArgs()
        d.base, d.p = blk.base, 0.0
        blk._drop = d
        blk.drop = ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)

    size = ctypes.sizeof(_lib.PnaPygConvTrainArgs)
    for tweak in (base_field(Fi=3), base_field(n_scaler=4), base_field(workspace_bytes=64), base_field(residual=1), base_field(snorm_n=dummy.data_ptr()),
                  y_field(struct_size=size - 8), y_field(aggr=None), y_field(packed=None), y_field(w_enc=dummy.data_ptr(), b_enc=dummy.data_ptr()), with_drop):
        _refused(plain, cuda_device, tweak)
    assert b"pna_pyg_conv_train" in L.pna_last_error()
    for tweak in (y_field(w_enc=None, b_enc=None), y_field(b_enc=None), lambda which, base, q, blk, y: setattr(q, "edge_dim", 65)):
        _refused(edge, cuda_device, tweak)
