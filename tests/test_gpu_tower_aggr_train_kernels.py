"""pna_tower_aggr_train_fwd_f32 / pna_tower_aggr_train_bwd_f32 through ctypes (PNALayer's training forward and backward for any 1-4
distinct aggregators out of mean sum max min std var as one C call each: models/dgl/aggregators.py:6-26, 50-51 under
models/dgl/pna_layer.py:55-76, 130-145 in train mode): the saved aggregate, z and the BatchNorm statistics against float64, every
gradient per element against oracle.torch_oracle.dgl_layer_train_step with the case's list in float64 (under the key's mask for the
dropout cases), bitwise repeatability, the bits of the three older entry pairs on mean max min std, E == 0, the argument checks."""
import ctypes

import pytest
import torch

import tower_aggr_train_cases as C
from pna_amd import _lib
from pna_amd import functional as PF
from tower_aggr_train_run import Run

pytestmark = pytest.mark.gpu

CASES = C.KERNEL_CASES + C.DROP_CASES
_runs = {}


def _run(name, dev, old=False):
    if (name, old) not in _runs:
        _runs[(name, old)] = Run(C.case(name), dev, old=old, repeat=2)
    return _runs[(name, old)]


@pytest.mark.parametrize("name", CASES)
def test_z_statistics_and_output_against_float64(cuda_device, name):
    """z per element with the project's bar 1e-5 |ref| + 2e-6 sum |w| |operand| (bench.py); the batch statistics, the running statistics
    and the output with the bars of test_gpu_tower_train_kernels.py; a dropout case's mask is functional.dropout_mask's."""
    r = _run(name, cuda_device)
    ref = r.ref
    if r.key is not None:
        assert torch.equal(PF.dropout_mask(r.meta["N"], r.meta["out_dim"], *r.key, cuda_device).cpu(), ref.mask)
    err = (r.z.double().cpu() - ref.z).abs()
    tol = 1e-5 * ref.z.abs() + 2e-6 * ref.mass
    print(f"[tower_aggr_train] z: max err / tol = {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all()), (err / tol).max().item()
    torch.testing.assert_close(r.stats[0].double().cpu(), ref.mean, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(r.stats[1].double().cpu(), ref.invstd, rtol=1e-5, atol=1e-6)
    for t in range(r.T):
        bn = f"towers.{t}.batchnorm_h."
        torch.testing.assert_close(r.running[bn + "running_mean"].double().cpu(), ref.running[bn + "running_mean"], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(r.running[bn + "running_var"].double().cpu(), ref.running[bn + "running_var"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(r.out.cpu(), ref.out.float(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", C.KERNEL_CASES)
def test_saved_aggregate_is_the_lists_blocks_in_list_order(cuda_device, name):
    """a (V, T A Fi) against the float64 statistics of the call's OWN saved x_cat / x_edge, block by block in list order: the sum, mean,
    max, min of (x_src[u] + x_dst[v]) [+ x_edge[k]], the std and var of the message without the destination term; rows without in-edges
    are zero in every block; var is exactly 0 on in-degree-1 rows; row_mean where std or var is listed without mean."""
    r = _run(name, cuda_device)
    V, T, Fi, A = r.meta["N"], r.T, r.Fi, r.A
    TFi = T * Fi
    csr = r.g.csr
    rowptr, col = csr.rowptr.cpu().long(), csr.col.cpu().long()
    deg = rowptr[1:] - rowptr[:-1]
    dst = torch.repeat_interleave(torch.arange(V), deg)
    xs, xd = r.x_cat[:, :TFi].double().cpu(), r.x_cat[:, TFi:].double().cpu()
    m0 = xs[col] + (r.fwd["x_edge"].double().cpu() if r.ed else 0.0)
    m = m0 + xd[dst]
    idx = dst[:, None].expand(-1, TFi)
    D = deg.clamp(min=1).double()[:, None]
    s = torch.zeros(V, TFi, dtype=torch.float64).index_add_(0, dst, m)
    s0 = torch.zeros(V, TFi, dtype=torch.float64).index_add_(0, dst, m0)
    q0 = torch.zeros(V, TFi, dtype=torch.float64).index_add_(0, dst, m0 * m0)
    var = torch.relu(q0 / D - (s0 / D) ** 2)
    has = (deg > 0)[:, None]
    want = {"sum": s, "mean": s / D, "var": var, "std": torch.sqrt(var + 1e-5) * has,
            "max": torch.full((V, TFi), -float("inf"), dtype=torch.float64).scatter_reduce_(0, idx, m, "amax").masked_fill(~has, 0.0),
            "min": torch.full((V, TFi), float("inf"), dtype=torch.float64).scatter_reduce_(0, idx, m, "amin").masked_fill(~has, 0.0)}
    got = r.a.double().cpu().reshape(V, T, A, Fi)
    scale = torch.zeros(V, TFi, dtype=torch.float64).index_add_(0, dst, m.abs()).clamp(min=1.0)
    for i, n in enumerate(r.meta["aggregators"].split()):
        g, w = got[:, :, i].reshape(V, TFi), want[n]
        if n in ("max", "min"):
            assert bool(((g - w).abs() <= 3e-7 * scale).all()), n                  # one of the messages, each two fp32 additions
        elif n == "var":                                                           # E[x^2] - E[x]^2 in fp32: absolute error ~ eps E[x^2]
            assert bool(((g - w).abs() <= 4e-6 * (q0 / D) + 1e-12).all()), n
            assert bool((g[deg == 1] == 0).all())
        elif n == "std":
            assert bool(((g - w).abs() <= 1e-4 * w + 2e-6 * (q0 / D) / w.clamp(min=1e-3)).all()), n
        else:
            assert bool(((g - w).abs() <= 2e-6 * (scale if n == "sum" else scale / D)).all()), n
        assert bool((g[deg == 0] == 0).all()), n
    names = r.meta["aggregators"].split()
    if ("std" in names or "var" in names) and "mean" not in names:
        torch.testing.assert_close(r.row_mean.double().cpu(), s0 / D, rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("name", CASES)
def test_gradients_per_element_against_float64(cuda_device, name):
    r = _run(name, cuda_device)
    C.check_step(r.meta, r.ref, r.out, r.gh, r.grads)
    if r.ed:
        C.check_grad_e(r.ref, r.ge)


@pytest.mark.parametrize("name", CASES)
def test_a_second_call_gives_identical_bits(cuda_device, name):
    r = _run(name, cuda_device)
    first, second = r.history
    assert first.keys() == second.keys()
    for k in first:
        assert torch.equal(first[k], second[k]), k


@pytest.mark.parametrize("name", ["std_plain", "std_edge", "drop_std_plain", "drop_std_edge"])
def test_the_standard_list_keeps_the_older_entry_points_bits(cuda_device, name):
    """mean max min std, three scalers: the forward's out and every saved tensor equal the older entry pair's bit for bit; with edge
    features (with and without dropout) so does every gradient -- both backwards are the per-edge formulation.  The plain backward (its
    pull differs from the ranked one) is held to the float64 bars."""
    new, old = _run(name, cuda_device), _run(name, cuda_device, old=True)
    assert new.fwd.keys() == old.fwd.keys()
    for k in new.fwd:
        assert torch.equal(new.fwd[k], old.fwd[k]), k
    if new.ed:
        assert new.bwd.keys() == old.bwd.keys()
        for k in new.bwd:
            assert torch.equal(new.bwd[k], old.bwd[k]), k
    C.check_step(new.meta, new.ref, new.out, new.gh, new.grads)
    if new.ed:
        C.check_grad_e(new.ref, new.ge)


@pytest.mark.parametrize("name", ["no_edges", "no_edges_edge"])
def test_a_batch_without_edges_succeeds(cuda_device, name):
    r = _run(name, cuda_device)
    assert r.g.csr.col.numel() == 0 and bool((r.a == 0).all())
    assert all(bool(torch.isfinite(v).all()) for v in r.bwd.values())
    Fi = r.Fi
    for t in range(r.T):
        assert bool((r.grads[C.pre_w(t)][:, :Fi] == 0).all()) and bool((r.grads[C.pre_w(t)][:, 2 * Fi:] == 0).all())      # nothing flows through a message


def _refused(case, dev, tweak):
    """Both calls return PNA_E_INVALID under `tweak` and write nothing: out, grad_h and the gradient buffers keep their NaN fill."""
    r = Run(case, dev, tweak=tweak, expect=-1)
    assert bool(torch.isnan(r.out).all()) and bool(torch.isnan(r.gh).all()) and bool(torch.isnan(r.z).all())
    assert all(bool(torch.isnan(v).all()) for v in r.grads.values())
    assert r.ge is None or bool(torch.isnan(r.ge).all())


def test_out_of_scope_lists_and_missing_tensors_are_refused(cuda_device):
    L = _lib.lib()
    L.pna_last_error.restype = ctypes.c_char_p
    hand, std_only, edge = C.case("hand"), C.case("std_only"), C.case("edge3_sum")      # sum var max min | std | sum with edge features

    def block(**kw):
        def tweak(which, base, q, blk):
            for k, v in kw.items():
                setattr(blk, k, v)
        return tweak

    def aggr(*codes):
        def tweak(which, base, q, blk):
            blk.n_aggr = len(codes)
            for i, c in enumerate(codes):
                blk.aggr[i] = c
        return tweak

    def base_field(**kw):
        def tweak(which, base, q, blk):
            for k, v in kw.items():
                setattr(base, k, v)
        return tweak

    size = ctypes.sizeof(_lib.PnaTowerAggrTrainArgs)
    for tweak in (block(n_aggr=0), block(n_aggr=5), aggr(1, 5, 2, 2), aggr(1, 6, 2, 3), aggr(1, -1, 2, 3), block(struct_size=size - 8), block(struct_size=0),
                  block(base=None), base_field(argmax=None), base_field(argmin=None), base_field(workspace_bytes=64), base_field(Fi=3), base_field(n_scaler=4)):
        _refused(hand, cuda_device, tweak)
    assert b"pna_tower_aggr_train" in L.pna_last_error() and b"n_aggr" in L.pna_last_error()
    _refused(std_only, cuda_device, block(row_mean=None))

    def no_pos_t(which, base, q, blk):                       # (the forward does not read pos_t: only the backward is refused)
        if which == "bwd":
            blk.pos_t = None
    r = Run(hand, cuda_device, tweak=lambda which, base, q, blk: None)
    assert bool(torch.isfinite(r.gh).all())
    with pytest.raises(AssertionError, match="pna_tower_aggr_train_bwd_f32"):
        Run(hand, cuda_device, tweak=no_pos_t)

    def other_base(which, base, q, blk):
        other = _lib.PnaTowerTrainArgs()
        ctypes.memmove(ctypes.byref(other), ctypes.byref(base), ctypes.sizeof(other))
        blk._other = other
        q.base = ctypes.cast(ctypes.pointer(other), ctypes.c_void_p)
    _refused(edge, cuda_device, other_base)

    def bad_drop(p):
        def tweak(which, base, q, blk):
            d = _lib.PnaTowerDropArgs()
            d.base, d.p = blk.base, p
            blk._drop = d
            blk.drop = ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)
        return tweak
    for p in (1.0, -0.1, float("nan")):
        _refused(hand, cuda_device, bad_drop(p))
    # max is not listed: argmax may be NULL
    r = Run(C.case("mpnn_sum"), cuda_device, tweak=lambda which, base, q, blk: (setattr(base, "argmax", None), setattr(base, "argmin", None)))
    C.check_step(r.meta, r.ref, r.out, r.gh, r.grads)
