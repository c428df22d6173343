"""pna_tower_train_fwd_f32 / pna_tower_train_bwd_f32 through ctypes (PNALayer's training forward and backward on a molecule batch as one
C call each: models/dgl/pna_layer.py:55-76, 130-145 in train mode): the saved state against the standalone gather's bits, z and the
BatchNorm statistics against float64, every gradient per element against oracle.torch_oracle.dgl_layer_train_step in float64, graph
norm off against a factor of ones, bitwise repeatability, the argument checks."""
import ctypes

import pytest
import torch

import tower_train_cases as C
from pna_amd import _lib, ops
from tower_train_run import Run

pytestmark = pytest.mark.gpu

CASES = C.KERNEL_CASES


def _Run(name, dev, **options):
    return Run(name, C.case(name), dev, **options)


_runs = {}


def _run(name, dev):
    if name not in _runs:
        _runs[name] = _Run(name, dev)
    return _runs[name]


@pytest.mark.parametrize("name", CASES)
def test_saved_state_has_the_gather_kernels_bits(cuda_device, name):
    """On the call's own saved x_cat, per tower mean | max | min and argmax / argmin equal pna_segreduce_fwd_f32's (n_tower = T, dst_term =
    x_dst, want_arg) bit for bit, and the std block equals that kernel's on x_src WITHOUT the destination term (the shift-free std of
    DESIGN.md 4.8.7): every case row has in-degree <= 128.  x_cat itself against float64 with the project's bar."""
    r = _run(name, cuda_device)
    csr = r.g.csr
    T, Fi = r.T, r.Fi
    TFi = T * Fi
    assert int((csr.rowptr[1:] - csr.rowptr[:-1]).max()) <= 128
    ident, amx, amn = ops.segreduce(csr.rowptr, csr.col, r.x_cat[:, :TFi], Fi, C.AGGS, [None], n_tower=T, tower_stride_in=Fi, dst_term=r.x_cat[:, TFi:],
                                    want_arg=True, heavy=r.g.heavy_schedule(), workspace=r.g.workspace, items=r.g.work_items())
    plain = ops.segreduce(csr.rowptr, csr.col, r.x_cat[:, :TFi], Fi, C.AGGS, [None], n_tower=T, tower_stride_in=Fi, heavy=r.g.heavy_schedule(),
                          workspace=r.g.workspace, items=r.g.work_items())
    got, with_dst, no_dst = (t[:, :4 * TFi].reshape(-1, T, 4, Fi) for t in (r.a, ident, plain))
    assert torch.equal(got[:, :, :3], with_dst[:, :, :3])                         # mean | max | min of x_src[u] + x_dst[v]
    assert torch.equal(got[:, :, 3], no_dst[:, :, 3])                             # std of x_src[u] alone
    assert torch.equal(r.amx, amx[:, :TFi]) and torch.equal(r.amn, amn[:, :TFi])
    meta, a, sd = r.meta, r.arrays, r.sd
    for t in range(T):
        ht = (a["h"][:, t * Fi:(t + 1) * Fi] if meta["divide_input"] else a["h"]).double()
        W, b = sd[C.pre_w(t)].double(), sd[C.pre_w(t)[:-6] + "bias"].double()
        for half, (ref, mass) in enumerate(((ht @ W[:, :Fi].t(), ht.abs() @ W[:, :Fi].abs().t()),
                                            (ht @ W[:, Fi:].t() + b, ht.abs() @ W[:, Fi:].abs().t() + b.abs()))):
            got = r.x_cat[:, half * TFi + t * Fi:half * TFi + (t + 1) * Fi].double().cpu()
            assert bool(((got - ref).abs() <= 1e-5 * ref.abs() + 2e-6 * mass).all()), (t, half)


@pytest.mark.parametrize("name", CASES)
def test_z_and_batch_statistics_against_float64(cuda_device, name):
    """z per element with the project's bar 1e-5 |ref| + 2e-6 sum |w| |operand| (bench.py); the batch statistics, the running
    statistics and the output with the bars of test_gpu_small_train_kernels.py."""
    r = _run(name, cuda_device)
    ref = r.ref
    err = (r.z.double().cpu() - ref.z).abs()
    tol = 1e-5 * ref.z.abs() + 2e-6 * ref.mass
    print(f"[tower_train] z: max err / tol = {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all()), (err / tol).max().item()
    torch.testing.assert_close(r.stats[0].double().cpu(), ref.mean, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(r.stats[1].double().cpu(), ref.invstd, rtol=1e-5, atol=1e-6)
    for t in range(r.T):
        bn = f"towers.{t}.batchnorm_h."
        torch.testing.assert_close(r.running[bn + "running_mean"].double().cpu(), ref.running[bn + "running_mean"], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(r.running[bn + "running_var"].double().cpu(), ref.running[bn + "running_var"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(r.out.cpu(), ref.out.float(), rtol=1e-5, atol=1e-5)
    # the saved pre-activation is the one the output was formed from: the backward's LeakyReLU mask is the forward's
    act = torch.where(r.p > 0, r.p, r.p * C.SLOPE)
    assert torch.equal(r.out, r.h + act if r.meta["residual"] else act)


@pytest.mark.parametrize("name", CASES)
def test_gradients_per_element_against_float64(cuda_device, name):
    r = _run(name, cuda_device)
    C.check_step(r.meta, r.ref, r.out, r.gh, r.grads)


@pytest.mark.parametrize("name", ["two_scalers", "zinc_last"])
def test_graph_norm_off_gives_the_bits_of_a_factor_of_ones(cuda_device, name):
    off, ones = _Run(name, cuda_device, snorm=None), _Run(name, cuda_device, snorm="ones")
    for t0, t1 in zip(off.history[0], ones.history[0]):
        assert torch.equal(t0, t1)


@pytest.mark.parametrize("name", ["tower_train_t4_div", "hand_res"])
def test_twenty_calls_give_identical_bits(cuda_device, name):
    r = _Run(name, cuda_device, repeat=20)
    for k, again in enumerate(r.history[1:]):
        for t0, t in zip(r.history[0], again):
            assert torch.equal(t0, t), k


def test_out_of_scope_arguments_are_refused(cuda_device):
    r = _run("hand_res", cuda_device)
    L = _lib.lib()
    st = _lib.stream_ptr(cuda_device)
    size = ctypes.sizeof(_lib.PnaTowerTrainArgs)

    def variant(**kw):
        a = _lib.PnaTowerTrainArgs()
        ctypes.memmove(ctypes.byref(a), ctypes.byref(r.args), size)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert L.pna_tower_train_bwd_f32(ctypes.byref(variant()), st) == 0           # (the unchanged block is accepted)
    torch.cuda.synchronize(cuda_device)
    bad = [dict(n_tower=0), dict(n_tower=9), dict(Fi=3), dict(Fi=129), dict(n_tower=8, Fi=65), dict(Fo=0), dict(Fo=65), dict(n_scaler=0), dict(n_scaler=4),
           dict(V=1), dict(divide_input=2), dict(Fo=7, residual=1), dict(workspace_bytes=r.args.workspace_bytes - 4), dict(struct_size=size - 8),
           dict(struct_size=0), dict(w_mix=None), dict(x_cat=None)]
    for kw in bad:
        for fn in (L.pna_tower_train_fwd_f32, L.pna_tower_train_bwd_f32):
            assert fn(ctypes.byref(variant(**kw)), st) == -1, kw
    assert L.pna_tower_train_bwd_f32(ctypes.byref(variant(n_items_t=r.args.n_items_t - 1)), st) == -1
    assert L.pna_tower_train_workspace_bytes(40, 100, 2, 3, 8, 3, 1) == -1
