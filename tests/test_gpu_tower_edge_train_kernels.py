"""pna_tower_edge_train_fwd_f32 / pna_tower_edge_train_bwd_f32 through ctypes (PNALayer with edge features, training forward and
backward on a molecule batch as one C call each: models/dgl/pna_layer.py:35-40, 55-76, 130-145 in train mode): the saved x_edge against
float64, the saved statistics against the standalone gather's bits, z and the BatchNorm statistics against float64, every gradient
(grad_e included) per element against oracle.torch_oracle.dgl_layer_train_step in float64, bitwise repeatability, the argument checks."""
import ctypes

import pytest
import torch

import tower_edge_train_cases as C
from pna_amd import _lib, ops
from tower_train_run import Run

pytestmark = pytest.mark.gpu

CASES = C.KERNEL_CASES


def _Run(name, dev, **options):
    return Run(name, C.case(name), dev, want_grad_e=name != "e_no_grad", **options)


_runs = {}


def _run(name, dev):
    if name not in _runs:
        _runs[name] = _Run(name, dev)
    return _runs[name]


@pytest.mark.parametrize("name", CASES)
def test_saved_x_edge_against_float64(cuda_device, name):
    """x_edge,t[k] = W_e,t e[eid[k]] in CSR order, per element within the dot-product bound (edge_dim + 1) 2^-24 sum |w| |e|."""
    r = _run(name, cuda_device)
    ref, mass = C.x_edge64(r.sd, r.arrays, r.meta)
    eid = r.g.csr.eid.cpu().long()
    assert torch.equal(torch.sort(eid).values, torch.arange(eid.numel()))
    err = (r.x_edge.double().cpu() - ref[eid]).abs()
    tol = (r.ed + 1) * 2.0 ** -24 * mass[eid]
    print(f"[tower_edge_train] x_edge: max err / tol = {(err / tol).max().item() if err.numel() else 0.0:.3f}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("name", CASES)
def test_saved_state_has_the_gather_kernels_bits(cuda_device, name):
    """On the call's own saved x_cat and x_edge, per tower mean | max | min and argmax / argmin equal pna_segreduce_fwd_f32's (x = x_src,
    dst_term = x_dst, edge_term = x_edge, want_arg) bit for bit, and the std block equals that kernel's WITHOUT the destination term:
    every case row has in-degree <= 128."""
    r = _run(name, cuda_device)
    csr = r.g.csr
    T, Fi = r.T, r.Fi
    TFi = T * Fi
    assert int((csr.rowptr[1:] - csr.rowptr[:-1]).max()) <= 128
    et = r.x_edge if r.x_edge.shape[0] else None
    ident, amx, amn = ops.segreduce(csr.rowptr, csr.col, r.x_cat[:, :TFi], Fi, C.AGGS, [None], n_tower=T, tower_stride_in=Fi, dst_term=r.x_cat[:, TFi:],
                                    edge_term=et, want_arg=True, heavy=r.g.heavy_schedule(), workspace=r.g.workspace, items=r.g.work_items())
    plain = ops.segreduce(csr.rowptr, csr.col, r.x_cat[:, :TFi], Fi, C.AGGS, [None], n_tower=T, tower_stride_in=Fi, edge_term=et,
                          heavy=r.g.heavy_schedule(), workspace=r.g.workspace, items=r.g.work_items())
    got, with_dst, no_dst = (t[:, :4 * TFi].reshape(-1, T, 4, Fi) for t in (r.a, ident, plain))
    assert torch.equal(got[:, :, :3], with_dst[:, :, :3])                         # mean | max | min of (x_src[u] + x_dst[v]) + x_edge[k]
    assert torch.equal(got[:, :, 3], no_dst[:, :, 3])                             # std of x_src[u] + x_edge[k]
    assert torch.equal(r.amx, amx[:, :TFi]) and torch.equal(r.amn, amn[:, :TFi])


@pytest.mark.parametrize("name", CASES)
def test_z_and_batch_statistics_against_float64(cuda_device, name):
    """The bars of tests/test_gpu_tower_train_kernels.py: z per element at 1e-5 |ref| + 2e-6 sum |w| |operand|; the batch statistics, the
    running statistics and the output."""
    r = _run(name, cuda_device)
    ref = r.ref
    err = (r.z.double().cpu() - ref.z).abs()
    tol = 1e-5 * ref.z.abs() + 2e-6 * ref.mass
    print(f"[tower_edge_train] z: max err / tol = {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all()), (err / tol).max().item()
    torch.testing.assert_close(r.stats[0].double().cpu(), ref.mean, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(r.stats[1].double().cpu(), ref.invstd, rtol=1e-5, atol=1e-6)
    for t in range(r.T):
        bn = f"towers.{t}.batchnorm_h."
        torch.testing.assert_close(r.running[bn + "running_mean"].double().cpu(), ref.running[bn + "running_mean"], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(r.running[bn + "running_var"].double().cpu(), ref.running[bn + "running_var"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(r.out.cpu(), ref.out.float(), rtol=1e-5, atol=1e-5)
    act = torch.where(r.p > 0, r.p, r.p * C.SLOPE)
    assert torch.equal(r.out, r.h + act if r.meta["residual"] else act)


@pytest.mark.parametrize("name", CASES)
def test_gradients_per_element_against_float64(cuda_device, name):
    """out, grad_h, every parameter gradient and the running statistics with tower_train_cases.check_step; grad_e at 1e-4 of its largest
    entry, 2e-3 on the touched edges.  e_no_grad: grad_e = NULL, everything else as usual."""
    r = _run(name, cuda_device)
    C.check_step(r.meta, r.ref, r.out, r.gh, r.grads, r.running)
    if name == "e_no_grad":
        assert r.ge is None
    else:
        assert tuple(r.ge.shape) == tuple(r.ref.grad_e.shape)
        C.check_grad_e(r.ref, r.ge)
    if name == "no_edges":                                                        # the W_e block: zero, not left unwritten
        for t in range(r.T):
            assert not bool(r.grads[C.pre_w(t)][:, 2 * r.Fi:].any())


@pytest.mark.parametrize("name", [C.GOLDEN, "hand"])
def test_twenty_calls_give_identical_bits(cuda_device, name):
    r = _Run(name, cuda_device, repeat=20)
    for k, again in enumerate(r.history[1:]):
        for t0, t in zip(r.history[0], again):
            assert torch.equal(t0, t), k


def test_out_of_scope_arguments_are_refused(cuda_device):
    """Each returns PNA_E_INVALID before any launch: the outputs of the accepted call before them keep their bits."""
    r = _run("hand", cuda_device)
    L = _lib.lib()
    st = _lib.stream_ptr(cuda_device)
    size, bsize = ctypes.sizeof(_lib.PnaTowerEdgeTrainArgs), ctypes.sizeof(_lib.PnaTowerTrainArgs)

    def variant(base=None, **kw):
        q = _lib.PnaTowerEdgeTrainArgs()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(r.q), size)
        b = _lib.PnaTowerTrainArgs()
        ctypes.memmove(ctypes.byref(b), ctypes.byref(r.args), bsize)
        for k, v in (base or {}).items():
            setattr(b, k, v)
        q.base = ctypes.cast(ctypes.pointer(b), ctypes.c_void_p)
        for k, v in kw.items():
            setattr(q, k, v)
        q._keep = b
        return q
    assert L.pna_tower_edge_train_bwd_f32(ctypes.byref(variant()), st) == 0      # (the unchanged block is accepted)
    torch.cuda.synchronize(cuda_device)
    before = [t.clone() for t in [r.gh, r.ge, r.x_edge, r.out] + list(r.grads.values())]
    both = [dict(struct_size=size - 8), dict(struct_size=0), dict(edge_dim=0), dict(edge_dim=65), dict(e=None), dict(ld_e=r.ed - 1), dict(eid=None),
            dict(base=dict(workspace_bytes=r.args.workspace_bytes - 1)), dict(base=dict(Fi=3)), dict(base=dict(struct_size=bsize - 8))]
    for kw in both:
        for fn in (L.pna_tower_edge_train_fwd_f32, L.pna_tower_edge_train_bwd_f32):
            assert fn(ctypes.byref(variant(**kw)), st) == -1, kw
    assert L.pna_tower_edge_train_bwd_f32(ctypes.byref(variant(pos_t=None)), st) == -1
    assert L.pna_tower_edge_train_bwd_f32(ctypes.byref(variant(ld_ge=r.ed - 1)), st) == -1
    torch.cuda.synchronize(cuda_device)
    for t0, t in zip(before, [r.gh, r.ge, r.x_edge, r.out] + list(r.grads.values())):
        assert torch.equal(t0, t)
    assert L.pna_tower_edge_train_workspace_bytes(40, 100, 2, 8, 8, 3, 1, 0) == -1
    assert L.pna_tower_edge_train_workspace_bytes(40, 100, 2, 8, 8, 3, 1, 65) == -1
