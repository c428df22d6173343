"""pna_set2set_fwd_f32 / pna_set2set_bwd_f32 on the GPU, called through ctypes on every case of tests/set2set_cases.py: out and the five
gradients per element against float64 within the case's bars (4 x the fp32 CPU oracle's own error + 2^-20 of the tensor's largest value),
grad b_ih bitwise grad b_hh, repeats bitwise, and the slab case against the same data run as two half batches."""
import ctypes

import pytest
import torch

import set2set_cases as C
from pna_amd import _lib
from pna_amd import functional as PF

pytestmark = pytest.mark.gpu


def _args(c, t):
    a = _lib.PnaSet2setArgs()
    a.B, a.N, a.D, a.steps, a.dtype = t["x"].shape[0], c["N"], c["D"], c["steps"], _lib.PNA_S2S_F32
    for f in ("x", "w_ih", "w_hh", "b_ih", "b_hh"):
        setattr(a, f, t[f].data_ptr())
    return a


def _forward(c, t):
    out = torch.full((t["x"].shape[0], 2 * c["D"]), float("nan"), device=t["x"].device)
    a = _args(c, t)
    a.out = out.data_ptr()
    _lib.check(_lib.lib().pna_set2set_fwd_f32(ctypes.byref(a), _lib.stream_ptr(out.device)), "pna_set2set_fwd_f32")
    return out


def _backward(c, t):
    """{'x': grad, 'w_ih': grad, ...}; every buffer starts as NaN, so an element the call leaves unwritten fails the comparison."""
    dev = t["x"].device
    B = t["x"].shape[0]
    grads = {k: torch.full_like(t[k], float("nan")) for k in ("x",) + C.PARAMS}
    nbytes = PF.set2set_workspace_bytes(B, c["N"], c["D"], c["steps"])
    assert nbytes == _lib.lib().pna_set2set_workspace_bytes(B, c["N"], c["D"], c["steps"]) > 0
    ws = torch.full((nbytes // 4 + 4,), float("nan"), device=dev)
    a = _args(c, t)
    a.grad_out = t["go"].data_ptr()
    for k, g in grads.items():
        setattr(a, "grad_" + k, g.data_ptr())
    a.workspace, a.workspace_bytes = ws.data_ptr() + (-ws.data_ptr()) % 16, nbytes
    _lib.check(_lib.lib().pna_set2set_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_set2set_bwd_f32")
    return grads


def _on(c, dev, rows=None):
    sl = slice(None) if rows is None else rows
    t = {k: c[k].to(dev) for k in C.PARAMS}
    t["x"], t["go"] = c["x"][sl].contiguous().to(dev), c["go"][sl].contiguous().to(dev)
    return t


@pytest.mark.parametrize("name", C.NAMES)
def test_forward_and_backward_against_float64(cuda_device, name):
    c = C.s2s_case(name)
    ref64, _, bars = C.references(name)
    t = _on(c, cuda_device)
    got = {"out": _forward(c, t)}
    got.update(_backward(c, t))
    torch.cuda.synchronize()
    ratios = {k: C.worst_ratio(got[k], ref64[k], bars[k]) for k in C.TENSORS}
    print("S2S_KERNEL", name, "worst err / bar", {k: round(v, 3) for k, v in ratios.items()})
    for k in C.TENSORS:
        assert torch.isfinite(got[k]).all(), k
        assert ((got[k].double().cpu() - ref64[k]).abs() <= bars[k]).all(), (name, k, ratios[k])
    assert torch.equal(got["b_ih"], got["b_hh"])                                   # one sum, stored twice


@pytest.mark.parametrize("name", ["n15", "slab", "n128"])
def test_repeats_give_identical_bits(cuda_device, name):
    c = C.s2s_case(name)
    t = _on(c, cuda_device)
    outs = [_forward(c, t) for _ in range(3)]
    grads = [_backward(c, t) for _ in range(3)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    for g in grads[1:]:
        for k in g:
            assert torch.equal(g[k], grads[0][k]), k


def test_slab_case_equals_two_half_batches(cuda_device):
    """B = 300 > PNA_S2S_MAX_SLABS: two graphs per workgroup.  The halves (150 each: one graph per workgroup) give the same out and grad_x
    bits, and parameter gradients whose sum is within the bars of the whole batch's."""
    c = C.s2s_case("slab")
    assert c["B"] > _lib.PNA_S2S_MAX_SLABS and -(-c["B"] // _lib.PNA_S2S_MAX_SLABS) == 2 and -(-(c["B"] // 2) // _lib.PNA_S2S_MAX_SLABS) == 1
    ref64, _, bars = C.references("slab")
    whole = _on(c, cuda_device)
    out, g = _forward(c, whole), _backward(c, whole)
    h = c["B"] // 2
    halves = [_on(c, cuda_device, slice(0, h)), _on(c, cuda_device, slice(h, None))]
    outs = [_forward(c, t) for t in halves]
    gs = [_backward(c, t) for t in halves]
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(outs), out) and torch.equal(torch.cat([gs[0]["x"], gs[1]["x"]]), g["x"])
    for k in C.PARAMS:
        both = gs[0][k].double() + gs[1][k].double()
        assert ((both - g[k].double()).abs().cpu() <= bars[k]).all(), k
        assert ((both.cpu() - ref64[k]).abs() <= bars[k]).all(), k


def test_null_gradient_pointers_are_skipped(cuda_device):
    """grad_x alone (one launch) and the parameters alone give the bits of the full call; nothing wanted is a no-op."""
    c = C.s2s_case("n15")
    t = _on(c, cuda_device)
    full = _backward(c, t)
    nbytes = PF.set2set_workspace_bytes(c["B"], c["N"], c["D"], c["steps"])
    ws = torch.empty(nbytes // 4 + 4, device=cuda_device)
    for keep in (("x",), C.PARAMS, ()):
        grads = {k: torch.full_like(t[k], float("nan")) for k in keep}
        a = _args(c, t)
        a.grad_out = t["go"].data_ptr()
        for k, g in grads.items():
            setattr(a, "grad_" + k, g.data_ptr())
        a.workspace, a.workspace_bytes = ws.data_ptr() + (-ws.data_ptr()) % 16, nbytes
        _lib.check(_lib.lib().pna_set2set_bwd_f32(ctypes.byref(a), _lib.stream_ptr(cuda_device)), "pna_set2set_bwd_f32")
        torch.cuda.synchronize()
        for k in keep:
            assert torch.equal(grads[k], full[k]), k
