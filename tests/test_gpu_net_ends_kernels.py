"""pna_embed_sum_*_f32 and pna_readout_*_f32 through ctypes (pna_net_ends.hip), the workspace filled with NaN before every call.
Embedding: the forward's bits are today's eager `0 + e_0 + e_1 + ...`; every gradient element within the serial-sum bound of float64
(n u sum |g| over the n rows that select it: tests/net_ends_cases.py), exactly 0.0 where nobody selects it; 20 bit-identical repeats;
PNA_E_INVALID outside the scope.  Readout: max values and arg rows are the bits of today's route, sum / mean and all gradients
within the same bound plus one rounding for the division."""
import ctypes

import pytest
import torch

import net_ends_cases as C
from pna_amd import _lib, nets, ops
from pna_amd import functional as PF
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu


def _embed_args(idx, tables, out=None, go=None, grads=None, ws=None):
    a = _lib.PnaEmbedSumArgs()
    a.V, a.n_table, a.F = idx.shape[0], len(tables), tables[0].shape[1]
    a.idx, a.ld_idx = idx.data_ptr(), idx.stride(0)
    for j, w in enumerate(tables):
        a.table[j], a.rows[j], a.ld_table[j] = w.data_ptr(), w.shape[0], w.stride(0)
    if out is not None:
        a.out, a.ld_out = out.data_ptr(), out.stride(0)
    if go is not None:
        a.grad_out, a.ld_go = go.data_ptr(), go.stride(0)
        for j, g in enumerate(grads):
            a.grad_table[j] = g.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    return a


def _embed_fwd(idx, tables):
    out = torch.full((idx.shape[0], tables[0].shape[1]), float("nan"), device=idx.device)
    a = _embed_args(idx, tables, out=out)
    _lib.check(_lib.lib().pna_embed_sum_fwd_f32(ctypes.byref(a), _lib.stream_ptr(idx.device)), "pna_embed_sum_fwd_f32")
    return out


def _embed_bwd(idx, tables, go):
    dev = idx.device
    rows, F = [w.shape[0] for w in tables], tables[0].shape[1]
    nbytes = PF.embed_sum_workspace_bytes(idx.shape[0], rows, F)
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float("nan"), device=dev)
    grads = [torch.full((r, F), float("nan"), device=dev) for r in rows]          # neither accumulated into nor assumed cleared
    a = _embed_args(idx, tables, go=go, grads=grads, ws=ws)
    _lib.check(_lib.lib().pna_embed_sum_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_embed_sum_bwd_f32")
    return grads


def _eager(idx, tables):
    out = 0
    for j, w in enumerate(tables):
        out = out + w.index_select(0, idx[:, j])
    return out


def _check_embed(idx, tables, go, idx_dev, repeats=20):
    """idx_dev: the device index the calls get, (V, T) of any row stride or 1-D for one table; idx: its (V, T) host values."""
    dev = idx_dev.device
    tab = [w.to(dev) for w in tables]
    rows = [w.shape[0] for w in tables]
    god = go.to(dev)
    out = _embed_fwd(idx_dev, tab)
    assert torch.equal(out, _eager(idx.to(dev), tab))
    grads = _embed_bwd(idx_dev, tab, god)
    for j, ((ref, n, mass), g) in enumerate(zip(C.embed_grad_ref64(idx, rows, go), grads)):
        err = (g.cpu().double() - ref).abs()
        bound = C.serial_sum_bound(n, mass)
        assert bool((err <= bound).all()), (j, float((err - bound).max()), float(err.max()))
        assert bool((g.cpu()[n == 0] == 0).all())
    for _ in range(repeats - 1):
        again = _embed_bwd(idx_dev, tab, god)
        assert all(torch.equal(x, y) for x, y in zip(grads, again))
    assert torch.equal(_embed_fwd(idx_dev, tab), out)
    return grads


@pytest.mark.parametrize("name", sorted(C.EMBED_CASES))
def test_embedding_case(cuda_device, name):
    V, F, rows, idx, tables, go = C.embed_case(name)
    idx_dev = idx.to(cuda_device)
    grads = _check_embed(idx, tables, go, idx_dev[:, 0] if len(rows) == 1 else idx_dev, repeats=20 if V < 10000 else 3)
    if name == "unselected_row":
        assert bool((grads[0][3] == 0).all()) and bool((grads[0][2] != 0).any())
    if name == "every_node_one_row":                                               # V terms in one element: the longest serial sum
        assert bool((grads[0][:3] == 0).all()) and bool((grads[0][3] != 0).all())


def test_embedding_index_as_a_strided_view(cuda_device):
    """What the nets pass: columns [2, 11) of a wider (V, 12) index tensor for the nine tables, one column of it for a single table."""
    V, F, rows, idx, tables, go = C.embed_case("three_slabs_17_f128_t9")
    wide = torch.full((V, 12), 10 ** 6, dtype=torch.int64)
    wide[:, 2:11] = idx
    wide = wide.to(cuda_device)
    view = wide[:, 2:11]
    assert view.stride() == (12, 1) and not view.is_contiguous()
    _check_embed(idx, tables, go, view, repeats=2)
    col = wide[:, 2]
    assert col.stride() == (12,)
    _check_embed(idx[:, :1], tables[:1], go, col, repeats=2)


def test_embedding_calls_refuse_what_is_outside_the_scope(cuda_device):
    L = _lib.lib()
    dev = cuda_device
    V = 10

    def call(rows, F, short=0):
        idx = torch.zeros(V, max(1, len(rows)), dtype=torch.int64, device=dev)
        tab = [torch.zeros(r, F, device=dev) for r in rows[:_lib.PNA_MAX_EMBED_TABLE]]
        out, go = torch.zeros(V, F, device=dev), torch.zeros(V, F, device=dev)
        ws = torch.zeros(1 << 20, device=dev)
        a = _embed_args(idx, tab, out=out, go=go, grads=[torch.zeros_like(w) for w in tab], ws=ws)
        a.n_table = len(rows)
        a.struct_size -= short
        return [fn(ctypes.byref(a), _lib.stream_ptr(dev)) for fn in (L.pna_embed_sum_fwd_f32, L.pna_embed_sum_bwd_f32)]
    assert call((3, 4), 8) == [0, 0]
    assert call((3,) * 17, 8) == [-1, -1]                                          # n_table = 17
    assert call((3, 4), 257) == [-1, -1]                                           # F = 257
    assert call((3, 4), 8, short=8) == [-1, -1] and b"struct_size" in L.pna_last_error()
    assert call((119, 137), 128) == [0, 0] and call((119, 138), 128) == [-1, -1]   # a table set over the LDS limit
    torch.cuda.synchronize()


# ---- readout ----------------------------------------------------------------------------------------------------------------------------
def _readout_args(off, V, F, op):
    a = _lib.PnaReadoutArgs()
    a.offsets, a.G, a.V, a.F, a.op = off.data_ptr(), off.numel() - 1, V, F, _lib.AGG_CODES[op]
    return a


def _readout_fwd(off, h, op):
    V, F = h.shape
    G = off.numel() - 1
    out = torch.full((G, F), float("nan"), device=h.device)
    arg = torch.full((G, F), -7, dtype=torch.int32, device=h.device)
    a = _readout_args(off, V, F, op)
    a.h, a.ldh, a.out, a.ld_out = h.data_ptr(), h.stride(0), out.data_ptr(), out.stride(0)
    if op == "max":
        a.argmax = arg.data_ptr()
    _lib.check(_lib.lib().pna_readout_fwd_f32(ctypes.byref(a), _lib.stream_ptr(h.device)), "pna_readout_fwd_f32")
    return out, arg


def _readout_bwd(off, V, go, op, arg):
    F = go.shape[1]
    gh = torch.full((V, F), float("nan"), device=go.device)                        # every element is written
    a = _readout_args(off, V, F, op)
    a.grad_out, a.ld_go, a.grad_h, a.ld_gh = go.data_ptr(), go.stride(0), gh.data_ptr(), gh.stride(0)
    if op == "max":
        a.argmax = arg.data_ptr()
    _lib.check(_lib.lib().pna_readout_bwd_f32(ctypes.byref(a), _lib.stream_ptr(go.device)), "pna_readout_bwd_f32")
    return gh


@pytest.fixture(scope="module")
def todays_route(cuda_device):
    """sizes name, F, tie -> (values per op, argmax) of today's readout_nodes (the generic aggregate over the readout graph), once."""
    memo = {}

    def get(sizes_name, F, tie):
        key = (sizes_name, F, tie)
        if key not in memo:
            sizes, h, _ = C.readout_case(sizes_name, F, tie)
            V = sum(sizes)
            g = Graph(torch.arange(V), torch.arange(V), V, sizes).to(cuda_device)
            hd = h.to(cuda_device)
            keep, PF.NET_ENDS_ROWS = PF.NET_ENDS_ROWS, 0
            try:
                vals = {op: nets.readout_nodes(g, hd, op) for op in C.READOUT_OPS}
            finally:
                PF.NET_ENDS_ROWS = keep
            rg = g._heavy[("readout", hd.device)]
            mx, amx, _ = ops.segreduce(rg.csr.rowptr, None, hd, F, ["max"], want_arg=True, heavy=rg.heavy_schedule(), workspace=rg.workspace,
                                       items=rg.work_items())
            assert torch.equal(mx, vals["max"])
            memo[key] = (vals, amx, rg.csr.rowptr)
        return memo[key]
    return get


@pytest.mark.parametrize("tie", [False, True])
@pytest.mark.parametrize("F", C.READOUT_F)
@pytest.mark.parametrize("sizes_name", sorted(C.READOUT_SIZES))
def test_readout_case(cuda_device, todays_route, sizes_name, F, tie):
    sizes, h, go = C.readout_case(sizes_name, F, tie)
    V = sum(sizes)
    vals, amx, rowptr = todays_route(sizes_name, F, tie)
    off = nets._readout_offsets(Graph(torch.arange(V), torch.arange(V), V, sizes), cuda_device)
    assert torch.equal(off, rowptr)                                                # the readout graph's rowptr
    hd, god = h.to(cuda_device), go.to(cuda_device)
    n = torch.tensor(sizes, dtype=torch.float64)
    mass = torch.stack([p.double().abs().sum(0) for p in torch.split(h, sizes)])
    for op in C.READOUT_OPS:
        out, arg = _readout_fwd(off, hd, op)
        ref, ref_arg = C.readout_ref64(h, sizes, op)
        if op == "max":
            assert torch.equal(out, vals["max"]) and torch.equal(arg, amx)
            assert torch.equal(out.cpu().double(), ref) and torch.equal(arg.cpu().long(), ref_arg)
        else:
            bound = C.serial_sum_bound(n, mass)
            if op == "mean":
                bound = bound / n[:, None] + C.U * ref.abs()                      # the sum's error divided, one rounding of the quotient
            err = (out.cpu().double() - ref).abs()
            assert bool((err <= bound).all()), (op, float((err - bound).max()))
            torch.testing.assert_close(out, vals[op], rtol=1e-5, atol=1e-5)        # (today's route sums in another order)
        gh = _readout_bwd(off, V, god, op, arg)
        gref = C.readout_grad_ref64(h, sizes, op, go)
        gerr = (gh.cpu().double() - gref).abs()
        gbound = C.U * gref.abs() if op == "mean" else torch.zeros_like(gref)      # one term each: exact, but for mean's division
        assert bool((gerr <= gbound).all()), (op, float(gerr.max()))
        for _ in range(19):
            o2, a2 = _readout_fwd(off, hd, op)
            assert torch.equal(o2, out) and (op != "max" or torch.equal(a2, arg))
            assert torch.equal(_readout_bwd(off, V, god, op, arg), gh)
    if tie:                                                                        # the gradient goes to the first of the two tied rows only
        g = sizes.index(sorted(sizes)[-2]) if len(sizes) > 1 else 0
        at = sum(sizes[:g])
        _, arg = _readout_fwd(off, hd, "max")
        gh = _readout_bwd(off, V, god, "max", arg)
        assert bool((arg[g] == at + 5).all()) and torch.equal(gh[at + 5], god[g]) and bool((gh[at + 11] == 0).all())


def test_readout_calls_refuse_what_is_outside_the_scope(cuda_device):
    L = _lib.lib()
    off = torch.tensor([0, 3, 8], dtype=torch.int32, device=cuda_device)

    def call(F, op="sum", short=0, G=2):
        h, out, arg = torch.zeros(8, F, device=cuda_device), torch.zeros(2, F, device=cuda_device), torch.zeros(2, F, dtype=torch.int32, device=cuda_device)
        a = _readout_args(off, 8, F, "sum")
        a.op = {"sum": 1, "mean": 0, "max": 2, "min": 3}[op]
        a.G = G
        a.h, a.ldh, a.out, a.ld_out, a.argmax = h.data_ptr(), F, out.data_ptr(), F, arg.data_ptr()
        a.struct_size -= short
        return L.pna_readout_fwd_f32(ctypes.byref(a), _lib.stream_ptr(cuda_device))
    assert call(512) == 0 and call(513) == -1 and call(0) == -1
    assert call(8, "max") == 0 and call(8, "min") == -1
    assert call(8, G=0) == -1
    assert call(8, short=8) == -1 and b"struct_size" in L.pna_last_error()
    torch.cuda.synchronize()
