"""Kernel-level float64 checks of pna_posttrans_dw_f32 and pna_posttrans_dw_grouped_f32 (pna_amd/csrc/pna_posttrans_dw.hip) on the cases of
posttrans_dw_cases.py, through a ctypes caller that owns every pointer and pitch: gy, a, h and grad_w sit inside larger buffers whose other
columns and rows hold NaN (inputs) or a canary (outputs), grad_b lies between canaries, the row scalers are followed by NaN, and the
workspace is filled with NaN before every call (the header: no initialisation needed).

  every case         |got - ref64| <= 1e-5 |ref64| + 2^-22 sum_m |terms| per element of grad_w and grad_b; canaries intact
  integer cases      the float64 result bit for bit
  wide cases         N = 129, 200, 240 with one scaler: refused end to end (workspace_bytes -1, the call -1, ops.posttrans_dw None); no
                     kernel runs on them, and no other edge of the table depends on them
  grouped plans      hand-built tables, both a_plan_order settings (the padding rows of a plan-ordered `a` hold NaN)

Measured on an MI355X, worst err / bar over every case of the family: plain 0.311, grouped 0.268, integer cases 0 (the float64 bits), the
layer-level check at N = 136 0.397.  Before plan() refused N > 128 the wide cases returned exact zeros in rows 128 .. of
grad_w and grad_b (9e4 times the bar) and the layer-level check sat at 7e4."""
import ctypes

import numpy as np
import pytest
import torch

import posttrans_dw_cases as C
from pna_amd import _lib

pytestmark = pytest.mark.gpu

NAN = float("nan")
_cases, _runs, _worst = {}, {}, {}


def _plain(name):
    if "plain" not in _cases:
        _cases["plain"] = C.plain_cases()
    return _cases["plain"][name]


def _grouped(name):
    if "grouped" not in _cases:
        _cases["grouped"] = C.grouped_cases()
    return _cases["grouped"][name]


PLAIN_NAMES = [r[0] for r in C.PLAIN_TABLE] + [f"{n}/{v}" for v, names in C.PLAIN_VARIANTS.items() for n in names]
GROUPED_NAMES = [r[0] for r in C.GROUPED_PLANS] + [f"{n}/{v}" for v, names in C.GROUPED_VARIANTS.items() for n in names]


def _note(family, what, ratio):
    _worst[family] = max(_worst.get(family, 0.0), ratio)
    print(f"[dw edges] {what}: worst err / bar = {ratio:.4f} ({family} so far: {_worst[family]:.4f})")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _pitched(a, dev, extra_cols, tail_rows=2, fill=NAN):
    """(rows, cols) view of a (rows + tail_rows, cols + extra_cols) device buffer filled with `fill` around the data."""
    buf = torch.full((a.shape[0] + tail_rows, a.shape[1] + extra_cols), fill, dtype=torch.float32, device=dev)
    buf[:a.shape[0], :a.shape[1]] = _t(a, dev)
    return buf[:a.shape[0], :a.shape[1]]


def _vector(v, dev, fill=NAN):
    buf = torch.full((v.size + 8,), fill, dtype=torch.float32, device=dev)
    buf[:v.size] = _t(v, dev)
    return buf[:v.size]


class _Outputs:
    """grad_w as rows 1 .. N of an (N + 2, row length + 7) canary buffer, grad_b as elements 8 .. 8 + N of a canary vector, the workspace
    with NaN in its `nbytes` and a canary behind them."""

    def __init__(self, dev, N, cols, nbytes, bias):
        can = float(C.CANARY)
        self.N, self.cols, self.nfloat = N, cols, nbytes // 4
        self.wbuf = torch.full((N + 2, cols + 7), can, dtype=torch.float32, device=dev)
        self.gw = self.wbuf[1:N + 1, :cols]
        self.bbuf = torch.full((N + 16,), can, dtype=torch.float32, device=dev)
        self.gb = self.bbuf[8:8 + N] if bias else None
        self.ws = torch.full((self.nfloat + 64,), can, dtype=torch.float32, device=dev)
        self.ws[:self.nfloat] = NAN

    def read(self):
        """(grad_w, grad_b) on the host after checking that nothing but them and the workspace's own bytes changed."""
        can = C.CANARY.view(np.uint32)
        w, b = self.wbuf.cpu().numpy(), self.bbuf.cpu().numpy()
        assert (w[0].view(np.uint32) == can).all() and (w[-1].view(np.uint32) == can).all(), "the rows around grad_w were written"
        assert (w[:, self.cols:].view(np.uint32) == can).all(), "grad_w's padding columns were written"
        keep = np.ones(b.size, bool)
        if self.gb is not None:
            keep[8:8 + self.N] = False
        assert (b.view(np.uint32)[keep] == can).all(), "the floats around grad_b were written" if self.gb is not None else "a NULL grad_b was written"
        assert (self.ws[self.nfloat:].cpu().numpy().view(np.uint32) == can).all(), "the floats behind the workspace were written"
        return w[1:-1, :self.cols].copy(), (b[8:8 + self.N].copy() if self.gb is not None else None)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class PlainCall:
    """One pna_posttrans_dw_f32 call over a case: owns every device buffer.  `bias=False` passes grad_b = NULL, `nbytes` overrides the
    workspace size (the refused shapes have none of their own)."""

    def __init__(self, dev, c, bias=None, nbytes=None, gy=None, a=None):
        L = _lib.lib()
        self.dev, self.c = dev, c
        M, N, S, K, Kh = c["M"], c["N"], c["S"], c["K"], c["Kh"]
        self.bias = c["bias"] if bias is None else bias
        self.need = L.pna_posttrans_dw_workspace_bytes(M, N, S, K, Kh)
        nbytes = self.need if nbytes is None else nbytes
        self.gy = _pitched(c["gy"] if gy is None else gy, dev, 3)
        self.a = _pitched(c["a"] if a is None else a, dev, 4)
        self.h = _pitched(c["h"], dev, 5) if Kh else None
        self.scales = [None if rs is None else _vector(rs, dev) for rs in c["scales"]]
        self.out = _Outputs(dev, N, Kh + S * K, max(nbytes, 0), self.bias)
        p = self.args = _lib.PnaPosttransDwArgs()
        p.gy, p.ldg, p.M, p.N, p.n_scaler = _ptr(self.gy), self.gy.stride(0), M, N, S
        p.a, p.lda, p.K, p.Kh = _ptr(self.a), self.a.stride(0), K, Kh
        if Kh:
            p.h, p.ldh = _ptr(self.h), self.h.stride(0)
        for s, rs in enumerate(self.scales):
            p.row_scale[s] = None if rs is None else rs.data_ptr()
        p.grad_w, p.ldw, p.grad_b = _ptr(self.out.gw), self.out.gw.stride(0), _ptr(self.out.gb)
        p.workspace, p.workspace_bytes = _ptr(self.out.ws), nbytes
        assert p.ldg > N and p.lda > K and p.ldw > Kh + S * K and (not Kh or p.ldh > Kh)

    def run(self):
        self.out.ws[:self.out.nfloat] = NAN
        rc = _lib.lib().pna_posttrans_dw_f32(ctypes.byref(self.args), _lib.stream_ptr(self.dev))
        torch.cuda.synchronize(self.dev)
        return rc


class GroupedCall:
    def __init__(self, dev, c, a_plan, bias=True, n_entries=None):
        L = _lib.lib()
        self.dev, self.c = dev, c
        N, S, K, Kh = c["N"], c["S"], c["K"], c["Kh"]
        self.need = L.pna_posttrans_dw_grouped_workspace_bytes(N, K, Kh, c["n_entries"])
        assert self.need == c["n_entries"] * C.ENTRY_BYTES
        self.gy = _pitched(c["gy"], dev, 3)
        self.a = _pitched(C.a_in_plan_order(c) if a_plan else c["a"], dev, 4)
        self.h = _pitched(c["h"], dev, 5) if Kh else None
        self.tables = [_t(c[k], dev) for k in ("row_perm", "tile_group", "wg_range", "wg_entry", "entry_group")]
        self.scale = _t(c["group_scale"], dev)
        self.out = _Outputs(dev, N, Kh + S * K, self.need, bias)
        # every index the kernels follow stays inside the buffers above
        assert c["row_perm"].max() < c["n_nodes"] and c["row_perm"].size == C.TILE * c["tile_group"].size
        assert c["wg_range"].min() >= 0 and c["wg_range"].max() <= c["tile_group"].size and c["wg_range"].shape == (c["n_wg"], 2)
        assert c["entry_group"].max() < c["group_scale"].shape[0] and c["tile_group"].max() < c["group_scale"].shape[0]
        runs = [sum(1 for t in range(lo, hi) if t == lo or c["tile_group"][t] != c["tile_group"][t - 1]) for lo, hi in c["wg_range"]]
        assert all(r == 0 or c["wg_entry"][w] + r <= c["n_entries"] for w, r in enumerate(runs))
        p = self.args = _lib.PnaPosttransDwGroupedArgs()
        p.gy, p.ldg, p.N, p.n_scaler = _ptr(self.gy), self.gy.stride(0), N, S
        p.a, p.lda, p.K, p.Kh = _ptr(self.a), self.a.stride(0), K, Kh
        if Kh:
            p.h, p.ldh = _ptr(self.h), self.h.stride(0)
        p.row_perm, p.tile_group, p.wg_range, p.wg_entry, p.entry_group = (_ptr(t) for t in self.tables)
        p.n_workgroups, p.n_entries, p.group_scale = c["n_wg"], c["n_entries"], _ptr(self.scale)
        p.grad_w, p.ldw, p.grad_b = _ptr(self.out.gw), self.out.gw.stride(0), _ptr(self.out.gb)
        p.workspace, p.workspace_bytes, p.a_plan_order = _ptr(self.out.ws), self.need, 1 if a_plan else 0

    def run(self):
        self.out.ws[:self.out.nfloat] = NAN
        rc = _lib.lib().pna_posttrans_dw_grouped_f32(ctypes.byref(self.args), _lib.stream_ptr(self.dev))
        torch.cuda.synchronize(self.dev)
        return rc


def _run_plain(name, dev):
    """(grad_w, grad_b, the same of a second call) of the case, once per module."""
    if ("plain", name) not in _runs:
        call = PlainCall(dev, _plain(name))
        _lib.check(call.run(), "pna_posttrans_dw_f32")
        first = call.out.read()
        _lib.check(call.run(), "pna_posttrans_dw_f32")
        _runs[("plain", name)] = first + call.out.read()
    return _runs[("plain", name)]


def _run_grouped(name, a_plan, dev):
    if ("grouped", name, a_plan) not in _runs:
        call = GroupedCall(dev, _grouped(name), a_plan)
        _lib.check(call.run(), "pna_posttrans_dw_grouped_f32")
        first = call.out.read()
        _lib.check(call.run(), "pna_posttrans_dw_grouped_f32")
        _runs[("grouped", name, a_plan)] = first + call.out.read()
    return _runs[("grouped", name, a_plan)]


def _check(c, gw, gb, r, family, what, skip_rows=(), skip_cols=()):
    rows = np.setdiff1d(np.arange(gw.shape[0]), skip_rows)
    cols = np.setdiff1d(np.arange(gw.shape[1]), skip_cols)
    sub = np.ix_(rows, cols)
    ratio, k = C.worst_ratio(gw[sub], r["gw"][sub], r["floor_w"][sub])
    if gb is not None:
        ratio = max(ratio, C.worst_ratio(gb[rows], r["gb"][rows], r["floor_b"][rows])[0])
    _note(family, what, ratio)
    assert ratio <= 1.0, (what, ratio, np.unravel_index(k, (rows.size, cols.size)))
    if c["variant"] == "int" and not len(skip_rows) and not len(skip_cols):
        assert C.same_bits(gw, r["gw"]) and (gb is None or C.same_bits(gb, r["gb"])), f"{what}: not the float64 result bit for bit"


@pytest.mark.parametrize("name", PLAIN_NAMES)
def test_plain_kernel_against_float64(cuda_device, name):
    c = _plain(name)
    L = _lib.lib()
    if c["refused"]:
        # one scaler and more than 128 columns of gy: wider than the two 64-column blocks the kernel stages -- refused end to end
        from pna_amd import ops
        assert L.pna_posttrans_dw_workspace_bytes(c["M"], c["N"], c["S"], c["K"], c["Kh"]) == -1
        call = PlainCall(cuda_device, c, nbytes=c["slabs"] * C.SLAB_BYTES)
        assert call.run() == -1 and "pna_posttrans_dw_f32" in L.pna_last_error().decode() and "N <= 128" in L.pna_last_error().decode()
        gw, gb = call.out.read()
        can = C.CANARY.view(np.uint32)
        assert (gw.view(np.uint32) == can).all() and (gb.view(np.uint32) == can).all()
        dev = cuda_device
        assert ops.posttrans_dw(_t(c["gy"], dev), _t(c["a"], dev), c["K"], _t(c["h"], dev) if c["Kh"] else None, [None]) is None
        return
    assert L.pna_posttrans_dw_workspace_bytes(c["M"], c["N"], c["S"], c["K"], c["Kh"]) == c["slabs"] * C.SLAB_BYTES
    gw, gb, gw2, gb2 = _run_plain(name, cuda_device)
    assert (gb is not None) == c["bias"]
    _check(c, gw, gb, C.ref_plain(c), "integer" if c["variant"] == "int" else "plain", f"plain {name}")
    assert np.array_equal(gw.view(np.uint32), gw2.view(np.uint32)) and (gb is None or np.array_equal(gb.view(np.uint32), gb2.view(np.uint32)))


@pytest.mark.parametrize("a_plan", [0, 1])
@pytest.mark.parametrize("name", GROUPED_NAMES)
def test_grouped_kernel_against_float64(cuda_device, name, a_plan):
    c = _grouped(name)
    gw, gb, gw2, gb2 = _run_grouped(name, bool(a_plan), cuda_device)
    _check(c, gw, gb, C.ref_grouped(c), "integer" if c["variant"] == "int" else "grouped", f"grouped {name} a_plan_order={a_plan}")
    assert np.array_equal(gw.view(np.uint32), gw2.view(np.uint32)) and np.array_equal(gb.view(np.uint32), gb2.view(np.uint32))


def test_grouped_kernel_same_tiles_under_every_grid(cuda_device):
    """The seven tiles of mixed7 under 1, 2, 3 and 5 workgroups: the same operands and row order, tables that differ by where the runs are
    cut -- each inside the bar of the ONE reference."""
    base = _grouped("mixed7_wg1")
    r = C.ref_grouped(base)
    entries = set()
    for n_wg in C.EDGES_WORKGROUPS:
        c = _grouped(f"mixed7_wg{n_wg}")
        assert c["n_wg"] == n_wg and all(np.array_equal(c[k], base[k], equal_nan=True) for k in ("gy", "a", "h", "group_scale", "row_perm", "tile_group"))
        entries.add(c["n_entries"])
        for a_plan in (False, True):
            gw, gb, _, _ = _run_grouped(c["name"], a_plan, cuda_device)
            _check(c, gw, gb, r, "grouped", f"grouped {c['name']} a_plan_order={int(a_plan)}")
    assert len(entries) > 1


@pytest.mark.parametrize("name", ["m33_n65_r383", "m257_n80_s3"])
def test_null_grad_b_with_and_without_h(cuda_device, name):
    """grad_b = NULL next to an h panel, and without one (the scaler blocks alone): grad_w keeps its bits, nothing is written for grad_b."""
    c = _plain(name)
    gw_ref = _run_plain(name, cuda_device)[0]
    call = PlainCall(cuda_device, c, bias=False)
    _lib.check(call.run(), "pna_posttrans_dw_f32")
    gw, gb = call.out.read()
    assert gb is None and np.array_equal(gw.view(np.uint32), gw_ref.view(np.uint32))
    no_h = dict(c, Kh=0, h=None)
    call = PlainCall(cuda_device, no_h, bias=False)
    _lib.check(call.run(), "pna_posttrans_dw_f32")
    gw0, gb0 = call.out.read()
    assert gb0 is None and np.array_equal(gw0.view(np.uint32), gw_ref[:, c["Kh"]:].view(np.uint32))
    for a_plan in (False, True):
        g = _grouped("aba")
        call = GroupedCall(cuda_device, g, a_plan, bias=False)
        _lib.check(call.run(), "pna_posttrans_dw_grouped_f32")
        gwg, gbg = call.out.read()
        assert gbg is None and np.array_equal(gwg.view(np.uint32), _run_grouped("aba", a_plan, cuda_device)[0].view(np.uint32))


def test_non_finite_inputs_stay_in_their_rows_and_columns(cuda_device):
    """The header: non-finite inputs give NaN in the columns / rows they touch -- and nowhere else."""
    c = _plain("m33_n65_r383")
    N, S, K, Kh = c["N"], c["S"], c["K"], c["Kh"]
    r = C.ref_plain(c)
    m0, n0, k0 = 20, 64, 299
    gy = c["gy"].copy()
    gy[m0, n0] = np.nan
    call = PlainCall(cuda_device, c, gy=gy)
    _lib.check(call.run(), "pna_posttrans_dw_f32")
    gw, gb = call.out.read()
    assert np.isnan(gw[n0]).all() and np.isnan(gb[n0])
    _check(c, gw, gb, r, "plain", "plain m33_n65_r383 with a NaN in gy", skip_rows=[n0])
    a = c["a"].copy()
    a[m0, k0] = np.inf
    call = PlainCall(cuda_device, c, a=a)
    _lib.check(call.run(), "pna_posttrans_dw_f32")
    gw, gb = call.out.read()
    cols = [Kh + s * K + k0 for s in range(S)]
    assert np.isnan(gw[:, cols]).all()
    _check(c, gw, gb, r, "plain", "plain m33_n65_r383 with an Inf in a", skip_cols=cols)


def test_argument_checks_name_the_entry_point(cuda_device):
    L = _lib.lib()
    c = _plain("m8_n16_r128")
    st = _lib.stream_ptr(cuda_device)

    def refused(call, fn, entry, word):
        call.out.ws[:call.out.nfloat] = NAN
        rc = fn(ctypes.byref(call.args), st)
        torch.cuda.synchronize(cuda_device)
        msg = L.pna_last_error().decode()
        assert rc == -1 and entry in msg and word in msg, (rc, msg)
        gw, gb = call.out.read()
        assert (gw.view(np.uint32) == C.CANARY.view(np.uint32)).all()

    def plain_call(**k):
        return PlainCall(cuda_device, c, **k)
    call = plain_call()
    call.args.struct_size = ctypes.sizeof(call.args) - 8
    refused(call, L.pna_posttrans_dw_f32, "pna_posttrans_dw_f32", "struct_size")
    call = plain_call()
    call.args.ldw = c["Kh"] + c["S"] * c["K"] - 1
    refused(call, L.pna_posttrans_dw_f32, "pna_posttrans_dw_f32", "leading dimension")
    call = plain_call()
    call.args.row_scale[0] = call.scales[1].data_ptr()                # with the h panel and grad_b
    refused(call, L.pna_posttrans_dw_f32, "pna_posttrans_dw_f32", "row_scale[0]")
    call = plain_call(bias=False)                                     # ... with the h panel alone (grad_b = NULL)
    call.args.row_scale[0] = call.scales[1].data_ptr()
    refused(call, L.pna_posttrans_dw_f32, "pna_posttrans_dw_f32", "row_scale[0]")
    call = PlainCall(cuda_device, dict(c, Kh=0, h=None))              # ... and with grad_b alone
    call.args.row_scale[0] = call.scales[1].data_ptr()
    refused(call, L.pna_posttrans_dw_f32, "pna_posttrans_dw_f32", "row_scale[0]")
    call = plain_call()
    call.args.workspace_bytes = call.need - 4
    refused(call, L.pna_posttrans_dw_f32, "pna_posttrans_dw_f32", "workspace")
    call = plain_call()
    call.args.K = 385 - c["Kh"] - 1                                   # R = 385 (never launched: no buffer is that wide)
    assert L.pna_posttrans_dw_workspace_bytes(c["M"], c["N"], c["S"], call.args.K, c["Kh"]) == -1
    refused(call, L.pna_posttrans_dw_f32, "pna_posttrans_dw_f32", "unsupported shape")
    g = _grouped("aba")
    call = GroupedCall(cuda_device, g, False)
    call.args.struct_size = ctypes.sizeof(call.args) - 8
    refused(call, L.pna_posttrans_dw_grouped_f32, "pna_posttrans_dw_grouped_f32", "struct_size")
    call = GroupedCall(cuda_device, g, False)
    call.args.N = 81
    assert L.pna_posttrans_dw_grouped_workspace_bytes(81, g["K"], g["Kh"], g["n_entries"]) == -1
    refused(call, L.pna_posttrans_dw_grouped_f32, "pna_posttrans_dw_grouped_f32", "N <= 80")
    call = GroupedCall(cuda_device, g, False)
    call.args.K = 385 - g["Kh"] - 1
    refused(call, L.pna_posttrans_dw_grouped_f32, "pna_posttrans_dw_grouped_f32", "unsupported shape")
    call = GroupedCall(cuda_device, g, False)
    call.args.ldw = g["Kh"] + g["S"] * g["K"] - 1
    refused(call, L.pna_posttrans_dw_grouped_f32, "pna_posttrans_dw_grouped_f32", "leading dimension")
    call = GroupedCall(cuda_device, g, False)
    call.args.workspace_bytes = call.need - 4
    refused(call, L.pna_posttrans_dw_grouped_f32, "pna_posttrans_dw_grouped_f32", "workspace")


def test_layer_gradient_at_136_columns_with_one_scaler(cuda_device):
    """functional.posttrans under autograd at M = 4096 (autograd.DW_MIN_ROWS), one scaler, N = 136, F = 16 and an h panel -- the shape a
    PNASimpleLayer with scalers = identity reaches -- against the same step in float64, with the kernel's own bar: it holds whichever
    route the backward takes for the shape."""
    from pna_amd import autograd, functional
    M, N, F = 4096, 136, 16
    K = 4 * F
    assert M >= autograd.DW_MIN_ROWS
    gen = torch.Generator(device=cuda_device).manual_seed(136)
    agg = torch.randn(M, K, device=cuda_device, generator=gen) * 3.0 + 0.5
    h = torch.randn(M, F, device=cuda_device, generator=gen)
    w = (torch.randn(N, F + K, device=cuda_device, generator=gen) / 8.0).requires_grad_()
    b = torch.randn(N, device=cuda_device, generator=gen).requires_grad_()
    gy = torch.randn(M, N, device=cuda_device, generator=gen)
    y = functional.posttrans(agg, K, w, b, [None], h)
    y.backward(gy)
    g64, x64 = gy.double(), torch.cat([h, agg], dim=1).double()
    want, floor = g64.t() @ x64, g64.abs().t() @ x64.abs()
    ratio = C.worst_ratio(w.grad.cpu().numpy(), want.cpu().numpy(), floor.cpu().numpy())[0]
    ratio_b = C.worst_ratio(b.grad.cpu().numpy(), g64.sum(0).cpu().numpy(), g64.abs().sum(0).cpu().numpy())[0]
    print(f"[dw edges] layer N = 136, one scaler: worst err / bar = {ratio:.4f} (weight), {ratio_b:.4f} (bias)")
    assert w.grad[128:].abs().sum().item() > 0 and ratio <= 1.0 and ratio_b <= 1.0, (ratio, ratio_b)
    y64 = x64 @ w.detach().double().t() + b.detach().double()
    fl = x64.abs() @ w.detach().double().abs().t() + b.detach().double().abs()
    assert ((y.detach().double() - y64).abs() <= 1e-5 * y64.abs() + 2.0 ** -22 * fl).all()
