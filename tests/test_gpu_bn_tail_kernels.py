"""pna_bn_tail_fwd_f32 / pna_bn_tail_bwd_f32 through ctypes (pna_bn_tail.hip).  Every output buffer and the workspace are filled with NaN
before every call (pitched outputs: NaN in the N columns, a sentinel in the padding, which must survive); the workspace has exactly
pna_bn_tail_workspace_bytes(M, N) bytes and a sentinel word after it must survive.  Each random case of tests/bn_tail_cases.py: every
tensor against float64 within its per-element bars, no element excluded, and three runs with identical bits; the exact cases bit for
bit, the derivative at a pre-activation of exactly 0 included.  Then the NULL and momentum options, the backward's scope, a NaN and an
Inf that must stay in their column, and the refusals.  Every case prints its worst error / bar ratio per tensor (DESIGN.md quotes them)."""
import ctypes
import math

import pytest
import torch

import bn_tail_cases as C
from pna_amd import _lib

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENTINEL = C.SENTINEL
PITCH_KEYS = ("y", "residual", "out", "go", "grad_y")


def _pitch(c, key):
    return None if c["pitches"] is None else c["pitches"][PITCH_KEYS.index(key)]


def _place(t, ld, dev):
    """-> (buffer, view): t on the device, as the first columns of rows ld wide (padding: the sentinel) when ld is given."""
    if t is None:
        return None, None
    t = t.to(dev)
    return C.pitched(t, ld) if ld is not None else (t, t)


def _dev(c, dev, y=None):
    d = {"c": c, "dev": dev}
    _, d["y"] = _place(c["y"] if y is None else y, _pitch(c, "y"), dev)
    _, d["residual"] = _place(c["residual"], _pitch(c, "residual"), dev)
    _, d["go"] = _place(c["go"], _pitch(c, "go"), dev)
    for k in ("gamma", "beta"):
        d[k] = None if c[k] is None else c[k].to(dev)
    return d


def _ptr(t):
    return None if t is None else t.data_ptr()


def _workspace(c, dev):
    """-> (buffer, bytes): exactly the bytes the library asks for, NaN, and one sentinel word behind them."""
    nbytes = _lib.lib().pna_bn_tail_workspace_bytes(c["M"], c["N"])
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4 + 1,), NAN, device=dev)
    ws[-1] = SENTINEL
    return ws, nbytes


def _args(d):
    c = d["c"]
    a = _lib.PnaBnTailArgs()
    a.y, a.ldy, a.M, a.N, a.relu = d["y"].data_ptr(), d["y"].stride(0), c["M"], c["N"], c["relu"]
    a.gamma, a.beta = _ptr(d["gamma"]), _ptr(d["beta"])
    a.eps, a.momentum = c["eps"], c["momentum"]
    return a


def _out_buffer(M, N, ld, dev):
    """-> (buffer, view): NaN in the (M, N) view, the sentinel in the padding of rows ld wide."""
    view = torch.full((M, N), NAN, device=dev)
    return C.pitched(view, ld) if ld is not None else (view, view)


def _fwd(d, ws=None):
    """One forward -> dict: out (view), out_buf, save_mean, save_invstd, running_mean, running_var (None: NULL was passed), ws."""
    c, dev = d["c"], d["dev"]
    M, N = c["M"], c["N"]
    f = {}
    f["out_buf"], f["out"] = _out_buffer(M, N, _pitch(c, "out"), dev)
    f["save_mean"], f["save_invstd"] = torch.full((N,), NAN, device=dev), torch.full((N,), NAN, device=dev)
    f["running_mean"] = None if c["rm0"] is None else c["rm0"].to(dev).clone()
    f["running_var"] = None if c["rv0"] is None else c["rv0"].to(dev).clone()
    f["ws"], nbytes = _workspace(c, dev) if ws is None else ws
    a = _args(d)
    a.running_mean, a.running_var = _ptr(f["running_mean"]), _ptr(f["running_var"])
    if d["residual"] is not None:
        a.residual, a.ld_res = d["residual"].data_ptr(), d["residual"].stride(0)
    a.out, a.ld_out = f["out"].data_ptr(), f["out"].stride(0)
    a.save_mean, a.save_invstd = f["save_mean"].data_ptr(), f["save_invstd"].data_ptr()
    a.workspace, a.workspace_bytes = f["ws"].data_ptr(), nbytes
    _lib.check(_lib.lib().pna_bn_tail_fwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_bn_tail_fwd_f32")
    assert float(f["ws"][-1]) == SENTINEL
    if _pitch(c, "out") is not None:
        assert bool((f["out_buf"][:, N:] == SENTINEL).all())
    return f


def _bwd(d, f, ws=None, fill=NAN):
    """One backward from the forward's saved statistics alone -> dict: grad_y (view), gy_buf, grad_gamma, grad_beta (a gradient in the
    case's null_grads is passed as NULL; its buffer is returned all the same)."""
    c, dev = d["c"], d["dev"]
    M, N = c["M"], c["N"]
    b = {}
    b["gy_buf"], b["grad_y"] = _out_buffer(M, N, _pitch(c, "grad_y"), dev)
    b["grad_gamma"], b["grad_beta"] = torch.full((N,), fill, device=dev), torch.full((N,), fill, device=dev)
    wsb, nbytes = _workspace(c, dev) if ws is None else ws
    a = _args(d)
    a.momentum = -1.0
    a.save_mean, a.save_invstd = f["save_mean"].data_ptr(), f["save_invstd"].data_ptr()
    a.workspace, a.workspace_bytes = wsb.data_ptr(), nbytes
    a.grad_out, a.ld_go = d["go"].data_ptr(), d["go"].stride(0)
    a.grad_y, a.ld_gy = b["grad_y"].data_ptr(), b["grad_y"].stride(0)
    a.grad_gamma = None if "grad_gamma" in c["null_grads"] else b["grad_gamma"].data_ptr()
    a.grad_beta = None if "grad_beta" in c["null_grads"] else b["grad_beta"].data_ptr()
    _lib.check(_lib.lib().pna_bn_tail_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_bn_tail_bwd_f32")
    assert float(wsb[-1]) == SENTINEL
    if _pitch(c, "grad_y") is not None:
        assert bool((b["gy_buf"][:, N:] == SENTINEL).all())
    return b


def _both(d):
    f = _fwd(d)
    b = _bwd(d, f)
    return {k: v for k, v in dict(f, **b).items() if k not in ("ws", "out_buf", "gy_buf")}


def _same_bits(a, b):
    """Bitwise equality of two result dicts (NaN equal to NaN)."""
    return all((a[k] is None and b[k] is None) or torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)) for k in a)


@pytest.mark.parametrize("name", C.NAMES)
def test_case_against_float64_within_the_bars(cuda_device, name):
    c = C.case(name)
    d = _dev(c, cuda_device)
    got = _both(d)
    names = C.tensors_of(c)
    worst = {k: C.worst_ratio(got[k].cpu(), c["ref"][k], c["bars"][k]) for k in names}
    print("BN_RATIO", name, " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    if len(set(c["kinds"])) > 1:                                                  # the statistics cases: per kind of column
        for kind in C.KINDS:
            cols = [i for i, k in enumerate(c["kinds"]) if k == kind]
            per = {k: C.worst_ratio(got[k].cpu()[..., cols], c["ref"][k][..., cols], c["bars"][k][..., cols]) for k in names}
            print("BN_RATIO_KIND", name, kind, " ".join(f"{k}={v:.4f}" for k, v in per.items()))
    assert all(bool(torch.isfinite(got[k]).all()) for k in names)
    assert all(v <= 1.0 for v in worst.values()), worst
    for k in c["null_grads"]:                                                     # a NULL gradient: its buffer was never named
        assert bool(torch.isnan(got[k]).all())
    if c["rm0"] is not None and c["momentum"] < 0:                                # momentum < 0: the running pair is left alone
        assert torch.equal(got["running_mean"].cpu(), c["rm0"]) and torch.equal(got["running_var"].cpu(), c["rv0"])
    if c["rm0"] is not None and c["momentum"] == 0:
        assert torch.equal(got["running_mean"].cpu(), c["rm0"]) and torch.equal(got["running_var"].cpu(), c["rv0"])
    if c["momentum"] == 1:                                                        # the batch values themselves, the variance unbiased
        assert torch.equal(got["running_mean"], got["save_mean"])
        M = c["M"]
        var_unbiased = (1.0 / got["save_invstd"].double().cpu() ** 2 - float(torch.tensor(c["eps"], dtype=torch.float32))) * M / (M - 1)
        torch.testing.assert_close(got["running_var"].double().cpu(), var_unbiased, rtol=1e-6, atol=0)
    for k, kind in enumerate(c["kinds"]):                                         # a constant column: var == 0 exactly
        if kind == "const":
            assert float(got["save_mean"][k]) == float(c["y"][0, k])
            assert float(got["save_invstd"][k]) == float(torch.tensor(1 / math.sqrt(float(torch.tensor(c["eps"], dtype=torch.float32))), dtype=torch.float32))
            if c["relu"] == 0 and c["residual"] is None:
                assert bool((got["out"][:, k] == float(c["beta"][k])).all())      # z == beta bit for bit
            else:
                assert torch.equal(got["out"][:, k].cpu(), c["residual"][:, k] + max(float(c["beta"][k]), 0.0))
    for _ in range(2):                                                            # three runs, identical bits
        assert _same_bits(got, _both(d))


@pytest.mark.parametrize("name", C.EXACT_NAMES)
def test_exact_case_bit_for_bit(cuda_device, name):
    c = C.exact_case(name)
    got = _both(_dev(c, cuda_device))
    for k in C.tensors_of(c):
        want = c["ref"][k].float()                                                # (exact for all but running_var: tests/test_bn_tail_cases_host.py)
        assert torch.equal(got[k].cpu(), want), (name, k, float((got[k].cpu() - want).abs().max()))


def test_null_and_momentum_options_leave_their_buffers_alone(cuda_device):
    c = C.case("n33")
    d = _dev(c, cuda_device)
    full = _both(d)
    # running statistics NULL: the same out and saved statistics
    f = _fwd(_dev(dict(c, rm0=None, rv0=None), cuda_device))
    assert f["running_mean"] is None and all(torch.equal(f[k], full[k]) for k in ("out", "save_mean", "save_invstd"))
    # momentum < 0 with the pair given: bitwise untouched, everything else the same
    f = _fwd(_dev(dict(c, momentum=-0.5), cuda_device))
    assert torch.equal(f["running_mean"].cpu(), c["rm0"]) and torch.equal(f["running_var"].cpu(), c["rv0"])
    assert all(torch.equal(f[k], full[k]) for k in ("out", "save_mean", "save_invstd"))
    # momentum = 1: the batch values
    f = _fwd(_dev(dict(c, momentum=1.0), cuda_device))
    assert torch.equal(f["running_mean"], f["save_mean"]) and torch.equal(f["save_mean"], full["save_mean"])
    # grad_gamma / grad_beta NULL: their buffers keep the sentinel, the other gradients their bits
    for nulls in (("grad_gamma",), ("grad_beta",), ("grad_gamma", "grad_beta")):
        dn = _dev(dict(c, null_grads=nulls), cuda_device)
        b = _bwd(dn, _fwd(dn), fill=SENTINEL)
        for k in ("grad_y", "grad_gamma", "grad_beta"):
            if k in nulls:
                assert bool((b[k] == SENTINEL).all()), (nulls, k)
            else:
                assert torch.equal(b[k], full[k]), (nulls, k)


def test_backward_reads_y_grad_out_and_the_saved_statistics_only(cuda_device):
    c = C.case("m1025")
    d = _dev(c, cuda_device)
    f = _fwd(d)
    fresh = _bwd(d, f)                                                            # a fresh NaN workspace
    nbytes = _lib.lib().pna_bn_tail_workspace_bytes(c["M"], c["N"])
    reused = _bwd(d, f, ws=(f["ws"], nbytes))                                     # the forward's own
    assert _same_bits(fresh, reused)
    # ... and from copies of the two saved vectors alone: nothing else of the forward is named in _bwd's struct (residual, out and the
    # running pair are NULL there)
    alone = _bwd(d, {"save_mean": f["save_mean"].clone(), "save_invstd": f["save_invstd"].clone()})
    assert _same_bits(fresh, alone)
    assert all(bool(torch.isfinite(fresh[k]).all()) for k in ("grad_y", "grad_gamma", "grad_beta"))


@pytest.mark.parametrize("value", [NAN, float("inf")])
def test_a_nan_or_an_inf_stays_in_its_column(cuda_device, value):
    c = C.case("n33")                                                             # 521 rows, 33 columns: column 32 is the clamped lanes'
    base = _both(_dev(c, cuda_device))
    for r, col in ((0, 5), (300, 7), (100, 32)):                                  # row 0, an interior element, the last column
        y = c["y"].clone()
        y[r, col] = value
        got = _both(_dev(c, cuda_device, y=y))
        others = [k for k in range(c["N"]) if k != col]
        for k in C.tensors_of(c):
            a, b = got[k][..., others], base[k][..., others]
            assert torch.equal(a, b), (value, r, col, k)                           # every other column: the bits of the run without it
        # its own column: what torch gives -- mean non-finite, invstd NaN, every output of the column NaN
        assert not math.isfinite(float(got["save_mean"][col])) and math.isnan(float(got["save_invstd"][col]))
        assert not math.isfinite(float(got["running_mean"][col])) and math.isnan(float(got["running_var"][col]))
        assert bool(torch.isnan(got["out"][:, col]).all()) and bool(torch.isnan(got["grad_y"][:, col]).all())
        assert math.isnan(float(got["grad_gamma"][col]))


def test_calls_refuse_what_is_outside_the_scope_and_write_nothing(cuda_device):
    L = _lib.lib()
    c = C.case("n33")
    M, N = c["M"], c["N"]
    d = _dev(c, cuda_device)
    good_f = _fwd(d)
    good_b = _bwd(d, good_f)
    stream = _lib.stream_ptr(cuda_device)
    nbytes = L.pna_bn_tail_workspace_bytes(M, N)

    def sentinels(*shapes):
        return [torch.full(s, SENTINEL, device=cuda_device) for s in shapes]

    def fwd_args():
        out, mean, invstd, ws = sentinels((M, N), (N,), (N,), (nbytes // 4,))
        rm, rv = c["rm0"].to(cuda_device), c["rv0"].to(cuda_device)
        a = _args(d)
        a.running_mean, a.running_var = rm.data_ptr(), rv.data_ptr()
        a.residual, a.ld_res = d["residual"].data_ptr(), N
        a.out, a.ld_out, a.save_mean, a.save_invstd = out.data_ptr(), N, mean.data_ptr(), invstd.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        return a, {"out": out, "save_mean": mean, "save_invstd": invstd, "ws": ws, "running_mean": rm, "running_var": rv}

    def untouched(t):
        return (all(bool((t[k] == SENTINEL).all()) for k in t if not k.startswith("running"))
                and all(torch.equal(t[k].cpu(), c[{"running_mean": "rm0", "running_var": "rv0"}[k]]) for k in t if k.startswith("running")))

    short = ctypes.sizeof(_lib.PnaBnTailArgs) - 8
    for kw in [{"M": 1}, {"N": 0}, {"N": 129}, {"ldy": N - 1}, {"ld_res": N - 1}, {"ld_out": N - 1}, {"workspace_bytes": nbytes - 1},
               {"running_mean": None}, {"running_var": None}, {"struct_size": short}, {"y": None}, {"out": None}, {"save_mean": None},
               {"save_invstd": None}, {"workspace": None}]:
        a, t = fwd_args()
        for k, v in kw.items():
            setattr(a, k, v)
        assert L.pna_bn_tail_fwd_f32(ctypes.byref(a), stream) < 0, kw
        assert b"pna_bn_tail_fwd_f32" in L.pna_last_error(), (kw, L.pna_last_error())
        torch.cuda.synchronize()
        assert untouched(t), kw

    def bwd_args():
        gy, gg, gb, ws = sentinels((M, N), (N,), (N,), (nbytes // 4,))
        a = _args(d)
        a.momentum = -1.0
        a.save_mean, a.save_invstd = good_f["save_mean"].data_ptr(), good_f["save_invstd"].data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        a.grad_out, a.ld_go, a.grad_y, a.ld_gy = d["go"].data_ptr(), N, gy.data_ptr(), N
        a.grad_gamma, a.grad_beta = gg.data_ptr(), gb.data_ptr()
        return a, {"grad_y": gy, "grad_gamma": gg, "grad_beta": gb, "ws": ws}

    for kw in [{"M": 1}, {"N": 0}, {"N": 129}, {"ldy": N - 1}, {"ld_go": N - 1}, {"ld_gy": N - 1}, {"workspace_bytes": nbytes - 1},
               {"struct_size": short}, {"y": None}, {"grad_out": None}, {"grad_y": None}, {"save_mean": None}, {"save_invstd": None},
               {"workspace": None}]:
        a, t = bwd_args()
        for k, v in kw.items():
            setattr(a, k, v)
        assert L.pna_bn_tail_bwd_f32(ctypes.byref(a), stream) < 0, kw
        assert b"pna_bn_tail_bwd_f32" in L.pna_last_error(), (kw, L.pna_last_error())
        torch.cuda.synchronize()
        assert untouched(t), kw
    assert L.pna_bn_tail_fwd_f32(None, stream) < 0 and b"pna_bn_tail_fwd_f32" in L.pna_last_error()
    assert L.pna_bn_tail_bwd_f32(None, stream) < 0 and b"pna_bn_tail_bwd_f32" in L.pna_last_error()
    a, t = fwd_args()                                                             # and the same structs inside the scope run
    assert L.pna_bn_tail_fwd_f32(ctypes.byref(a), stream) == 0
    assert all(torch.equal(t[k], good_f[k]) for k in ("out", "save_mean", "save_invstd", "running_mean", "running_var"))
    a, t = bwd_args()
    assert L.pna_bn_tail_bwd_f32(ctypes.byref(a), stream) == 0 and all(torch.equal(t[k], good_b[k]) for k in ("grad_y", "grad_gamma", "grad_beta"))
