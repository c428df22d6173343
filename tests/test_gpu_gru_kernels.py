"""pna_gru_cell_fwd_f32 / pna_gru_cell_bwd_f32 through ctypes (pna_gru.hip), every output buffer and the workspace filled with NaN before
every call.  Each case: `out` and the saved state r, z, n, gh_n and all six gradients against float64 within the DERIVED per-element bars of
tests/gru_cases.py (no element excluded), and 20 repeats with identical bits.  Then: row-strided views, saturated gates, a NaN and an Inf
row, the need_* flags, and the argument checks.  Every case prints its worst error / bar ratio per tensor (DESIGN.md 4.20 quotes them)."""
import ctypes

import pytest
import torch

import gru_cases as C
from pna_amd import _lib
from pna_amd import functional as PF

pytestmark = pytest.mark.gpu
GRADS = ("x", "h") + C.PARAMS
SENTINEL = -7.25


def _args(d):
    """d: device tensors x, h, w_ih, w_hh (b_ih, b_hh, out, saved, go, grad buffers as present)."""
    a = _lib.PnaGruCellArgs()
    a.V, a.I, a.Hc, a.input_size, a.hidden_size = d["x"].shape[0], d["x"].shape[1], d["h"].shape[1], d["w_ih"].shape[1], d["w_hh"].shape[1]
    a.dtype = _lib.PNA_GRU_F32
    a.x, a.ldx, a.h, a.ldh = d["x"].data_ptr(), d["x"].stride(0), d["h"].data_ptr(), d["h"].stride(0)
    a.w_ih, a.ld_wih, a.w_hh, a.ld_whh = d["w_ih"].data_ptr(), d["w_ih"].stride(0), d["w_hh"].data_ptr(), d["w_hh"].stride(0)
    a.b_ih, a.b_hh = d["b_ih"].data_ptr(), d["b_hh"].data_ptr()
    return a


def _fwd(d, save=True):
    dev, V, H = d["x"].device, d["x"].shape[0], d["w_hh"].shape[1]
    out = torch.full((V, H), float("nan"), device=dev)
    saved = torch.full((4, V, H), float("nan"), device=dev) if save else None
    a = _args(d)
    a.out, a.ld_out = out.data_ptr(), out.stride(0)
    a.saved = saved.data_ptr() if save else None
    _lib.check(_lib.lib().pna_gru_cell_fwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_gru_cell_fwd_f32")
    return out, saved


def _bwd(d, saved, go, need=(1,) * 6, fill=float("nan")):
    dev, V, H = go.device, d["x"].shape[0], d["w_hh"].shape[1]
    I, Hc, IN = d["x"].shape[1], d["h"].shape[1], d["w_ih"].shape[1]
    nbytes = PF.gru_cell_workspace_bytes(V, I, Hc, H)
    assert nbytes > 0
    ws = torch.full((nbytes // 4 + 4,), float("nan"), device=dev)
    g = {"x": torch.full((V, I), fill, device=dev), "h": torch.full((V, Hc), fill, device=dev),
         "w_ih": torch.full((3 * H, IN), fill, device=dev), "w_hh": torch.full((3 * H, H), fill, device=dev),
         "b_ih": torch.full((3 * H,), fill, device=dev), "b_hh": torch.full((3 * H,), fill, device=dev)}
    a = _args(d)
    a.saved, a.grad_out, a.ld_go = saved.data_ptr(), go.data_ptr(), go.stride(0)
    a.grad_x, a.ld_gx, a.grad_h, a.ld_gh = g["x"].data_ptr(), g["x"].stride(0), g["h"].data_ptr(), g["h"].stride(0)
    a.grad_w_ih, a.grad_w_hh, a.grad_b_ih, a.grad_b_hh = g["w_ih"].data_ptr(), g["w_hh"].data_ptr(), g["b_ih"].data_ptr(), g["b_hh"].data_ptr()
    a.need_x, a.need_h, a.need_w_ih, a.need_w_hh, a.need_b_ih, a.need_b_hh = need
    a.workspace, a.workspace_bytes = ws.data_ptr() + (-ws.data_ptr()) % 16, nbytes
    _lib.check(_lib.lib().pna_gru_cell_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_gru_cell_bwd_f32")
    return g


def _dev(c, dev):
    return {k: v.to(dev) for k, v in c.items()}


def _check(c, dev, tag, repeats=20, grads=GRADS):
    """The whole check of one case; returns (out, saved, gradients) on the device."""
    d = _dev(c, dev)
    f, g64 = C.gru_grad_ref64(*C.case_params(c), c["go"])
    bars = C.gru_bars(*C.case_params(c), c["go"])
    out, saved = _fwd(d)
    got = {"out": out, "r": saved[0], "z": saved[1], "n": saved[2], "gh_n": saved[3]}
    worst = {k: C.worst_ratio(v.cpu(), f[k], bars[k]) for k, v in got.items()}
    g = _bwd(d, saved, d["go"])
    for k in grads:
        worst[k] = C.worst_ratio(g[k].cpu(), g64[k], bars[k])
    print("GRU_RATIO", tag, " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    for _ in range(repeats - 1):
        out2, saved2 = _fwd(d)
        g2 = _bwd(d, saved2, d["go"])
        assert torch.equal(out, out2) and torch.equal(saved, saved2) and all(torch.equal(g[k], g2[k]) for k in g)
    return d, out, saved, g


@pytest.mark.parametrize("width,V", C.KERNEL_CASES, ids=[f"{w}-{v}" for w, v in C.KERNEL_CASES])
def test_case_against_float64_within_the_derived_bars(cuda_device, width, V):
    _check(C.gru_case(width, V), cuda_device, f"{width}-{V}")


def test_forward_without_a_saved_state_gives_the_same_bits(cuda_device):
    d = _dev(C.gru_case("h75", 33), cuda_device)
    assert torch.equal(_fwd(d, save=False)[0], _fwd(d)[0])


def test_row_strided_views_give_the_bits_of_the_contiguous_call(cuda_device):
    c = C.gru_case("pad_x", 3 * C.SLAB + 17)
    d = _dev(c, cuda_device)
    out, saved = _fwd(d)
    g = _bwd(d, saved, d["go"])
    wide = {}
    for k, lead, tail in (("x", 3, 5), ("h", 0, 7), ("go", 2, 1)):
        buf = torch.full((c[k].shape[0], lead + c[k].shape[1] + tail), float("nan"), device=cuda_device)
        buf[:, lead:lead + c[k].shape[1]] = d[k]
        wide[k] = buf[:, lead:lead + c[k].shape[1]]
        assert wide[k].stride(0) > wide[k].shape[1] and wide[k].stride(1) == 1
    dv = dict(d, x=wide["x"], h=wide["h"])
    out_v, saved_v = _fwd(dv)
    g_v = _bwd(dv, saved_v, wide["go"])
    assert torch.equal(out, out_v) and torch.equal(saved, saved_v) and all(torch.equal(g[k], g_v[k]) for k in g)


@pytest.mark.parametrize("scale", [30.0, 100.0])
@pytest.mark.parametrize("width,V", [("mt_later", 33), ("h75", C.SLAB + 1)])
def test_saturated_gates_are_exact_and_finite(cuda_device, width, V, scale):
    c = C.gru_case(width, V, scale=scale)
    d, out, saved, g = _check(c, cuda_device, f"{width}-{V}-scale{scale:g}", repeats=2)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(saved).all()) and all(bool(torch.isfinite(t).all()) for t in g.values())
    f = C.gru_ref64(*C.case_params(c))
    n_exact = 0
    for i, k in enumerate(("r", "z", "n")):
        want = f[k].float()                                                      # float64 rounded to fp32
        sat = (want == 0) | (want.abs() == 1)
        n_exact += int(sat.sum())
        assert torch.equal(saved[i].cpu()[sat], want[sat]), k
    assert n_exact >= 50                                                          # the case does saturate (the largest |pre-activation| is `scale`; most are smaller)


def test_a_nan_row_and_an_inf_row_stay_in_their_rows(cuda_device):
    c = C.gru_case("mt_later", 33)
    c["x"][5, 3] = float("nan")
    c["x"][20] = float("inf")                                                    # a whole row: inf - inf in every projection
    bad = torch.zeros(33, dtype=torch.bool)
    bad[5] = bad[20] = True
    d = _dev(c, cuda_device)
    out, saved = _fwd(d)
    g = _bwd(d, saved, d["go"])
    clean = {k: (v[~bad] if k in ("x", "h", "go") else v) for k, v in c.items()}
    f, g64 = C.gru_grad_ref64(*C.case_params(clean), clean["go"])
    bars = C.gru_bars(*C.case_params(clean), clean["go"])
    for got, ref, bar in ((out, f["out"], bars["out"]), (g["x"], g64["x"], bars["x"]), (g["h"], g64["h"], bars["h"])):
        got = got.cpu()
        assert not bool(torch.isfinite(got[bad]).any())                           # non-finite in those rows ...
        assert bool(torch.isfinite(got[~bad]).all())                              # ... only
        assert C.worst_ratio(got[~bad], ref, bar) <= 1.0                          # a row's result depends on that row alone
    full = C.gru_ref64(*C.case_params(c))
    assert not bool(torch.isfinite(full["out"][bad]).any())                       # (float64 agrees that the whole rows are lost)


def test_a_gradient_not_asked_for_is_not_written(cuda_device):
    c = C.gru_case("pad_h", C.SLAB + 1)
    d = _dev(c, cuda_device)
    out, saved = _fwd(d)
    full = _bwd(d, saved, d["go"])
    for off in range(6):
        need = tuple(0 if i == off else 1 for i in range(6))
        g = _bwd(d, saved, d["go"], need=need, fill=SENTINEL)
        for i, k in enumerate(GRADS):
            if i == off:
                assert bool((g[k] == SENTINEL).all()), k
            else:
                assert torch.equal(g[k], full[k]), (GRADS[off], k)
    only_x = _bwd(d, saved, d["go"], need=(1, 0, 0, 0, 0, 0), fill=SENTINEL)
    assert torch.equal(only_x["x"], full["x"]) and all(bool((only_x[k] == SENTINEL).all()) for k in GRADS[1:])
    none = _bwd(d, saved, d["go"], need=(0,) * 6, fill=SENTINEL)
    assert all(bool((none[k] == SENTINEL).all()) for k in GRADS)


def test_calls_refuse_what_is_outside_the_scope_and_launch_nothing(cuda_device):
    L = _lib.lib()
    c = C.gru_case("mt_later", 17)
    d = _dev(c, cuda_device)
    good_out, saved = _fwd(d)
    stream = _lib.stream_ptr(cuda_device)

    def fwd_args():
        out = torch.full((17, 16), SENTINEL, device=cuda_device)
        a = _args(d)
        a.out, a.ld_out = out.data_ptr(), out.stride(0)
        return a, out

    def bwd_args():
        g = {"x": torch.full((17, 16), SENTINEL, device=cuda_device), "h": torch.full((17, 16), SENTINEL, device=cuda_device),
             "w_ih": torch.full((48, 16), SENTINEL, device=cuda_device), "w_hh": torch.full((48, 16), SENTINEL, device=cuda_device),
             "b_ih": torch.full((48,), SENTINEL, device=cuda_device), "b_hh": torch.full((48,), SENTINEL, device=cuda_device)}
        nbytes = PF.gru_cell_workspace_bytes(17, 16, 16, 16)
        ws = torch.empty(nbytes // 4 + 4, device=cuda_device)
        a = _args(d)
        a.saved, a.grad_out, a.ld_go = saved.data_ptr(), d["go"].data_ptr(), d["go"].stride(0)
        a.grad_x, a.ld_gx, a.grad_h, a.ld_gh = g["x"].data_ptr(), 16, g["h"].data_ptr(), 16
        a.grad_w_ih, a.grad_w_hh, a.grad_b_ih, a.grad_b_hh = g["w_ih"].data_ptr(), g["w_hh"].data_ptr(), g["b_ih"].data_ptr(), g["b_hh"].data_ptr()
        a.need_x = a.need_h = a.need_w_ih = a.need_w_hh = a.need_b_ih = a.need_b_hh = 1
        a.workspace, a.workspace_bytes = ws.data_ptr() + (-ws.data_ptr()) % 16, nbytes
        return a, g, ws

    fwd_bad = [({"dtype": 1}, b"fp32 only"), ({"input_size": 129}, b"input_size"), ({"input_size": 0}, b"input_size"),
               ({"hidden_size": 129}, b"hidden_size"), ({"hidden_size": 1}, b"hidden_size"), ({"V": 1}, b"V >= 2"),
               ({"I": 0}, b"I <= input_size"), ({"I": 17}, b"I <= input_size"), ({"Hc": 0}, b"Hc <= hidden_size"), ({"Hc": 17}, b"Hc <= hidden_size"),
               ({"x": None}, b"needs x"), ({"ldx": 15}, b"needs x"), ({"h": None}, b"needs h"), ({"ldh": 15}, b"needs h"),
               ({"w_ih": None}, b"w_ih"), ({"ld_wih": 15}, b"w_ih"), ({"w_hh": None}, b"w_hh"), ({"ld_whh": 15}, b"w_hh"),
               ({"b_ih": None}, b"b_ih"), ({"b_hh": None}, b"b_hh"), ({"out": None}, b"needs out"), ({"ld_out": 15}, b"needs out"),
               ({"struct_size": ctypes.sizeof(_lib.PnaGruCellArgs) - 8}, b"struct_size")]
    for kw, clause in fwd_bad:
        a, out = fwd_args()
        for k, v in kw.items():
            setattr(a, k, v)
        assert L.pna_gru_cell_fwd_f32(ctypes.byref(a), stream) == -1, kw
        assert clause in L.pna_last_error(), (kw, L.pna_last_error())
        assert bool((out == SENTINEL).all()), kw                                  # nothing was launched
    bwd_bad = [({"saved": None}, b"saved"), ({"grad_out": None}, b"grad_out"), ({"ld_go": 15}, b"grad_out"), ({"grad_x": None}, b"grad_x"),
               ({"ld_gx": 15}, b"grad_x"), ({"grad_h": None}, b"grad_h"), ({"ld_gh": 15}, b"grad_h"), ({"grad_w_ih": None}, b"gradient buffer"),
               ({"grad_b_hh": None}, b"gradient buffer"), ({"workspace": None}, b"workspace"), ({"workspace_bytes": 64}, b"workspace"),
               ({"V": 1}, b"V >= 2"), ({"dtype": 1}, b"fp32 only"), ({"struct_size": 8}, b"struct_size")]
    for kw, clause in bwd_bad:
        a, g, ws = bwd_args()
        for k, v in kw.items():
            setattr(a, k, v)
        assert L.pna_gru_cell_bwd_f32(ctypes.byref(a), stream) == -1, kw
        assert clause in L.pna_last_error(), (kw, L.pna_last_error())
        assert all(bool((t == SENTINEL).all()) for t in g.values()), kw
    a, g, ws = bwd_args()
    a.workspace = a.workspace + 4                                                 # misaligned
    assert L.pna_gru_cell_bwd_f32(ctypes.byref(a), stream) == -1 and b"aligned" in L.pna_last_error()
    a, out = fwd_args()                                                           # and the same struct inside the scope runs
    assert L.pna_gru_cell_fwd_f32(ctypes.byref(a), stream) == 0 and torch.equal(out, good_out)
