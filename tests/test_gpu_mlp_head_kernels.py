"""pna_mlp_head_fwd_f32 / pna_mlp_head_bwd_f32 through ctypes (pna_mlp_head.hip), every output buffer and the workspace filled with NaN
before every call.  Each random case: y and all gradients against float64 within the bars of tests/mlp_head_cases.py (no element
excluded) and three repeats with identical bits; the exact cases bit for bit, the derivative at a pre-activation of 0 included.  Then:
forward bits with and without a backward, row-strided views, a 2 V-row call against its halves, a NaN and an Inf row, the need_* flags,
and the argument checks.  Every case prints its worst error / bar ratio per tensor (DESIGN.md 4.25 quotes them)."""
import ctypes

import pytest
import torch

import mlp_head_cases as C
from pna_amd import _lib
from pna_amd import functional as PF

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
NAN = float("nan")


def _dev(c, dev):
    """The case's tensors on the device; x as a view of wider rows where the case asks for it."""
    x = c["x"].to(dev)
    if c["x_pad"] is not None:
        x = C.strided(x, *c["x_pad"])
        assert x.stride(0) > x.shape[1] and x.stride(1) == 1
    return {"x": x, "ws": [w.to(dev) for w in c["ws"]], "bs": [None if b is None else b.to(dev) for b in c["bs"]], "go": c["go"].to(dev),
            "acts": c["acts"]}


def _args(d):
    a = _lib.PnaMlpHeadArgs()
    a.V, a.n_layers = d["x"].shape[0], len(d["ws"])
    a.widths[0] = d["x"].shape[1]
    a.x, a.ldx = d["x"].data_ptr(), d["x"].stride(0)
    for l, (w, b, act) in enumerate(zip(d["ws"], d["bs"], d["acts"])):
        a.widths[l + 1] = w.shape[0]
        a.act[l], a.slope[l] = C.act_code(act)
        a.w[l], a.ldw[l] = w.data_ptr(), w.stride(0)
        a.b[l] = None if b is None else b.data_ptr()
    return a


def _fwd(d):
    dev = d["x"].device
    y = torch.full((d["x"].shape[0], d["ws"][-1].shape[0]), NAN, device=dev)
    a = _args(d)
    a.y, a.ldy = y.data_ptr(), y.stride(0)
    _lib.check(_lib.lib().pna_mlp_head_fwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_mlp_head_fwd_f32")
    return y


def _names(d):
    L = len(d["ws"])
    return ["x"] + [f"w{l}" for l in range(L)] + [f"b{l}" for l in range(L) if d["bs"][l] is not None]


def _bwd(d, go=None, need=None, fill=NAN):
    """-> {name: gradient buffer}; need: names wanted (default all)."""
    dev, V, L = d["x"].device, d["x"].shape[0], len(d["ws"])
    go = d["go"] if go is None else go
    names = _names(d)
    need = names if need is None else need
    widths = [d["x"].shape[1]] + [w.shape[0] for w in d["ws"]]
    nbytes = PF.mlp_head_workspace_bytes(V, widths)
    assert nbytes > 0
    ws = torch.full((nbytes // 4 + 4,), NAN, device=dev)
    g = {"x": torch.full((V, widths[0]), fill, device=dev)}
    for l in range(L):
        g[f"w{l}"] = torch.full(tuple(d["ws"][l].shape), fill, device=dev)
        if d["bs"][l] is not None:
            g[f"b{l}"] = torch.full((widths[l + 1],), fill, device=dev)
    a = _args(d)
    a.grad_out, a.ld_go = go.data_ptr(), go.stride(0)
    a.grad_x, a.ld_gx, a.need_x = g["x"].data_ptr(), g["x"].stride(0), int("x" in need)
    for l in range(L):
        a.grad_w[l], a.need_w[l] = g[f"w{l}"].data_ptr(), int(f"w{l}" in need)
        if f"b{l}" in g:
            a.grad_b[l], a.need_b[l] = g[f"b{l}"].data_ptr(), int(f"b{l}" in need)
    a.workspace, a.workspace_bytes = ws.data_ptr() + (-ws.data_ptr()) % 16, nbytes
    _lib.check(_lib.lib().pna_mlp_head_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_mlp_head_bwd_f32")
    return g


@pytest.mark.parametrize("name", C.NAMES)
def test_case_against_float64_within_the_bars(cuda_device, name):
    c = C.mlp_case(name)
    d = _dev(c, cuda_device)
    y = _fwd(d)
    g = _bwd(d)
    got = dict(g, y=y)
    worst = {k: C.worst_ratio(got[k].cpu(), c["ref"][k], c["bars"][k]) for k in C.tensors_of(c)}
    print("MLP_RATIO", name, " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    assert sorted(got) == sorted(C.tensors_of(c))
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    assert all(v <= 1.0 for v in worst.values()), worst
    for _ in range(2):                                                            # three runs, identical bits
        y2, g2 = _fwd(d), _bwd(d)
        assert torch.equal(y, y2) and all(torch.equal(g[k], g2[k]) for k in g)


@pytest.mark.parametrize("name", C.EXACT_NAMES)
def test_exact_case_bit_for_bit(cuda_device, name):
    c = C.exact_case(name)
    d = _dev(c, cuda_device)
    got = dict(_bwd(d), y=_fwd(d))
    for k in C.tensors_of(c):
        assert torch.equal(got[k].cpu().double(), c["ref"][k]), (name, k, float((got[k].cpu().double() - c["ref"][k]).abs().max()))


def test_forward_bits_do_not_depend_on_a_following_backward(cuda_device):
    d = _dev(C.mlp_case("cls10"), cuda_device)
    alone = _fwd(d)
    before = _fwd(d)
    _bwd(d)
    assert torch.equal(alone, before) and torch.equal(alone, _fwd(d))


def test_row_strided_views_give_the_bits_of_the_contiguous_call(cuda_device):
    c = C.mlp_case("w127")
    d = _dev(c, cuda_device)
    y, g = _fwd(d), _bwd(d)
    dv = dict(d, x=C.strided(d["x"], 3, 5), ws=[C.strided(w, 1, 2) for w in d["ws"]])
    go = C.strided(d["go"], 2, 1)
    assert dv["x"].stride(0) > dv["x"].shape[1] and go.stride(0) > go.shape[1] and dv["ws"][0].stride(0) > dv["ws"][0].shape[1]
    y_v, g_v = _fwd(dv), _bwd(dv, go=go)
    assert torch.equal(y, y_v) and all(torch.equal(g[k], g_v[k]) for k in g)
    # the strided case itself against its contiguous copy
    c = C.mlp_case("strided")
    d = _dev(c, cuda_device)
    dc = dict(d, x=d["x"].contiguous())
    assert torch.equal(_fwd(d), _fwd(dc)) and all(torch.equal(a, b) for a, b in zip(_bwd(d).values(), _bwd(dc).values()))


def test_a_call_on_2v_rows_gives_the_bits_of_its_two_halves(cuda_device):
    c = C.mlp_case("zinc")
    d = _dev(c, cuda_device)
    V = c["x"].shape[0]
    both = dict(d, x=torch.cat([d["x"], d["x"].flip(0)]), go=torch.cat([d["go"], d["go"].flip(0)]))
    second = dict(d, x=d["x"].flip(0).contiguous(), go=d["go"].flip(0).contiguous())
    y, gx = _fwd(both), _bwd(both, need=["x"])["x"]
    assert torch.equal(y[:V], _fwd(d)) and torch.equal(y[V:], _fwd(second))
    assert torch.equal(gx[:V], _bwd(d, need=["x"])["x"]) and torch.equal(gx[V:], _bwd(second, need=["x"])["x"])


def test_a_nan_row_and_an_inf_row_stay_in_their_rows(cuda_device):
    c = C.mlp_case("mt")
    x = c["x"].clone()
    x[5, 3] = NAN
    x[20] = float("inf")                                                         # a whole row: inf - inf in the first layer
    bad = torch.zeros(x.shape[0], dtype=torch.bool)
    bad[5] = bad[20] = True
    d = _dev(dict(c, x=x), cuda_device)
    y, gx = _fwd(d).cpu(), _bwd(d, need=["x"])["x"].cpu()
    assert not bool(torch.isfinite(y[bad]).any())                                # y: non-finite in those rows ...
    for got, k in ((y, "y"), (gx, "x")):
        assert bool(torch.isfinite(got[~bad]).all())                              # ... only
        assert C.worst_ratio(got[~bad], c["ref"][k][~bad], c["bars"][k]) <= 1.0   # a row's result depends on that row alone
    # (grad_x of the two rows is what torch's derivative selects give at a NaN pre-activation: the slope's branch, a finite number)
    want = C.mlp_grad_ref(x, c["ws"], c["bs"], c["acts"], c["go"])["x"]
    assert torch.equal(torch.isfinite(gx[bad]), torch.isfinite(want[bad]))


def test_a_gradient_not_asked_for_is_not_written(cuda_device):
    c = C.mlp_case("ragged")
    d = _dev(c, cuda_device)
    names = _names(d)
    full = _bwd(d)
    for off in names:
        g = _bwd(d, need=[n for n in names if n != off], fill=SENTINEL)
        for k in names:
            if k == off:
                assert bool((g[k] == SENTINEL).all()), k
            else:
                assert torch.equal(g[k], full[k]), (off, k)
    only_x = _bwd(d, need=["x"], fill=SENTINEL)
    assert torch.equal(only_x["x"], full["x"]) and all(bool((only_x[k] == SENTINEL).all()) for k in names[1:])
    only_b = _bwd(d, need=["b1"], fill=SENTINEL)
    assert torch.equal(only_b["b1"], full["b1"]) and all(bool((only_b[k] == SENTINEL).all()) for k in names if k != "b1")
    none = _bwd(d, need=[], fill=SENTINEL)
    assert all(bool((none[k] == SENTINEL).all()) for k in names)


def test_calls_refuse_what_is_outside_the_scope_and_launch_nothing(cuda_device):
    L = _lib.lib()
    c = C.mlp_case("ragged")                                                      # 17 rows, 5-3-2
    d = _dev(c, cuda_device)
    good = _fwd(d)
    stream = _lib.stream_ptr(cuda_device)

    def put(a, kw):
        for k, v in kw.items():
            if isinstance(k, tuple):
                getattr(a, k[0])[k[1]] = v
            else:
                setattr(a, k, v)

    def fwd_args():
        y = torch.full((17, 2), SENTINEL, device=cuda_device)
        a = _args(d)
        a.y, a.ldy = y.data_ptr(), y.stride(0)
        return a, y

    for kw, clause in [({"n_layers": 0}, b"n_layers"), ({"n_layers": 5}, b"n_layers"), ({("widths", 1): 129}, b"every width"),
                       ({("widths", 0): 0}, b"every width"), ({"V": 0}, b"V >= 1"), ({("act", 0): 7}, b"every act"), ({"x": None}, b"needs x"),
                       ({"ldx": 4}, b"needs x"), ({("w", 0): None}, b"every w"), ({("ldw", 1): 2}, b"every w"), ({"y": None}, b"needs y"),
                       ({"ldy": 1}, b"needs y"), ({"struct_size": ctypes.sizeof(_lib.PnaMlpHeadArgs) - 8}, b"struct_size")]:
        a, y = fwd_args()
        put(a, kw)
        assert L.pna_mlp_head_fwd_f32(ctypes.byref(a), stream) == -1, kw
        assert clause in L.pna_last_error(), (kw, L.pna_last_error())
        assert bool((y == SENTINEL).all()), kw                                    # nothing was launched

    def bwd_args():
        g = {"x": torch.full((17, 5), SENTINEL, device=cuda_device), "w0": torch.full((3, 5), SENTINEL, device=cuda_device),
             "w1": torch.full((2, 3), SENTINEL, device=cuda_device), "b1": torch.full((2,), SENTINEL, device=cuda_device)}
        nbytes = PF.mlp_head_workspace_bytes(17, [5, 3, 2])
        ws = torch.empty(nbytes // 4 + 4, device=cuda_device)
        a = _args(d)
        a.grad_out, a.ld_go = d["go"].data_ptr(), d["go"].stride(0)
        a.grad_x, a.ld_gx, a.need_x = g["x"].data_ptr(), 5, 1
        a.grad_w[0], a.grad_w[1], a.grad_b[1] = g["w0"].data_ptr(), g["w1"].data_ptr(), g["b1"].data_ptr()
        a.need_w[0] = a.need_w[1] = a.need_b[1] = 1
        a.workspace, a.workspace_bytes = ws.data_ptr() + (-ws.data_ptr()) % 16, nbytes
        return a, g, ws

    for kw, clause in [({"grad_out": None}, b"grad_out"), ({"ld_go": 1}, b"grad_out"), ({"grad_x": None}, b"grad_x"), ({"ld_gx": 4}, b"grad_x"),
                       ({("grad_w", 1): None}, b"gradient buffer"), ({("grad_b", 1): None}, b"gradient buffer"), ({("need_b", 0): 1}, b"gradient buffer"),
                       ({"workspace": None}, b"workspace"), ({"workspace_bytes": 64}, b"workspace"), ({"V": 0}, b"V >= 1"),
                       ({("widths", 2): 129}, b"every width"), ({"struct_size": 8}, b"struct_size")]:
        a, g, ws = bwd_args()
        put(a, kw)
        assert L.pna_mlp_head_bwd_f32(ctypes.byref(a), stream) == -1, kw
        assert clause in L.pna_last_error(), (kw, L.pna_last_error())
        assert all(bool((t == SENTINEL).all()) for t in g.values()), kw
    a, g, ws = bwd_args()
    a.workspace = a.workspace + 4                                                 # misaligned
    assert L.pna_mlp_head_bwd_f32(ctypes.byref(a), stream) == -1 and b"aligned" in L.pna_last_error()
    a, y = fwd_args()                                                             # and the same struct inside the scope runs
    assert L.pna_mlp_head_fwd_f32(ctypes.byref(a), stream) == 0 and torch.equal(y, good)
    a, g, ws = bwd_args()
    full = _bwd(d)
    assert L.pna_mlp_head_bwd_f32(ctypes.byref(a), stream) == 0 and all(torch.equal(g[k], full[k]) for k in g)
