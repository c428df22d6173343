"""Host side of the BatchNorm tail's kernel tests (no GPU): the float64 reference of tests/bn_tail_cases.py against float64
nn.BatchNorm1d under autograd; the bars -- attainable (fp32 torch on the CPU meets every one at half its size) and biting (seven planted
errors each exceed one twofold); the ReLU kink margin of every random case; the exact cases' representability; the summation of
pna_bn_tail.hip emulated in numpy fp32, with the column-wide shift y[0, c] it used before and with the per-thread median it uses now; and
autograd.bn_tail_applies clause by clause.  (The struct's layout is pinned field by field by tests/test_abi_layout.py.)"""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_tail_cases as C
from pna_amd import autograd as AG


def _any_case(name):
    return C.case(name) if name in C.CASES else C.exact_case(name)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES + C.EXACT_NAMES)
def test_float64_closed_form_is_float64_batchnorm1d_under_autograd(name):
    c = _any_case(name)
    N, ref = c["N"], c["ref"]
    m = float(torch.tensor(c["momentum"], dtype=torch.float32))
    bn = nn.BatchNorm1d(N, eps=float(torch.tensor(c["eps"], dtype=torch.float32)), momentum=max(m, 0.0)).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.ones(N) if c["gamma"] is None else c["gamma"].double())
        bn.bias.copy_(torch.zeros(N) if c["beta"] is None else c["beta"].double())
        if c["rm0"] is not None:
            bn.running_mean.copy_(c["rm0"].double())
            bn.running_var.copy_(c["rv0"].double())
    y = c["y"].double().requires_grad_(True)
    z = bn(y)
    out = (F.relu(z) if c["relu"] else z) + (0 if c["residual"] is None else c["residual"].double())
    out.backward(c["go"].double())
    # (two float64 evaluations differ by the rounding of the mean, 2^-53 |mean|, in units of the spread: 1e-11 for mean 1000, sigma 0.01)
    close = dict(rtol=1e-11, atol=1e-13 * (1 + float((ref["save_mean"].abs() * ref["save_invstd"]).max())))
    torch.testing.assert_close(ref["out"], out.detach(), **close)
    torch.testing.assert_close(ref["z"], z.detach(), **close)
    torch.testing.assert_close(ref["save_mean"], c["y"].double().mean(0), **close)
    torch.testing.assert_close(ref["save_invstd"], 1 / torch.sqrt(c["y"].double().var(0, unbiased=False) + bn.eps), **close)
    # grad_y of two rows is a difference of nearly equal terms times 1 / std: compare at the size of the terms
    scale = float((bn.weight.detach().abs() * ref["save_invstd"]).max()) * max(1.0, float(c["go"].abs().max()))
    assert float((ref["grad_y"] - y.grad).abs().max()) <= 1e-11 * scale
    torch.testing.assert_close(ref["grad_gamma"], bn.weight.grad, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(ref["grad_beta"], bn.bias.grad, rtol=1e-10, atol=1e-9)
    if c["rm0"] is None:
        assert ref["running_mean"] is None and ref["running_var"] is None
    elif m < 0:
        assert torch.equal(ref["running_mean"], c["rm0"].double()) and torch.equal(ref["running_var"], c["rv0"].double())
    else:
        torch.testing.assert_close(ref["running_mean"], bn.running_mean, **close)
        torch.testing.assert_close(ref["running_var"], bn.running_var, **close)


def test_the_case_list_is_the_one_the_kernel_needs():
    rows = sorted(s["M"] for n, s in C.CASES.items() if n.startswith("m") and n[1:].isdigit())
    assert rows == [2, 3, 7, 8, 9, 511, 512, 513, 1024, 1025] and all(C.CASES[f"m{M}"]["N"] == 33 for M in rows)
    widths = sorted(s["N"] for n, s in C.CASES.items() if n.startswith("n") and n[1:].isdigit())
    assert widths == [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128] and all(C.CASES[f"n{N}"]["M"] == 521 for N in widths)
    # 257 and 514 workgroups: k_bn_finalize's 256 threads stride over them, thread 0 twice and three times
    assert (C.CASES["wg257"]["M"], C.CASES["wg513"]["M"]) == (131073, 262657)
    assert -(-C.CASES["wg257"]["M"] // C.WG_ROWS) == 257 and -(-C.CASES["wg513"]["M"] // C.WG_ROWS) == 514
    for name in ("pitched", "stats_b"):
        p, N = C.CASES[name]["pitches"], C.CASES[name]["N"]
        assert len(set(p)) == 5 and min(p) > N and any(v % 2 for v in p)
    assert sorted(C.CASES[n]["momentum"] for n in ("mom_neg", "mom0", "m8", "mom1")) == [-1.0, 0.0, 0.1, 1.0]
    for name in C.STATS_NAMES:
        c = C.case(name)
        assert (c["M"], c["N"]) == (4101, 33) and set(c["kinds"]) == set(C.KINDS)


# ---- the bars --------------------------------------------------------------------------------------------------------------------------
def _leaves(c):
    N = c["N"]
    y = c["y"].clone().requires_grad_(True)
    w = (torch.ones(N) if c["gamma"] is None else c["gamma"].clone()).requires_grad_(True)
    b = (torch.zeros(N) if c["beta"] is None else c["beta"].clone()).requires_grad_(True)
    return y, w, b


def _finish32(c, z, mean, invstd, y, w, b, running):
    out = F.relu(z) if c["relu"] else z
    out = out if c["residual"] is None else c["residual"] + out
    out.backward(c["go"])
    got = {"save_mean": mean.detach(), "save_invstd": invstd.detach(), "out": out.detach(), "grad_y": y.grad, "grad_gamma": w.grad, "grad_beta": b.grad}
    if c["rm0"] is not None:
        got["running_mean"], got["running_var"] = running
    return got


def _torch32(c):
    """fp32 torch on the CPU, the operation written with its tensor functions: torch.var_mean for the statistics, the centred affine
    form, relu, the add, torch.lerp for the running pair, and autograd for every gradient."""
    M = c["M"]
    y, w, b = _leaves(c)
    var, mean = torch.var_mean(y, 0, unbiased=False)
    invstd = torch.rsqrt(var + c["eps"])
    z = (y - mean) * (w * invstd) + b
    running = (c["rm0"], c["rv0"])
    if c["rm0"] is not None and c["momentum"] >= 0:
        running = (torch.lerp(c["rm0"], mean.detach(), c["momentum"]), torch.lerp(c["rv0"], var.detach() * (M / (M - 1)), c["momentum"]))
    return _finish32(c, z, mean, invstd, y, w, b, running)


def _batch_norm32(c):
    """fp32 F.batch_norm in training mode on the CPU (torch.native_batch_norm is the same kernel and also returns the saved statistics),
    relu, the add, autograd."""
    y, w, b = _leaves(c)
    keeps = c["rm0"] is not None and c["momentum"] >= 0
    rm, rv = (c["rm0"].clone(), c["rv0"].clone()) if keeps else (None, None)
    z, mean, invstd = torch.native_batch_norm(y, w, b, rm, rv, True, c["momentum"], c["eps"])
    z2 = F.batch_norm(c["y"], None if rm is None else c["rm0"].clone(), None if rv is None else c["rv0"].clone(), w.detach(), b.detach(), True,
                      max(c["momentum"], 0.0), c["eps"])
    assert torch.equal(z.detach(), z2)
    return _finish32(c, z, mean, invstd, y, w, b, (rm, rv) if keeps else (c["rm0"], c["rv0"]))


# Where F.batch_norm's CPU kernel itself is less accurate than the component bars (its column mean is a plain fp32 sum, and its variance
# is taken about that mean), measured worst ratios -- the cases are kept, the bars are the project's, and _torch32 meets them:
#   m3       running_var 0.74: three fp32 roundings of a value near 1 against the 2^-23 the bar gives the result (within the bar, above half)
#   wg257    save_mean 0.76, running_mean 0.70 (131073 rows);   wg513  save_mean 2.5, running_mean 2.3, out 1.02 (262657 rows)
#   stats_a  save_invstd 9.7, save_mean 1.2, grad_y 1.3;   stats_b  save_invstd 10.2, save_mean 2.2, running_mean 1.2: the columns of
#            mean 1000, sigma 0.01, whose fp32 mean is off by 1.5e-4 = 0.015 sigma, and the row-0 columns of sigma 0.01
BATCH_NORM32_MISSES = ("m3", "wg257", "wg513", "stats_a", "stats_b")


@pytest.mark.parametrize("name", C.NAMES)
def test_the_bars_are_attainable_fp32_torch_meets_each_at_half(name):
    c = C.case(name)
    got = _torch32(c)
    worst = {k: C.worst_ratio(got[k], c["ref"][k], c["bars"][k]) for k in C.tensors_of(c)}
    assert sorted(got) == sorted(set(C.tensors_of(c)) | {"grad_gamma", "grad_beta"})
    assert all(v <= 0.5 for v in worst.values()), worst
    for k in C.tensors_of(c):                                                  # and every bar is a finite number, none negative
        assert bool((c["bars"][k] >= 0).all()) and bool(torch.isfinite(c["bars"][k]).all()), k


@pytest.mark.parametrize("name", [n for n in C.NAMES if n not in BATCH_NORM32_MISSES])
def test_fp32_batch_norm_of_torch_meets_each_bar_at_half(name):
    c = C.case(name)
    got = _batch_norm32(c)
    worst = {k: C.worst_ratio(got[k], c["ref"][k], c["bars"][k]) for k in C.tensors_of(c)}
    assert all(v <= 0.5 for v in worst.values()), worst


BITE_CASES = ["m2", "m3", "m7", "m9", "n33", "n65", "norelu", "nores"]


@pytest.mark.parametrize("plant", C.PLANTS)
def test_the_bars_bite_a_planted_error_exceeds_one_twofold(plant):
    hits = {}
    for name in BITE_CASES:
        c = C.case(name)
        bad = C.planted(c, plant)
        worst = max(C.worst_ratio(bad[k], c["ref"][k], c["bars"][k]) for k in C.tensors_of(c))
        if worst >= 2.0:
            hits[name] = worst
    assert hits, plant
    if plant != "flip_mask":                                                   # (norelu has no mask to flip)
        assert "m3" in hits or "n33" in hits, (plant, hits)


@pytest.mark.parametrize("name", C.NAMES)
def test_no_element_sits_on_the_relu_kink(name):
    c = C.case(name)
    assert C.kink_margin(c) >= 1.0
    assert c["kink_rounds"] <= C.MAX_ROUNDS
    for k, kind in enumerate(c["kinds"]):                                      # the moves left the statistics cases what they are
        col = c["y"][:, k].double()
        if kind == "const":
            assert bool((col == col[0]).all())
            assert float(c["ref"]["save_invstd"][k]) == pytest.approx(1 / math.sqrt(float(torch.tensor(c["eps"], dtype=torch.float32))), rel=1e-15)
            assert bool((c["ref"]["z"][:, k] == c["beta"][k].double()).all())
        elif kind in C.ROW0_KINDS:
            rest = col[8:512]
            assert float((col[0] - rest.mean()).abs()) > 90 * float(rest.std())


@pytest.mark.parametrize("name", C.EXACT_NAMES)
def test_exact_cases_are_exactly_representable(name):
    c = C.exact_case(name)
    ref = c["ref"]
    assert torch.equal(ref["save_mean"], torch.zeros(c["N"], dtype=torch.float64))
    assert torch.equal(ref["save_invstd"], torch.full((c["N"],), 0.5, dtype=torch.float64))
    assert int((c["y"] == 1).sum()) == int((c["y"] == -1).sum()) == c["M"] * c["N"] // 2
    zero = ref["z"] == 0
    assert int(zero.sum()) >= c["M"] and int(zero.any(0).sum()) >= c["N"] // 3   # pre-activations of exactly 0, in many columns
    for k in ("out", "grad_y", "grad_gamma", "grad_beta", "running_mean"):
        assert torch.equal(ref[k].float().double(), ref[k]), k
    for k in ("out", "grad_y"):                                                # ... with room: multiples of 2^-16 below 2^7
        assert torch.equal((ref[k] * 2 ** 16).round(), ref[k] * 2 ** 16) and float(ref[k].abs().max()) < 2 ** 7, k
    # the terms of the column sums are quarters (g') and eighths (g' xhat) of at most 2.5: any partial sum of 1032 of them is exact in fp32
    assert float(c["go"].abs().max()) <= 2.5 and torch.equal(c["go"] * 4, (c["go"] * 4).round())
    assert bool(ref["grad_y"].abs().sum() > 0) and bool(ref["grad_gamma"].abs().sum() > 0)
    if c["M"] & (c["M"] - 1):
        gp = torch.where(ref["z"] > 0, c["go"].double(), torch.zeros_like(ref["z"]))
        assert bool((gp.sum(0) % 258 == 0).all()) and bool(((gp * c["y"].double()).sum(0) % 258 == 0).all())       # the means: over 1032


# ---- the kernel's summation, emulated in numpy fp32 ----------------------------------------------------------------------------------------
def _lane_sums(y, lo, hi, lane, shift):
    """The fp32 sums of d = y - shift and d^2 over rows lo + lane, lo + lane + 8, .. < hi, in row order: (s, q) [N] fp32."""
    rows = y[lo + lane:hi:C.ROW_LANES]
    s = np.zeros(y.shape[1], np.float32)
    q = np.zeros(y.shape[1], np.float32)
    for r in rows:
        d = (r - shift).astype(np.float32)
        s = (s + d).astype(np.float32)
        q = (q + (d * d).astype(np.float32)).astype(np.float32)
    return s, q


def _invstd_of(S, Q, M, eps):
    md = S / M
    var = np.maximum(Q / M - md * md, 0.0)
    return 1.0 / np.sqrt(var + float(np.float32(eps)))


def emulate_column_wide_shift(y, eps):
    """save_invstd of the summation pna_bn_tail.hip had: one shift K_c = y[0, c], eight row lanes added in fp32, float64 across groups."""
    y = y.numpy()
    M = y.shape[0]
    K = y[0]
    S = np.zeros(y.shape[1])
    Q = np.zeros(y.shape[1])
    for lo in range(0, M, C.WG_ROWS):
        hi = min(lo + C.WG_ROWS, M)
        ts = np.zeros(y.shape[1], np.float32)
        tq = np.zeros(y.shape[1], np.float32)
        for lane in range(C.ROW_LANES):
            s, q = _lane_sums(y, lo, hi, lane, K)
            ts, tq = (ts + s).astype(np.float32), (tq + q).astype(np.float32)
        S, Q = S + ts.astype(np.float64), Q + tq.astype(np.float64)
    return _invstd_of(S, Q, M, eps)


def emulate_thread_median_shift(y, eps):
    """save_invstd of the summation it has now: every thread shifts by the median of its first three rows; row lanes, then workgroups
    (stored as fp32 pairs), re-based and added in float64."""
    y = y.numpy()
    M = y.shape[0]
    S = Q = K0 = None
    for lo in range(0, M, C.WG_ROWS):
        hi = min(lo + C.WG_ROWS, M)
        Sw = Qw = Kw = None
        for lane in range(min(C.ROW_LANES, hi - lo)):
            rows = np.arange(lo + lane, hi, C.ROW_LANES)
            first = y[np.minimum(rows[0] + C.ROW_LANES * np.arange(3), rows[-1])]
            k = np.median(first, axis=0).astype(np.float32)
            s, q = _lane_sums(y, lo, hi, lane, k)
            if Kw is None:
                Kw, Sw, Qw = k.astype(np.float64), np.zeros(y.shape[1]), np.zeros(y.shape[1])
            n, dk, s, q = float(len(rows)), k.astype(np.float64) - Kw, s.astype(np.float64), q.astype(np.float64)
            Sw, Qw = Sw + (s + n * dk), Qw + (q + 2.0 * dk * s + n * dk * dk)
        pair = lambda v: v.astype(np.float32).astype(np.float64) + (v - v.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
        Sw, Qw = pair(Sw), pair(Qw)
        if K0 is None:
            K0, S, Q = Kw, np.zeros(y.shape[1]), np.zeros(y.shape[1])
        n, dk = float(hi - lo), Kw - K0
        S, Q = S + (Sw + n * dk), Q + (Qw + 2.0 * dk * Sw + n * dk * dk)
    return _invstd_of(S, Q, M, eps)


def _invstd_ratio(c, emulate):
    got = torch.from_numpy(emulate(c["y"], c["eps"]))
    return ((got - c["ref"]["save_invstd"]).abs() / c["bars"]["save_invstd"]).numpy()


@pytest.mark.parametrize("name", ["m3", "m9", "m513", "m1025", "n65", "norelu"])
def test_both_shifts_meet_the_statistics_bar_on_ordinary_cases(name):
    c = C.case(name)
    assert _invstd_ratio(c, emulate_column_wide_shift).max() <= 1.0
    assert _invstd_ratio(c, emulate_thread_median_shift).max() <= 1.0


@pytest.mark.parametrize("name", C.STATS_NAMES)
def test_an_unusual_first_row_breaks_the_column_wide_shift_and_not_the_thread_median(name):
    """Why the statistics cases exist: with K_c = y[0, c] and row 0 at 100 sigma every workgroup sums d^2 ~ 10^4 sigma^2 in fp32 and the
    variance cancels -- the emulation exceeds the 1e-5 bar of save_invstd on those columns (what the GPU showed before the shift was
    changed: DESIGN.md) and meets it on the plain, the large-mean and the constant ones.  The per-thread median meets it on all."""
    c = C.case(name)
    old = _invstd_ratio(c, emulate_column_wide_shift)
    new = _invstd_ratio(c, emulate_thread_median_shift)
    kinds = np.array(c["kinds"])
    row0 = np.isin(kinds, ["row0_100", "row0_1000", "row0_100_small"])
    print("BN_EMULATED", name, " ".join(f"{k}: old {old[kinds == k].max():.3g} new {new[kinds == k].max():.3g}" for k in C.KINDS))
    assert old[row0].max() > 1.0
    assert old[np.isin(kinds, ["plain", "bigmean", "const"])].max() <= 1.0
    assert new.max() <= 0.5


# ---- the predicate -----------------------------------------------------------------------------------------------------------------------
class _OnGpu:
    """What bn_tail_applies looks at of a tensor, with is_cuda forced: the host has no device to put one on."""

    def __init__(self, t, is_cuda=True):
        self.t, self.is_cuda, self.dtype, self.shape = t, is_cuda, t.dtype, t.shape

    def dim(self):
        return self.t.dim()

    def stride(self, i):
        return self.t.stride(i)


def test_bn_tail_applies_clause_by_clause(monkeypatch):
    monkeypatch.setattr(AG, "BN_TAIL", True)
    y = torch.zeros(6, 5)
    bn = nn.BatchNorm1d(5).train()
    assert AG.bn_tail_applies(bn, _OnGpu(y), None)
    assert AG.bn_tail_applies(bn, _OnGpu(y), _OnGpu(torch.zeros(6, 5)))
    pitched = torch.zeros(6, 8)[:, :5]
    assert pitched.stride(0) == 8 and AG.bn_tail_applies(bn, _OnGpu(pitched), None)            # a row-pitched y is served
    assert AG.bn_tail_applies(nn.BatchNorm1d(128).train(), _OnGpu(torch.zeros(2, 128)), None)     # the limits themselves
    assert not AG.bn_tail_applies(nn.BatchNorm1d(5, momentum=None).train(), _OnGpu(y), None)
    assert not AG.bn_tail_applies(nn.BatchNorm1d(5, track_running_stats=False).train(), _OnGpu(y), None)
    assert not AG.bn_tail_applies(nn.BatchNorm1d(5).eval(), _OnGpu(y), None)
    assert not AG.bn_tail_applies(nn.BatchNorm1d(129).train(), _OnGpu(torch.zeros(6, 129)), None)
    assert not AG.bn_tail_applies(bn, _OnGpu(torch.zeros(1, 5)), None)
    assert not AG.bn_tail_applies(bn.double(), _OnGpu(y.double()), None)
    bn = bn.float()
    assert not AG.bn_tail_applies(bn, _OnGpu(torch.zeros(5, 6).t()), None)                     # y.stride(1) != 1
    assert not AG.bn_tail_applies(bn, y, None) and not AG.bn_tail_applies(bn, _OnGpu(y, is_cuda=False), None)   # a CPU tensor
    assert not AG.bn_tail_applies(bn, _OnGpu(y), _OnGpu(torch.zeros(6, 4)))
    assert not AG.bn_tail_applies(bn, _OnGpu(y), _OnGpu(torch.zeros(6, 5, dtype=torch.float64)))
    assert not AG.bn_tail_applies(bn, _OnGpu(y), _OnGpu(torch.zeros(6, 5), is_cuda=False))
    monkeypatch.setattr(AG, "BN_TAIL", False)
    assert not AG.bn_tail_applies(bn, _OnGpu(y), None)
