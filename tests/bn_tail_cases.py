"""Cases and references of the streaming BatchNorm tail (pna_bn_tail_fwd_f32 / _bwd_f32, autograd.BnTailFn).  Everything here runs on
the host; no autograd.

The reference, `bn_tail_ref`, is the closed form of the header comment of pna_bn_tail_args written out in float64 from the fp32 inputs
(tests/test_bn_tail_cases_host.py checks it against nn.BatchNorm1d(...).double() under autograd):

    mean_c, var_c (biased) of y[:, c];  save_mean = mean,  save_invstd = 1 / sqrt(var + eps);  xhat = (y - mean) save_invstd
    z = xhat gamma + beta;  out = residual + (relu ? max(z, 0) : z)
    running_mean = (1 - m) running_mean + m mean;  running_var = (1 - m) running_var + m var M / (M - 1)     (m < 0 or NULL: left alone)
    g' = grad_out where z > 0 (relu) or everywhere;  grad_beta = sum_r g';  grad_gamma = sum_r g' xhat
    grad_y = gamma save_invstd (g' - mean_r g' - xhat mean_r(g' xhat))

BARS are per element: a float64 tensor of the reference's shape beside every reference tensor, computed by first-order propagation of

    save_invstd   1e-5 relative                                   (the project's bar for statistics: BASELINE.json)
    save_mean     2^-23 |mean_c| + 1e-5 sigma_c                   (the rounding of the stored fp32 value; sigma_c = sqrt(var_c))
    running_*     the same bars (for the variance: 2e-5 (var + eps), what 1e-5 of save_invstd is in var, times M / (M - 1)) scaled by
                  the momentum, + 2^-23 of the result
    out           through z = (y - mean) gamma invstd + beta: |gamma| invstd bar(mean) + |xhat gamma| 1e-5,
                  + 2^-22 ((|y| + |mean|) |gamma| invstd + |beta| + |residual|): the absolute terms of the expression written out
    grad_beta     1e-5 sum_r |g'|
    grad_gamma    1e-5 sum_r |g' xhat| + sum_r |g'| bar(xhat),   bar(xhat) = invstd bar(mean) + 1e-5 |xhat|
    grad_y        with a = gamma invstd, m1 = mean g', m2 = mean g' xhat, T = |g'| + |m1| + |xhat m2|:
                  |a| (bar(grad_beta) / M + |xhat| bar(grad_gamma) / M + |m2| bar(xhat)) + 1e-5 |a| T
                  + 2^-22 |a| (|g'| + |m1| + (|y| + |mean|) invstd |m2|)

They are ceilings worked out from the formats and the statistics bar, not fits to any implementation.

THE RELU KINK, with no element left out.  An element whose z lies within the error those bars allow at z ~ 0 could legitimately take the
other branch.  There |xhat gamma| = |beta|, so that error is  e_z = 1e-5 |beta_c| + |gamma_c| invstd_c (bar(mean_c) + 2^-24 (|y| + |mean_c|)).
After drawing y every element with |z| < delta = 4 e_z is moved away from the kink (to |z| ~ 3 delta, on the side it was on) and everything
is recomputed, until none is left (`kink_margin`; the host test asserts min |z| / delta >= 1 for every random case).  The masks of any
implementation within the bars and of the reference then agree, and no row is excluded.

EXACT cases: y in {-1, +1} in equal numbers per column and eps = 3, so mean = 0, var = 1, save_invstd = 0.5 exactly; gamma a power of
two, beta such that z == 0 on some elements (beta = +-gamma / 2: where the kernel's !(z > 0) must give a zero derivative, as F.relu
does), residual and grad_out quarters.  Every sum is then exact in fp32 in any order.  M = 512: the means of g' are sums over 512, exact.
M = 1032 (three workgroups, the last of 8 rows): 1032 is no power of two, so grad_out is drawn in +- pairs inside every mask class and
then moved by y / 2: the class sums are +-258 and the two column means 0 or +-1/4, +-1/8.  Every output is compared bit for bit
(running_var, whose M / (M - 1) is no dyadic number, after one rounding of the float64 reference to fp32)."""
import functools
import math

import torch

U23 = 2.0 ** -23
U22 = 2.0 ** -22
U24 = 2.0 ** -24
STAT = 1e-5                     # the statistics bar
SENTINEL = -7.25                # what the padding columns of pitched buffers hold
WG_ROWS = 512                   # rows of one workgroup of pna_bn_tail.hip
ROW_LANES = 8                   # its row lanes

KINDS = ("plain", "bigmean", "row0_100", "row0_1000", "row0_100_small", "rows0_512", "rows0_7", "const")
ROW0_KINDS = ("row0_100", "row0_1000", "row0_100_small", "rows0_512", "rows0_7")

_D = dict(relu=1, gamma=True, beta=True, residual=True, running=True, momentum=0.1, eps=1e-5, pitches=None, stats=False, null_grads=(), seed=0)


def _spec(M, N, **k):
    return dict(_D, M=M, N=N, **k)


CASES = {}
for _M in (2, 3, 7, 8, 9, 511, 512, 513, 1024, 1025):                        # fewer rows than row lanes; around one and two workgroups
    CASES[f"m{_M}"] = _spec(_M, 33)
for _N in (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128):              # the strip edges
    CASES[f"n{_N}"] = _spec(521, _N)
CASES["wg257"] = _spec(131073, 5)                                            # more than 256 workgroups: k_bn_finalize's loop goes round
CASES["wg513"] = _spec(262657, 5)                                            # 513 full workgroups and one row: three iterations for thread 0
#                                                        ldy, ld_res, ld_out, ld_go, ld_gy: all different, all > N, odd ones among them
CASES["pitched"] = _spec(530, 70, pitches=(72, 71, 80, 75, 96))
CASES["norelu"] = _spec(300, 40, relu=0)
CASES["gamma_only"] = _spec(300, 40, beta=False)
CASES["beta_only"] = _spec(300, 40, gamma=False)
CASES["noaffine"] = _spec(300, 40, gamma=False, beta=False)
CASES["nores"] = _spec(300, 40, residual=False)
CASES["norunning"] = _spec(300, 40, running=False)
CASES["mom_neg"] = _spec(300, 40, momentum=-1.0)
CASES["mom0"] = _spec(300, 40, momentum=0.0)
CASES["mom1"] = _spec(300, 40, momentum=1.0)
CASES["no_ggamma"] = _spec(300, 40, null_grads=("grad_gamma",))
CASES["no_gbeta"] = _spec(300, 40, null_grads=("grad_beta",))
CASES["no_gg_gb"] = _spec(300, 40, null_grads=("grad_gamma", "grad_beta"))
CASES["stats_a"] = _spec(4101, 33, stats=True)                               # column c is of kind KINDS[c % 8]
CASES["stats_b"] = _spec(4101, 33, stats=True, relu=0, residual=False, pitches=(35, 34, 40, 37, 48), seed=1)
NAMES = list(CASES)
STATS_NAMES = ["stats_a", "stats_b"]
MAX_ROUNDS = 8


def bn_tail_ref(y, gamma, beta, residual, go, rm, rv, eps, momentum, relu, plant=None):
    """-> dict of float64 tensors: save_mean, save_invstd, out, running_mean, running_var (None without running statistics), grad_y,
    grad_gamma, grad_beta, and z (the pre-activation, not an output).  plant: one deliberate error (the host test's `bars bite`)."""
    y = y.double()
    M, N = y.shape
    one = torch.ones(N, dtype=torch.float64)
    g = one if gamma is None else gamma.double()
    b = 0 * one if beta is None else beta.double()
    eps = float(torch.tensor(eps, dtype=torch.float32))
    ys = y[:-1] if plant == "drop_last_row" else y
    mean = ys.sum(0) / M
    var = ((ys - mean) ** 2).sum(0) / M if plant == "drop_last_row" else ((y - mean) ** 2).mean(0)
    var_n = var * M / (M - 1) if plant == "unbiased_norm" else var
    invstd = 1.0 / torch.sqrt(var_n + eps)
    xhat = (y - mean) * invstd
    z = xhat * g + b
    act = torch.where(z > 0, z, torch.zeros_like(z)) if relu else z
    out = act if residual is None else residual.double() + act
    r = {"save_mean": mean, "save_invstd": invstd, "out": out, "z": z, "running_mean": None, "running_var": None}
    if rm is not None:
        m = float(torch.tensor(momentum, dtype=torch.float32))
        if m >= 0:
            r["running_mean"] = (1 - m) * rm.double() + m * mean
            r["running_var"] = (1 - m) * rv.double() + m * (var if plant == "biased_running" else var * M / (M - 1))
        else:
            r["running_mean"], r["running_var"] = rm.double().clone(), rv.double().clone()
    keep = (z > 0) if relu else torch.ones_like(z, dtype=torch.bool)
    go = go.double()
    if plant == "flip_mask":                                                 # at the element where it matters most
        i = int((go * g * invstd).abs().argmax())
        keep = keep.clone()
        keep[i // N, i % N] = ~keep[i // N, i % N]
    gp = torch.where(keep, go, torch.zeros_like(go))
    r["grad_beta"] = gp.sum(0)
    r["grad_gamma"] = ((go if plant == "ggamma_nomask" else gp) * xhat).sum(0)
    m1 = gp.sum(0) / (M - 1 if plant == "mean_g_m1" else M)
    m2 = (gp * xhat).mean(0)
    r["grad_y"] = g * invstd * (gp - m1 - xhat * m2)
    if plant == "strip_unwritten":
        c0 = 32 * ((N - 1) // 32)
        r["out"], r["grad_y"] = r["out"].clone(), r["grad_y"].clone()
        r["out"][:, c0:] = float("nan")
        r["grad_y"][:, c0:] = float("nan")
    return r


PLANTS = ("unbiased_norm", "biased_running", "drop_last_row", "strip_unwritten", "flip_mask", "mean_g_m1", "ggamma_nomask")


def bn_tail_bars(c, ref):
    """The per-element bars of the module docstring for case c and its float64 reference."""
    y = c["y"].double()
    M, N = y.shape
    g = torch.ones(N, dtype=torch.float64) if c["gamma"] is None else c["gamma"].double().abs()
    b = torch.zeros(N, dtype=torch.float64) if c["beta"] is None else c["beta"].double().abs()
    mean, invstd = ref["save_mean"], ref["save_invstd"]
    eps = float(torch.tensor(c["eps"], dtype=torch.float32))
    var = 1.0 / invstd ** 2 - eps
    var = torch.where(var > 0, var, torch.zeros_like(var))
    b_mean = U23 * mean.abs() + STAT * torch.sqrt(var)
    b_inv = STAT * invstd
    bars = {"save_mean": b_mean, "save_invstd": b_inv}
    if ref["running_mean"] is not None:
        m = max(0.0, float(torch.tensor(c["momentum"], dtype=torch.float32)))
        bars["running_mean"] = m * b_mean + U23 * ref["running_mean"].abs()
        bars["running_var"] = m * 2 * STAT * (var + eps) * M / (M - 1) + U23 * ref["running_var"].abs()
    xhat = (y - mean) * invstd
    b_xhat = invstd * b_mean + STAT * xhat.abs()
    res = 0 if c["residual"] is None else c["residual"].double().abs()
    a = g * invstd
    span = (y.abs() + mean.abs()) * invstd                                   # |y invstd| + |mean invstd|: the terms of xhat written out
    bars["out"] = a * b_mean + STAT * (xhat * g).abs() + U22 * (span * g + b + res)
    keep = (ref["z"] > 0) if c["relu"] else torch.ones_like(y, dtype=torch.bool)
    gp = torch.where(keep, c["go"].double(), torch.zeros_like(y))
    bars["grad_beta"] = STAT * gp.abs().sum(0)
    bars["grad_gamma"] = STAT * (gp * xhat).abs().sum(0) + (gp.abs() * b_xhat).sum(0)
    m1, m2 = gp.mean(0), (gp * xhat).mean(0)
    T = gp.abs() + m1.abs() + (xhat * m2).abs()
    bars["grad_y"] = (a * (bars["grad_beta"] / M + xhat.abs() * bars["grad_gamma"] / M + m2.abs() * b_xhat) + STAT * a * T
                      + U22 * a * (gp.abs() + m1.abs() + span * m2.abs()))
    return bars


def tensors_of(c):
    """The names of the tensors a case checks (a NULL output has none)."""
    names = ["save_mean", "save_invstd", "out"] + (["running_mean", "running_var"] if c["rm0"] is not None else []) + ["grad_y"]
    return names + [k for k in ("grad_gamma", "grad_beta") if k not in c["null_grads"]]


def kink_delta(c, ref):
    """delta (M, N): four times the z error the bars allow at z ~ 0."""
    y = c["y"].double()
    N = y.shape[1]
    g = torch.ones(N, dtype=torch.float64) if c["gamma"] is None else c["gamma"].double().abs()
    b = torch.zeros(N, dtype=torch.float64) if c["beta"] is None else c["beta"].double().abs()
    mean, invstd = ref["save_mean"], ref["save_invstd"]
    var = torch.clamp(1.0 / invstd ** 2 - float(torch.tensor(c["eps"], dtype=torch.float32)), min=0)
    b_mean = U23 * mean.abs() + STAT * torch.sqrt(var)
    return 4 * (STAT * b + g * invstd * (b_mean + U24 * (y.abs() + mean.abs())))


def kink_margin(c):
    """min over the elements of |z| / delta (inf without a ReLU)."""
    if not c["relu"]:
        return math.inf
    return float((c["ref"]["z"].abs() / kink_delta(c, c["ref"])).min())


def _ref_of(c, plant=None):
    return bn_tail_ref(c["y"], c["gamma"], c["beta"], c["residual"], c["go"], c["rm0"], c["rv0"], c["eps"], c["momentum"], c["relu"], plant)


def planted(c, plant):
    return _ref_of(c, plant)


def _draw(s, name):
    M, N = s["M"], s["N"]
    gen = torch.Generator().manual_seed(1000 * NAMES.index(name) + s["seed"])

    def randn(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64)

    def rand(*shape):
        return torch.rand(*shape, generator=gen, dtype=torch.float64)
    spread = 0.5 + 3 * rand(N)
    centre = 20 * randn(N)
    noise = randn(M, N)
    kinds = ["plain"] * N
    if s["stats"]:
        kinds = [KINDS[c % len(KINDS)] for c in range(N)]
        for c, kind in enumerate(kinds):
            spread[c], centre[c] = 1.0, 5.0
            if kind == "bigmean":
                spread[c], centre[c] = 0.01, 1000.0                         # (why the sums are shifted at all)
            elif kind == "row0_100_small":
                spread[c] = 0.01
            elif kind == "const":
                spread[c], centre[c] = 0.0, 3.0 + c
    y = noise * spread + centre
    for c, kind in enumerate(kinds):                                         # the unusual first rows: a hub node sorted to the front
        if kind in ("row0_100", "row0_100_small"):
            y[0, c] = centre[c] + 100 * spread[c]
        elif kind == "row0_1000":
            y[0, c] = centre[c] + 1000 * spread[c]
        elif kind == "rows0_512":
            y[0, c] = y[512, c] = centre[c] + 100 * spread[c]
        elif kind == "rows0_7":
            y[:8, c] = centre[c] + 100 * spread[c]
    sign = torch.where(rand(N) < 0.25, -1.0, 1.0).double()
    gamma = (sign * (0.5 + rand(N))).float() if s["gamma"] else None
    beta = randn(N).float() if s["beta"] else None
    if beta is not None:
        for c, kind in enumerate(kinds):
            if kind == "const":
                beta[c] = 0.75 if c % 16 < 8 else -0.75                      # z == beta there: moving y could not take it off the kink
    c = {"name": name, "y": y.float(), "gamma": gamma, "beta": beta, "residual": randn(M, N).float() if s["residual"] else None,
         "go": randn(M, N).float(), "rm0": randn(N).float() if s["running"] else None, "rv0": (0.5 + rand(N)).float() if s["running"] else None,
         "eps": s["eps"], "momentum": s["momentum"], "relu": s["relu"], "pitches": s["pitches"], "null_grads": tuple(s["null_grads"]),
         "kinds": kinds, "M": M, "N": N}
    return c


@functools.lru_cache(maxsize=None)
def _case(name):
    c = _draw(CASES[name], name)
    const = torch.tensor([k == "const" for k in c["kinds"]])
    rounds = 0
    while True:
        ref = _ref_of(c)
        if not c["relu"]:
            break
        delta = kink_delta(c, ref)
        near = ref["z"].abs() < delta
        if not bool(near.any()):
            break
        rounds += 1
        assert rounds <= MAX_ROUNDS and not bool(near[:, const].any()), (name, rounds, int(near.sum()))
        g = torch.ones(c["N"], dtype=torch.float64) if c["gamma"] is None else c["gamma"].double()
        side = torch.where(ref["z"] < 0, -1.0, 1.0).double()                 # the side it was on (z == 0: up)
        want = side * 3 * delta                                              # z after the move, up to the statistics' own shift
        y = c["y"].double()
        y = torch.where(near, y + (want - ref["z"]) / (g * ref["save_invstd"]), y)
        c["y"] = y.float()
    c["kink_rounds"] = rounds
    c["ref"] = ref
    c["bars"] = bn_tail_bars(c, ref)
    return c


def case(name):
    """The case's dict -- y, residual, go (M, N), gamma, beta, rm0, rv0 [N] as host fp32 (None: a NULL argument), eps, momentum, relu,
    pitches, null_grads, kinds (per column), and ref / bars (float64) -- computed once and shared: callers leave it unchanged."""
    return _case(name)


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar over every element (0 / 0 = 0; a NaN or a wrong shape: inf)."""
    if tuple(got.shape) != tuple(ref.shape):
        return math.inf
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
    if bool(torch.isnan(ratio).any()):
        return math.inf
    return float(ratio.max()) if ratio.numel() else 0.0


def pitched(t, ld, fill=SENTINEL):
    """(buffer (M, ld) filled with `fill`, its view [:, :N] holding t) on t's device."""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf, buf[:, :t.shape[1]]


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------
EXACT = {"e512": (512, 40, 1), "e1032": (1032, 33, 2)}
EXACT_NAMES = list(EXACT)


@functools.lru_cache(maxsize=None)
def exact_case(name):
    M, N, seed = EXACT[name]
    gen = torch.Generator().manual_seed(seed)
    y = torch.empty(M, N)
    for c in range(N):                                                       # +-1 in equal numbers, another order in every column
        y[:, c] = torch.where(torch.randperm(M, generator=gen) < M // 2, 1.0, -1.0)
    gamma = torch.tensor([(1.0, 2.0, 0.5, -1.0, -2.0)[c % 5] for c in range(N)])
    # beta: gamma / 2 (z == 0 where y gamma < 0), - gamma / 2 (z == 0 where y gamma > 0), 0, and 4 (every element passes)
    beta = torch.tensor([(0.5, -0.5, 0.0, 8.0)[c % 4] for c in range(N)]) * gamma
    beta = torch.where(torch.arange(N) % 4 == 3, beta.abs(), beta)

    def quarters(*shape):
        return torch.randint(-8, 9, shape, generator=gen).float() / 4
    go = quarters(M, N)
    if M & (M - 1):                                                          # no power of two: the two column means must be 0
        for c in range(N):
            for cls in (y[:, c] > 0, y[:, c] < 0):                           # g' is grad_out on a union of these classes
                idx = cls.nonzero().flatten()
                assert idx.numel() % 2 == 0
                half = idx.numel() // 2
                go[idx[half:], c] = -go[idx[:half], c]
            go[:, c] += 0.5 * y[:, c]                                        # ... or a multiple of 1032 / 4: +-258 per class
    c = {"name": name, "y": y, "gamma": gamma, "beta": beta, "residual": quarters(M, N), "go": go, "rm0": quarters(N), "rv0": quarters(N).abs() + 1,
         "eps": 3.0, "momentum": 0.5, "relu": 1, "pitches": None, "null_grads": (), "kinds": ["exact"] * N, "M": M, "N": N}
    c["ref"] = _ref_of(c)
    return c
