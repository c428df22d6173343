"""Cases and references of the one-call dense PNALayer (pna_dense_layer_fwd_f32 / _bwd_f32, autograd.DenseLayerFn).

A case is a dict: the layer's configuration, x (B, N, in), adj (B, N, N), the layer's state_dict and a cotangent `go`, all fp32 on the CPU,
continuous random.  The reference is oracle.torch_oracle.dense_layer_forward in float64 and float64 autograd through it; the yardstick is
the SAME function run in fp32 on the CPU:

    bar(tensor) = 4 max|oracle32 - ref64| + 2^-20 max|ref64|          one number per tensor, every element checked against it

(4: another summation order, the precedent of test_gpu_layers.py).  The bar may not exceed CAP = 1e-4 max|ref64| for any tensor of any
case: test_dense_layer_host.py asserts that for every case below, so a lenient bar cannot hide a failure.

For max / min the builder asserts in float64 that the best and the runner-up of every column differ by more than 1e-4 of the column's
spread, so fp32 and float64 pick the same entry.  Every row and column has an entry (a ring i -> i + 1 under the random edges).
"""
import functools

import torch

from oracle import torch_oracle as TO

AVG_D = {"log": 1.3862943649291992, "lin": 3.25}     # fp32-representable, so the device scalar and the float64 reference hold one value
CAP = 1e-4
FLOOR = 2.0 ** -20

#          name      N    B   T  Fi  Fo  divide self_loop  aggregators          scalers                                    weights    seed
CASES = {
    "n1":      (1,   1,   1, 1,  1,  True,  True,  "mean max min std", ("identity",),                                "binary",   1),
    "n2":      (2,   3,   4, 2,  4,  False, False, "mean max min std", ("identity", "amplification", "attenuation"), "binary",   2),
    "n15":     (15,  3,   4, 4,  4,  True,  False, "mean max min std", ("identity", "amplification", "attenuation"), "binary",   3),
    "n16":     (16,  1,   3, 5,  7,  True,  True,  "std min",          ("linear", "inverse_linear"),                 "binary",   4),
    "n17":     (17,  3,   1, 64, 64, True,  False, "mean max min std", ("identity", "linear", "inverse_linear"),     "binary",   5),
    "n17w":    (17,  1,   8, 8,  8,  False, False, "max",              ("amplification",),                           "binary",   6),
    "n64":     (64,  1,   8, 8,  8,  True,  False, "max",              ("attenuation",),                             "binary",   7),
    "n65":     (65,  3,   4, 4,  4,  False, True,  "mean max min std", ("identity", "inverse_linear"),               "weighted", 8),
    "n128":    (128, 1,   4, 4,  4,  True,  False, "mean max min std", ("identity", "amplification", "attenuation"), "binary",   9),
    "n128s":   (128, 1,   1, 1,  1,  True,  False, "std min",          ("linear",),                                  "binary",   10),
    "slab":    (2,   257, 4, 2,  4,  True,  False, "mean max min std", ("identity", "amplification"),                "binary",   50),
    "neg":     (15,  3,   4, 2,  4,  True,  False, "mean max min std", ("identity", "linear"),                       "negative", 42),
}
NAMES = list(CASES)     # (seeds: the first tried, except slab and neg -- there the fp32 oracle's own std cancellation broke the cap)


def make_layer(c, device="cpu", avg_d=None):
    from pna_amd.pytorch.pna.layer import PNALayer
    layer = PNALayer(c["in_features"], c["out_features"], c["aggregators"], c["scalers"], AVG_D if avg_d is None else avg_d, towers=c["T"],
                     self_loop=c["self_loop"], divide_input=c["divide_input"], device="cpu")
    layer.load_state_dict(c["sd"], strict=True)
    return layer.to(device)


def _adjacency(B, N, kind, gen):
    """Random directed edges at ~30 % over the ring i -> i + 1 (every row and column has an entry); N = 1: the single self edge."""
    if N == 1:
        return torch.ones(B, 1, 1)
    adj = (torch.rand(B, N, N, generator=gen) < 0.3).float()
    idx = torch.arange(N)
    adj[:, idx, (idx + 1) % N] = 1.0
    if kind in ("weighted", "negative"):
        adj = adj * (0.25 + 1.5 * torch.rand(B, N, N, generator=gen))              # positive, non-integer
    if kind == "negative":                                                          # one negative weight per graph, off the ring: counted by
        for b in range(B):                                                          # mean / std, masked out of max / min
            adj[b, 3, 7] = -0.375
    return adj


def _near_ties(c):
    """float64: the (b, i) of every runner-up P_i that comes within 1e-4 of the column's spread of the best over {i : a'_ij > 0}, per tower-
    feature, column j and for max and min alike; empty when fp32 and float64 are sure to pick the same entry."""
    x, adj = c["x"].double(), c["adj"].double()
    B, N, _ = adj.shape
    if c["self_loop"]:
        adj = adj + torch.eye(N, dtype=torch.float64)
    Fi = c["Fi"]
    bad = set()
    mask = (adj > 0).unsqueeze(-1)                                                  # (B, i, j, 1)
    assert mask.any(dim=1).all(), "a column without an entry"
    if N < 2:
        return bad
    for t in range(c["T"]):
        w = c["sd"][f"towers.{t}.pretrans.fully_connected.0.linear.weight"].double()[:, :Fi]
        xt = x[:, :, t * Fi:(t + 1) * Fi] if c["divide_input"] else x
        Pi = (xt @ w.t()).unsqueeze(2).expand(B, N, N, Fi)
        for sign in (1.0, -1.0):
            v = torch.where(mask, sign * Pi, torch.tensor(-float("inf"), dtype=torch.float64))
            top, idx = torch.topk(v, 2, dim=1)
            lo = torch.where(mask, sign * Pi, torch.tensor(float("inf"), dtype=torch.float64)).min(dim=1).values
            close = torch.isfinite(top[:, 1]) & ~(top[:, 0] - top[:, 1] > 1e-4 * (top[:, 0] - lo))
            for b, _, _ in close.nonzero().tolist():
                bad.update((b, int(i)) for i in idx[b, 1][close[b]].tolist())
    return bad


@functools.lru_cache(maxsize=None)
def dense_case(name):
    N, B, T, Fi, Fo, divide, self_loop, aggs, scalers, kind, seed = CASES[name]
    gen = torch.Generator().manual_seed(1000 + seed)
    in_f = T * Fi if divide else Fi
    c = dict(name=name, N=N, B=B, T=T, Fi=Fi, Fo=Fo, divide_input=divide, self_loop=self_loop, aggregators=aggs.split(), scalers=list(scalers),
             in_features=in_f, out_features=T * Fo)
    A, S = len(c["aggregators"]), len(scalers)
    sd = {}
    for t in range(T):
        sd[f"towers.{t}.pretrans.fully_connected.0.linear.weight"] = torch.randn(Fi, 2 * Fi, generator=gen) / (2 * Fi) ** 0.5
        sd[f"towers.{t}.pretrans.fully_connected.0.linear.bias"] = 0.2 * torch.randn(Fi, generator=gen)
        sd[f"towers.{t}.posttrans.fully_connected.0.linear.weight"] = torch.randn(Fo, (1 + A * S) * Fi, generator=gen) / ((1 + A * S) * Fi) ** 0.5
        sd[f"towers.{t}.posttrans.fully_connected.0.linear.bias"] = 0.2 * torch.randn(Fo, generator=gen)
    sd["mixing_network.linear.weight"] = torch.randn(T * Fo, T * Fo, generator=gen) / (T * Fo) ** 0.5
    sd["mixing_network.linear.bias"] = 0.2 * torch.randn(T * Fo, generator=gen)
    c["sd"] = sd
    c["x"] = torch.randn(B, N, in_f, generator=gen)
    c["adj"] = _adjacency(B, N, kind, gen)
    c["go"] = torch.randn(B, N, T * Fo, generator=gen)
    assert (c["adj"].sum(-1) > 0.2).all()                                           # the scalers divide by D and by log(D + 1)
    if "max" in c["aggregators"] or "min" in c["aggregators"]:
        for _ in range(100):                                                        # a runner-up too close to the best: draw that node's row again
            bad = _near_ties(c)
            if not bad:
                break
            for b, i in sorted(bad):
                c["x"][b, i] = torch.randn(in_f, generator=gen)
        assert not _near_ties(c), "a near-tie between the best and the runner-up"
    return c


def oracle_run(c, dtype):
    """dense_layer_forward in `dtype` on the CPU and autograd through it: {'out': ..., 'x': grad, <parameter name>: grad}."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in c["sd"].items()}
    x = c["x"].to(dtype).clone().requires_grad_(True)
    avg = {k: torch.tensor(v, dtype=dtype) for k, v in AVG_D.items()}
    out = TO.dense_layer_forward(sd, x, c["adj"].to(dtype), c["aggregators"], c["scalers"], avg, c["T"], c["divide_input"], c["self_loop"])
    names = list(sd)
    grads = torch.autograd.grad(out, [x] + [sd[k] for k in names], c["go"].to(dtype))
    res = {"out": out.detach(), "x": grads[0]}
    res.update({k: g for k, g in zip(names, grads[1:])})
    return res


def references_of(c):
    """(ref64, oracle32, bars) of a case dict."""
    r64, r32 = oracle_run(c, torch.float64), oracle_run(c, torch.float32)
    bars = {k: 4.0 * float((r32[k].double() - r64[k]).abs().max()) + FLOOR * float(r64[k].abs().max()) for k in r64}
    return r64, r32, bars


@functools.lru_cache(maxsize=None)
def references(name):
    """references_of the named case: computed once and shared; nobody writes into them."""
    return references_of(dense_case(name))


def cap_of(ref64):
    return {k: CAP * float(v.abs().max()) for k, v in ref64.items()}


def worst_ratio(got, ref64, bar):
    """max |got - ref64| / bar (0 / 0 = 0: a tensor that is exactly zero in the reference has a zero bar)."""
    err = float((got.double().cpu() - ref64).abs().max())
    return 0.0 if err == 0.0 else (float("inf") if bar == 0.0 else err / bar)
