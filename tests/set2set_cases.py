"""Cases and references of the one-call Set2Set readout (pna_set2set_fwd_f32 / _bwd_f32, autograd.Set2SetFn, layers.Set2Set).

A case is a dict: x (B, N, D), the four nn.LSTM(2D, D) parameters (gate order i, f, g, o) and a cotangent `go` (B, 2D), all fp32 on the
CPU.  x and go are randn; the parameters are uniform(-k, k) * scale with k = D^-1/2 (nn.LSTM's own initialisation at scale 1), b_ih and b_hh
drawn independently.  The reference is `set2set_ref`, a plain-torch restatement of models/layers.py:81-98 runnable in any dtype, in float64
with float64 autograd through it; the yardstick is the SAME function run in fp32 on the CPU (tests/dense_layer_cases.py's convention):

    bar(tensor) = 4 max|oracle32 - ref64| + 2^-20 max|ref64|          one number per tensor, every element checked against it

(4: another summation order).  The bar may not exceed CAP = 1e-4 max|ref64| for any tensor of any case: test_set2set_host.py asserts that
for every case below, so a lenient bar cannot hide a failure.  The functions are smooth: no element is excluded.
"""
import functools

import torch

CAP = 1e-4
FLOOR = 2.0 ** -20
SLABS = 256                # PNA_S2S_MAX_SLABS (test_set2set_host.py holds the two together)

#          name      N    B    D   steps  weight scale  x scale  seed
CASES = {
    "n1":      (1,   1,   2,  None, 1.0, 1.0, 1),
    "n2":      (2,   3,   2,  None, 1.0, 1.0, 2),
    "n15":     (15,  16,  16, None, 1.0, 1.0, 3),          # the multitask shape
    "n17":     (17,  3,   32, None, 1.0, 1.0, 4),
    "n64":     (64,  2,   31, None, 1.0, 1.0, 5),
    "n128":    (128, 2,   32, None, 1.0, 1.0, 6),          # the LDS edge
    "n128s":   (128, 1,   2,  None, 1.0, 1.0, 7),
    "n97":     (97,  4,   16, None, 1.0, 1.0, 8),
    "steps3":  (15,  3,   16, 3,    1.0, 1.0, 9),
    "slab":    (5,   300, 16, None, 1.0, 1.0, 10),         # more graphs than slabs: two graphs per workgroup
    "w3":      (128, 2,   32, None, 3.0, 1.0, 29),         # saturated gates
    "d1":      (9,   3,   1,  None, 1.0, 1.0, 12),
    "sat":     (15,  3,   16, None, 1.0, 4.0, 31),         # x scaled by 4: a saturated softmax
}
NAMES = list(CASES)     # (seeds: the first tried, except w3 and sat -- there the recurrence is so sensitive for most seeds that the fp32 oracle
#                         alone breaks the cap, by up to 20 x; theirs were picked among seeds 20 .. 31 for a bar under a tenth of the cap)
PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh")
TENSORS = ("out", "x") + PARAMS


def set2set_ref(x, w_ih, w_hh, b_ih, b_hh, steps):
    """models/layers.py:81-98 with the one-step LSTM written out (torch gate order i, f, g, o); any dtype."""
    B, N, D = x.shape
    h = x.new_zeros(B, D)
    c = x.new_zeros(B, D)
    q_star = x.new_zeros(B, 2 * D)
    for _ in range(steps):
        z = q_star @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
        i, f, g, o = z.split(D, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        e = (x * h.unsqueeze(1)).sum(-1)                               # (B, N)
        a = torch.softmax(e, dim=1)
        r = (a.unsqueeze(-1) * x).sum(1)
        q_star = torch.cat([h, r], dim=1)
    return q_star


@functools.lru_cache(maxsize=None)
def s2s_case(name):
    N, B, D, steps, wscale, xscale, seed = CASES[name]
    gen = torch.Generator().manual_seed(2000 + seed)
    k = D ** -0.5

    def uniform(*shape):
        return (torch.rand(*shape, generator=gen) * 2.0 - 1.0) * (k * wscale)
    c = dict(name=name, N=N, B=B, D=D, steps=steps or N)
    c["x"] = torch.randn(B, N, D, generator=gen) * xscale
    c["w_ih"], c["w_hh"] = uniform(4 * D, 2 * D), uniform(4 * D, D)
    c["b_ih"], c["b_hh"] = uniform(4 * D), uniform(4 * D)
    c["go"] = torch.randn(B, 2 * D, generator=gen)
    return c


def lstm_state_dict(c):
    return {"weight_ih_l0": c["w_ih"], "weight_hh_l0": c["w_hh"], "bias_ih_l0": c["b_ih"], "bias_hh_l0": c["b_hh"]}


def oracle_run(c, dtype):
    """set2set_ref in `dtype` on the CPU and autograd through it: {'out': ..., 'x': grad, 'w_ih': grad, ...}."""
    x = c["x"].to(dtype).clone().requires_grad_(True)
    ps = [c[k].to(dtype).clone().requires_grad_(True) for k in PARAMS]
    out = set2set_ref(x, *ps, c["steps"])
    grads = torch.autograd.grad(out, [x] + ps, c["go"].to(dtype))
    res = {"out": out.detach(), "x": grads[0]}
    res.update(dict(zip(PARAMS, grads[1:])))
    return res


def references_of(c):
    """(ref64, oracle32, bars) of a case dict."""
    r64, r32 = oracle_run(c, torch.float64), oracle_run(c, torch.float32)
    bars = {k: 4.0 * float((r32[k].double() - r64[k]).abs().max()) + FLOOR * float(r64[k].abs().max()) for k in r64}
    return r64, r32, bars


@functools.lru_cache(maxsize=None)
def references(name):
    """references_of the named case: computed once and shared; nobody writes into them."""
    return references_of(s2s_case(name))


def cap_of(ref64):
    return {k: CAP * float(v.abs().max()) for k, v in ref64.items()}


def worst_ratio(got, ref64, bar):
    """max |got - ref64| / bar (0 / 0 = 0: a tensor that is exactly zero in the reference has a zero bar)."""
    err = float((got.double().cpu() - ref64).abs().max())
    return 0.0 if err == 0.0 else (float("inf") if bar == 0.0 else err / bar)
