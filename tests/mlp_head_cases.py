"""Cases and references of the one-call MLP heads (pna_mlp_head_fwd_f32 / _bwd_f32, autograd.MlpHeadFn, nets.MLPReadout, layers.MLP).
Everything here runs on the host.

    y = f_L(... f_1(x))      f_l(h) = act_l(h W_l^T + b_l)      act: "none", "relu" or ("leaky", slope)

The reference is `mlp_grad_ref`, written without autograd and runnable in any dtype (tests/test_mlp_head_host.py checks it in float64
against float64 autograd through nn.Linear, F.relu and F.leaky_relu).  Two kinds of cases:

RANDOM cases: x and the cotangent randn, weights and biases uniform in +-in^-1/2.  The yardstick is the SAME function run in fp32 on the
CPU (tests/dense_layer_cases.py's convention):

    bar(tensor) = 4 max|oracle32 - ref64| + 2^-20 max|ref64|          one number per tensor, every element checked against it

and no bar may exceed CAP = 1e-4 max|ref64|.  The activations have a kink: a hidden unit whose float64 pre-activation lies within the fp32
error of 0 could legitimately flip, so the seeds are CHOSEN such that no unit is at risk (`at_risk`; the host test asserts it for every
case), and nothing is excluded.  A unit is at risk when |a64| <= E_a,
    E_a = gamma(K + 1) (|h| |W|^T + |b|) + E_h |W|^T + 2 u |a64|,   gamma(K) = K u / (1 - K u),  u = 2^-24  (tests/gru_cases.py's dot_gamma),
with E_h the previous layer's E_a + u |h| (the activations are 1-Lipschitz for |slope| <= 1).

EXACT cases test the kink itself: x, weights, biases and the cotangent are small integers or integers over a power of two, the LeakyReLU
slope is 0.25, so every partial sum of the forward, the backward and the slab sums is an integer multiple of one power of two q and below
2^24 q (`exact_bound`) -- fp32 arithmetic is then exact in any order and the GPU must give the float64 reference bit for bit, the
derivative at a pre-activation of exactly 0 included (0 for ReLU, the slope for LeakyReLU: torch's values)."""
import functools
import math

import torch

U = 2.0 ** -24
CAP = 1e-4
FLOOR = 2.0 ** -20
SLAB = 64                       # _lib.PNA_MLP_SLAB_ROWS (tests/test_mlp_head_host.py pins the two together)
MAX_SLABS = 64
ACT_CODES = {"none": 0, "relu": 1, "leaky": 2}      # _lib.PNA_MLP_ACT_*

R, N0 = "relu", "none"
LK = ("leaky", 0.01)

#  name        V     widths                  acts              bias per layer        x (lead, tail) columns   seed
CASES = {
    "zinc":     (128,  (70, 35, 17, 1),        (R, R, N0),       (True, True, True),   None,    0),     # MLPReadout(70, 1)
    "cls10":    (128,  (70, 35, 17, 10),       (R, R, N0),       (True, True, True),   None,    0),     # MLPReadout(70, 10)
    "mt":       (240,  (16, 16, 16, 3),        (LK, LK, LK),     (True, True, True),   None,    0),     # the multitask head, 16 x 15 rows
    "one_row":  (1,    (4, 2, 1),              (R, N0),          (True, True),         None,    3),
    "ragged":   (17,   (5, 3, 2),              (R, N0),          (False, True),        None,    0),     # a ragged tile, a NULL bias
    "one":      (19,   (75, 70),               (R,),             (True,),              None,    0),     # one layer, its activation the last
    "w1":       (16,   (1, 1, 1),              (R, N0),          (True, True),         None,    0),
    "slabs":    (4200, (16, 16, 3),            (R, N0),          (True, True),         None,    0),     # 64 slabs of 66 rows
    "w127":     (20,   (127, 65, 33, 2),       (R, R, N0),       (True, True, True),   None,    0),
    "w128":     (33,   (128, 128, 128),        (R, N0),          (True, True),         None,    0),
    "four":     (20,   (24, 24, 24, 24, 3),    (R, R, R, N0),    (True, True, True, True), None, 0),
    "w128x3":   (33,   (128, 128, 128, 128),   (R, R, N0),       (True, True, False),  None,    5),
    "strided":  (40,   (20, 12, 5),            (LK, N0),         (True, True),         (3, 5),  0),     # x a view of wider rows
    "nobias":   (65,   (16, 16, 16, 3),        (LK, LK, LK),     (False, False, False), None,   0),
}
NAMES = list(CASES)      # (seeds: the first of at most 32 tried without a unit at risk and with no gradient tensor all zero -- the first tried, except
#                          one_row, whose one row has both hidden units dead at seeds 0 .. 2, and w128x3: 3 of 32 qualify)
MAX_SEEDS = 32


def dot_gamma(K):
    return K * U / (1.0 - K * U)


def slab_rows(V):
    return max(SLAB, -(-V // MAX_SLABS))


def act_parts(act):
    """-> (kind, slope)"""
    return (act, 0.0) if isinstance(act, str) else (act[0], float(act[1]))


def act_code(act):
    kind, slope = act_parts(act)
    return ACT_CODES[kind], slope


def _act(a, act):
    kind, slope = act_parts(act)
    if kind == "relu":
        return torch.where(a > 0, a, torch.zeros_like(a))
    if kind == "leaky":
        return torch.where(a > 0, a, a * slope)
    return a


def _dact(a, act):
    """The derivative, torch's value at 0: 0 for ReLU, the slope for LeakyReLU."""
    kind, slope = act_parts(act)
    one = torch.ones_like(a)
    if kind == "relu":
        return torch.where(a > 0, one, torch.zeros_like(a))
    if kind == "leaky":
        return torch.where(a > 0, one, one * slope)
    return one


def mlp_ref(x, ws, bs, acts):
    """-> (pre-activations [a_1 .. a_L], layer inputs [h_0 .. h_L]) in x's dtype; h_L is y."""
    hs, pre = [x], []
    for w, b, act in zip(ws, bs, acts):
        a = hs[-1] @ w.t()
        if b is not None:
            a = a + b
        pre.append(a)
        hs.append(_act(a, act))
    return pre, hs


def mlp_grad_ref(x, ws, bs, acts, go, dtype=torch.float64):
    """-> dict: y, x (the gradient of sum(y * go) by x), w0 .. , b0 .. (None for a missing bias), without autograd, computed in `dtype`."""
    x, go = x.to(dtype), go.to(dtype)
    ws = [w.to(dtype) for w in ws]
    bs = [None if b is None else b.to(dtype) for b in bs]
    pre, hs = mlp_ref(x, ws, bs, acts)
    out = {"y": hs[-1]}
    g = go
    for l in range(len(ws) - 1, -1, -1):
        dz = g * _dact(pre[l], acts[l])
        out[f"w{l}"] = dz.t() @ hs[l]
        out[f"b{l}"] = None if bs[l] is None else dz.sum(0)
        g = dz @ ws[l]
    out["x"] = g
    return out


def tensors_of(c):
    """The names of the tensors a case checks: y, x and every parameter gradient that exists."""
    L = len(c["ws"])
    return ["y", "x"] + [f"w{l}" for l in range(L)] + [f"b{l}" for l in range(L) if c["bs"][l] is not None]


def at_risk(c):
    """The number of hidden (activated) units whose float64 pre-activation lies within the fp32 error bound of 0."""
    x, ws, bs, acts = c["x"].double(), [w.double() for w in c["ws"]], [None if b is None else b.double() for b in c["bs"]], c["acts"]
    pre, hs = mlp_ref(x, ws, bs, acts)
    E_h = torch.zeros_like(x)
    n = 0
    for l, (w, b, act) in enumerate(zip(ws, bs, acts)):
        K = w.shape[1]
        mass = hs[l].abs() @ w.abs().t() + (0 if b is None else b.abs())
        E_a = dot_gamma(K + 1) * mass + E_h @ w.abs().t() + 2 * U * pre[l].abs()
        if act_parts(act)[0] != "none":
            n += int((pre[l].abs() <= E_a).sum())
        E_h = E_a + U * hs[l + 1].abs()
    return n


def strided(t, lead, tail, fill=float("nan")):
    """t as a view of rows `lead` + `tail` columns wider (unit column stride, a row pitch above the width), on t's device."""
    buf = torch.full((t.shape[0], lead + t.shape[1] + tail), fill, dtype=t.dtype, device=t.device)
    buf[:, lead:lead + t.shape[1]] = t
    return buf[:, lead:lead + t.shape[1]]


def _make(V, widths, acts, bias, seed):
    gen = torch.Generator().manual_seed(seed)
    ws, bs = [], []
    for l in range(len(widths) - 1):
        k = 1.0 / math.sqrt(widths[l])
        ws.append((torch.rand(widths[l + 1], widths[l], generator=gen) * 2 - 1) * k)
        bs.append((torch.rand(widths[l + 1], generator=gen) * 2 - 1) * k if bias[l] else None)
    return {"x": torch.randn(V, widths[0], generator=gen), "ws": ws, "bs": bs, "acts": list(acts),
            "go": torch.randn(V, widths[-1], generator=gen)}


@functools.lru_cache(maxsize=None)
def _case(name):
    V, widths, acts, bias, x_pad, seed = CASES[name]
    c = _make(V, widths, acts, bias, 1000 * NAMES.index(name) + seed)
    c["x_pad"] = x_pad
    c["ref"] = mlp_grad_ref(c["x"], c["ws"], c["bs"], c["acts"], c["go"])
    o32 = mlp_grad_ref(c["x"], c["ws"], c["bs"], c["acts"], c["go"], dtype=torch.float32)
    c["oracle32"] = o32
    c["bars"] = {k: 4 * float((o32[k].double() - c["ref"][k]).abs().max()) + FLOOR * float(c["ref"][k].abs().max()) for k in tensors_of(c)}
    return c


def mlp_case(name):
    """The case's dict -- x (V, widths[0]), ws, bs, acts, go (V, widths[L]) as host fp32, x_pad, and ref (float64), oracle32, bars --
    computed once and shared: callers leave it unchanged."""
    return _case(name)


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar over every element (0 / 0 = 0)."""
    err = (got.double() - ref).abs()
    if not err.numel() or float(err.max()) == 0.0:
        return 0.0
    return float(err.max()) / bar


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------
L4 = ("leaky", 0.25)
#  name     V    widths               acts               bias                  value bound  denominator  seed
EXACT = {
    "e_leaky": (40, (16, 8, 3),         (L4, L4),         (True, True),         2, 1, 1),
    "e_four":  (33, (5, 16, 16, 16, 2), (R, R, L4, N0),   (True, True, True, True), 1, 1, 2),
    "e_half":  (17, (3, 4, 1),          (R, L4),          (False, True),        3, 2, 3),
}
EXACT_NAMES = list(EXACT)


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """Integers in [-bound, bound] over `denominator` (a power of two) everywhere; shared, left unchanged."""
    V, widths, acts, bias, bound, den, seed = EXACT[name]
    gen = torch.Generator().manual_seed(seed)

    def ints(*shape):
        return torch.randint(-bound, bound + 1, shape, generator=gen).float() / den
    ws = [ints(widths[l + 1], widths[l]) for l in range(len(widths) - 1)]
    bs = [ints(widths[l + 1]) if bias[l] else None for l in range(len(widths) - 1)]
    c = {"x": ints(V, widths[0]), "ws": ws, "bs": bs, "acts": list(acts), "go": ints(V, widths[-1]), "x_pad": None, "den": den}
    c["ref"] = mlp_grad_ref(c["x"], c["ws"], c["bs"], c["acts"], c["go"])
    return c


def exact_bound(c):
    """-> (M, q): every partial sum of the forward, the backward and the slab sums, in any order, is a multiple of q (a power of two) and
    at most M in magnitude -- M from the same recurrences on absolute values with every activation taken as the identity."""
    q = (1.0 / c["den"]) ** 2                                    # x and the cotangent
    for act in c["acts"]:
        q = q / c["den"]                                         # a weight
        if act_parts(act)[0] == "leaky":
            q = q * act_parts(act)[1]                            # 0.25
    ax, ago = c["x"].double().abs(), c["go"].double().abs()
    aw = [w.double().abs() for w in c["ws"]]
    hs, M = [ax], float(ax.max())
    for w, b in zip(aw, c["bs"]):
        hs.append(hs[-1] @ w.t() + (0 if b is None else b.double().abs()))
        M = max(M, float(hs[-1].max()))
    g = ago
    for l in range(len(aw) - 1, -1, -1):
        M = max(M, float((g.t() @ hs[l]).max()), float(g.sum(0).max()))
        g = g @ aw[l]
        M = max(M, float(g.max()))
    return M, q


def zero_preactivations(c):
    """How many pre-activations of activated layers are exactly 0 in float64."""
    pre, _ = mlp_ref(c["x"].double(), [w.double() for w in c["ws"]], [None if b is None else b.double() for b in c["bs"]], c["acts"])
    return sum(int((a == 0).sum()) for a, act in zip(pre, c["acts"]) if act_parts(act)[0] != "none")
