"""Shared inputs, float64 references and conditions of the one-call PNAConv training tests (test_pyg_train_cases_host.py,
test_gpu_pyg_train_kernels.py, test_gpu_pyg_train_layers.py): a torch restatement of models/pytorch_geometric/pna.py:120-159 with
pre_layers == post_layers == 1 and of its training step loss = sum(out * R) -- output, grad_x, grad_edge_attr and every parameter
gradient, evaluated in float64 (the reference) and in fp32 (the bars' measure of conditioning).  The max / min gradient goes to the
FIRST extremal edge in CSR order (edges sorted by destination, stably), the generic route's rule.  Every reference is computed once per
session and never modified.

The bars are tower_train_cases.close's; the conditions are tower_train_cases' with the PyG message (the edge term included): a
destination is ill-conditioned when its std, evaluated in fp32 against float64, is off by more than 1e-4 relative, or when its max /
min is a near-tie (4e-7).  A builder asserts that they are at most 15 % of the nodes; the seeds were picked on the CPU so the float64
oracle alone satisfies that (test_pyg_train_cases_host.py checks it for every case)."""
import functools
import math
import types

import torch

from tower_train_cases import close

A4 = ("mean", "min", "max", "std")
#        name: (V, edges drawn, towers, divide_input, F_in, F_out, aggregators, scalers, edge_dim, seed)
CASES = {
    "v17_t5": (17, 50, 5, False, 6, 5, A4, ("identity",), None, 2),                                      # T F_out = 25; F_in = 6: K padding
    "v33_edge64": (33, 100, 1, False, 4, 8, ("mean", "max", "var"), ("identity", "linear"), 64, 1),      # T = 1, F_in = 4, the widest edge tile
    "v33_div_edge1": (33, 90, 2, True, 6, 4, A4, ("amplification", "attenuation", "inverse_linear"), 1, 1),
    "sum_only": (17, 40, 2, True, 4, 3, ("sum",), ("identity", "linear"), None, 1),
    "var_neg": (33, 80, 3, False, 8, 4, ("mean", "max", "var"), ("identity", "linear"), None, 1),      # three equal messages into node 0
    "zinc": (45, 300, 5, False, 75, 15, A4, ("identity", "amplification", "attenuation"), 50, 5),       # PyG's ZINC example layer
    # (without edges avg_deg is 0: only the scalers whose deg == 0 rule is a constant stay finite, in the reference too)
    "no_edges": (17, 0, 2, False, 4, 3, A4, ("identity", "inverse_linear"), None, 1),
    "no_edges_edge": (17, 0, 2, True, 4, 3, A4, ("identity", "attenuation"), 3, 1),
}
ISOLATED = 2          # the last nodes (the last 16-row tile) receive no edge


def avg_deg_of(dst, V):
    """The layer's avg_deg dictionary (pna.py:84-91) of a batch's in-degrees, and the degree histogram it is computed from."""
    d = torch.bincount(dst, minlength=V)
    hist = torch.bincount(d).long()
    h = hist.float()
    bins = torch.arange(len(h))
    tot = h.sum()
    return hist, {"lin": ((bins * h).sum() / tot).item(), "log": (((bins + 1).log() * h).sum() / tot).item(), "exp": ((bins.exp() * h).sum() / tot).item()}


def state_dict(T, Fi, Fo, A, S, ed, gen):
    sd, C = {}, T * Fo
    Kpre, Kpost = (3 if ed else 2) * Fi, (1 + A * S) * Fi
    for t in range(T):
        sd[f"pre_nns.{t}.0.weight"] = torch.randn(Fi, Kpre, generator=gen) / math.sqrt(Kpre)
        sd[f"pre_nns.{t}.0.bias"] = 0.1 * torch.randn(Fi, generator=gen)
        sd[f"post_nns.{t}.0.weight"] = torch.randn(Fo, Kpost, generator=gen) / math.sqrt(Kpost)
        sd[f"post_nns.{t}.0.bias"] = 0.1 * torch.randn(Fo, generator=gen)
    if ed:
        sd["edge_encoder.weight"] = torch.randn(Fi, ed, generator=gen) / math.sqrt(ed)
        sd["edge_encoder.bias"] = 0.1 * torch.randn(Fi, generator=gen)
    sd["lin.weight"] = torch.randn(C, C, generator=gen) / math.sqrt(C)
    sd["lin.bias"] = 0.1 * torch.randn(C, generator=gen)
    return sd


def _first_extremal(m, dst, V, sign):
    """max (sign 1) or min (sign -1) of the CSR-ordered messages m (E, F) per destination, 0 for a row without in-edges; the gradient goes
    to the first extremal edge."""
    E, F = m.shape
    out = torch.zeros(V, F, dtype=m.dtype)
    if E == 0:
        return out
    idx = dst[:, None].expand(-1, F)
    top = torch.full((V, F), -float("inf"), dtype=m.dtype).scatter_reduce(0, idx, sign * m.detach(), "amax")
    pos = torch.arange(E)[:, None].expand(-1, F)
    first = torch.full((V, F), E, dtype=torch.long).scatter_reduce(0, idx, torch.where(sign * m.detach() == top[dst], pos, E), "amin")
    has = first < E
    return torch.where(has, m.gather(0, first.clamp(max=E - 1)), out)


def forward(sd, meta, x, edge_index, edge_attr, parts=None):
    """PNAConv's forward on tensors of one dtype; sd values may require gradients.  parts: a dict that receives the CSR-ordered messages
    of every tower (`msg`, `msg0` = without the destination term) for the conditions."""
    T, Fi, div, ed, V = meta["towers"], meta["F_in"], meta["divide_input"], meta["edge_dim"], x.shape[0]
    order = torch.sort(edge_index[1], stable=True).indices
    src, dst = edge_index[0][order], edge_index[1][order]
    deg = torch.bincount(dst, minlength=V).to(x.dtype)[:, None]
    D = deg.clamp(min=1)
    enc = edge_attr[order] @ sd["edge_encoder.weight"].t() + sd["edge_encoder.bias"] if ed else None
    avg = meta["avg_deg"]
    outs = []
    for t in range(T):
        xt = x[:, t * Fi:(t + 1) * Fi] if div else x
        W, b = sd[f"pre_nns.{t}.0.weight"], sd[f"pre_nns.{t}.0.bias"]
        m0 = xt[src] @ W[:, Fi:2 * Fi].t() + (enc @ W[:, 2 * Fi:].t() if ed else 0.0)
        m = m0 + (xt[dst] @ W[:, :Fi].t() + b)
        if parts is not None:
            parts.setdefault("msg", []).append(m.detach())
            parts.setdefault("msg0", []).append(m0.detach())
        s = torch.zeros(V, Fi, dtype=x.dtype).index_add(0, dst, m)
        mean = s / D
        var = torch.zeros(V, Fi, dtype=x.dtype).index_add(0, dst, m * m) / D - mean * mean
        blocks = {"sum": s, "mean": mean, "var": var, "std": torch.sqrt(torch.relu(var) + 1e-5)}
        if "max" in meta["aggregators"]:
            blocks["max"] = _first_extremal(m, dst, V, 1.0)
        if "min" in meta["aggregators"]:
            blocks["min"] = -_first_extremal(-m, dst, V, 1.0)
        agg = torch.cat([blocks[n] for n in meta["aggregators"]], dim=1)
        scaled = []
        for n in meta["scalers"]:
            if n == "identity":
                f = torch.ones_like(deg)
            elif n == "amplification":
                f = torch.log(deg + 1) / avg["log"]
            elif n == "attenuation":
                f = torch.where(deg == 0, torch.ones_like(deg), avg["log"] / torch.log(deg + 1).clamp(min=1e-30))
            elif n == "linear":
                f = deg / avg["lin"]
            else:
                assert n == "inverse_linear", n
                f = torch.where(deg == 0, torch.ones_like(deg), avg["lin"] / D)
            scaled.append(agg * f)
        outs.append(torch.cat([xt] + scaled, dim=1) @ sd[f"post_nns.{t}.0.weight"].t() + sd[f"post_nns.{t}.0.bias"])
    return torch.cat(outs, dim=1) @ sd["lin.weight"].t() + sd["lin.bias"]


def step(sd, meta, a, dtype):
    """The training step in `dtype`: -> dict(out, grad_x, grad_e (None without edge features), grads {state-dict key: gradient})."""
    cast = lambda t: t.to(dtype)      # noqa: E731
    p = {k: cast(v).clone().requires_grad_(True) for k, v in sd.items()}
    x = cast(a["x"]).clone().requires_grad_(True)
    ea = cast(a["edge_attr"]).clone().requires_grad_(True) if meta["edge_dim"] else None
    out = forward(p, meta, x, a["edge_index"], ea)
    wanted = [x] + ([ea] if ea is not None else []) + list(p.values())
    got = torch.autograd.grad((out * cast(a["R"])).sum(), wanted, allow_unused=True)
    got = [torch.zeros_like(w) if g is None else g for g, w in zip(got, wanted)]
    n = 2 if ea is not None else 1
    return dict(out=out.detach(), grad_x=got[0], grad_e=got[1] if ea is not None else None, grads=dict(zip(p.keys(), got[n:])))


def ill_conditioned(sd, meta, a):
    """-> (ill destinations, nodes their gradients touch): tower_train_cases.ill_conditioned's two criteria on the PyG messages."""
    V = a["x"].shape[0]
    parts = {}
    forward({k: v.double() for k, v in sd.items()}, meta, a["x"].double(), a["edge_index"], a["edge_attr"].double(), parts)
    order = torch.sort(a["edge_index"][1], stable=True).indices
    src, dst = a["edge_index"][0][order], a["edge_index"][1][order]
    deg = torch.bincount(dst, minlength=V).clamp(min=1).double()[:, None]
    rho, ties = torch.zeros(V, dtype=torch.float64), torch.zeros(V, dtype=torch.bool)
    for m, m0 in zip(parts.get("msg", []), parts.get("msg0", [])):
        if m.shape[0] == 0:
            continue
        stds = []
        for dt in (torch.float64, torch.float32):
            z = m0.to(dt)
            m1 = torch.zeros(V, z.shape[1], dtype=dt).index_add_(0, dst, z) / deg.to(dt)
            m2 = torch.zeros(V, z.shape[1], dtype=dt).index_add_(0, dst, z * z) / deg.to(dt)
            stds.append(torch.sqrt(torch.relu(m2 - m1 * m1) + 1e-5).double())
        rho = torch.maximum(rho, ((stds[1] - stds[0]).abs() / stds[0]).max(dim=1).values)
        idx = dst[:, None].expand(-1, m.shape[1])
        for sign in (1.0, -1.0):
            top = torch.full((V, m.shape[1]), -float("inf"), dtype=torch.float64).scatter_reduce_(0, idx, sign * m, "amax")
            near = ((top[dst] - sign * m) <= 4e-7 * top[dst].abs().clamp(min=1e-30)).double()
            ties |= (torch.zeros(V, m.shape[1], dtype=torch.float64).index_add_(0, dst, near) >= 2).any(1)
    ill = (rho > 1e-4) | ties
    touched = ill.clone()
    touched[src[ill[dst]]] = True
    return ill, touched


def build(V, E, T, div, Fi, Fo, aggregators, scalers, ed, seed, name=""):
    gen = torch.Generator().manual_seed(seed)
    if E:
        src, dst = torch.randint(0, V, (E,), generator=gen), torch.randint(0, V - ISOLATED, (E,), generator=gen)
        if name == "var_neg":
            dst = 1 + dst % (V - ISOLATED - 1)                # node 0 is fed by the three equal edges below only
        key = torch.unique(src * V + dst)                     # no repeated edge (tower_train_cases._random_case)
        key = key[torch.randperm(key.numel(), generator=gen)]  # edge_index order is not CSR order
        src, dst = key // V, key % V
        if name == "var_neg":
            src, dst = torch.cat([src[:5], torch.tensor([3, 3, 3]), src[5:]]), torch.cat([dst[:5], torch.tensor([0, 0, 0]), dst[5:]])
    else:
        src = dst = torch.zeros(0, dtype=torch.long)
    ei = torch.stack([src, dst])
    in_c, C = (T * Fi if div else Fi), T * Fo
    x = torch.randn(V, in_c, generator=gen)
    ea = torch.randn(ei.shape[1], ed or 0, generator=gen)
    sd = state_dict(T, Fi, Fo, len(aggregators), len(scalers), ed, gen)
    R = torch.randn(V, C, generator=gen)
    hist, avg = avg_deg_of(dst, V)
    meta = dict(N=V, in_c=in_c, out_c=C, towers=T, divide_input=div, F_in=Fi, F_out=Fo, edge_dim=ed or 0, aggregators=list(aggregators),
                scalers=list(scalers), avg_deg=avg)
    return meta, dict(edge_index=ei, x=x, edge_attr=ea, R=R, deg_hist=hist), sd


def reference(meta, a, sd, name=""):
    r64, r32 = step(sd, meta, a, torch.float64), step(sd, meta, a, torch.float32)
    ill, touched = ill_conditioned(sd, meta, a)
    frac = float(ill.sum()) / meta["N"]
    assert frac <= 0.15, (name, frac)
    return types.SimpleNamespace(out=r64["out"], grad_x=r64["grad_x"], grad_e=r64["grad_e"], grads=r64["grads"], ref32=r32, ill=ill, touched=touched,
                                 frac=frac)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (meta, arrays, state_dict, ref) of CASES[name]."""
    meta, a, sd = build(*CASES[name], name=name)
    return meta, a, sd, reference(meta, a, sd, name)


def check_step(ref, out, grad_x, grads, grad_e=None):
    """tower_train_cases.check_step's bars: out 1e-5, grad_x 1e-4, pre_nn weights 3e-4 and every other parameter 1e-5 of the largest
    gradient entry (+ 4 x the fp32 oracle's own error where ill rows exist), ill rows at 2e-3; grad_edge_attr like grad_x."""
    n_ill = int(ref.ill.sum())
    close(out, ref.out, "out", 1e-5, n_ill, ref.ill)
    close(grad_x, ref.grad_x, "grad_x", 1e-4, n_ill, ref.touched)
    wscale = max(v.abs().max().item() for v in ref.ref32["grads"].values())
    assert set(grads) == set(ref.grads), set(grads) ^ set(ref.grads)
    for k, g in grads.items():
        pre = k.startswith("pre_nns") and k.endswith("weight")
        close(g, ref.grads[k], k, 3e-4 if pre else 1e-5, n_ill, scale=wscale, ref=ref.ref32["grads"][k])
    if ref.grad_e is not None and ref.grad_e.numel():
        close(grad_e, ref.grad_e, "grad_edge_attr", 1e-4, n_ill, scale=max(1.0, ref.grad_e.abs().max().item()), ref=ref.ref32["grad_e"])
