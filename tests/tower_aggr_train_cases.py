"""Shared inputs, float64 references and tolerance helpers of the one-call PNALayer training tests FOR ANY LIST OF AGGREGATORS
(test_tower_aggr_train_host.py, test_gpu_tower_aggr_train_kernels.py, test_gpu_tower_aggr_train_layers.py): pna_tower_aggr_train_fwd_f32 /
_bwd_f32 against oracle.torch_oracle.dgl_layer_train_step(..., aggregators=<list>, ...), which takes any list.  Every reference is
computed once per session and never modified.

The bars (check_step, close, check_grad_e) and the two caps are those of tower_train_cases / tower_edge_train_cases, unchanged: a case
builder asserts that the ill-conditioned destinations (those modules' lists: the std of the source-side messages off by more than 1e-4
in fp32, or a max / min near-tie -- kept whole for every aggregator list: a superset of what a shorter list can be sensitive to) are
at most 15 % of the nodes and that no float64 mixing pre-activation lies within 1e-5 of the largest of zero.  The seeds, and the keys of
the dropout cases, were picked on the CPU so that the oracle alone meets both and the fp32 oracle passes the bars on its own
(test_tower_aggr_train_host.py runs exactly that).  The dropout cases' reference is the oracle with the mask of the key (the mask rule
of include/pna_amd.h restated in tower_drop_train_cases.host_mask; the GPU tests assert that functional.dropout_mask gives that mask)."""
import functools
import math
import types

import torch
import torch.nn.functional as Fnn

import tower_edge_train_cases as TE
import tower_train_cases as TT
from oracle import torch_oracle as O
from small_train_cases import hand_graph
from tower_drop_train_cases import host_mask, pmin_of
from tower_edge_train_cases import check_grad_e  # noqa: F401  (re-exported to the tests)
from tower_train_cases import SCALERS, SLOPE, check_step, close, conditions, post_w, pre_w  # noqa: F401  (re-exported to the tests)

CODES = {"mean": 0, "sum": 1, "max": 2, "min": 3, "std": 4, "var": 5}

#        name: (T, divide_input, Fi, Fo, nodes, edges, n_scaler, residual, list, edge_dim, seed)
RANDOM = {
    "mpnn_sum": (5, True, 22, 16, 45, 100, 1, False, "sum", 0, 1),                      # realworld_benchmark/README.md:91's widths
    "mpnn_max": (5, True, 22, 16, 45, 100, 1, False, "max", 0, 15),
    "sum_var_min": (2, False, 12, 6, 33, 90, 2, True, "sum var min", 0, 1),
    "std_only": (1, False, 20, 20, 33, 90, 3, True, "std", 0, 1),                       # row_mean required
    "var_mean": (2, True, 8, 8, 24, 60, 3, True, "var mean", 0, 1),                     # order, var's mask
    "reordered": (4, True, 6, 6, 40, 100, 3, True, "mean min max std", 0, 1),           # the list today's routes refuse
    "mean_sum_max": (3, True, 8, 8, 24, 60, 1, True, "mean sum max", 0, 1),
    # rows without in-edges, in-degree-1 rows (var exactly 0, its gradient masked), the arg tie
    "hand": (2, True, 8, 8, 40, 0, 3, True, "sum var max min", 0, 1),
    "wide": (1, False, 128, 8, 24, 100, 3, False, "min std sum max", 0, 4),             # K = 512, the plain weight-gradient kernel, a lane's second column
    "fi65_one": (1, False, 65, 8, 24, 100, 1, False, "mean", 0, 1),
    "edge3_sum": (2, True, 8, 8, 24, 60, 3, True, "sum", 3, 1),
    "edge50_max_var": (5, True, 14, 12, 45, 100, 2, False, "max var", 50, 1),
    # the bitwise comparisons against the three older entry pairs: mean max min std, three scalers
    "std_plain": (2, True, 8, 8, 24, 60, 3, True, "mean max min std", 0, 1),
    "std_edge": (2, True, 8, 8, 24, 60, 3, True, "mean max min std", 3, 1),
    "no_edges": (2, True, 8, 8, 8, 0, 3, True, "sum var", 0, 1),                        # E == 0
    "no_edges_edge": (2, True, 8, 8, 8, 0, 3, True, "max std", 3, 1),
}
KERNEL_CASES = [n for n in RANDOM if not n.startswith("std_")]
#        name: (base case, p, seed, offset)
DROP = {
    "drop_mpnn_max": ("mpnn_max", 0.2, 11, 0),
    "drop_edge3_sum": ("edge3_sum", 0.2, (3 << 32) | 7, 4096),
    "drop_std_plain": ("std_plain", 0.2, 5, 8),
    "drop_std_edge": ("std_edge", 0.2, 5, 8),
}
DROP_CASES = ["drop_mpnn_max", "drop_edge3_sum"]


def codes_of(meta):
    return [CODES[n] for n in meta["aggregators"].split()]


def _random_case(T, div, Fi, Fo, nodes, edges, S, residual, aggs, ed, seed, hand):
    gen = torch.Generator().manual_seed(seed)
    if hand:
        src, dst = hand_graph()
    elif edges == 0:
        src, dst = torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long)
    else:
        src, dst = torch.randint(0, nodes, (edges,), generator=gen), torch.randint(0, nodes, (edges,), generator=gen)
        key = torch.unique(src * nodes + dst)                 # no repeated edge (tower_train_cases: variance 0 exactly in float64)
        key = key[torch.randperm(key.numel(), generator=gen)]  # the ORIGINAL edge order is not the CSR's
        src, dst = key // nodes, key % nodes
    E, A = src.numel(), len(aggs.split())
    in_dim, C = (T * Fi if div else Fi), T * Fo
    h = torch.randn(nodes, in_dim, generator=gen)
    e = torch.randn(E, ed, generator=gen)
    if hand:
        # the arg tie of hand_graph(): nodes 7 and 8 both feed node 6; exact in EVERY arithmetic with these rows on a coarse binary grid
        # (tower_edge_train_cases explains why; the pretrans weights and biases go on a grid below)
        h[8] = h[7]
        h[[6, 7, 8]] = torch.round(h[[6, 7, 8]] * 32) / 32
    sd = {}
    Kp = (1 + A * S) * Fi
    for t in range(T):
        sd[f"towers.{t}.batchnorm_h.weight"] = 0.5 + torch.rand(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.bias"] = 0.3 * torch.randn(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.running_mean"] = 0.1 * torch.randn(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.running_var"] = 0.5 + torch.rand(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.num_batches_tracked"] = torch.tensor(3)
        sd[pre_w(t)] = torch.randn(Fi, 2 * Fi + ed, generator=gen) / math.sqrt(2 * Fi + ed)
        sd[pre_w(t)[:-6] + "bias"] = 0.1 * torch.randn(Fi, generator=gen)
        if hand:
            sd[pre_w(t)] = torch.round(sd[pre_w(t)] * 256) / 256
            sd[pre_w(t)[:-6] + "bias"] = torch.round(sd[pre_w(t)[:-6] + "bias"] * 256) / 256
        sd[post_w(t)] = torch.randn(Fo, Kp, generator=gen) / math.sqrt(Kp)
        sd[post_w(t)[:-6] + "bias"] = 0.1 * torch.randn(Fo, generator=gen)
    sd["mixing_network.linear.weight"] = torch.randn(C, C, generator=gen) / math.sqrt(C)
    sd["mixing_network.linear.bias"] = 0.1 * torch.randn(C, generator=gen)
    deg = torch.bincount(dst, minlength=nodes).double()
    avg_log = torch.log(deg + 1).mean().float() if E else torch.tensor(1.0)
    snorm = (0.15 + 0.2 * torch.rand(nodes, 1, generator=gen))
    R = torch.randn(nodes, C, generator=gen)
    meta = dict(N=nodes, in_dim=in_dim, out_dim=C, towers=T, divide_input=div, edge_dim=ed, aggregators=aggs, scalers=SCALERS[S], residual=residual,
                graph_norm=True)
    return meta, dict(src=src, dst=dst, h=h, e=e, snorm_n=snorm, avg_log=avg_log, R=R), sd


def masked_layer_forward(sd, a, meta, h, e, mask, running=None):
    """PNALayer.forward in TRAIN mode for the case's aggregator list with the towers' dropout as a given mask of factors (V, towers Fo),
    None = no dropout: oracle.tower_forward per tower, times the mask (models/dgl/pna_layer.py:75), cat, the mixing Linear + LeakyReLU
    (:141), the residual (:143-144).  Operands in the dtype of h."""
    dt = h.dtype
    T, div, edge = meta["towers"], meta["divide_input"], meta["edge_dim"] > 0
    it = meta["in_dim"] // T if div else meta["in_dim"]
    running = {} if running is None else running
    outs = [O.tower_forward(sd, f"towers.{t}", a["src"], a["dst"], meta["N"], h[:, t * it:(t + 1) * it] if div else h, e, a["snorm_n"].to(dt),
                            meta["aggregators"].split(), meta["scalers"].split(), a["avg_log"].to(dt), True, True, edge, running=running) for t in range(T)]
    h_cat = torch.cat(outs, dim=1)
    if mask is not None:
        h_cat = h_cat * mask.to(dt)
    out = Fnn.leaky_relu(Fnn.linear(h_cat, sd["mixing_network.linear.weight"], sd["mixing_network.linear.bias"]), SLOPE)
    return h + out if (meta["residual"] and meta["in_dim"] == meta["out_dim"]) else out


def _step(sd, a, meta, dtype, mask=None):
    """The oracle's training step in `dtype` for the case's list -> (out, grad_h, grad_e or None, parameter gradients, running statistics):
    without a mask oracle.dgl_layer_train_step itself (the residual it applies whenever the widths agree taken out again for a case
    without one), with a mask the same step through masked_layer_forward."""
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t   # noqa: E731
    edge = meta["edge_dim"] > 0
    sdd = {k: cast(v) for k, v in sd.items()}
    if mask is None:
        out, gh, ge, gp, running = O.dgl_layer_train_step(sdd, a["src"], a["dst"], meta["N"], cast(a["h"]), cast(a["e"]), cast(a["snorm_n"]),
                                                          meta["aggregators"].split(), meta["scalers"].split(), cast(a["avg_log"]), meta["towers"],
                                                          meta["divide_input"], edge, cast(a["R"]))
        if not meta["residual"] and meta["in_dim"] == meta["out_dim"]:
            out, gh = out - cast(a["h"]), gh - cast(a["R"])
    else:
        params = {k: v.clone().requires_grad_(True) for k, v in sdd.items() if v.is_floating_point() and "running" not in k}
        live = dict(sdd)
        live.update(params)
        h = cast(a["h"]).clone().requires_grad_(True)
        e = cast(a["e"]).clone().requires_grad_(True) if edge else cast(a["e"])
        running = {}
        out = masked_layer_forward(live, a, meta, h, e, mask, running)
        (out * cast(a["R"])).sum().backward()
        out, gh, ge, gp = out.detach(), h.grad, (e.grad if edge else None), {k: v.grad for k, v in params.items()}
    # (a graph without edges: autograd never reaches the pretrans parameters or e and reports None -- their gradient is zero)
    gp = {k: (torch.zeros_like(sdd[k]) if g is None else g) for k, g in gp.items()}
    if edge:
        ge = torch.zeros_like(cast(a["e"])) if ge is None else ge
    return out, gh, (ge if edge else None), gp, running


def _tower_z(sd, a, meta, dtype):
    """(z (V, C), mass (V, C)) -- the BatchNorms' input (c_t + W_post,t [h_t | scaled aggregate]) snorm_n and the bar's mass
    sum |w| |operand| -- of the reference's formulas in `dtype` for the case's list."""
    T, N, ed = meta["towers"], meta["N"], meta["edge_dim"]
    it = meta["in_dim"] // T if meta["divide_input"] else meta["in_dim"]
    src, dst = a["src"].long(), a["dst"].long()
    zs, ms = [], []
    for t in range(T):
        ht = (a["h"][:, t * it:(t + 1) * it] if meta["divide_input"] else a["h"]).to(dtype)
        W, b = sd[pre_w(t)].to(dtype), sd[pre_w(t)[:-6] + "bias"].to(dtype)
        msg = torch.cat([ht[src], ht[dst]] + ([a["e"].to(dtype)] if ed else []), dim=1) @ W.t() + b
        agg = O.reduce_bucketed(msg, src, dst, N, meta["aggregators"].split(), meta["scalers"].split(), a["avg_log"].to(dtype))
        Wp, c = sd[post_w(t)].to(dtype), sd[post_w(t)[:-6] + "bias"].to(dtype)
        x = torch.cat([ht, agg], dim=1)
        zs.append((x @ Wp.t() + c) * a["snorm_n"].to(dtype))
        ms.append((x.abs() @ Wp.abs().t() + c.abs()) * a["snorm_n"].to(dtype))
    return torch.cat(zs, dim=1), torch.cat(ms, dim=1)


def build(name, seed=None):
    """(meta, arrays, state_dict) of RANDOM[name], under `seed` instead of the table's when given (the CPU pick)."""
    *shape, seed0 = RANDOM[name]
    return _random_case(*shape, seed0 if seed is None else seed, hand=name == "hand")


def reference(meta, a, sd, mask=None):
    """-> (ref, fraction of ill-conditioned nodes, smallest |p| / largest |p|): the float64 step (under `mask`), z and its mass, the batch
    statistics, the fp32 step the bars measure conditioning with, the ill-conditioned lists."""
    out64, gh64, ge64, gp64, run64 = _step(sd, a, meta, torch.float64, mask)
    o32, gh32, ge32, gp32, run32 = _step(sd, a, meta, torch.float32, mask)
    z64, mass = _tower_z(sd, a, meta, torch.float64)
    mean64 = z64.mean(0)
    var64 = ((z64 - mean64) ** 2).mean(0)
    if meta["edge_dim"]:
        ill, touched, touched_edges = TE.ill_conditioned(meta, a, sd)
    else:
        (ill, touched), touched_edges = TT.ill_conditioned(meta, a, sd), None
    ref = types.SimpleNamespace(out=out64, grad_h=gh64, grad_e=ge64, grads=gp64, running=run64, z=z64, mass=mass, mean=mean64, var=var64,
                                invstd=1.0 / torch.sqrt(var64 + 1e-5), ill=ill, touched=touched, touched_edges=touched_edges, mask=mask,
                                ref32=dict(out=o32, grad_h=gh32, grad_e=ge32, grads=gp32, running=run32))
    return ref, float(ill.sum()) / meta["N"], pmin_of(out64, a, meta)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (meta, arrays, state_dict, ref, key): RANDOM[name] with key None, or DROP[name] = its base case under the mask of key =
    (p, seed, offset).  Asserts the two caps."""
    key = None
    if name in DROP:
        base, *key = DROP[name]
        key = tuple(key)
        meta, a, sd = build(base)
        mask = torch.from_numpy(host_mask(meta["N"], meta["out_dim"], *key))
    else:
        meta, a, sd = build(name)
        mask = None
    ref, frac, pmin = reference(meta, a, sd, mask)
    assert frac <= 0.15, (name, frac)
    assert pmin >= 1e-5, (name, pmin)
    return meta, a, sd, ref, key
