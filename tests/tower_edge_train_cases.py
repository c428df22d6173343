"""Shared inputs, float64 references and tolerance helpers of the one-call PNALayer training tests WITH EDGE FEATURES
(test_gpu_tower_edge_train_kernels.py, test_gpu_tower_edge_train_layers.py): pna_tower_edge_train_fwd_f32 / _bwd_f32 against
oracle.torch_oracle.dgl_layer_train_step(..., edge_features=True, ...).  Every reference is computed once per session and never modified.

A case builder asserts the two conditions of tower_train_cases: the ill-conditioned destinations (the list
tests/test_gpu_backward.py::test_tower_layer_training_step_golden derives with edge features: the std of a_u + W_e e evaluated in fp32
against float64 off by more than 1e-4 relative, or a max / min near-tie) are at most 15 % of the nodes, and no float64 mixing
pre-activation lies within 1e-5 of the largest of zero.  The list extends to the touched nodes and to the touched edges, ill[dst].  The
seeds of the random cases were picked on the CPU so the oracle alone satisfies both."""
import functools
import math
import types

import torch

from conftest import load_golden
from oracle import torch_oracle as O
from small_train_cases import hand_graph
from tower_train_cases import AGGS, SCALERS, SLOPE, check_step, close, post_w, pre_w  # noqa: F401  (re-exported to the tests)

#        name: (T, divide_input, Fi, Fo, edge_dim, nodes, edges, n_scaler, residual, seed)
RANDOM = {
    "zinc_edge_first": (5, True, 14, 14, 50, 45, 100, 3, True, 1),
    "zinc_edge_last": (5, True, 14, 12, 50, 45, 100, 3, False, 1),
    "hand": (2, True, 8, 8, 3, 40, 0, 3, True, 1),
    "ed1": (1, False, 12, 12, 1, 17, 50, 1, True, 1),                 # one tower, one scaler, edge_dim 1, E not a multiple of 16
    "ed64_fi4": (2, True, 4, 4, 64, 24, 70, 3, True, 1),              # both limits
    "fi80": (2, False, 80, 8, 5, 24, 120, 3, False, 1),               # 5 Fi + 1 > 384: the plain weight-gradient kernel
    "no_edges": (2, True, 8, 8, 3, 8, 0, 3, True, 1),                 # E = 0
    "e_no_grad": (3, False, 12, 4, 7, 17, 50, 2, True, 1),            # run with grad_e = NULL
}
GOLDEN = "tower_train_t3_edgefeat"
KERNEL_CASES = [GOLDEN] + list(RANDOM)


def _random_case(T, div, Fi, Fo, ed, nodes, edges, S, residual, seed, hand):
    gen = torch.Generator().manual_seed(seed)
    if hand:
        src, dst = hand_graph()
    elif edges == 0:
        src, dst = torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long)
    else:
        src, dst = torch.randint(0, nodes, (edges,), generator=gen), torch.randint(0, nodes, (edges,), generator=gen)
        key = torch.unique(src * nodes + dst)                 # no repeated edge (tower_train_cases: variance 0 exactly in float64)
        key = key[torch.randperm(key.numel(), generator=gen)]  # the ORIGINAL edge order is not the CSR's: eid is a real permutation
        src, dst = key // nodes, key % nodes
    E = src.numel()
    in_dim, C = (T * Fi if div else Fi), T * Fo
    h = torch.randn(nodes, in_dim, generator=gen)
    e = torch.randn(E, ed, generator=gen)
    if hand:
        h[8] = h[7]                                           # the arg tie of hand_graph(): nodes 7 and 8 both feed node 6 ...
        k7, k8 = (int(torch.nonzero((src == u) & (dst == 6))[0]) for u in (7, 8))
        e[k8] = e[k7]                                         # ... through edges with equal feature rows
        # The tie has to be exact in EVERY arithmetic, the float64 oracle's included: a library GEMM may round two equal input rows
        # differently by their position in the matrix (it did, on one host, at K = 19), and then the oracle has no tie.  With the
        # operands of these two messages on a coarse binary grid (inputs: multiples of 2^-5; pretrans weights and biases, below:
        # multiples of 2^-8) every product and every partial sum is exact in fp32 and float64, whatever the order.
        for rows, t in (((6, 7, 8), h), ((k7, k8), e)):
            t[list(rows)] = torch.round(t[list(rows)] * 32) / 32
    sd = {}
    Kp = (1 + 4 * S) * Fi
    for t in range(T):
        sd[f"towers.{t}.batchnorm_h.weight"] = 0.5 + torch.rand(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.bias"] = 0.3 * torch.randn(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.running_mean"] = 0.1 * torch.randn(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.running_var"] = 0.5 + torch.rand(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.num_batches_tracked"] = torch.tensor(3)
        sd[pre_w(t)] = torch.randn(Fi, 2 * Fi + ed, generator=gen) / math.sqrt(2 * Fi + ed)
        sd[pre_w(t)[:-6] + "bias"] = 0.1 * torch.randn(Fi, generator=gen)
        if hand:                                              # (the exact tie: see above)
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
    meta = dict(N=nodes, in_dim=in_dim, out_dim=C, towers=T, divide_input=div, edge_dim=ed, aggregators="mean max min std",
                scalers=SCALERS[S], residual=residual, graph_norm=True)
    return meta, dict(src=src, dst=dst, h=h, e=e, snorm_n=snorm, avg_log=avg_log, R=R), sd


def _step(sd, a, meta, dtype):
    """The oracle's training step with edge features in `dtype` -> (out, grad_h, grad_e, parameter gradients, running statistics); the
    oracle applies the residual whenever the widths agree -- taken out again for a case without one."""
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t   # noqa: E731
    sdd = {k: cast(v) for k, v in sd.items()}
    out, gh, ge, gp, running = O.dgl_layer_train_step(sdd, a["src"], a["dst"], meta["N"], cast(a["h"]), cast(a["e"]), cast(a["snorm_n"]), AGGS,
                                                      meta["scalers"].split(), cast(a["avg_log"]), meta["towers"], meta["divide_input"], True, cast(a["R"]))
    if not meta["residual"] and meta["in_dim"] == meta["out_dim"]:
        out, gh = out - cast(a["h"]), gh - cast(a["R"])
    # (a graph without edges: autograd never reaches the pretrans parameters or e and reports None -- their gradient is zero)
    gp = {k: (torch.zeros_like(sdd[k]) if g is None else g) for k, g in gp.items()}
    ge = torch.zeros_like(cast(a["e"])) if ge is None else ge
    return out, gh, ge, gp, running


def _widths(meta):
    T = meta["towers"]
    return T, (meta["in_dim"] // T if meta["divide_input"] else meta["in_dim"])


def _tower_z(sd, a, meta, dtype):
    """(z (V, C), mass (V, C)) of the reference's formulas in `dtype`, the pretrans on [h_u | h_v | e]."""
    T, it = _widths(meta)
    N = meta["N"]
    src, dst = a["src"].long(), a["dst"].long()
    zs, ms = [], []
    for t in range(T):
        ht = (a["h"][:, t * it:(t + 1) * it] if meta["divide_input"] else a["h"]).to(dtype)
        W, b = sd[pre_w(t)].to(dtype), sd[pre_w(t)[:-6] + "bias"].to(dtype)
        msg = torch.cat([ht[src], ht[dst], a["e"].to(dtype)], dim=1) @ W.t() + b
        agg = O.reduce_bucketed(msg, src, dst, N, AGGS, meta["scalers"].split(), a["avg_log"].to(dtype))
        Wp, c = sd[post_w(t)].to(dtype), sd[post_w(t)[:-6] + "bias"].to(dtype)
        x = torch.cat([ht, agg], dim=1)
        zs.append((x @ Wp.t() + c) * a["snorm_n"].to(dtype))
        ms.append((x.abs() @ Wp.abs().t() + c.abs()) * a["snorm_n"].to(dtype))
    return torch.cat(zs, dim=1), torch.cat(ms, dim=1)


def x_edge64(sd, a, meta):
    """(x_edge, mass) in float64 and the ORIGINAL edge order: (E, T Fi) = per tower W_e,t e and sum |w| |e|."""
    T, it = _widths(meta)
    e = a["e"].double()
    We = [sd[pre_w(t)].double()[:, 2 * it:] for t in range(T)]
    return torch.cat([e @ w.t() for w in We], dim=1), torch.cat([e.abs() @ w.abs().t() for w in We], dim=1)


def ill_conditioned(meta, a, sd):
    """test_tower_layer_training_step_golden's list with edge features: destinations whose std (of a_u + W_e e, evaluated in fp32 against
    float64) is off by more than 1e-4 relative, or whose max / min is a near-tie.  -> (ill, touched nodes, touched edges)."""
    srcl, dstl = a["src"].long(), a["dst"].long()
    N = meta["N"]
    T, it = _widths(meta)
    rho, ties = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.bool)
    deg = torch.zeros(N, dtype=torch.float64).index_add_(0, dstl, torch.ones(dstl.numel(), dtype=torch.float64)).clamp(min=1)
    for t in range(T):
        W, b = sd[pre_w(t)].double(), sd[pre_w(t)[:-6] + "bias"].double()
        ht = (a["h"][:, t * it:(t + 1) * it] if meta["divide_input"] else a["h"]).double()
        part_a = ht[srcl] @ W[:, :it].t() + a["e"].double() @ W[:, 2 * it:].t()
        stds = []
        for dt in (torch.float64, torch.float32):
            x = part_a.to(dt)
            m1 = torch.zeros(N, x.shape[1], dtype=dt).index_add_(0, dstl, x) / deg[:, None].to(dt)
            m2 = torch.zeros(N, x.shape[1], dtype=dt).index_add_(0, dstl, x * x) / deg[:, None].to(dt)
            stds.append(torch.sqrt(torch.relu(m2 - m1 * m1) + 1e-5).double())
        rho = torch.maximum(rho, ((stds[1] - stds[0]).abs() / stds[0]).max(dim=1).values)
        mfull = part_a + ht[dstl] @ W[:, it:2 * it].t() + b
        idx = dstl[:, None].expand(-1, mfull.shape[1])
        for sign in (1.0, -1.0):
            top = torch.full((N, mfull.shape[1]), -float("inf"), dtype=torch.float64).scatter_reduce_(0, idx, sign * mfull, "amax")
            near = ((top[dstl] - sign * mfull) <= 4e-7 * top[dstl].abs().clamp(min=1e-30)).double()
            ties |= (torch.zeros(N, mfull.shape[1], dtype=torch.float64).index_add_(0, dstl, near) >= 2).any(1)
    ill = (rho > 1e-4) | ties
    touched = ill.clone()
    touched[srcl[ill[dstl]]] = True
    return ill, touched, ill[dstl]


def conditions(meta, a, sd, out64):
    """(ill, touched nodes, touched edges, fraction of ill nodes, smallest |p| / largest |p| of the float64 mixing pre-activation)."""
    ill, touched, touched_edges = ill_conditioned(meta, a, sd)
    y = out64 - a["h"].double() if meta["residual"] else out64
    p = torch.where(y > 0, y, y / SLOPE)
    return ill, touched, touched_edges, float(ill.sum()) / meta["N"], (p.abs().min() / p.abs().max()).item()


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (meta, arrays, state_dict, ref): tower_train_cases.case's reference (so tower_train_cases.check_step applies to it) + grad_e in
    float64 and fp32 and the touched edges."""
    if name in RANDOM:
        T, div, Fi, Fo, ed, nodes, edges, S, residual, seed = RANDOM[name]
        meta, a, sd = _random_case(T, div, Fi, Fo, ed, nodes, edges, S, residual, seed, hand=name == "hand")
        o32, gh32, ge32, gp32, run32 = _step(sd, a, meta, torch.float32)
        ref32 = dict(out=o32, grad_h=gh32, grad_e=ge32, grads=gp32, running=run32)
    else:
        meta, a, sd = load_golden(name)
        meta = dict(meta, residual=True)
        ref32 = dict(out=a["out"], grad_h=a["grad_h"], grad_e=a["grad_e"], grads={k[5:]: v for k, v in a.items() if k.startswith("grad/")},
                     running={k[6:]: v for k, v in a.items() if k.startswith("after/")})
    out64, gh64, ge64, gp64, run64 = _step(sd, a, meta, torch.float64)
    z64, mass = _tower_z(sd, a, meta, torch.float64)
    mean64 = z64.mean(0)
    var64 = ((z64 - mean64) ** 2).mean(0)
    ill, touched, touched_edges, frac, pmin = conditions(meta, a, sd, out64)
    assert frac <= 0.15, (name, frac)
    assert pmin >= 1e-5, (name, pmin)
    ref = types.SimpleNamespace(out=out64, grad_h=gh64, grad_e=ge64, grads=gp64, running=run64, z=z64, mass=mass, mean=mean64, var=var64,
                                invstd=1.0 / torch.sqrt(var64 + 1e-5), ref32=ref32, ill=ill, touched=touched, touched_edges=touched_edges)
    return meta, a, sd, ref


def check_grad_e(ref, grad_e):
    """The golden test's bar for edge gradients: 1e-4 of the largest entry, 2e-3 on the in-edges of the ill-conditioned destinations."""
    assert tuple(grad_e.shape) == tuple(ref.grad_e.shape)
    if grad_e.numel():                                        # (a graph without edges: an empty gradient)
        close(grad_e, ref.grad_e, "grad_e", 1e-4, int(ref.ill.sum()), ref.touched_edges)
