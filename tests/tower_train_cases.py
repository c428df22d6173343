"""Shared inputs, float64 references and tolerance helpers of the one-call PNALayer training tests (test_gpu_tower_train_kernels.py,
test_gpu_tower_train_layers.py): pna_tower_train_fwd_f32 / pna_tower_train_bwd_f32 against oracle.torch_oracle.dgl_layer_train_step.
Every reference is computed once per session and never modified.

A case builder asserts the two conditions that keep a comparison against float64 meaningful: the ill-conditioned destinations (the list
tests/test_gpu_backward.py::test_tower_layer_training_step_golden derives: std off by > 1e-4 in fp32, or a max / min near-tie) are at
most 15 % of the nodes, and no float64 mixing pre-activation lies within 1e-5 of the largest of zero (a LeakyReLU sign decided by
rounding moves gradients by O(1)).  The seeds of the random cases were picked on the CPU so the oracle alone satisfies both."""
import functools
import math
import types

import torch

from conftest import load_golden
from oracle import torch_oracle as O
from small_train_cases import hand_graph

AGGS = ["mean", "max", "min", "std"]
SCALERS = {1: "identity", 2: "identity amplification", 3: "identity amplification attenuation"}
SLOPE = 0.01

#        name: (T, divide_input, Fi, Fo, nodes, edges, n_scaler, residual, seed)
RANDOM = {
    "zinc_first": (5, False, 75, 15, 45, 100, 3, True, 6),
    "zinc_last": (5, True, 15, 14, 45, 100, 3, False, 2),
    "hand_res": (2, True, 8, 8, 40, 0, 3, True, 1),
    "hand_nores": (2, True, 8, 8, 40, 0, 3, False, 1),
    "one_tower": (1, False, 20, 20, 33, 90, 1, True, 1),
    "two_scalers": (3, False, 12, 4, 17, 50, 2, True, 1),
    "wide": (8, True, 16, 16, 33, 100, 3, True, 1),
    # the two shapes outside pna_posttrans_dw_f32's limits: the plain weight-gradient kernel (5 Fi + 1 > 384; n_scaler Fo > 240)
    "fi80": (2, False, 80, 8, 24, 120, 3, False, 1),
    "fo96": (1, False, 8, 96, 24, 100, 3, False, 1),
}
KERNEL_CASES = ["tower_train_t4_div"] + list(RANDOM)


def pre_w(t):
    return f"towers.{t}.pretrans.fully_connected.0.linear.weight"


def post_w(t):
    return f"towers.{t}.posttrans.fully_connected.0.linear.weight"


def _random_case(T, div, Fi, Fo, nodes, edges, S, residual, seed, hand):
    gen = torch.Generator().manual_seed(seed)
    if hand:
        src, dst = hand_graph()
    else:
        src, dst = torch.randint(0, nodes, (edges,), generator=gen), torch.randint(0, nodes, (edges,), generator=gen)
        key = torch.unique(src * nodes + dst)                 # no repeated edge: a destination fed twice by one source has variance 0 exactly
        src, dst = key // nodes, key % nodes                  # in float64 and rounding noise in fp32 -- ill-conditioned by construction
    in_dim, C = (T * Fi if div else Fi), T * Fo
    h = torch.randn(nodes, in_dim, generator=gen)
    if hand:
        h[8] = h[7]                                           # the arg tie of hand_graph(): nodes 7 and 8 both feed node 6
    sd = {}
    Kp = (1 + 4 * S) * Fi
    for t in range(T):
        sd[f"towers.{t}.batchnorm_h.weight"] = 0.5 + torch.rand(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.bias"] = 0.3 * torch.randn(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.running_mean"] = 0.1 * torch.randn(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.running_var"] = 0.5 + torch.rand(Fo, generator=gen)
        sd[f"towers.{t}.batchnorm_h.num_batches_tracked"] = torch.tensor(3)
        sd[pre_w(t)] = torch.randn(Fi, 2 * Fi, generator=gen) / math.sqrt(2 * Fi)
        sd[pre_w(t)[:-6] + "bias"] = 0.1 * torch.randn(Fi, generator=gen)
        sd[post_w(t)] = torch.randn(Fo, Kp, generator=gen) / math.sqrt(Kp)
        sd[post_w(t)[:-6] + "bias"] = 0.1 * torch.randn(Fo, generator=gen)
    sd["mixing_network.linear.weight"] = torch.randn(C, C, generator=gen) / math.sqrt(C)
    sd["mixing_network.linear.bias"] = 0.1 * torch.randn(C, generator=gen)
    deg = torch.bincount(dst, minlength=nodes).double()
    avg_log = torch.log(deg + 1).mean().float()
    snorm = (0.15 + 0.2 * torch.rand(nodes, 1, generator=gen))
    R = torch.randn(nodes, C, generator=gen)
    meta = dict(N=nodes, in_dim=in_dim, out_dim=C, towers=T, divide_input=div, edge_dim=0, aggregators="mean max min std",
                scalers=SCALERS[S], residual=residual, graph_norm=True)
    return meta, dict(src=src, dst=dst, h=h, e=torch.zeros(src.numel(), 0), snorm_n=snorm, avg_log=avg_log, R=R), sd


def _step(sd, a, meta, dtype):
    """The oracle's training step in `dtype`; the oracle applies the residual whenever the widths agree -- taken out again for a case
    without one (out - h, grad_h - R: the residual is one addition each way)."""
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t   # noqa: E731
    sdd = {k: cast(v) for k, v in sd.items()}
    out, gh, _, gp, running = O.dgl_layer_train_step(sdd, a["src"], a["dst"], meta["N"], cast(a["h"]), cast(a["e"]), cast(a["snorm_n"]), AGGS,
                                                     meta["scalers"].split(), cast(a["avg_log"]), meta["towers"], meta["divide_input"], False, cast(a["R"]))
    if not meta["residual"] and meta["in_dim"] == meta["out_dim"]:
        out, gh = out - cast(a["h"]), gh - cast(a["R"])
    return out, gh, gp, running


def _tower_z(sd, a, meta, dtype):
    """(z (V, C), mass (V, C)) -- the BatchNorms' input (c_t + W_post,t [h_t | scaled aggregate]) snorm_n and the bar's mass
    sum |w| |operand| -- of the reference's formulas in `dtype`."""
    T, N = meta["towers"], meta["N"]
    it = meta["in_dim"] // T if meta["divide_input"] else meta["in_dim"]
    src, dst = a["src"].long(), a["dst"].long()
    zs, ms = [], []
    for t in range(T):
        ht = (a["h"][:, t * it:(t + 1) * it] if meta["divide_input"] else a["h"]).to(dtype)
        W, b = sd[pre_w(t)].to(dtype), sd[pre_w(t)[:-6] + "bias"].to(dtype)
        msg = torch.cat([ht[src], ht[dst]], dim=1) @ W.t() + b
        agg = O.reduce_bucketed(msg, src, dst, N, AGGS, meta["scalers"].split(), a["avg_log"].to(dtype))
        Wp, c = sd[post_w(t)].to(dtype), sd[post_w(t)[:-6] + "bias"].to(dtype)
        x = torch.cat([ht, agg], dim=1)
        zs.append((x @ Wp.t() + c) * a["snorm_n"].to(dtype))
        ms.append((x.abs() @ Wp.abs().t() + c.abs()) * a["snorm_n"].to(dtype))
    return torch.cat(zs, dim=1), torch.cat(ms, dim=1)


def ill_conditioned(meta, a, sd):
    """test_tower_layer_training_step_golden's list: destinations whose std (of the source-side messages, evaluated in fp32 against
    float64) is off by more than 1e-4 relative, or whose max / min is a near-tie.  -> (ill, touched_nodes)."""
    srcl, dstl = a["src"].long(), a["dst"].long()
    N, T = meta["N"], meta["towers"]
    it = meta["in_dim"] // T if meta["divide_input"] else meta["in_dim"]
    rho, ties = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.bool)
    deg = torch.zeros(N, dtype=torch.float64).index_add_(0, dstl, torch.ones(dstl.numel(), dtype=torch.float64)).clamp(min=1)
    for t in range(T):
        W, b = sd[pre_w(t)].double(), sd[pre_w(t)[:-6] + "bias"].double()
        ht = (a["h"][:, t * it:(t + 1) * it] if meta["divide_input"] else a["h"]).double()
        part_a = ht[srcl] @ W[:, :it].t()
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
    return ill, touched


def conditions(meta, a, sd, out64):
    """(ill, touched nodes, fraction of ill nodes, smallest |p| / largest |p| of the float64 mixing pre-activation)."""
    ill, touched = ill_conditioned(meta, a, sd)
    y = out64 - a["h"].double() if meta["residual"] else out64
    p = torch.where(y > 0, y, y / SLOPE)
    return ill, touched, float(ill.sum()) / meta["N"], (p.abs().min() / p.abs().max()).item()


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (meta, arrays, state_dict, ref): ref holds the float64 step (out, grad_h, parameter gradients, running statistics, z of the
    BatchNorms' input and its mass, the batch statistics), the fp32 step the bars measure conditioning with (the reference's own golden
    values where the case is a golden fixture, the oracle evaluated in fp32 otherwise) and the ill-conditioned lists."""
    if name in RANDOM:
        T, div, Fi, Fo, nodes, edges, S, residual, seed = RANDOM[name]
        meta, a, sd = _random_case(T, div, Fi, Fo, nodes, edges, S, residual, seed, hand=name.startswith("hand"))
        o32, gh32, gp32, run32 = _step(sd, a, meta, torch.float32)
        ref32 = dict(out=o32, grad_h=gh32, grads=gp32, running=run32)
    else:
        meta, a, sd = load_golden(name)
        ref32 = dict(out=a["out"], grad_h=a["grad_h"], grads={k[5:]: v for k, v in a.items() if k.startswith("grad/")},
                     running={k[6:]: v for k, v in a.items() if k.startswith("after/")})
    out64, gh64, gp64, run64 = _step(sd, a, meta, torch.float64)
    z64, mass = _tower_z(sd, a, meta, torch.float64)
    z32, _ = _tower_z(sd, a, meta, torch.float32)
    mean64 = z64.mean(0)
    var64 = ((z64 - mean64) ** 2).mean(0)
    ill, touched, frac, pmin = conditions(meta, a, sd, out64)
    assert frac <= 0.15, (name, frac)
    assert pmin >= 1e-5, (name, pmin)
    ref = types.SimpleNamespace(out=out64, grad_h=gh64, grads=gp64, running=run64, z=z64, z32=z32.double(), mass=mass, mean=mean64, var=var64,
                                invstd=1.0 / torch.sqrt(var64 + 1e-5), ref32=ref32, ill=ill, touched=touched)
    return meta, a, sd, ref


def close(got, exact, what, base, n_ill, loose_rows=None, scale=None, ref=None):
    """The per-element bar of test_tower_layer_training_step_golden: `base` x the largest entry (+ 4 x the fp32 reference's own error on
    the tensor for parameter tensors when the ill-conditioned list is non-empty), the listed rows held to 2e-3."""
    diff, scale = (got.double().cpu() - exact).abs(), scale or max(1.0, exact.abs().max().item())
    tol = torch.full_like(diff, base * scale)
    if ref is not None:
        tol = tol + (4.0 * (ref.double() - exact).abs().max() if n_ill else 0.0)
    if loose_rows is not None and bool(loose_rows.any()):
        assert diff[loose_rows].max().item() <= 2e-3 * scale, (what, "loose rows", diff[loose_rows].max().item())
        diff, tol = diff[~loose_rows], tol[~loose_rows]
    print(f"[tower_train] {what}: max err / tol = {(diff / tol).max().item() if diff.numel() else 0.0:.3f}")
    assert not bool((diff > tol).any()), (what, int((diff > tol).sum()), (diff / tol).max().item(), n_ill)


def check_step(meta, ref, out, grad_h, grads, running=None):
    """out, grad_h, {state-dict key: gradient} and (optionally) {buffer key: running statistic} against the float64 step."""
    n_ill = int(ref.ill.sum())
    close(out, ref.out, "out", 1e-5, n_ill, ref.ill)
    close(grad_h, ref.grad_h, "grad_h", 1e-4, n_ill, ref.touched)
    wscale = max(v.abs().max().item() for v in ref.ref32["grads"].values())
    assert set(grads) == set(ref.grads), set(grads) ^ set(ref.grads)
    for k, g in grads.items():
        pre = "pretrans" in k and k.endswith("weight")
        close(g, ref.grads[k], k, 3e-4 if pre else 1e-5, n_ill, scale=wscale, ref=ref.ref32["grads"][k])
    for k, b in (running or {}).items():
        torch.testing.assert_close(b.cpu(), ref.ref32["running"][k], rtol=1e-5, atol=1e-6)
