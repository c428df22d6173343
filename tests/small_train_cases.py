"""Shared inputs, float64 references and tolerance helpers of the one-call training tests (test_gpu_small_train_kernels.py,
test_gpu_small_train_layers.py): pna_simple_train_fwd_f32 / pna_simple_train_bwd_f32 against oracle.torch_oracle.  Every reference is
computed once per session and never modified."""
import functools
import math
import types

import torch

from conftest import load_golden
from oracle import torch_oracle as O

AGGS = ["mean", "max", "min", "std"]
SCALERS = {1: ["identity"], 2: ["identity", "amplification"], 3: ["identity", "amplification", "attenuation"]}
W_KEY, B_KEY = "posttrans.fully_connected.0.linear.weight", "posttrans.fully_connected.0.linear.bias"


def _random_graph(nodes, edges, gen):
    src = torch.randint(0, nodes, (edges,), generator=gen)
    dst = torch.randint(0, nodes, (edges,), generator=gen)
    return src, dst


def hand_graph():
    """40 nodes: node 0 has no in-edges (but out-edges); nodes 1..5 have exactly one in-edge, and node 30's only out-edge is the one into
    node 1; node 6 has the two in-neighbours 7 and 8, whose feature rows are made identical (an arg tie: the earlier edge 7 -> 6 wins); every
    other node has 2..6 in-edges."""
    gen = torch.Generator().manual_seed(40)
    src, dst = [30, 0, 0, 9, 10], [1, 2, 3, 4, 5]
    src += [7, 8]
    dst += [6, 6]
    for v in range(7, 40):
        d = int(torch.randint(2, 7, (1,), generator=gen))
        for u in torch.randint(0, 30, (d,), generator=gen).tolist():     # (never from node 30: its single out-edge stays single)
            src.append(u)
            dst.append(v)
    return torch.tensor(src), torch.tensor(dst)


def _random_case(F, N, S, nodes, edges, seed, residual, graph=None, tie=None):
    gen = torch.Generator().manual_seed(seed)
    src, dst = graph if graph is not None else _random_graph(nodes, edges, gen)
    h = torch.randn(nodes, F, generator=gen)
    if tie is not None:
        h[tie[1]] = h[tie[0]]
    K = 4 * F * S
    sd = {"batchnorm_h.weight": 0.5 + torch.rand(N, generator=gen), "batchnorm_h.bias": 0.3 * torch.randn(N, generator=gen),
          "batchnorm_h.running_mean": 0.1 * torch.randn(N, generator=gen), "batchnorm_h.running_var": 0.5 + torch.rand(N, generator=gen),
          "batchnorm_h.num_batches_tracked": torch.tensor(3),
          W_KEY: torch.randn(N, K, generator=gen) / math.sqrt(K), B_KEY: 0.1 * torch.randn(N, generator=gen)}
    deg = torch.bincount(dst, minlength=nodes).double()
    avg_log = torch.log(deg + 1).mean().float()
    R = torch.randn(nodes, N, generator=gen)
    meta = dict(N=nodes, F=F, out_dim=N, aggregators="mean max min std", scalers=" ".join(SCALERS[S]), residual=residual)
    return meta, dict(src=src, dst=dst, h=h, avg_log=avg_log, R=R), sd


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (meta, arrays, state_dict, ref): ref holds the float64 step (out, grad_h, parameter gradients, running statistics, pre-ReLU
    values, z of the Linear, the identity-scaled aggregate, the bar's mass sum |w a|) and the fp32 step the bar measures conditioning with
    (the reference's own golden values where the case is a golden fixture, the oracle evaluated in fp32 otherwise)."""
    if name.startswith("simple_train_"):
        meta, a, sd = load_golden(name)
        ref32 = dict(out=a["out"], grad_h=a["grad_h"], grads={k[5:]: v for k, v in a.items() if k.startswith("grad/")})
    else:
        meta, a, sd = {
            "narrow": lambda: _random_case(4, 1, 1, 17, 60, 3, False),
            "wide": lambda: _random_case(128, 128, 3, 33, 150, 5, True),
            "hand_res": lambda: _random_case(8, 8, 3, 40, 0, 11, True, graph=hand_graph(), tie=(7, 8)),
            "hand_nores": lambda: _random_case(8, 8, 3, 40, 0, 11, False, graph=hand_graph(), tie=(7, 8)),
        }[name]()
        o32, gh32, gp32, _, _ = O.simple_layer_train_step(sd, a["src"], a["dst"], meta["N"], a["h"], AGGS, meta["scalers"].split(), a["avg_log"],
                                                          a["R"], residual=meta["residual"])
        ref32 = dict(out=o32, grad_h=gh32, grads=gp32)
    scalers = meta["scalers"].split()
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    out64, gh64, gp64, rm64, rv64, pre64 = O.simple_layer_train_step(sd64, a["src"], a["dst"], meta["N"], a["h"].double(), AGGS, scalers,
                                                                      a["avg_log"].double(), a["R"].double(), residual=meta["residual"],
                                                                      return_pre_relu=True)
    h64 = a["h"].double()
    agg_s = O.reduce_bucketed(h64[a["src"].long()], a["src"], a["dst"], meta["N"], AGGS, scalers, a["avg_log"].double())
    agg_i = O.reduce_bucketed(h64[a["src"].long()], a["src"], a["dst"], meta["N"], AGGS, ["identity"], a["avg_log"].double())
    z64 = agg_s @ sd64[W_KEY].t() + sd64[B_KEY]
    mass = agg_s.abs() @ sd64[W_KEY].abs().t() + sd64[B_KEY].abs()
    mean64 = z64.mean(0)
    invstd64 = 1.0 / torch.sqrt(((z64 - mean64) ** 2).mean(0) + 1e-5)
    ref = types.SimpleNamespace(out=out64, grad_h=gh64, grads=gp64, rm=rm64, rv=rv64, pre=pre64, z=z64, a=agg_i, mass=mass, mean=mean64,
                                invstd=invstd64, ref32=ref32)
    return meta, a, sd, ref


def risk_of(meta, a, ref):
    """The ReLU-flip exclusion of tests/test_gpu_backward.py::test_simple_layer_training_step_golden: (risk columns, rows of h a flip can
    reach, number of pre-ReLU values within 1e-5 of zero) -- with the same cap on that number."""
    z64 = ref.pre
    risk = z64.abs() < 1e-5 * max(1.0, z64.abs().max().item())
    risk_nodes = risk.any(1)
    nb = torch.zeros(meta["N"], dtype=torch.bool)
    nb[a["src"].long()[risk_nodes[a["dst"].long()]]] = True
    n_risk = int(risk.sum())
    assert n_risk <= max(2, 2e-4 * risk.numel()), f"{n_risk} pre-ReLU values within 1e-5 of zero: the case is degenerate"
    return risk.any(0), risk_nodes | nb, n_risk


def close(got, ref32, ref64, what, exclude_rows=None, n_risk=0):
    """The per-element bar of that test: 1e-5 |ref64| + 4 x the fp32 reference's own error on the element's row + 2e-6 x the tensor's
    largest entry; excluded entries keep 1e-4 of the largest entry against the fp32 reference."""
    got, ref32 = got.double().cpu(), ref32.double()
    ref_err = (ref32 - ref64).abs()
    ref_err = ref_err.max(dim=1, keepdim=True).values if ref_err.dim() == 2 else ref_err
    tol = 1e-5 * ref64.abs() + 4.0 * ref_err + 2e-6 * ref64.abs().max().clamp(min=1e-30)
    err = (got - ref64).abs()
    print(f"[small_train] {what}: max err / tol = {(err / tol).max().item():.3f}, max err = {err.max().item():.3e}")
    bad = err > tol
    if exclude_rows is not None and bool(exclude_rows.any()):
        bad[exclude_rows] = False
        assert ((got - ref32).abs()[exclude_rows].max().item() <= 1e-4 * max(1.0, ref32.abs().max().item())), what
    assert not bool(bad.any()), (what, int(bad.sum()), (err / tol).max().item(), n_risk)


def check_gradients(meta, a, ref, grad_h, grads):
    """grads: {state-dict key: gradient} of the four parameters."""
    risk_cols, risk_rows_h, n_risk = risk_of(meta, a, ref)
    close(grad_h, ref.ref32["grad_h"], ref.grad_h, "grad_h", risk_rows_h, n_risk)
    for k, g in grads.items():
        if k == B_KEY:
            # (in front of a batch-statistics BatchNorm the bias's true gradient is 0: bound by the weight gradient's noise level)
            wmax = ref.grads[W_KEY].abs().max().item()
            print(f"[small_train] grad bias: max {g.abs().max().item():.3e}, bar {1e-4 * wmax:.3e}")
            assert g.abs().max().item() <= 1e-4 * wmax, k
            continue
        excl = risk_cols if g.dim() <= 2 and g.shape[0] == risk_cols.numel() else None
        close(g, ref.ref32["grads"][k], ref.grads[k], k, excl, n_risk)
