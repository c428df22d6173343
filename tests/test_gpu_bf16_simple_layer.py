"""bf16 inference of PNASimpleLayer (pna_bf16_gather.hip: pna_segreduce_fwd_bf16, pna_bf16_contract.hip: pna_posttrans_bf16) against the accuracy contract.

The reference value is the layer evaluated in float64 on the exact bf16 values of the features and of every parameter
(oracle/torch_oracle.py).  With u = 2^-8 and z the scaled aggregates, per output element of a one-layer posttrans:

    |got - ref64| <= 2u |ref64| + 4u M_j,
    M_j = |gamma_j| / sqrt(var_j + eps) (sum_k |W_jk| (|z_k| + phi_k) + |b_j| + |mu_j|) + |beta_j| + |h_j| [residual]

phi_k = the fp32 statistics floor of conftest.check_blocks (0 for max / min).  Two posttrans layers: the masses propagate
through both, with 8u.  Accumulating over the edges in bf16 breaks this bar on a hub row (shown in test_hub_row_and_empty_rows)."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden, mass_stats
from oracle import torch_oracle as O
from pna_amd import ops
from pna_amd.dgl.pna_layer import PNASimpleLayer
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu

U = 2.0 ** -8
C_EPS = 2e-6           # conftest.check_blocks
GOLDEN = ["simple_f75", "simple_f20_order", "simple_f33_post2", "simple_f80_hiv", "simple_f16_default_init",
          "groups_f75", "groups_f96_two_scalers", "groups_f128", "groups_f64_n72"]


def _f64(t):
    return t.detach().float().cpu().double()


def _sd64(layer):
    return {k: (_f64(v) if v.is_floating_point() else v.cpu()) for k, v in layer.state_dict().items()}


def _scale64(name, D, avg_log):
    D = D.astype(np.float64)
    with np.errstate(divide="ignore"):
        if name == "identity":
            return np.ones_like(D)
        if name == "amplification":
            return np.log(D + 1) / avg_log
        return np.where(D > 0, avg_log / np.log(D + 1), 0.0)


def reference(layer, src, dst, N, h_bf, rows=None, z_override=None):
    """(ref64 (R, out), tolerance (R, out), z64 (R, A*S*F)) of the bf16 layer on destination rows `rows` (all when None): float64
    on the exact bf16 values.  z_override replaces the float64 aggregate (to push an emulated aggregate through the same layer)."""
    src = torch.as_tensor(src).long().cpu()
    dst = torch.as_tensor(dst).long().cpu()
    if rows is None:
        rows = torch.arange(N)
    rows = torch.as_tensor(rows).long()
    local = torch.full((N,), -1, dtype=torch.long)
    local[rows] = torch.arange(rows.numel())
    keep = local[dst] >= 0
    s_sub, d_sub = src[keep], local[dst[keep]]
    R = rows.numel()
    h64 = _f64(h_bf)
    sd = _sd64(layer)
    avg_log = float(layer.avg_d["log"])
    aggs, scalers, F = layer.aggregators, layer.scalers, layer.in_dim
    z = O.reduce_bucketed(h64[s_sub], s_sub, d_sub, R, aggs, scalers, torch.tensor(avg_log, dtype=torch.float64))
    if z_override is not None:
        z = z_override
    # phi: the fp32 statistics floor of every aggregate column (scaled like the column)
    rp, order, deg = O.csr_by_dst(s_sub, d_sub, R)
    msgs = h64[s_sub[order]].numpy()
    m1, m2, w = mass_stats(rp.numpy(), msgs)
    s1 = np.zeros_like(m1)
    nz = (rp[1:] > rp[:-1]).numpy()
    if len(msgs):
        s1[nz] = np.add.reduceat(msgs, rp[:-1].numpy()[nz], axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_abs = m1 / w
        f_var = C_EPS * (m2 / w + 2 * mean_abs * mean_abs)
        std64 = np.sqrt(np.maximum(m2 / w - (s1 / w) ** 2, 0) + 1e-5)
        floors = {"sum": C_EPS * m1, "mean": C_EPS * mean_abs, "var": f_var, "std": f_var / (2 * np.maximum(std64, np.sqrt(1e-5))),
                  "max": np.zeros_like(m1), "min": np.zeros_like(m1)}
    floors = {k: np.nan_to_num(v, nan=0.0, posinf=0.0) for k, v in floors.items()}
    D = deg.numpy()
    phi = np.concatenate([np.abs(_scale64(s, D, avg_log))[:, None] * floors[a] for s in scalers for a in aggs], axis=1)
    mass = np.abs(z.numpy()) + phi
    x = z
    k = 0
    while f"posttrans.fully_connected.{k}.linear.weight" in sd:
        k += 1
    for i in range(k):
        W, b = sd[f"posttrans.fully_connected.{i}.linear.weight"], sd[f"posttrans.fully_connected.{i}.linear.bias"]
        x = torch.nn.functional.linear(x, W, b)
        if i < k - 1:
            x = torch.relu(x)
        mass = mass @ np.abs(W.numpy()).T + np.abs(b.numpy())
    if layer.batch_norm:
        g, beta = sd["batchnorm_h.weight"].numpy(), sd["batchnorm_h.bias"].numpy()
        mu, var = sd["batchnorm_h.running_mean"].numpy(), sd["batchnorm_h.running_var"].numpy()
        x = O.batchnorm_eval(sd, "batchnorm_h", x)
        mass = np.abs(g) / np.sqrt(var + 1e-5) * (mass + np.abs(mu)) + np.abs(beta)
    x = torch.relu(x)
    if layer.residual:
        x = h64[rows] + x
        mass = mass + np.abs(h64[rows].numpy())
    ref = x.numpy()
    tol = 2 * U * np.abs(ref) + (4 if k == 1 else 8) * U * mass
    return ref, tol, z.numpy()


def assert_contract(got, ref, tol, what):
    got = got.float().cpu().double().numpy()
    err = np.abs(got - ref)
    bad = ~(err <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the contract, worst err {err[bad].max():.3e} at {np.argwhere(bad)[:3]}"


def make_layer(F, out_dim, aggs, scalers, avg_log, bn, res, layers=1, seed=0, device="cuda"):
    torch.manual_seed(seed)
    layer = PNASimpleLayer(F, out_dim, aggs, scalers, {"log": torch.tensor(avg_log)}, 0.0, bn, res, posttrans_layers=layers)
    with torch.no_grad():
        for fc in layer.posttrans.fully_connected:
            fc.linear.bias.uniform_(-0.5, 0.5)
        b = layer.batchnorm_h
        b.weight.uniform_(0.5, 1.5)
        b.bias.uniform_(-0.5, 0.5)
        b.running_mean.uniform_(-0.3, 0.3)
        b.running_var.uniform_(0.5, 2.0)
    return layer.to(device).eval().to(torch.bfloat16)


def run(layer, g, h):
    with torch.no_grad():
        return layer(g, h)


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_fixtures_in_bf16(cuda_device, name):
    meta, a, sd = load_golden(name)
    layer = PNASimpleLayer(meta["F"], meta["out_dim"], meta["aggregators"], meta["scalers"], {"log": a["avg_log"]}, 0.0,
                           meta["batch_norm"], meta["residual"], posttrans_layers=meta["posttrans_layers"])
    layer.load_state_dict(sd)
    layer = layer.to(cuda_device).eval().to(torch.bfloat16)
    g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
    h = a["h"].to(cuda_device).to(torch.bfloat16)
    with torch.no_grad():
        assert layer._bf16_path(g, h)
    out = run(layer, g, h)
    assert out.dtype == torch.bfloat16 and out.shape == (meta["N"], meta["out_dim"])
    ref, tol, _ = reference(layer, a["src"], a["dst"], meta["N"], h)
    assert_contract(out, ref, tol, name)


def _random_graph(V, E, n_hubs, hub_deg, n_empty, seed):
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, V, (E,), generator=gen)
    dst = torch.randint(n_empty, V, (E,), generator=gen)           # rows [0, n_empty) get no in-edges
    hs = torch.randint(0, V, (n_hubs * hub_deg,), generator=gen)
    hd = torch.arange(n_empty, n_empty + n_hubs).repeat_interleave(hub_deg)
    return torch.cat([src, hs]), torch.cat([dst, hd])


CONFIGS = [   # F, out_dim, aggregators, scalers, batch_norm, residual
    (16, 16, "mean max min std", "identity amplification attenuation", True, True),
    (33, 20, "sum var max", "identity", False, False),
    (33, 33, "mean sum", "attenuation amplification", True, True),
    (75, 75, "mean max min std", "identity amplification attenuation", True, True),
    (75, 96, "var min std", "amplification", False, False),
    (128, 128, "max std sum mean var min", "identity attenuation", True, False),
    (128, 64, "mean max min std", "identity amplification attenuation", False, False),
    (64, 64, "mean max min std", "identity amplification attenuation", False, True),
]


@pytest.mark.parametrize("layout", ["contiguous", "pitched"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"F{c[0]}_N{c[1]}_{c[2].replace(' ', '-')}_S{len(c[3].split())}_bn{int(c[4])}_res{int(c[5])}")
def test_shapes_aggregators_scalers_epilogue(cuda_device, cfg, layout):
    F, N, aggs, scalers, bn, res = cfg
    V = 3000
    src, dst = _random_graph(V, 24000, 3, 700, 5, seed=F + N)
    g = Graph(src, dst, V).to(cuda_device)
    layer = make_layer(F, N, aggs, scalers, 1.7, bn, res, seed=F * N)
    x = torch.randn(V, F, generator=torch.Generator().manual_seed(F)) * 1.5 + 0.25
    if layout == "pitched":
        P = 80 if F <= 80 else 136
        buf = torch.full((V, P), float("nan"))
        buf[:, :F] = x
        h = buf.to(cuda_device).to(torch.bfloat16)[:, :F]
        assert h.stride(0) == P
    else:
        h = x.to(cuda_device).to(torch.bfloat16)
    out = run(layer, g, h)
    ref, tol, _ = reference(layer, src, dst, V, h)
    assert_contract(out, ref, tol, f"{cfg} {layout}")


def test_hub_row_and_empty_rows(cuda_device):
    """A hub of in-degree 24 000 (through the heavy-row segments) and rows with no in-edges meet the contract; accumulating the
    hub's edges in bf16 instead (emulated on the host) does not."""
    V, F = 30000, 75
    gen = torch.Generator().manual_seed(7)
    src, dst = synth_powerlaw_with_hub(V, 24000, gen)
    g = Graph(src, dst, V).to(cuda_device)
    deg = torch.bincount(dst, minlength=V)
    assert int(deg.max()) >= 20000 and int((deg == 0).sum()) >= 10
    layer = make_layer(F, F, "mean max min std sum", "identity amplification attenuation", 2.3, True, True, seed=3)
    h = (torch.rand(V, F, generator=gen) * 2.0 - 0.5).to(cuda_device).to(torch.bfloat16)
    out = run(layer, g, h)
    hub = int(torch.argmax(deg))
    empty = torch.nonzero(deg == 0).flatten()[:8]
    rows = torch.cat([torch.tensor([hub]), empty, torch.arange(100, 400)])
    ref, tol, z = reference(layer, src, dst, V, h, rows=rows)
    assert_contract(out[rows.to(cuda_device)], ref, tol, "hub graph")
    # the aggregate of the empty rows is exactly 0: the output there is the epilogue of the bias alone
    agg = ops.segreduce_bf16(g.csr.rowptr, g.csr.col, h, F, layer.aggregators, heavy=g.heavy_schedule(), workspace=g.workspace)
    assert torch.count_nonzero(agg[empty.to(cuda_device)]) == 0
    # host emulation of bf16 accumulation over the hub's edges: sum and mean rounded to bf16 after every edge
    col = src[dst == hub]
    msgs = h[col.to(cuda_device)].float().cpu()
    acc = torch.zeros(F, dtype=torch.bfloat16)
    for k in range(msgs.shape[0]):
        acc = (acc.float() + msgs[k]).to(torch.bfloat16)
    D = msgs.shape[0]
    z_emul = torch.from_numpy(z[:1].copy())
    A = len(layer.aggregators)
    for s in range(len(layer.scalers)):
        sc = _scale64(layer.scalers[s], np.array([D]), float(layer.avg_d["log"]))[0]
        z_emul[0, (s * A + 0) * F:(s * A + 1) * F] = (acc.double() / D) * sc          # mean
        z_emul[0, (s * A + 4) * F:(s * A + 5) * F] = acc.double() * sc                # sum
    out_emul, _, _ = reference(layer, src, dst, V, h, rows=torch.tensor([hub]), z_override=z_emul)
    err_emul = np.abs(out_emul - ref[:1])
    assert (err_emul > tol[:1]).any(), "the contract does not tell bf16 accumulation from fp32 accumulation"


def synth_powerlaw_with_hub(V, hub_deg, gen):
    """A ring-free random graph whose rows [0, 16) have no in-edges and whose row 16 has `hub_deg` in-edges."""
    E = 8 * V
    src = torch.randint(0, V, (E,), generator=gen)
    dst = torch.randint(17, V, (E,), generator=gen)
    hs = torch.randint(0, V, (hub_deg,), generator=gen)
    hd = torch.full((hub_deg,), 16, dtype=torch.long)
    return torch.cat([src, hs]), torch.cat([dst, hd])


@pytest.mark.parametrize("F,pitch", [(75, 75), (75, 80), (128, 128), (20, 20)])
def test_segreduce_max_min_bit_exact(cuda_device, F, pitch):
    V = 5000
    src, dst = _random_graph(V, 40000, 2, 600, 4, seed=F)
    g = Graph(src, dst, V).to(cuda_device)
    x = torch.randn(V, pitch, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    h = x.to(cuda_device)[:, :F]
    aggs = ["max", "mean", "min", "var"]
    agg = ops.segreduce_bf16(g.csr.rowptr, g.csr.col, h, F, aggs, heavy=g.heavy_schedule(), workspace=g.workspace)
    assert agg.dtype == torch.bfloat16 and agg.shape == (V, 4 * F) and agg.stride(0) % 8 == 0
    agg = agg.float().cpu().numpy()
    rp = g.csr.rowptr.cpu().numpy().astype(np.int64)
    col = g.csr.col.cpu().numpy().astype(np.int64)
    xs = x[:, :F].float().numpy()
    mx = np.zeros((V, F), np.float32)
    mn = np.zeros((V, F), np.float32)
    nz = rp[1:] > rp[:-1]
    mx[nz] = np.maximum.reduceat(xs[col], rp[:-1][nz], axis=0)
    mn[nz] = np.minimum.reduceat(xs[col], rp[:-1][nz], axis=0)
    assert np.array_equal(agg[:, :F], mx)
    assert np.array_equal(agg[:, 2 * F:3 * F], mn)


def _bench_graph(V, E, device):
    from pna_amd.synth import powerlaw_graph
    src, dst = powerlaw_graph(V, E, seed=1234, device=device)
    return src, dst, Graph(src, dst, V)


def test_determinism_c3(cuda_device):
    V, E, F = 1_000_000, 10_000_000, 75
    src, dst, g = _bench_graph(V, E, cuda_device)
    layer = make_layer(F, F, "mean max min std", "identity amplification attenuation", 2.0, True, True, seed=11)
    h = torch.randn(V, F, device=cuda_device).to(torch.bfloat16)
    first = run(layer, g, h)
    for _ in range(19):
        assert torch.equal(run(layer, g, h), first)


@pytest.mark.parametrize("shape", [(1_000_000, 10_000_000, 75), (2_000_000, 20_000_000, 128)], ids=["C3", "C5"])
def test_fullsize_sampled_rows(cuda_device, shape):
    V, E, F = shape
    src, dst, g = _bench_graph(V, E, cuda_device)
    layer = make_layer(F, F, "mean max min std", "identity amplification attenuation", float(torch.log(torch.bincount(dst.cpu(), minlength=V).double() + 1).mean()),
                       True, True, seed=5)
    h = torch.randn(V, F, device=cuda_device).to(torch.bfloat16)
    out = run(layer, g, h)
    deg = torch.bincount(dst.cpu(), minlength=V)
    gen = torch.Generator().manual_seed(99)
    rows = torch.cat([torch.topk(deg, 8).indices, torch.randint(0, V, (248,), generator=gen)])
    ref, tol, _ = reference(layer, src.cpu(), dst.cpu(), V, h.cpu(), rows=rows)
    assert_contract(out[rows.to(cuda_device)], ref, tol, f"V={V} F={F}")


def test_fp32_forward_unchanged_by_bf16_calls(cuda_device):
    V, E, F = 50_000, 500_000, 75
    src, dst, g = _bench_graph(V, E, cuda_device)
    layer32 = make_layer(F, F, "mean max min std", "identity amplification attenuation", 2.0, True, True, seed=2).float()
    layer16 = copy.deepcopy(layer32).to(torch.bfloat16)
    h = torch.randn(V, F, device=cuda_device)
    before = run(layer32, g, h)
    for _ in range(2):
        run(layer16, g, h.to(torch.bfloat16))
    after = run(layer32, g, h)
    assert before.dtype == torch.float32 and torch.equal(before, after)
