"""Kernel-level checks of pna_bf16_gather.hip (pna_gather_bf16) and pna_bf16_contract.hip (pna_contract_bf16): one rounding each, inputs exact bf16,
reference float64 on those values.  The bar is the merged contract of the bf16 simple layer,

    |got - ref64| <= 2u |ref64| + 4u M_j,      u = 2^-8,

with M_j the absolute mass of the output element, the sum of the absolute values of the terms that enter it: for the contraction
sum |W| |a| (with the row and column factors) + |bias| + |residual|; for the gather the aggregate's formula over absolute terms
(bf16_tower_ref.aggregate_mass: mean |m|, sum |m|, E[m^2] + E[m]^2 for var, its root for std, |max|, |min|) plus phi, the fp32
statistics floor of tests/test_gpu_bf16_simple_layer.py (bf16_tower_ref.stat_floor).  The mass of var cannot be |var|: the contract
prescribes var = E[m^2] - E[m]^2 in fp32, whose error for two nearly equal messages of size 1.5 is an ulp of 2.4 (2.4e-7) however
small the var is -- the first run of this test met exactly that row (in-degree 2, var 7.3e-7 in float64, 4.8e-7 in fp32).
max / min are bit-exact: the fp32 message, its max, one rounding."""
import numpy as np
import pytest
import torch

import bf16_tower_ref as B
from pna_amd import ops
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu

U = B.U
AGGS = ["mean", "sum", "max", "min", "std", "var"]


def _random_graph(V, E, n_hubs, hub_deg, n_empty, seed):
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, V, (E,), generator=gen)
    dst = torch.randint(n_empty, V, (E,), generator=gen)           # rows [0, n_empty) get no in-edges
    hs = torch.randint(0, V, (n_hubs * hub_deg,), generator=gen)
    hd = torch.arange(n_empty, n_empty + n_hubs).repeat_interleave(hub_deg)
    return torch.cat([src, hs]), torch.cat([dst, hd])


def _rows(n, F, layout, gen, device, scale=1.5, shift=0.25):
    """(n, F) bf16 rows on the device: contiguous, or a view into a wider buffer whose other columns are NaN."""
    x = (torch.randn(n, F, generator=gen) * scale + shift).to(torch.bfloat16)
    if layout == "pitched":
        P = (F + 7) // 8 * 8 + 8
        buf = torch.full((n, P), float("nan"), dtype=torch.bfloat16)
        buf[:, :F] = x
        v = buf.to(device)[:, :F]
        assert v.stride(0) == P
        return v
    return x.to(device)


def _gather_case(device, V, src, dst, F, mode, layout, seed, aggs=AGGS, block_stride=None):
    """Runs pna_gather_bf16 -> (got (V, A bs) fp64 on the host, per-edge float64 messages in the caller's edge order, fp32 messages)."""
    gen = torch.Generator().manual_seed(seed)
    g = Graph(src, dst, V).to(device)
    E = src.numel()
    x = _rows(V, F, layout, gen, device)
    d = _rows(V, F, layout, gen, device, 0.7, -0.1)
    er = et = None
    if mode == "types":
        er = _rows(4, F, layout, gen, device, 0.5, 0.0)
        types = torch.randint(0, 4, (E,), generator=gen)
        et = types.to(device)[g.csr.eid.long()].to(torch.int32).contiguous()     # CSR order
    elif mode == "edges":
        ee = _rows(E, F, layout, gen, device, 0.5, 0.0)                           # caller's edge order
        er = ee[g.csr.eid.long()]
        if layout == "pitched":
            buf = torch.full((E, (F + 7) // 8 * 8 + 8), float("nan"), dtype=torch.bfloat16, device=device)
            buf[:, :F] = er
            er = buf[:, :F]
    got = ops.gather_bf16(g.csr.rowptr, g.csr.col, x, F, aggs, dst_term=d, edge_rows=er, edge_type=et, block_stride=block_stride,
                          heavy=g.heavy_schedule(), workspace=g.workspace)
    x64, d64 = B.f64(x), B.f64(d)
    m32 = x.float().cpu()[src] + d.float().cpu()[dst]
    m64 = x64[src] + d64[dst]
    if mode == "types":
        m32, m64 = m32 + er.float().cpu()[types], m64 + B.f64(er)[types]
    elif mode == "edges":
        m32, m64 = m32 + ee.float().cpu(), m64 + B.f64(ee)
    return got, m64, m32, g


def _check_gather(got, m64, m32, src, dst, V, F, aggs, bs, what):
    z = B.aggregate64(m64, src, dst, V, aggs)
    tol = 2 * U * z.abs() + 4 * U * (B.aggregate_mass(m64, src, dst, V, aggs) + B.stat_floor(m64, src, dst, V, aggs))
    A = len(aggs)
    gotv = torch.stack([B.f64(got[:, a * bs:a * bs + F]) for a in range(A)], 1).reshape(V, A * F)
    err = (gotv - z).abs()
    bad = ~(err <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the contract, worst {float(err[bad].max()):.3e} at {bad.nonzero()[:3].tolist()}"
    # max / min: the fp32 message, its max / min, one rounding -- bit for bit
    z32 = B.aggregate64(m32, src, dst, V, ["max", "min"]).to(torch.bfloat16)
    for j, name in enumerate(("max", "min")):
        if name in aggs:
            a = aggs.index(name)
            assert torch.equal(got[:, a * bs:a * bs + F].cpu(), z32[:, j * F:(j + 1) * F]), f"{what}: {name} not bit-exact"


@pytest.mark.parametrize("layout", ["contiguous", "pitched"])
@pytest.mark.parametrize("mode", ["dst", "types", "edges"])
@pytest.mark.parametrize("F", [30, 33, 75, 375], ids=["F6x5", "F33", "F75", "F5x75"])
def test_gather_with_destination_and_edge_terms(cuda_device, F, mode, layout):
    V = 3000
    src, dst = _random_graph(V, 24000, 3, 700, 5, seed=F)
    bs = (F + 7) // 8 * 8 if layout == "pitched" else None          # padded blocks (16-byte stores) / dense blocks
    got, m64, m32, _ = _gather_case(cuda_device, V, src, dst, F, mode, layout, seed=F + len(mode), block_stride=bs)
    bs = bs or F
    assert got.dtype == torch.bfloat16 and got.stride(0) % 8 == 0
    _check_gather(got, m64, m32, src, dst, V, F, AGGS, bs, f"F={F} {mode} {layout}")
    if bs != F:                                                      # the padding columns of every block are written as zeros
        for a in range(len(AGGS) - 1):
            assert torch.count_nonzero(got[:, a * bs + F:(a + 1) * bs]) == 0


def test_gather_hub_row_and_empty_rows(cuda_device):
    """A hub of in-degree 24 000 (through the heavy-row segments) and rows with no in-edges meet the contract; accumulating the
    hub's messages in bf16 instead (emulated on the host) does not."""
    V, F = 30000, 75
    gen = torch.Generator().manual_seed(7)
    E = 8 * V
    src = torch.cat([torch.randint(0, V, (E,), generator=gen), torch.randint(0, V, (24000,), generator=gen)])
    dst = torch.cat([torch.randint(17, V, (E,), generator=gen), torch.full((24000,), 16, dtype=torch.long)])
    deg = torch.bincount(dst, minlength=V)
    assert int(deg.max()) >= 24000 and int((deg == 0).sum()) >= 10
    aggs = ["mean", "max", "min", "std", "sum"]
    got, m64, m32, g = _gather_case(cuda_device, V, src, dst, F, "types", "pitched", seed=3, aggs=aggs, block_stride=80)
    assert g.heavy_schedule().n_heavy >= 1
    hub, empty = 16, torch.nonzero(deg == 0).flatten()
    rows = torch.cat([torch.tensor([hub]), empty[:8], torch.arange(100, 400)])
    local = torch.full((V,), -1, dtype=torch.long)
    local[rows] = torch.arange(rows.numel())
    keep = local[dst] >= 0
    s_sub, d_sub, R = src[keep], local[dst[keep]], rows.numel()
    _check_gather(got[rows.to(cuda_device)], m64[keep], m32[keep], s_sub, d_sub, R, F, aggs, 80, "hub graph")
    assert torch.count_nonzero(got[empty.to(cuda_device)]) == 0
    # host emulation of bf16 accumulation over the hub's messages: the running sum rounded to bf16 after every edge
    mh = m64[dst == hub]
    acc = torch.zeros(F, dtype=torch.bfloat16)
    for k in range(mh.shape[0]):
        acc = (acc.float() + mh[k].float()).to(torch.bfloat16)
    z = B.aggregate64(m64[keep], s_sub, d_sub, R, aggs)[0]
    tol = 2 * U * z.abs() + 4 * U * (B.aggregate_mass(m64[keep], s_sub, d_sub, R, aggs)[0] + B.stat_floor(m64[keep], s_sub, d_sub, R, aggs)[0])
    assert ((acc.double() - z[4 * F:5 * F]).abs() > tol[4 * F:5 * F]).any(), "the contract does not tell bf16 from fp32 accumulation (sum)"
    assert ((acc.double() / mh.shape[0] - z[:F]).abs() > tol[:F]).any(), "the contract does not tell bf16 from fp32 accumulation (mean)"


def _contract_case(device, M, K, N, S, identity, self_k, row_post, bn, slope, residual, seed, a_pitch=None):
    gen = torch.Generator().manual_seed(seed)
    bf = torch.bfloat16

    def rnd(*shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, generator=gen) * scale + shift

    a = rnd(M, K).to(bf)
    if a_pitch:
        buf = torch.full((M, a_pitch), float("nan"), dtype=bf)
        buf[:, :K] = a
        a_dev = buf.to(device)[:, :K]
    else:
        a_dev = a.to(device)
    W = (rnd(S, N, K) / K ** 0.5).to(bf)
    bias = rnd(N, scale=0.5).to(bf)
    scales = [None if (identity and s == 0) else (rnd(M).abs() + 0.3).float() for s in range(S)]
    h = Wh = None
    if self_k:
        h, Wh = rnd(M, self_k).to(bf), (rnd(1, N, self_k) / self_k ** 0.5).to(bf)
    post = (torch.rand(M, generator=gen) * 0.5 + 0.1).float() if row_post else None
    cs = (torch.rand(N, generator=gen) + 0.5).float() if bn else None
    ct = rnd(N, scale=0.5).float() if bn else None
    res = rnd(M, N).to(bf) if residual else None
    dev = lambda t: None if t is None else t.to(device)
    y = ops.contract_bf16(a_dev, K, ops.contract_image_bf16(W.to(device)), N, [dev(s) for s in scales], dev(bias),
                          h_self=dev(h), w_self=None if Wh is None else ops.contract_image_bf16(Wh.to(device)),
                          row_post=dev(post), col_scale=dev(cs), col_shift=dev(ct), slope=slope, residual=dev(res))
    d = lambda t: t.double()
    z = d(bias).expand(M, N).clone()
    mass = d(bias).abs().expand(M, N).clone()
    for s in range(S):
        sc = torch.ones(M, 1, dtype=torch.float64) if scales[s] is None else d(scales[s])[:, None]
        z += sc * (d(a) @ d(W[s]).T)
        mass += sc.abs() * (d(a).abs() @ d(W[s]).abs().T)
    if self_k:
        z += d(h) @ d(Wh[0]).T
        mass += d(h).abs() @ d(Wh[0]).abs().T
    if row_post:
        z, mass = z * d(post)[:, None], mass * d(post)[:, None]
    if bn:
        z, mass = z * d(cs) + d(ct), mass * d(cs).abs() + d(ct).abs()
    z = torch.where(z < 0, slope * z, z)
    if residual:
        z, mass = z + d(res), mass + d(res).abs()
    return y, z, 2 * U * z.abs() + 4 * U * mass


CONTRACT = [   # K, N, S, identity scaler, Kh of the self operand, row_post, folded BatchNorm, slope, residual
    (320, 16, 1, True, 0, False, False, 1.0, False),         # a plain Linear (the pretrans projections)
    (75, 752, 1, True, 0, False, False, 1.0, False),         # ... 5 x 75 towers: column slabs, 2-byte operand loads
    (320, 30, 3, True, 30, True, True, 1.0, False),          # the posttrans of a ZINC layer: self block shares block 0
    (320, 75, 3, True, 75, True, True, 1.0, False),
    (1504, 75, 3, True, 75, True, True, 1.0, False),         # 4 aggregators x round8(5 x 75)
    (320, 80, 3, False, 80, True, True, 0.0, True),          # no identity scaler: the self block has its own accumulators
    (320, 128, 3, False, 64, False, True, 0.01, True),       # ... at 8 column tiles: one row tile per wavefront
    (320, 128, 3, True, 128, True, False, 1.0, False),
    (160, 128, 2, False, 40, True, True, 0.0, False),
    (160, 16, 2, True, 16, False, False, 0.01, True),
    (96, 30, 1, False, 30, True, True, 0.01, False),
    (96, 75, 2, True, 0, False, True, 0.0, True),
    (72, 80, 1, True, 0, False, False, 0.01, True),          # the mixing network: Linear, LeakyReLU, residual
    (75, 75, 1, True, 0, False, False, 0.01, True),
    (128, 128, 3, False, 0, True, False, 0.0, False),
    (40, 30, 2, False, 0, False, False, 1.0, True),
]


@pytest.mark.parametrize("cfg", CONTRACT, ids=lambda c: f"K{c[0]}_N{c[1]}_S{c[2]}_id{int(c[3])}_self{c[4]}_post{int(c[5])}_bn{int(c[6])}_slope{c[7]}_res{int(c[8])}")
def test_contraction_epilogue_variants(cuda_device, cfg):
    K, N, S, identity, self_k, row_post, bn, slope, residual = cfg
    for M, pitch in ((1000, None), (257, K + 8 if K % 8 == 0 else K + 5)):
        y, ref, tol = _contract_case(cuda_device, M, K, N, S, identity, self_k, row_post, bn, slope, residual, seed=K + N + S, a_pitch=pitch)
        assert y.dtype == torch.bfloat16 and y.shape == (M, N)
        err = (B.f64(y) - ref).abs()
        bad = ~(err <= tol)
        assert not bad.any(), f"{cfg} M={M}: {int(bad.sum())} elements outside the contract, worst {float(err[bad].max()):.3e} at {bad.nonzero()[:3].tolist()}"


def test_twenty_launches_give_identical_bits(cuda_device):
    V, F = 200_000, 75
    src, dst = _random_graph(V, 2_000_000, 4, 5000, 3, seed=1)
    g = Graph(src, dst, V).to(cuda_device)
    gen = torch.Generator().manual_seed(2)
    x, d, er = _rows(V, F, "pitched", gen, cuda_device), _rows(V, F, "pitched", gen, cuda_device), _rows(4, F, "pitched", gen, cuda_device)
    et = torch.randint(0, 4, (src.numel(),), generator=gen).to(torch.int32).to(cuda_device)
    W = ops.contract_image_bf16((torch.randn(3, F, 4 * 80, generator=gen) / 18).to(torch.bfloat16).to(cuda_device))
    Wh = ops.contract_image_bf16((torch.randn(1, F, F, generator=gen) / 9).to(torch.bfloat16).to(cuda_device))
    amp, att = g.degree_scalers(2.0)

    def once():
        agg = ops.gather_bf16(g.csr.rowptr, g.csr.col, x, F, ["mean", "max", "min", "std"], dst_term=d, edge_rows=er, edge_type=et,
                              block_stride=80, heavy=g.heavy_schedule(), workspace=g.workspace)
        return agg, ops.contract_bf16(agg, 320, W, F, [None, amp, att], h_self=x, w_self=Wh, slope=0.01)

    agg0, y0 = once()
    for _ in range(19):
        agg, y = once()
        assert torch.equal(agg, agg0) and torch.equal(y, y0)


def test_fullsize_gather_sampled_rows(cuda_device):
    """F = 75, V = 1 M, E = 10 M (the flagship graph) with a destination term: the 8 highest-degree rows and 248 seeded random rows."""
    from pna_amd.synth import powerlaw_graph
    V, E, F = 1_000_000, 10_000_000, 75
    src, dst = powerlaw_graph(V, E, seed=1234, device=cuda_device)
    g = Graph(src, dst, V)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(V, 80, generator=gen).to(torch.bfloat16).to(cuda_device)[:, :F]
    d = (torch.randn(V, 80, generator=gen) * 0.5).to(torch.bfloat16).to(cuda_device)[:, :F]
    aggs = ["mean", "max", "min", "std"]
    got = ops.gather_bf16(g.csr.rowptr, g.csr.col, x, F, aggs, dst_term=d, block_stride=80, heavy=g.heavy_schedule(), workspace=g.workspace)
    src, dst = src.cpu().long(), dst.cpu().long()
    deg = torch.bincount(dst, minlength=V)
    rows = torch.cat([torch.topk(deg, 8).indices, torch.randint(0, V, (248,), generator=torch.Generator().manual_seed(99))])
    rows = torch.unique(rows)
    local = torch.full((V,), -1, dtype=torch.long)
    local[rows] = torch.arange(rows.numel())
    keep = local[dst] >= 0
    s_sub, d_sub = src[keep], local[dst[keep]]
    xc, dc = x.cpu(), d.cpu()
    m32 = xc[s_sub].float() + dc[dst[keep]].float()
    m64 = xc[s_sub].double() + dc[dst[keep]].double()
    _check_gather(got[rows.to(cuda_device)], m64, m32, s_sub, d_sub, rows.numel(), F, aggs, 80, "full size")
