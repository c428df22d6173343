"""Kernel-level checks of what the bf16 PyG front end adds to the device code: the PyG statistics rules in finish_stats (codes
var_raw and std_pyg, through pna_segreduce_fwd_bf16 and pna_gather_bf16) and pna_edge_mlp_bf16.  Inputs are exact bf16 values, the
references float64 on those values, u = 2^-8.

Statistics: |got - ref64| <= 2u |ref64| + 4u (M + phi), M the absolute mass of the aggregate and phi the fp32 floor (DESIGN.md 4.11:
bf16_tower_ref.aggregate_mass, stat_floor); max / min bit-exact.
Edge MLP: the host knows z_1 = R(relu((x_src + x_dst) + edge row)) bit for bit (float32 adds in the kernel's order), so the bound of
the last layer is 2u |ref64| + 4u (|W| z + |b|), a hidden layer's bound propagated through |W| of the next (bf16_pyg_ref.edge_mlp_models)."""
import numpy as np
import pytest
import torch

import bf16_pyg_ref as R
import bf16_tower_ref as B
from pna_amd import ops
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu

U = B.U
BF = torch.bfloat16
KERNEL_AGGS = ["sum", "mean", "min", "max", "var_raw", "std_pyg"]        # the six PyG aggregators under their kernel names
REF_AGGS = ["sum", "mean", "min", "max", "var", "std"]
EMPTY_STD_BF16 = torch.tensor(np.sqrt(np.float32(1e-5))).to(BF)           # R(sqrtf(1e-5f))
DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 13]


def _degree_graph(copies, hub, seed):
    """Rows with the prescribed in-degrees, `copies` times over (more than one workgroup), and one row of `hub` in-edges."""
    deg = torch.tensor(DEGREES * copies + [hub])
    V = deg.numel()
    gen = torch.Generator().manual_seed(seed)
    dst = torch.repeat_interleave(torch.arange(V), deg)
    dst = dst[torch.randperm(dst.numel(), generator=gen)]
    src = torch.randint(0, V, (dst.numel(),), generator=gen)
    return src, dst, V, deg


def _rows(n, F, pitch, gen, device, scale=1.5, shift=0.25):
    """(n, F) bf16 rows on the device at row pitch `pitch` (None: contiguous); the other columns of the buffer are NaN."""
    x = (torch.randn(n, F, generator=gen) * scale + shift).to(BF)
    if pitch is None:
        return x.to(device)
    buf = torch.full((n, pitch), float("nan"), dtype=BF)
    buf[:, :F] = x
    v = buf.to(device)[:, :F]
    assert v.stride(0) == pitch
    return v


def _blocks(got, A, bs, F):
    return torch.stack([B.f64(got[:, a * bs:a * bs + F]) for a in range(A)], 1).reshape(got.shape[0], A * F)


def _check_stats(got, m64, m32, src, dst, V, F, bs, what):
    z = R.aggregate64(m64, src, dst, V, REF_AGGS)
    tol = R.aggregate_bound(m64, src, dst, V, REF_AGGS)
    err = (_blocks(got, 6, bs, F) - z).abs()
    bad = ~(err <= tol)
    print(f"{what}: worst error / bound {float((err / tol.clamp(min=1e-300)).max()):.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the contract, worst {float(err[bad].max()):.3e} at {bad.nonzero()[:3].tolist()}"
    z32 = R.aggregate64(m32.double(), src, dst, V, ["min", "max"]).to(BF)
    for j, a in enumerate((2, 3)):
        assert torch.equal(got[:, a * bs:a * bs + F].cpu(), z32[:, j * F:(j + 1) * F]), f"{what}: {REF_AGGS[a]} not bit-exact"


@pytest.mark.parametrize("entry", ["plain", "message"])
@pytest.mark.parametrize("F,pitch", [(5, 7), (16, None), (75, 80)], ids=["F5_pitch7", "F16", "F75_pitch80"])
def test_pyg_statistics_rules(cuda_device, F, pitch, entry):
    src, dst, V, deg = _degree_graph(25, 1003, seed=F)
    g = Graph(src, dst, V).to(cuda_device)
    assert g.heavy_schedule().n_heavy == 1                          # the 1003-edge row goes through the heavy-row segments
    gen = torch.Generator().manual_seed(F + 1)
    x = _rows(V, F, pitch, gen, cuda_device)
    bs = (F + 7) // 8 * 8 if pitch == 80 else F
    kw = dict(block_stride=bs, heavy=g.heavy_schedule(), workspace=g.workspace)
    if entry == "plain":
        call = lambda aggs: ops.segreduce_bf16(g.csr.rowptr, g.csr.col, x, F, aggs, **kw)          # noqa: E731
        m32, m64 = x.float().cpu()[src], B.f64(x)[src]
    else:
        d = _rows(V, F, pitch, gen, cuda_device, 0.7, -0.1)
        call = lambda aggs: ops.gather_bf16(g.csr.rowptr, g.csr.col, x, F, aggs, dst_term=d, **kw)  # noqa: E731
        m32, m64 = x.float().cpu()[src] + d.float().cpu()[dst], B.f64(x)[src] + B.f64(d)[dst]
    got = call(KERNEL_AGGS)
    assert got.dtype == BF
    _check_stats(got, m64, m32, src, dst, V, F, bs, f"F={F} {entry}")
    # rows without in-edges: every block 0, std_pyg exactly R(sqrtf(1e-5f)); the DGL code `std` on the same input still gives 0
    empty = (deg == 0).nonzero().flatten().to(cuda_device)
    assert empty.numel() == 25
    rows = got[empty].cpu()
    for a in range(5):
        assert torch.count_nonzero(rows[:, a * bs:a * bs + F]) == 0, KERNEL_AGGS[a]
    assert torch.equal(rows[:, 5 * bs:5 * bs + F], EMPTY_STD_BF16.expand(25, F))
    dgl = call(["mean", "sum", "max", "min", "std", "var"])
    assert torch.count_nonzero(dgl[empty]) == 0
    # ... and on rows WITH in-edges the two std codes are the same number, var the clamped var_raw
    full = (deg > 0).nonzero().flatten().to(cuda_device)
    assert torch.equal(dgl[full][:, 4 * bs:4 * bs + F], got[full][:, 5 * bs:5 * bs + F])
    assert torch.equal(dgl[:, 5 * bs:5 * bs + F], torch.relu(got[:, 4 * bs:4 * bs + F]))
    if bs != F:                                                     # the padding columns of every block are zeros, std_pyg's too
        for a in range(5):
            assert torch.count_nonzero(got[:, a * bs + F:(a + 1) * bs]) == 0


def test_unclamped_variance_goes_negative_where_fp32_does(cuda_device):
    """bf16 messages alone never give a negative fp32 variance (squares of 8-bit significands are exact), so the message gather:
    every source row 256.0, destination term bf16(0.01 N(0,1)), in-degrees 5, 11 and 13.  All messages of a row are equal, the
    float64 variance is 0, and fp32 E[m^2] - E[m]^2 lands on either side of it."""
    F, per = 16, 128
    deg = torch.tensor([5] * per + [11] * per + [13] * per)
    V = deg.numel()
    gen = torch.Generator().manual_seed(3)
    dst = torch.repeat_interleave(torch.arange(V), deg)
    src = torch.randint(0, V, (dst.numel(),), generator=gen)
    g = Graph(src, dst, V).to(cuda_device)
    x = torch.full((V, F), 256.0, dtype=BF, device=cuda_device)
    d = (0.01 * torch.randn(V, F, generator=gen)).to(BF).to(cuda_device)
    raw = ops.gather_bf16(g.csr.rowptr, g.csr.col, x, F, ["var_raw"], dst_term=d)
    var = ops.gather_bf16(g.csr.rowptr, g.csr.col, x, F, ["var"], dst_term=d)
    # the kernel's fp32 formula restated: s and q in edge order, mean = s / D, var = q / D - mean * mean
    m = (x.float().cpu() + d.float().cpu()).numpy()
    D = deg.numpy().astype(np.float32)[:, None]
    s, q = np.zeros_like(m), np.zeros_like(m)
    for k in range(int(deg.max())):
        on = (deg.numpy() > k)[:, None]
        s = np.where(on, s + m, s).astype(np.float32)
        q = np.where(on, (q + (m * m).astype(np.float32)).astype(np.float32), q)
    mean = (s / D).astype(np.float32)
    host = ((q / D).astype(np.float32) - (mean * mean).astype(np.float32)).astype(np.float32)
    neg = [int((raw[i * per:(i + 1) * per] < 0).sum()) for i in range(3)]
    print({"negative elements per in-degree (of 2048)": dict(zip((5, 11, 13), neg)),
           "host restatement": [int((host[i * per:(i + 1) * per] < 0).sum()) for i in range(3)]})
    assert sum(neg) > 0, "var_raw is clamped"
    assert torch.equal(torch.from_numpy(host).to(BF), raw.cpu()), "var_raw is not the fp32 formula of pna_rowstats.h"
    assert torch.equal(torch.relu(raw), var)
    m64 = (B.f64(x) + B.f64(d))[dst]
    z, tol = R.aggregate64(m64, src, dst, V, ["var"]), R.aggregate_bound(m64, src, dst, V, ["var"])
    assert float(z.abs().max()) < 1e-9
    for out in (raw, var):
        assert ((B.f64(out) - z).abs() <= tol).all()


# ---- pna_edge_mlp_bf16 ----------------------------------------------------------------------------------------------------------
CANARY = 0x7FA5          # a NaN bit pattern no result takes


def _edge_mlp_case(device, T, F, L, E, mode, seed, integers=False):
    """Runs pna_edge_mlp_bf16 on pitched operands whose padding columns are NaN -> (out view, whole out buffer, host copies)."""
    gen = torch.Generator().manual_seed(seed)
    Fp, V = (F + 7) // 8 * 8, 37
    W_ = T * Fp

    def rows(n, scale, shift):
        buf = torch.full((n, W_ + 16), float("nan"), dtype=BF)
        v = buf[:, 8:8 + W_].view(n, T, Fp)
        if integers:
            v[:, :, :F] = torch.randint(int(shift), int(shift + scale), (n, T, F), generator=gen).to(BF)
        else:
            v[:, :, :F] = (torch.randn(n, T, F, generator=gen) * scale + shift).to(BF)
        return buf

    xs, xd = (rows(V, 3, 0), rows(V, 3, -1)) if integers else (rows(V, 1.0, 0.2), rows(V, 0.7, -0.1))
    col = torch.randint(0, V, (E,), generator=gen).to(torch.int32)
    row = torch.randint(0, V, (E,), generator=gen).to(torch.int32)
    er = et = None
    if mode == "edges":
        er = rows(E, 0.5, 0.0)
    elif mode == "table":
        er = rows(4, 0.5, 0.0)
        et = torch.randint(0, 4, (E,), generator=gen).to(torch.int32)
        if E > 1:
            et[0], et[E // 2] = -3, 9                                 # outside the table: clamped to rows 0 and 3
    if integers:
        nz = [None, 3, 8]                                             # non-zeros per weight row: every sum stays below 256
        Ws = [[torch.zeros(F, F) for _ in range(L - 1)] for _ in range(T)]
        for t in range(T):
            for l in range(L - 1):
                k = F if L == 2 else min(F, nz[l + 1])
                for n in range(F):
                    c = torch.randperm(F, generator=gen)[:k]
                    Ws[t][l][n, c] = torch.randint(-1, 2, (k,), generator=gen).float()
        bs = [[torch.randint(-1, 2, (F,), generator=gen).float() for _ in range(L - 1)] for _ in range(T)]
    else:
        Ws = [[torch.randn(F, F, generator=gen) / F ** 0.5 for _ in range(L - 1)] for _ in range(T)]
        bs = [[torch.randn(F, generator=gen) * 0.3 for _ in range(L - 1)] for _ in range(T)]
    Ws = [[w.to(BF) for w in t] for t in Ws]
    bs = [[b.to(BF) for b in t] for t in bs]
    img, bias = ops.edge_mlp_image_bf16([[w.to(device) for w in t] for t in Ws], [[b.to(device) for b in t] for t in bs])
    assert img.shape == (T, L - 1, (F + 15) // 16 * 16, (Fp + 31) // 32 * 32)
    buf = torch.full((E + 2, W_ + 16), CANARY, dtype=torch.int16).view(BF).to(device)
    out = buf[1:E + 1, 8:8 + W_]
    dev = lambda t: None if t is None else t.to(device)               # noqa: E731
    view = lambda t: None if t is None else dev(t)[:, 8:8 + W_]       # noqa: E731
    run = lambda: ops.edge_mlp_bf16(dev(col), dev(row), view(xs), view(xd), n_tower=T, F=F, w_img=img, bias=bias,   # noqa: E731
                                    edge_rows=view(er), edge_type=dev(et), out=out)
    run()
    host = dict(xs=xs[:, 8:8 + W_].view(V, T, Fp), xd=xd[:, 8:8 + W_].view(V, T, Fp),
                er=None if er is None else er[:, 8:8 + W_].view(-1, T, Fp), col=col.long(), row=row.long(),
                et=None if et is None else et.long().clamp(0, 3), W=Ws, b=bs)
    return out, buf, host, run


def _check_edge_mlp(out, buf, host, T, F, E, what, exact=False):
    Fp = (F + 7) // 8 * 8
    got = out.cpu().view(E, T, Fp)
    whole = buf.cpu().view(torch.int16)
    inner = torch.zeros_like(whole, dtype=torch.bool)
    inner[1:E + 1, 8:8 + T * Fp] = True
    assert bool((whole[~inner] == torch.tensor(CANARY, dtype=torch.int16)).all()), f"{what}: a store outside the output rows"
    assert torch.count_nonzero(got[:, :, F:].float().nan_to_num(nan=1.0)) == 0, f"{what}: padding columns are not zero"
    worst = 0.0
    for t in range(T):
        er = None if host["er"] is None else host["er"][:, t, :F]
        ref, bound = R.edge_mlp_models(host["xs"][:, t, :F], host["xd"][:, t, :F], er, host["col"], host["row"], host["et"],
                                       [w.double() for w in host["W"][t]], [b.double() for b in host["b"][t]])
        g64 = got[:, t, :F].double()
        if exact:
            assert torch.equal(g64, ref), f"{what}: tower {t} differs from the exact integer result at {(g64 != ref).nonzero()[:3].tolist()}"
            continue
        err = (g64 - ref).abs()
        bad = ~(err <= bound)
        assert not bad.any(), f"{what}: tower {t}: {int(bad.sum())} elements outside the contract, worst {float(err[bad].max()):.3e}"
        if E:
            worst = max(worst, float((err / bound).max()))
    print(f"{what}: worst error / bound {worst:.3f}")


# every T, F, L, E and edge-term mode of the issue's lists; every (F, L) pair; every E at the production width 75
EDGE_MLP_CASES = [
    (1, 5, 2, 200, "none"), (2, 5, 3, 200, "edges"), (5, 16, 2, 200, "table"), (1, 16, 3, 200, "none"),
    (2, 75, 2, 200, "edges"), (5, 75, 3, 200, "table"), (2, 128, 2, 200, "table"), (1, 128, 3, 200, "edges"),
    (5, 75, 2, 0, "edges"), (2, 75, 3, 1, "table"), (1, 75, 2, 17, "none"), (2, 5, 2, 17, "table"), (5, 128, 3, 17, "none"),
    (2, 75, 2, 100003, "table"), (1, 16, 3, 100003, "edges"),
]


@pytest.mark.parametrize("T,F,L,E,mode", EDGE_MLP_CASES, ids=lambda v: str(v))
def test_edge_mlp_meets_its_contract(cuda_device, T, F, L, E, mode):
    out, buf, host, _ = _edge_mlp_case(cuda_device, T, F, L, E, mode, seed=T * 1000 + F * 10 + L)
    _check_edge_mlp(out, buf, host, T, F, E, f"T={T} F={F} L={L} E={E} {mode}")


@pytest.mark.parametrize("T,F,L,mode", [(2, 75, 2, "none"), (2, 75, 3, "none"), (5, 16, 3, "none"), (1, 128, 3, "none")], ids=lambda v: str(v))
def test_edge_mlp_is_exact_on_small_integers(cuda_device, T, F, L, mode):
    """z_1 in {0..3}, weights in {-1, 0, 1}, every sum below 256: nothing rounds, the output equals the float64 result bit for bit --
    a wrong fragment mapping (A rows, B columns, the C / D lane map, the transpose of a hidden layer) cannot hide."""
    E = 203
    out, buf, host, _ = _edge_mlp_case(cuda_device, T, F, L, E, mode, seed=F + L, integers=True)
    z1 = torch.relu(host["xs"][:, :, :F].float()[host["col"]] + host["xd"][:, :, :F].float()[host["row"]])
    assert 0 <= float(z1.min()) and float(z1.max()) <= 3 and len(torch.unique(z1)) == 4
    _check_edge_mlp(out, buf, host, T, F, E, f"integers T={T} F={F} L={L}", exact=True)
    assert float(out.float().abs().max()) < 256 and len(torch.unique(out.float())) > 8


def test_edge_mlp_repeats_bit_for_bit(cuda_device):
    out, _, _, run = _edge_mlp_case(cuda_device, 5, 75, 3, 5000, "table", seed=9)
    first = out.clone()
    for _ in range(20):
        run()
        assert torch.equal(out.view(torch.int16), first.view(torch.int16))
