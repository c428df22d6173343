"""The equivalences inside the bf16 kernel family (pna_bf16_gather.hip, pna_bf16_contract.hip), bit for bit:

  * pna_segreduce_fwd_bf16 is pna_gather_bf16 without message terms.  One difference is real and kept: a message gather without
    terms still adds its (absent) destination term as +0.0, so a gathered -0.0 becomes +0.0 before max / min see it; the plain
    gather folds the loaded value itself.  Only the sign of a zero under max / min can differ, and it is asserted here for both.
  * pna_posttrans_bf16 computes what pna_contract_bf16 computes on the same weight image, without self operand and row post factor
    (k_posttrans_bf16 is the faster specialisation of k_contract_bf16<S, 0, NT> and stays a kernel of its own: this pins that the
    two may be merged or diverge only knowingly).  relu differs from slope = 0 in the sign of a zero only (relu: +0.0, slope 0:
    z * 0 = -0.0 for z < 0), asserted here as well.
"""
import pytest
import torch

from pna_amd import ops
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu

AGGS = ["mean", "sum", "max", "min", "std", "var"]
BF = torch.bfloat16


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _r8(n):
    return (n + 7) // 8 * 8


# ---- plain gather == message gather without terms ---------------------------------------------------------------------------
V, HUB, ALL_NEG0_ROW, NEG0_COL = 200, 14, 13, 2


def _graph():
    """Rows 0..9 empty, row 10 of in-degree 1, rows 11 / 12 / 13 of in-degree 3 / 4 / 5 (the four-in-flight loop and its tail), row 14 a
    hub of in-degree 300 (above the heavy threshold of 128: three segments, the last one ragged), ~1 700 edges over the other rows."""
    gen = torch.Generator().manual_seed(11)
    src = [torch.randint(0, V, (1700,), generator=gen)]
    dst = [torch.randint(15, V, (1700,), generator=gen)]
    for row, deg in ((10, 1), (11, 3), (12, 4), (13, 5), (HUB, 300)):
        src.append(torch.randint(0, V, (deg,), generator=gen))
        dst.append(torch.full((deg,), row, dtype=torch.long))
    return torch.cat(src), torch.cat(dst)


@pytest.fixture(scope="module")
def gather_graph(cuda_device):
    src, dst = _graph()
    g = Graph(src, dst, V).to(cuda_device)
    hs = g.heavy_schedule()
    deg = torch.bincount(dst, minlength=V)
    assert hs.n_heavy == 1 and hs.n_seg == 3 and deg[:10].sum() == 0 and deg[10:14].tolist() == [1, 3, 4, 5]
    return g, src, dst


@pytest.mark.parametrize("stride", ["bs8", "bsodd"])
@pytest.mark.parametrize("layout", ["vec", "elem"])
@pytest.mark.parametrize("F", [5, 12, 80])
def test_plain_gather_is_the_message_gather_without_terms(gather_graph, cuda_device, F, layout, stride):
    g, src, dst = gather_graph
    gen = torch.Generator().manual_seed(100 + F)
    x = (torch.randn(V, F, generator=gen) * 1.5 + 0.25).to(BF)
    x[torch.rand(V, F, generator=gen) < 0.05] = -0.0
    x[src[dst == ALL_NEG0_ROW], NEG0_COL] = -0.0                   # -0.0 on every in-edge of one row
    assert int((x.view(torch.int16) == -32768).sum()) > F
    # 16-byte pieces: pitch round8(F), the tail columns readable (and NaN: they never reach a result); element loads: an odd pitch
    P = _r8(F) if layout == "vec" else (F + 1) | 1
    buf = torch.full((V, P), float("nan"), dtype=BF)
    buf[:, :F] = x
    xd = buf.to(cuda_device)[:, :F]
    assert xd.stride(0) == P and xd.data_ptr() % 16 == 0
    bs = _r8(F) if stride == "bs8" else (F if F % 8 else F + 3)
    assert (bs % 8 == 0) == (stride == "bs8")
    kw = dict(block_stride=bs, heavy=g.heavy_schedule(), workspace=g.workspace)
    plain = ops.segreduce_bf16(g.csr.rowptr, g.csr.col, xd, F, AGGS, **kw)
    msg = ops.gather_bf16(g.csr.rowptr, g.csr.col, xd, F, AGGS, **kw)
    A = len(AGGS)
    cols = torch.arange(plain.shape[1])
    if bs % 8:                                                      # element stores define only the F columns of every block
        cols = cols[cols % bs < F]
    assert plain.shape[1] == (A - 1) * bs + F and msg.shape[1] >= plain.shape[1]
    pb, mb = _bits(plain)[:, cols], _bits(msg)[:, cols]
    # the one place the two may differ: a zero under max / min (see the module docstring)
    zero_mm = ((pb & 0x7fff) == 0) & ((cols // bs == 2) | (cols // bs == 3))[None, :]
    diff = (pb != mb) & ~zero_mm
    assert not diff.any(), f"{int(diff.sum())} elements differ, first at {diff.nonzero()[:3].tolist()}"
    assert ((mb[zero_mm] & 0x7fff) == 0).all(), "a zero of the plain gather is no zero of the message gather"
    assert (mb[zero_mm] == 0).all(), "message gather without terms: x + (+0.0) is never -0.0"
    for a in (2, 3):                                                # max, min over messages that are all -0.0
        c = a * bs + NEG0_COL
        assert int(_bits(plain)[ALL_NEG0_ROW, c]) == -32768 and int(_bits(msg)[ALL_NEG0_ROW, c]) == 0
    assert int(_bits(plain)[ALL_NEG0_ROW, 1 * bs + NEG0_COL]) == 0  # the sum starts at +0.0
    assert (pb[:10] == 0).all() and (mb[:10] == 0).all()           # rows without in-edges
    assert pb[HUB].ne(0).any()


# ---- posttrans == contraction on the same image -----------------------------------------------------------------------------
M = 130                                                             # one full 128-row workgroup plus two rows


@pytest.mark.parametrize("K", [8, 40, 320])
@pytest.mark.parametrize("N", [20, 64, 75, 128])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_posttrans_is_the_contraction_without_self_operand(cuda_device, S, N, K):
    gen = torch.Generator().manual_seed(1000 * S + 10 * N + K)
    dev = cuda_device

    def rnd(*shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, generator=gen) * scale + shift

    buf = torch.full((M, K + 8), float("nan"), dtype=BF)
    buf[:, :K] = rnd(M, K).to(BF)
    a = buf.to(dev)[:, :K]
    assert a.stride(0) % 8 == 0 and a.data_ptr() % 16 == 0
    img = ops.contract_image_bf16((rnd(S, N, K) / K ** 0.5).to(BF).to(dev))
    assert tuple(img.shape) == (S, 16 * ops._lib.lib().pna_posttrans_bf16_tiles(N), (K + 31) // 32 * 32)
    pool = [None, rnd(M, scale=0.3, shift=1.0).to(dev), rnd(M, scale=0.3, shift=1.0).to(dev)]
    bias = rnd(N, scale=0.5).to(BF).to(dev)
    cs, ct = rnd(N, scale=0.2, shift=1.0).to(dev), rnd(N, scale=0.3).to(dev)
    res = torch.full((M, N + 3), float("nan"), dtype=BF)
    res[:, :N] = rnd(M, N).to(BF)
    res = res.to(dev)[:, :N]

    for scales in ([pool] if S == 3 else [pool[:S], pool[3 - S:]]):
        pt = lambda *args, **kw: _bits(ops.posttrans_bf16(a, K, img, N, scales, *args, **kw))    # noqa: E731
        ctr = lambda *args, **kw: _bits(ops.contract_bf16(a, K, img, N, scales, *args, **kw))    # noqa: E731
        # no activation: equal bits
        plain = pt()
        assert torch.equal(plain, ctr())
        with_bias = pt(bias)
        assert torch.equal(with_bias, ctr(bias)) and not torch.equal(with_bias, plain)
        full = pt(bias, epilogue=True, col_scale=cs, col_shift=ct, residual=res)
        assert torch.equal(full, ctr(bias, col_scale=cs, col_shift=ct, residual=res)) and not torch.equal(full, with_bias)
        # relu against slope = 0: equal values; relu gives +0.0 where slope = 0 gives z * 0 = -0.0
        p_relu = ops.posttrans_bf16(a, K, img, N, scales, bias, epilogue=True, relu=True, col_scale=cs, col_shift=ct)
        c_relu = ops.contract_bf16(a, K, img, N, scales, bias, col_scale=cs, col_shift=ct, slope=0.0)
        assert torch.equal(p_relu, c_relu) and not p_relu.isnan().any()
        pbits = _bits(p_relu)
        assert (pbits == 0).any() and not (pbits == -32768).any(), "relu leaves a -0.0"
        assert (_bits(c_relu)[pbits == 0] == -32768).any(), "slope = 0 no longer gives -0.0 for a negative z"
        p_rr = ops.posttrans_bf16(a, K, img, N, scales, bias, epilogue=True, relu=True, residual=res)
        assert torch.equal(p_rr, ops.contract_bf16(a, K, img, N, scales, bias, slope=0.0, residual=res))
        # epilogue = False: relu, col_scale and residual are ignored even when set
        assert torch.equal(pt(bias, epilogue=False, relu=True, col_scale=cs, col_shift=ct, residual=res), with_bias)
