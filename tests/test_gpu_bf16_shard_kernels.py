"""pna_pack_rows_bf16 and pna_gather_rows_bf16 (pna_bf16_shard.hip) against code that exists without them, bit for bit: the pack
against index_select, the row-list / split-table gather against ONE whole-V ops.segreduce_bf16 / ops.gather_bf16 call on the
concatenated table.  Rows that a launch does not list keep what they held."""
import pytest
import torch

pytestmark = pytest.mark.gpu

V, E = 4000, 40000
AGGS = ["mean", "max", "min", "std"]
SENTINEL = 0x7FC1                                  # a NaN pattern no kernel writes


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graph(dev):
    """powerlaw_graph(4000, 40000, seed=11) from the host generator (hubs of 243 and 153 in-edges) with the in-edges of a few nodes
    deleted, its light rows cut into two random halves."""
    from pna_amd import Graph
    from pna_amd.synth import powerlaw_graph
    src, dst = powerlaw_graph(V, E, seed=11, device="cpu")
    deg = torch.bincount(dst, minlength=V)
    assert {153, 243} <= set(deg.tolist())
    empty = torch.tensor([0, 7, 1999, 2000, V - 1])
    assert int(deg[empty].max()) <= 128            # the hubs stay
    keep = ~torch.isin(dst, empty)
    g = Graph(src[keep].to(dev), dst[keep].to(dev), V)
    hs = g.heavy_schedule()
    assert hs.n_heavy == int((deg > 128).sum()) >= 2
    d = (g.csr.rowptr[1:] - g.csr.rowptr[:-1]).cpu()
    assert int((d == 0).sum()) >= empty.numel()
    light = torch.nonzero(d <= hs.threshold).flatten()
    perm = light[torch.randperm(light.numel(), generator=torch.Generator().manual_seed(5))]
    half = perm.numel() // 2
    first, second = perm[:half].to(torch.int32).to(dev), perm[half:].to(torch.int32).to(dev)
    return g, hs, first, second


def _table(rows, F, pitch, dev, seed):
    t = torch.randn(rows, pitch, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).to(dev)
    return t[:, :F]


def _out(width, dev):
    buf = torch.full((V, (width + 7) // 8 * 8), SENTINEL, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return buf[:, :width]


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("width,pitch", [(20, 20), (75, 80), (75, 75), (3, 7), (128, 128)])
def test_pack_rows_bf16_is_index_select_with_a_zero_tail(dev, width, pitch):
    from pna_amd import ops
    idx = torch.randint(0, V, (5000,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    idx[0], idx[1], idx[2] = 0, V - 1, V - 1
    idx = idx.to(dev)
    tab = _table(V, width, pitch, dev, 2)
    want = tab[idx.long()]
    got = ops.pack_rows(tab, idx)
    assert got.dtype == torch.bfloat16 and got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    P = (width + 7) // 8 * 8
    for W in (P, P + 3):                           # 16-byte moves (when the table allows them too); 2-byte moves
        out = torch.full((5000, W), SENTINEL, dtype=torch.int16, device=dev).view(torch.bfloat16)
        assert ops.pack_rows(tab, idx, out=out) is out
        assert torch.equal(_bits(out[:, :width]), _bits(want))
        assert int(torch.count_nonzero(out[:, width:].view(torch.int16))) == 0


@pytest.mark.parametrize("F,pitch", [(20, 20), (75, 80)])
@pytest.mark.parametrize("terms", ["plain", "dst", "edge", "types"])
def test_two_row_list_launches_equal_one_whole_launch(dev, graph, F, pitch, terms):
    from pna_amd import ops
    g, hs, first, second = graph
    csr = g.csr
    n_edges = csr.col.numel()
    x = _table(V, F, pitch, dev, 3)
    kw = {}
    if terms != "plain":
        kw["dst_term"] = _table(V, F, pitch, dev, 4)
    if terms == "edge":
        kw["edge_rows"] = _table(n_edges, F, pitch, dev, 6)
    if terms == "types":
        kw["edge_rows"] = _table(4, F, pitch, dev, 6)
        kw["edge_type"] = torch.randint(0, 4, (n_edges,), generator=torch.Generator().manual_seed(7), dtype=torch.int32).to(dev)
    bs = (F + 7) // 8 * 8
    if terms == "plain":
        want = ops.segreduce_bf16(csr.rowptr, csr.col, x, F, AGGS, block_stride=bs, heavy=hs)
    else:
        want = ops.gather_bf16(csr.rowptr, csr.col, x, F, AGGS, block_stride=bs, heavy=hs, **kw)
    out = _out(want.shape[1], dev)
    assert ops.gather_rows_bf16(csr.rowptr, csr.col, x, F, AGGS, rows=first, block_stride=bs, out=out, **kw) is out
    listed = torch.zeros(V, dtype=torch.bool, device=dev)
    listed[first.long()] = True
    assert bool((_bits(out)[~listed] == SENTINEL).all()), "a row that was not listed was written"
    assert torch.equal(_bits(out)[listed], _bits(want)[listed])
    ops.gather_rows_bf16(csr.rowptr, csr.col, x, F, AGGS, rows=second, block_stride=bs, out=out, heavy=hs, **kw)
    assert torch.equal(_bits(out), _bits(want))
    # rows = None lists every row
    out2 = _out(want.shape[1], dev)
    ops.gather_rows_bf16(csr.rowptr, csr.col, x, F, AGGS, block_stride=bs, out=out2, heavy=hs, **kw)
    assert torch.equal(_bits(out2), _bits(want))


def test_pyg_codes_through_the_row_lists(dev, graph):
    from pna_amd import ops
    g, hs, first, second = graph
    csr = g.csr
    F, aggs = 75, ["mean", "std_pyg", "var_raw", "max"]
    x, d = _table(V, F, 80, dev, 3), _table(V, F, 80, dev, 4)
    want = ops.gather_bf16(csr.rowptr, csr.col, x, F, aggs, dst_term=d, block_stride=80, heavy=hs)
    out = _out(want.shape[1], dev)
    ops.gather_rows_bf16(csr.rowptr, csr.col, x, F, aggs, rows=first, dst_term=d, block_stride=80, out=out)
    ops.gather_rows_bf16(csr.rowptr, csr.col, x, F, aggs, rows=second, dst_term=d, block_stride=80, out=out, heavy=hs)
    assert torch.equal(_bits(out), _bits(want))


@pytest.mark.parametrize("F,pitch,halo_pitch", [(20, 20, 24), (75, 80, 88), (75, 80, 77)])
@pytest.mark.parametrize("terms", ["plain", "dst"])
def test_split_table_has_the_bits_of_one_table(dev, graph, F, pitch, halo_pitch, terms):
    """(75, 80, 77): a halo table that allows no 16-byte pieces takes BOTH tables to the 2-byte path."""
    from pna_amd import ops
    g, hs, first, second = graph
    csr = g.csr
    x = _table(V, F, pitch, dev, 3)
    n_local = V // 2
    halo = torch.zeros(V - n_local, halo_pitch, dtype=torch.bfloat16, device=dev)[:, :F]
    halo.copy_(x[n_local:])
    kw = {"dst_term": _table(V, F, pitch, dev, 4)} if terms == "dst" else {}
    bs = (F + 7) // 8 * 8
    if terms == "plain":
        want = ops.segreduce_bf16(csr.rowptr, csr.col, x, F, AGGS, block_stride=bs, heavy=hs)
    else:
        want = ops.gather_bf16(csr.rowptr, csr.col, x, F, AGGS, block_stride=bs, heavy=hs, **kw)
    out = _out(want.shape[1], dev)
    local = x[:n_local]
    ops.gather_rows_bf16(csr.rowptr, csr.col, local, F, AGGS, rows=first, x_halo=halo, n_local=n_local, block_stride=bs, out=out, **kw)
    ops.gather_rows_bf16(csr.rowptr, csr.col, local, F, AGGS, rows=second, x_halo=halo, n_local=n_local, block_stride=bs, out=out,
                         heavy=hs, **kw)
    assert torch.equal(_bits(out), _bits(want))
    # n_rows = 0 without the heavy schedule: nothing is written
    out3 = _out(want.shape[1], dev)
    none = torch.empty(0, dtype=torch.int32, device=dev)
    ops.gather_rows_bf16(csr.rowptr, csr.col, local, F, AGGS, rows=none, x_halo=halo, n_local=n_local, block_stride=bs, out=out3, **kw)
    torch.cuda.synchronize()
    assert bool((_bits(out3) == SENTINEL).all())
    with pytest.raises(ValueError):
        ops.gather_rows_bf16(csr.rowptr, csr.col, local, F, AGGS, rows=none, x_halo=halo, block_stride=bs, out=out3)


def test_an_empty_row_list_with_the_heavy_schedule_writes_the_hub_rows_only(dev, graph):
    from pna_amd import ops
    g, hs, first, second = graph
    csr = g.csr
    F = 75
    x = _table(V, F, 80, dev, 3)
    want = ops.segreduce_bf16(csr.rowptr, csr.col, x, F, AGGS, block_stride=80, heavy=hs)
    out = _out(want.shape[1], dev)
    ops.gather_rows_bf16(csr.rowptr, csr.col, x, F, AGGS, rows=torch.empty(0, dtype=torch.int32, device=dev), block_stride=80, out=out,
                         heavy=hs)
    hubs = hs.heavy_rows.long()
    rest = torch.ones(V, dtype=torch.bool, device=dev)
    rest[hubs] = False
    assert torch.equal(_bits(out)[hubs], _bits(want)[hubs]) and bool((_bits(out)[rest] == SENTINEL).all())
