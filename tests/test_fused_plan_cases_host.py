"""Host half of the hand-built degree plans of pna_fused_degree_f32 (fused_plan_cases.py): the builder follows the header and equals the
production builder on a real graph, the float64 layer reference is the reference's layer (oracle.torch_oracle in float64), and the bar and
the bit comparison BITE -- a numpy model of the kernel's data path with one defect at a time leaves them."""
import numpy as np
import pytest
import torch

import fused_plan_cases as C


def _cases():
    return {"ladder_75_75": lambda: C.make_case(75, 75, C.ladder_blocks(), seed=1),
            "ladder_33_17": lambda: C.make_case(33, 17, C.ladder_blocks(), seed=2, S=2, relu=2, slope=0.01),
            "padding_64_20": lambda: C.make_case(64, 20, C.padding_blocks(), seed=3, n_img=2, residual=False),
            "claim_40_16": lambda: C.make_case(40, 16, C.claim_blocks(), seed=4, n_img=2, S=1, bn=False),
            "tower_75_75": lambda: C.make_case(75, 75, C.ladder_blocks(C.LADDER[:16]), seed=5, tower=True, pre_add=True)}


@pytest.fixture(scope="module")
def cases():
    return {k: f() for k, f in _cases().items()}


def test_every_case_follows_the_header(cases):
    for name, c in cases.items():
        p = c["plan"]
        assert C.check_contract(p, x_rows=p["x_rows"]), name
        assert 0 in p["col"] and p["x_rows"] - 1 in p["col"], name
        assert p["M"] % C.TILE == 0 and (p["perm"] < 0).any(), name
    lad = cases["ladder_75_75"]["plan"]
    assert set(C.LADDER) <= set(lad["block_D"].tolist())
    d, live = lad["block_D"], lad["perm"].reshape(-1, 16)[:, 0] >= 0
    assert ((d[:-1] == 0) & ~live[:-1] & (d[1:] > 0)).any() and d[-1] == 0 and not live[-1]     # D = 0 in front of a live block, and last
    assert ((d == 0) & live).any()                                                               # live rows without in-edges too
    mixed = lad["block_D"].reshape(-1, 4)
    assert (np.array([len(set(t)) for t in mixed]) == 4).sum() >= 5 and (np.array([len(set(t)) for t in mixed]) == 1).sum() >= len(C.LADDER)
    chained = C.retile(lad, C.chain_order(lad["M"] // C.TILE, 7, 6))
    assert C.check_contract(chained, x_rows=lad["x_rows"])


def test_check_contract_rejects_broken_tables(cases):
    p = cases["ladder_75_75"]["plan"]
    b = int(np.nonzero(p["block_D"] == 5)[0][0])
    first = int(p["tile_desc"][b, 0])
    for what, mutate in [("copies of record D - 1", lambda t: t["tile_ids"].__setitem__((first + 6, 3), (t["tile_ids"][first + 4, 3] + 1) % 300)),
                         ("max(4, round_up(D, 4)) records", lambda t: t["tile_desc"].__setitem__((b, 1), 9)),
                         ("one weight image", lambda t: t["tile_desc"].__setitem__((b, 2), t["tile_desc"][b, 2] + 1)),
                         ("valid row", lambda t: t["tile_ids"].__setitem__((first, 0), 301))]:
        t = dict(p, tile_desc=p["tile_desc"].copy(), tile_ids=p["tile_ids"].copy())
        mutate(t)
        with pytest.raises(AssertionError):
            C.check_contract(t, x_rows=p["x_rows"])
            pytest.fail(f"check_contract accepted tables that break: {what}")


@pytest.fixture(scope="module")
def real_graph():
    """A small graph whose degrees 1, 2 and 5 fill whole degree_groups.TILE-row groups (two of them two tiles, with trailing padding)
    and whose other rows (degrees 0, 3, 4, 7) are rest rows."""
    from pna_amd import Graph, degree_groups as DG
    rng = np.random.default_rng(11)
    degs = np.concatenate([np.full(DG.TILE + 2, 1), np.full(DG.TILE, 2), np.full(DG.TILE + 70, 5), [0, 0, 3, 3, 3, 4, 7, 7]])
    rng.shuffle(degs)
    V = degs.size
    dst = np.repeat(np.arange(V), degs)
    src = rng.integers(0, V, dst.size)
    src[:2] = (0, V - 1)
    sh = rng.permutation(dst.size)
    g = Graph(torch.from_numpy(src[sh]), torch.from_numpy(dst[sh]), V)
    return g, DG.DegreePlan(g), src[sh], dst[sh]


def _virtual_csr(g, perm):
    rp, col = g.csr.rowptr.long().numpy(), g.csr.col.long().numpy()
    deg = np.where(perm >= 0, (rp[1:] - rp[:-1])[np.maximum(perm, 0)], 0)
    vrp = np.zeros(perm.size + 1, np.int64)
    vrp[1:] = np.cumsum(deg)
    vcol = np.concatenate([col[rp[n]:rp[n + 1]] for n in perm if n >= 0] + [np.zeros(0, np.int64)])
    return vrp, vcol


def test_builder_equals_the_production_plan_builder(real_graph):
    from pna_amd import degree_groups as DG
    g, plan, _, _ = real_graph
    assert plan.G == 3 and plan.NR == 8 and plan.NV == 5 * DG.TILE
    desc, ids, n_rec = plan.fused_tables()
    perm = plan.perm.numpy().astype(np.int64)
    vrp, vcol = _virtual_csr(g, perm)
    image = np.repeat(plan.tile_image.numpy(), DG.TILE // 16)
    d2, i2, n2 = C.tables(perm, image, vrp, vcol, placeholder=0)
    assert n2 == n_rec and np.array_equal(d2, desc.numpy()) and np.array_equal(i2, ids.numpy())
    t = dict(perm=perm, tile_desc=d2, tile_ids=i2, n_records=n2, tile=C.TILE, rowptr=vrp, col=vcol)
    assert C.check_contract(t, x_rows=g.num_nodes)
    assert C.check_contract(dict(perm=perm, tile_desc=desc.numpy(), tile_ids=ids.numpy(), n_records=n_rec, tile=C.TILE), x_rows=g.num_nodes)


def test_layer_reference_is_the_references_layer(real_graph):
    """layer_ref on the reference's own float64 aggregate equals oracle.torch_oracle's PNASimpleLayer in float64 to float64 noise (the
    contraction with W_i, the BatchNorm fold, ReLU and residual are the reference's); the C oracle's fp32 statistics -- what the GPU tests
    feed it -- sit within fp32 rounding of that aggregate."""
    from oracle import torch_oracle as TO
    from pna_amd import degree_groups as DG
    g, plan, src, dst = real_graph
    V, F = g.num_nodes, 24
    rng = np.random.default_rng(12)
    f32 = np.float32
    w = (rng.standard_normal((F, 12 * F)) / np.sqrt(12 * F)).astype(f32)
    sd32 = {"posttrans.fully_connected.0.linear.weight": w, "posttrans.fully_connected.0.linear.bias": rng.standard_normal(F).astype(f32),
            "batchnorm_h.running_mean": rng.standard_normal(F).astype(f32), "batchnorm_h.running_var": (0.5 + rng.random(F)).astype(f32),
            "batchnorm_h.weight": rng.standard_normal(F).astype(f32), "batchnorm_h.bias": rng.standard_normal(F).astype(f32)}
    sd = {k: torch.from_numpy(v).double() for k, v in sd32.items()}
    h = rng.standard_normal((V, F)).astype(f32)
    avg_log = torch.tensor(2.3, dtype=torch.float64)
    want, agg = TO.simple_layer_forward(sd, src, dst, V, torch.from_numpy(h).double(), ["mean", "max", "min", "std"],
                                        ["identity", "amplification", "attenuation"], avg_log, return_aggregate=True)
    perm = plan.perm.numpy().astype(np.int64)
    vrp, vcol = _virtual_csr(g, perm)
    image = np.repeat(plan.tile_image.numpy(), DG.TILE // 16)
    desc, ids, n_rec = C.tables(perm, image, vrp, vcol)
    Dg = plan.group_degree.numpy().astype(np.float64)
    scale = np.stack([np.ones_like(Dg), np.log(Dg + 1) / 2.3, 2.3 / np.log(Dg + 1)], axis=1)
    cs = sd32["batchnorm_h.weight"].astype(np.float64) / np.sqrt(sd32["batchnorm_h.running_var"].astype(np.float64) + 1e-5)
    p = dict(perm=perm.astype(np.int32), tile_desc=desc, tile_ids=ids, n_records=n_rec, rowptr=vrp, col=vcol, M=perm.size, n_nodes=V, x_rows=V,
             tile=C.TILE, block_D=desc[:, 1].astype(np.int64), block_image=image.astype(np.int64))
    c = dict(F=F, N=F, S=3, n_img=plan.G, plan=p, x=h, w_ref=w, scale=scale, bias=sd32["posttrans.fully_connected.0.linear.bias"], col_scale=cs,
             col_shift=sd32["batchnorm_h.bias"].astype(np.float64) - sd32["batchnorm_h.running_mean"].astype(np.float64) * cs,
             residual=h, relu=1, slope=0.0, tower=None)
    live = perm >= 0
    stats64 = np.zeros((perm.size, 4 * F))
    stats64[live] = agg.numpy()[perm[live], :4 * F]
    r = C.layer_ref(c, stats64)
    got, ref = r["ref"][live], want.numpy()[perm[live]]
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), np.abs(got - ref).max()
    s32 = C.oracle_stats(p, h, F)
    mean, std = stats64[live][:, :F], stats64[live][:, 3 * F:]
    assert (np.abs(s32[live][:, :F] - mean) <= 2e-6 * np.abs(stats64).max()).all()
    # (std = sqrt(E[x^2] - mean^2 + 1e-5): the cancellation's fp32 floor, 2e-6 (E[x^2] + 2 mean^2), through d std = d var / (2 std))
    assert (np.abs(s32[live][:, 3 * F:] - std) <= 1e-5 * std + 2e-6 * (std * std + 3 * mean * mean) / (2 * std)).all()
    assert np.array_equal(s32[live][:, F:3 * F], stats64[live][:, F:3 * F].astype(np.float32))      # max / min: selections


# ---- the bar bites ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def judged(cases):
    """Per case: the oracle's statistics and the float64 reference -- computed once, shared, never written to."""
    out = {}
    for name, c in cases.items():
        stats = C.oracle_stats(c["plan"], c["x"], c["F"])
        out[name] = (stats, C.layer_ref(c, stats))
    return out


def _verdict(c, stats, r, mut):
    """(statistics' bits equal on the live rows and zero on rows without in-edges, worst err / bar of the outputs)."""
    y, ms = C.model_layer(c, mut)
    p = c["plan"]
    live = p["perm"] >= 0
    D = np.repeat(p["block_D"], 16)
    bits = np.array_equal(ms[live].view(np.uint32), stats[live].view(np.uint32)) and not ms[D == 0].any()
    return bits, C.compare_y(y, c, r)[0]


def test_the_model_without_a_defect_passes(cases, judged):
    for name, c in cases.items():
        bits, worst = _verdict(c, *judged[name], None)
        assert bits and worst <= 1.0, (name, bits, worst)


@pytest.mark.parametrize("mut", C.MUTATIONS)
def test_the_bar_bites(cases, judged, mut):
    """Each defect leaves the comparison on at least one case: the outputs' bar -- or, for the reciprocal-multiply mean, whose error
    is a last-place one, the bit comparison of the statistics (it MUST be the bits that catch it)."""
    verdicts = {name: _verdict(c, *judged[name], mut) for name, c in cases.items()}
    if mut == "mean_by_reciprocal":
        assert any(not bits for bits, _ in verdicts.values()), verdicts
    else:
        assert any(worst > 1.0 for _, worst in verdicts.values()), verdicts
