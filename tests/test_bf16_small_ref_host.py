"""CPU-side checks of the kernel-level harness of pna_tower_layer_bf16 (bf16_small_ref.py) and of the entry point's refusals:
the independent weight images equal the product's byte for byte, the staged float64 model composed end to end is ref64 of
bf16_tower_ref.layer_models, every falsified model of the stage probes violates its stage's bar on the probes' own inputs (the bars
have teeth before a GPU is asked), and the argument checks that test_bf16_small_host.py leaves out refuse before any launch."""
import ctypes

import pytest
import torch

import bf16_small_ref as R
import bf16_tower_ref as B
from pna_amd import _lib
from pna_amd import functional as PF
from pna_amd import ops
from pna_amd.dgl.pna_layer import PNALayer, PNASimpleLayer

BF = torch.bfloat16


def _randomize(module, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in list(module.parameters()) + [b for n, b in module.named_buffers() if "running" in n]:
            p.copy_(torch.rand(p.shape, generator=gen) * 1.5 + 0.25 if p.dim() == 1 else torch.randn(p.shape, generator=gen))
    return module.eval().to(BF)


# towers, per-tower width, divide_input, scalers (never the canonical order), edge_dim, BatchNorm, mixing network
IMAGE_CONFIGS = [
    (1, 7, False, "attenuation identity", 0, True, True),
    (5, 16, True, "amplification", 3, False, True),
    (8, 33, False, "attenuation amplification identity", 0, True, False),
    (5, 75, False, "amplification identity attenuation", 6, True, True),
    (8, 7, True, "amplification identity", 4, False, False),
    (1, 75, True, "attenuation", 0, True, True),
    (5, 33, True, "attenuation identity", 2, True, True),
    (1, 16, False, "identity", 0, False, False),
    (8, 75, True, "attenuation identity amplification", 5, True, True),
]


@pytest.mark.parametrize("cfg", IMAGE_CONFIGS, ids=lambda c: f"T{c[0]}_Fi{c[1]}_div{int(c[2])}_S{len(c[3].split())}_ed{c[4]}_bn{int(c[5])}_mix{int(c[6])}")
def test_independent_images_equal_the_products(cfg):
    T, Fi, divide, scalers, ed, bn, with_mix = cfg
    in_dim, out_dim = (T * Fi if divide else Fi), T * 9
    layer = _randomize(PNALayer(in_dim, out_dim, "mean max min std", scalers, {"log": torch.tensor(1.5)}, 0.0, True, bn, towers=T,
                                divide_input=divide, edge_features=ed > 0, edge_dim=ed), seed=T * 100 + Fi)
    towers, mix = list(layer.towers), layer.mixing_network if with_mix else None
    theirs, ours = PF._small_images_bf16(towers, mix, divide), R.images_from_towers(towers, mix, divide)
    Fp, Fop, Kp, Khp = R.dims(T, Fi, 9, 4)
    S = len(scalers.split())
    assert ours["post"].numel() == T * S * Fop * Kp + T * Fop * Khp and ours["proj_bias"].numel() == 2 * T * Fp
    for k, img in ours.items():
        if img is None:
            assert theirs[k] is None, k
        else:
            assert theirs[k].dtype == img.dtype == BF and theirs[k].shape == img.shape, (k, theirs[k].shape, img.shape)
            assert torch.equal(theirs[k].view(torch.int16), img.view(torch.int16)), k
    assert (ours["edge"] is None) == (ed == 0) and (ours["mix"] is None) == (not with_mix)
    if with_mix:
        assert ours["mix"].shape == (R.rnd(out_dim, 16), R.rnd(out_dim, 32))
    # the folded BatchNorm: present with batch_norm only, fp32, gamma / sqrt(var + eps) and beta - mean * that
    assert (theirs["cs"] is None) == (theirs["ct"] is None) == (not bn)
    if bn:
        folds = [R.fold_batchnorm64(t.batchnorm_h) for t in towers]
        assert theirs["cs"].dtype == torch.float32
        assert torch.allclose(theirs["cs"].double(), torch.cat([f[0] for f in folds]), rtol=1e-6, atol=0)
        assert torch.allclose(theirs["ct"].double(), torch.cat([f[1] for f in folds]), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("cfg", [(7, 10, "mean sum max", "attenuation identity", True), (16, 16, "max", "amplification", False),
                                 (33, 20, "std var min mean", "attenuation amplification identity", True), (75, 75, "mean max min std", "identity", False)],
                         ids=lambda c: f"F{c[0]}_N{c[1]}_A{len(c[2].split())}_S{len(c[3].split())}_bn{int(c[4])}")
def test_independent_simple_layer_images_equal_the_products(cfg):
    F, N, aggs, scalers, bn = cfg
    layer = _randomize(PNASimpleLayer(F, N, aggs, scalers, {"log": torch.tensor(1.5)}, 0.0, bn, False), seed=F)
    theirs, ours = PF._small_simple_images_bf16(layer), R.images_from_simple_layer(layer)
    for k, img in ours.items():
        assert theirs[k].shape == img.shape and torch.equal(theirs[k].view(torch.int16), img.view(torch.int16)), k
    assert (theirs["cs"] is None) == (not bn)


def test_degree_graph_holds_every_row_class():
    for V, hub in ((1, 3), (15, R.HUB), (16, R.HUB), (17, R.HUB), (33, R.HUB), (700, R.HUB), (40, 203)):
        rowptr, col, dst = R.degree_graph(V, seed=V, hub=hub)
        R.assert_degree_classes(rowptr, V, hub)
        assert col.numel() == dst.numel() == int(rowptr[-1]) and int(col.max()) < V and int(col.min()) >= 0
        assert torch.equal(torch.bincount(dst, minlength=V), (rowptr[1:] - rowptr[:-1]).long())


# ---- the staged model is the existing reference -------------------------------------------------------------------------------------
MODEL_CONFIGS = [
    dict(towers=5, divide_input=True, aggregators=["mean", "max", "min", "std"], scalers=["identity", "amplification", "attenuation"],
         graph_norm=True, batch_norm=True, residual=True, edge_features=True),
    dict(towers=3, divide_input=False, aggregators=["sum", "var", "max"], scalers=["attenuation", "amplification"],
         graph_norm=False, batch_norm=False, residual=False, edge_features=False),
]


@pytest.mark.parametrize("cfg", MODEL_CONFIGS, ids=["T5_div_edge_bn_res", "T3_shared_plain"])
def test_staged_model_agrees_with_layer_models(cfg):
    T, Fi, V, ed, avg_log = cfg["towers"], 16 if cfg["divide_input"] else 33, 60, 6, 1.25
    in_dim = T * Fi if cfg["divide_input"] else Fi
    out_dim = in_dim if cfg["residual"] else T * 11
    layer = _randomize(PNALayer(in_dim, out_dim, cfg["aggregators"], cfg["scalers"], {"log": torch.tensor(avg_log)}, 0.0, cfg["graph_norm"],
                                cfg["batch_norm"], towers=T, divide_input=cfg["divide_input"], residual=cfg["residual"],
                                edge_features=cfg["edge_features"], edge_dim=ed if cfg["edge_features"] else 0), seed=T)
    assert layer.residual == cfg["residual"]
    gen = torch.Generator().manual_seed(T + 1)
    rowptr, col, dst = R.degree_graph(V, seed=T, hub=63)
    h = (torch.randn(V, in_dim, generator=gen) * 1.5 + 0.25).to(BF).double()
    sn = (torch.rand(V, 1, generator=gen) * 0.5 + 0.1).to(BF).double()
    rows = types = e = None
    if cfg["edge_features"]:
        rows = torch.randn(4, ed, generator=gen).to(BF).double()
        types = torch.randint(0, 4, (col.numel(),), generator=gen).to(torch.int32)
        e = rows[types.long()]
    sd = {k: (v.detach().double() if v.is_floating_point() else v) for k, v in layer.state_dict().items()}
    ref = B.layer_models(sd, cfg, col.long(), dst, V, h, e, sn, avg_log)[0]
    got = R.compose64(R.case_from_layer(layer, cfg, rowptr, col, dst, h, sn, avg_log, rows, types))
    assert got.shape == ref.shape == (V, out_dim)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), float((got - ref).abs().max())


# ---- teeth: every falsified model violates its stage's bar on the probe's own inputs --------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.GATHER)))
def test_gather_bar_rejects_a_skipped_tail_edge_and_unclamped_types(i):
    c = R.gather_case(i)
    x = R.emulated_x_cat(c)
    ref, tol = R.gather64(c, x), R.gather_tol(c, x)
    assert R.outside(ref, ref, tol) == 0 and R.outside(R.selections(c, x).double(), R.gather64(dict(c, aggs=["max", "min"]), x),
                                                         R.gather_tol(dict(c, aggs=["max", "min"]), x)) == 0
    assert R.outside(R.gather64(c, x, skip_tail3=True), ref, tol) > 0, "last edge of the rows with deg % 4 == 3 skipped"
    if R.GATHER[i]["bad_types"]:
        assert R.outside(R.gather64(c, x, clamp=False), ref, tol) > 0, "edge types not clamped"
    assert sum(k["bad_types"] for k in R.GATHER) >= 4


@pytest.mark.parametrize("i", range(len(R.TOWERS) + 1))
def test_towers_bar_rejects_the_falsified_contractions(i):
    c = R.towers_case(i) if i < len(R.TOWERS) else R.largest_tile_case()
    x = R.emulated_x_cat(c)
    ref, tol = R.towers_expect(c, x)
    T, S, A, Fi = c["T"], c["S"], len(c["aggs"]), c["Fi"]
    assert R.outside(ref, ref, tol) == 0
    for t in {0, T - 1}:
        assert R.outside(R.towers_expect(c, x, ("drop_self", t))[0], ref, tol) > 0, f"self block of tower {t} dropped"
        if Fi > 1:
            assert R.outside(R.towers_expect(c, x, ("shift_block", t, A - 1))[0], ref, tol) > 0, f"aggregator block {A - 1} of tower {t} shifted"
        if Fi % 8:
            assert R.outside(R.towers_expect(c, x, ("pad_weight", t))[0], ref, tol) > 0, f"padded column of tower {t} given weight 1"
    for s in range(1, S):
        assert R.outside(R.towers_expect(c, x, ("swap_scales", s - 1, s))[0], ref, tol) > 0, f"row scales {s - 1} and {s} swapped"


def test_towers_probe_covers_the_issue_sweep():
    cases = R.TOWERS
    assert {len(k["scales"]) for k in cases} == {1, 2, 3} and (False, True, False) in {k["scales"] for k in cases} and (True, True, True) in {k["scales"] for k in cases}
    assert {k["Fo"] for k in cases} >= {1, 14, 16, 17, 75, 130} and {k["Fi"] for k in cases} >= {1, 7, 20, 33, 75}
    assert {k["T"] for k in cases} >= {1, 3, 5, 8} and {k.get("divide", False) for k in cases} == {False, True}
    assert {k.get("slope", 1.0) for k in cases} == {1.0, 0.0, 0.01}
    for opt in ("post_bias", "row_post", "bn", "residual"):
        assert {k.get(opt, False) for k in cases} == {False, True}, opt
    assert {k["No"] for k in R.MIX} == {1, 16, 30, 75, 200} and {k["T"] * k["Fi"] for k in R.MIX} == {14, 70, 75, 128}
    assert {k.get("mix_bias", False) for k in R.MIX} == {False, True} and {k.get("slope", 1.0) for k in R.MIX} == {1.0, 0.0, 0.01}
    assert {k["V"] for k in R.GATHER} == {1, 15, 16, 17, 33, 700} and {k["Fi"] for k in R.GATHER} == {1, 7, 8, 33, 75}
    assert {k["T"] for k in R.GATHER} == {1, 5, 8} and {k["n_types"] for k in R.GATHER} >= {1, 2, 4}
    assert all(k["T"] * R.rnd(k["Fi"], 8) <= 512 for k in R.GATHER)
    T, nbytes = R.largest_tile_shape()
    assert 64 * 1024 < nbytes <= 160 * 1024 and ops.tower_layer_bf16_lds_bytes(T + 2, 33, 3, 2, False) > 160 * 1024
    assert 2 * (T + 1) * 40 > 4096 or ops.tower_layer_bf16_lds_bytes(T + 1, 33, 3, 2, False) > 160 * 1024


@pytest.mark.parametrize("i", range(len(R.MIX)))
def test_mix_bar_rejects_a_dropped_bias(i):
    c = R.mix_case(i)
    x = R.emulated_x_cat(c)
    ref, tol = R.mix_expect(c, x)
    assert R.outside(ref, ref, tol) == 0
    if R.MIX[i].get("mix_bias"):
        assert R.outside(R.mix_expect(c, x, ("drop_mix_bias",))[0], ref, tol) > 0, "mix_bias dropped"
    assert sum(bool(k.get("mix_bias")) for k in R.MIX) >= 3


# ---- refusals before any launch ----------------------------------------------------------------------------------------------------
def _args(**kw):
    """A ZINC-shaped call on placeholder pointers (never launched: every use below is refused first, or has V = 0)."""
    a = _lib.PnaTowerLayerBf16Args()
    a.V, a.n_tower, a.Fi, a.Fo, a.n_scaler, a.n_aggr, a.mix_slope = 100, 5, 75, 15, 3, 4, 0.01
    for i, code in enumerate((0, 2, 3, 4)):
        a.aggr[i] = code
    p = ctypes.c_void_p(64)
    a.rowptr = a.col = a.h = a.x_cat = a.proj_img = a.post_img = a.y = p
    a.ldh, a.ldx, a.ldy = 75, 800, 75
    for k, v in kw.items():
        setattr(a, k, v)
    return a


P64, P72 = ctypes.c_void_p(64), ctypes.c_void_p(72)
SIMPLE = dict(n_tower=1, Fi=80, Fo=80, ldh=80, ldy=80, no_self_panel=1, x_cat=None, proj_img=None)
EDGE = dict(edge_type=P64, edge_table=P64, ld_edge_table=400, n_edge_types=4)
REFUSED = [
    (dict(col_shift=P64), b"col_scale / col_shift"),
    (dict(col_scale=P64), b"col_scale / col_shift"),
    (dict(mix_slope=1.5), b"mix_slope"),
    (dict(mix_slope=float("nan")), b"mix_slope"),
    (dict(mix_slope=-0.01), b"mix_slope"),
    (dict(SIMPLE, n_tower=2), b"no_self_panel"),
    (dict(SIMPLE, mix_img=P64, No=80), b"no_self_panel"),
    (dict(SIMPLE, **EDGE), b"no_self_panel"),
    (dict(EDGE, n_edge_types=0), b"edge_type needs"),
    (dict(EDGE, n_edge_types=5), b"edge_type needs"),
    (dict(EDGE, ld_edge_table=404), b"edge_type needs"),          # wide enough (>= 5 * 80), not a multiple of 8
    (dict(EDGE, edge_table=P72), b"edge_type needs"),
    (dict(ldx=804), b"x_cat"),
    (dict(proj_img=P72), b"16-byte aligned"),
    (dict(mix_img=P72, No=75), b"16-byte aligned"),
    (dict(mix_img=P64, No=76, ldy=75), b"ldh / ldy / ld_res"),     # with a mixing network the rows of y hold No columns
    (dict(mix_img=P64, No=75, residual=P64, ld_res=74), b"ldh / ldy / ld_res"),
    (dict(mix_img=P64, No=0), b"No <= 4096"),
    (dict(mix_img=P64, No=4097, ldy=4097), b"No <= 4096"),
]


@pytest.mark.parametrize("kw,message", REFUSED, ids=lambda v: "_".join(f"{k}" for k in v) if isinstance(v, dict) else None)
def test_entry_point_refuses_before_any_launch(kw, message):
    L = _lib.lib()
    assert L.pna_tower_layer_bf16(ctypes.byref(_args(**kw)), None) == -1, kw
    assert message in L.pna_last_error(), (kw, L.pna_last_error())


def test_tile_just_over_160_kib_is_refused():
    """The first per-tower width whose tile ops.tower_layer_bf16_lds_bytes puts over 160 KiB is refused, the width before it passes
    the same check (V = 0: the entry point returns after its checks, nothing is launched)."""
    L = _lib.lib()
    for T, Fo, A, divide, No in ((5, 15, 4, False, 75), (1, 16, 8, False, None), (8, 16, 2, True, 128)):
        fits = [Fi for Fi in range(1, 2049) if ops.tower_layer_bf16_lds_bytes(T, Fi, Fo, A, divide, No=No) <= 160 * 1024]
        Fi = max(fits) + 1
        assert fits == list(range(1, Fi)) and Fi <= 2048
        over, under = ops.tower_layer_bf16_lds_bytes(T, Fi, Fo, A, divide, No=No), ops.tower_layer_bf16_lds_bytes(T, Fi - 1, Fo, A, divide, No=No)
        assert under <= 160 * 1024 < over
        kw = dict(V=0, n_tower=T, Fo=Fo, n_aggr=A, divide_input=int(divide), mix_img=P64 if No else None, No=No or 0)
        assert L.pna_tower_layer_bf16(ctypes.byref(_args(Fi=Fi, **kw)), None) == -1 and b"LDS" in L.pna_last_error(), (T, Fi, over)
        assert L.pna_tower_layer_bf16(ctypes.byref(_args(Fi=Fi - 1, **kw)), None) == 0, (T, Fi - 1, under, L.pna_last_error())
