"""pna_tower_layer_bf16 -- the bf16 tower layer of molecule batches as one C call -- and hipGraph capture of the bf16 layers and nets.

Accuracy: the bar of test_gpu_bf16_tower_layers.py, rho(gpu) <= 2 rho(emu) with rho(x) = max_j |x_j - ref64_j| / E_j over every
element, against the float64 models of bf16_tower_ref.py built from the layer's own state_dict.  Every test sets
functional.BF16_SMALL_ROWS itself and spies on ops.tower_layer_bf16, so none depends on the measured default.
Capture: a replay equals the eager call on the same inputs bit for bit (the kernels fix the order of every sum)."""
import copy

import pytest
import torch

import bf16_tower_ref as B
import test_gpu_bf16_simple_layer as SL
import test_gpu_bf16_tower_layers as TL
from conftest import load_golden
from pna_amd import functional as PF
from pna_amd import ops
from pna_amd.capture import GraphedForward
from pna_amd.dgl.pna_layer import PNALayer, PNASimpleLayer
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SMALL_FIXTURES = ["tower_f75", "tower_zinc_first", "tower_zinc_last", "tower_edgetype", "tower_edgetype_div", "tower_hiv_t8_div"]


@pytest.fixture
def spy(monkeypatch):
    """Calls of the one-call kernel's wrapper (their keyword arguments), and of the multi-launch gather."""
    seen = {"small": [], "gather": []}
    small, gather = ops.tower_layer_bf16, ops.gather_bf16
    monkeypatch.setattr(ops, "tower_layer_bf16", lambda *a, **k: (seen["small"].append(k), small(*a, **k))[1])
    monkeypatch.setattr(ops, "gather_bf16", lambda *a, **k: (seen["gather"].append(k), gather(*a, **k))[1])
    return seen


@pytest.mark.parametrize("rows", [1 << 20, 0], ids=["one_call", "multi_launch"])
@pytest.mark.parametrize("name", SMALL_FIXTURES)
def test_fixtures_take_the_one_call_kernel(cuda_device, monkeypatch, spy, name, rows):
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", rows)
    f = TL.layer_figures(name, cuda_device)
    print(f)
    assert (len(spy["small"]), len(spy["gather"])) == ((1, 0) if rows else (0, 1)), spy
    assert f["elements"] >= 2000
    assert f["rho_zero_output"] > 2 * f["rho_emu"] and f["rho_no_destination_term"] > 2 * f["rho_emu"], f   # the bar's own teeth
    assert f["rho_gpu"] <= 2 * f["rho_emu"], f


def _graph(V, E, n_empty, n_types, seed, hub=0):
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, V, (E,), generator=gen)
    dst = torch.randint(n_empty, V, (E,), generator=gen)            # rows [0, n_empty) have no in-edges
    if hub:
        src = torch.cat([src, torch.randint(0, V, (hub,), generator=gen)])
        dst = torch.cat([dst, torch.full((hub,), n_empty)])
    types = torch.randint(0, max(n_types, 1), (src.numel(),), generator=gen)
    return src, dst, types


def _random_layer(cfg, in_dim, out_dim, edge_dim, seed, posttrans_layers=1):
    torch.manual_seed(seed)
    layer = PNALayer(in_dim, out_dim, cfg["aggregators"], cfg["scalers"], {"log": torch.tensor(1.25)}, 0.0, cfg["graph_norm"],
                     cfg["batch_norm"], towers=cfg["towers"], divide_input=cfg["divide_input"], residual=cfg["residual"],
                     edge_features=edge_dim > 0, edge_dim=edge_dim, posttrans_layers=posttrans_layers)
    with torch.no_grad():
        for t in layer.towers:
            b = t.batchnorm_h
            b.weight.uniform_(0.5, 1.5)
            b.bias.uniform_(-0.5, 0.5)
            b.running_mean.uniform_(-0.3, 0.3)
            b.running_var.uniform_(0.5, 2.0)
            for fc in list(t.pretrans.fully_connected) + list(t.posttrans.fully_connected):
                fc.linear.bias.uniform_(-0.5, 0.5)
    return layer.eval().to(BF)


def _figures(layer, cfg, src, dst, V, h, e, sn, out, towers_only=False):
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in layer.state_dict().items()}
    ref, emu, E = B.layer_models(sd, cfg, src, dst, V, B.f64(h), None if e is None else B.f64(e), B.f64(sn), 1.25,
                                 stop_after_towers=towers_only)
    return {"rho_emu": B.rho(emu, ref, E), "rho_gpu": B.rho(B.f64(out), ref, E), "rho_zero_output": B.rho(torch.zeros_like(ref), ref, E)}


# towers, Fi (per-tower width), divide_input, aggregators, scalers, edge table, graph norm, BatchNorm, residual, mixing network, pitched
SHAPES = [
    (1, 16, False, "mean max min std", "identity amplification attenuation", False, True, True, True, True, False),
    (5, 33, False, "sum var max", "amplification", True, False, True, False, True, False),
    (8, 16, True, "mean sum", "attenuation identity", False, True, False, True, True, True),
    (5, 75, False, "mean max min std", "identity amplification attenuation", True, True, True, True, True, True),
    (1, 75, False, "var min std sum", "identity attenuation", False, False, False, False, False, False),
    (5, 16, True, "max std sum mean var min", "identity", True, True, True, False, False, True),
    (8, 33, False, "mean max min std", "amplification attenuation", False, True, True, False, False, False),
    (1, 33, True, "mean max min std", "identity amplification attenuation", True, False, False, True, True, True),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"T{s[0]}_Fi{s[1]}_div{int(s[2])}_{s[3].replace(' ', '-')}_S{len(s[4].split())}"
                                                          f"_et{int(s[5])}_gn{int(s[6])}_bn{int(s[7])}_res{int(s[8])}_mix{int(s[9])}_p{int(s[10])}")
def test_random_shapes(cuda_device, monkeypatch, spy, shape):
    T, Fi, divide, aggs, scalers, etab, gn, bn, res, mix, pitched = shape
    in_dim = T * Fi if divide else Fi
    Fo = (in_dim // T if res and in_dim % T == 0 else 16)
    out_dim = T * Fo
    if out_dim > 128:                                             # the bf16 layers serve at most 128 output columns
        Fo = 128 // T
        out_dim = T * Fo
    cfg = dict(towers=T, divide_input=divide, aggregators=aggs.split(), scalers=scalers.split(), graph_norm=gn, batch_norm=bn,
               residual=res and in_dim == out_dim, edge_features=etab)
    ed = 6 if etab else 0
    V = 700
    src, dst, types = _graph(V, 3000, 9, 3, seed=T * 100 + Fi)
    layer = _random_layer(cfg, in_dim, out_dim, ed, seed=Fi).to(cuda_device)
    gen = torch.Generator().manual_seed(Fi + T)
    x = (torch.randn(V, in_dim, generator=gen) * 1.5 + 0.25).to(BF)
    if pitched:
        buf = torch.full((V, (in_dim + 7) // 8 * 8 + 8), float("nan"), dtype=BF)
        buf[:, :in_dim] = x
        h = buf.to(cuda_device)[:, :in_dim]
        assert h.stride(0) % 8 == 0 and not h.is_contiguous()
    else:
        h = x.to(cuda_device)
    e = None
    if etab:
        e = (torch.randn(3, ed, generator=gen).to(BF))[types].to(cuda_device)
    g = Graph(src, dst, V, [300, 400]).to(cuda_device)
    sn = g.snorm_n().to(BF)
    assert int(torch.bincount(dst, minlength=V)[:9].sum()) == 0
    module = layer if mix else layer.towers[0]
    if not mix:                                                   # PNATower alone: tower 0 of the layer over its input slice
        cfg = dict(cfg, towers=1, divide_input=False)
        h = h[:, :Fi] if divide else h
    outs = {}
    with torch.no_grad():
        for rows in (1 << 20, 0):
            monkeypatch.setattr(PF, "BF16_SMALL_ROWS", rows)
            n = len(spy["small"])
            outs[rows] = module(g, h, e, sn)
            assert len(spy["small"]) == n + (1 if rows else 0)
    if mix:
        f = _figures(layer, cfg, src, dst, V, h, e, sn, outs[1 << 20])
    else:
        sd = {"towers.0." + k: v for k, v in module.state_dict().items()}
        holder = type("L", (), {"state_dict": lambda self: sd})()
        f = _figures(holder, cfg, src, dst, V, h, e, sn, outs[1 << 20], towers_only=True)
    f["max_diff_to_multi_launch"] = float((outs[1 << 20].float() - outs[0].float()).abs().max())     # (for information)
    print(f)
    assert outs[1 << 20].dtype == BF and outs[1 << 20].shape == outs[0].shape
    assert f["rho_zero_output"] > 2 * f["rho_emu"], f
    assert f["rho_gpu"] <= 2 * f["rho_emu"], f


@pytest.mark.parametrize("name", ["simple_f75", "simple_f20_order", "simple_f80_hiv", "simple_f16_default_init"])
def test_simple_layer_fixtures_take_the_one_call_kernel(cuda_device, monkeypatch, spy, name):
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 1 << 20)
    meta, a, sd = load_golden(name)
    layer = PNASimpleLayer(meta["F"], meta["out_dim"], meta["aggregators"], meta["scalers"], {"log": a["avg_log"]}, 0.0,
                           meta["batch_norm"], meta["residual"], posttrans_layers=meta["posttrans_layers"])
    layer.load_state_dict(sd)
    layer = layer.to(cuda_device).eval().to(BF)
    g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
    assert g.heavy_schedule().n_heavy == 0
    h = a["h"].to(cuda_device).to(BF)
    out = SL.run(layer, g, h)
    assert len(spy["small"]) == 1 and spy["small"][0]["no_self_panel"]
    assert out.dtype == BF and out.shape == (meta["N"], meta["out_dim"])
    ref, tol, _ = SL.reference(layer, a["src"], a["dst"], meta["N"], h)
    SL.assert_contract(out, ref, tol, name)
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 0)
    SL.assert_contract(SL.run(layer, g, h), ref, tol, name + " (multi-launch)")
    assert len(spy["small"]) == 1


def test_simple_layer_unaligned_rows(cuda_device, monkeypatch, spy):
    """(V, 75) contiguous rows are not 16-byte aligned: the 2-byte gather of the one-call kernel, with rows of in-degree 0."""
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 1 << 20)
    V = 500
    src, dst, _ = _graph(V, 2500, 7, 0, seed=4)
    g = Graph(src, dst, V).to(cuda_device)
    layer = SL.make_layer(75, 75, "mean sum max min std var", "identity amplification attenuation", 1.7, True, True, seed=2, device=cuda_device)
    h = (torch.randn(V, 75, generator=torch.Generator().manual_seed(3)) * 1.5 + 0.25).to(BF).to(cuda_device)
    out = SL.run(layer, g, h)
    assert len(spy["small"]) == 1
    ref, tol, _ = SL.reference(layer, src, dst, V, h)
    SL.assert_contract(out, ref, tol, "unaligned")


# ---- fallbacks ------------------------------------------------------------------------------------------------------------------
FALLBACK_CFG = dict(towers=5, divide_input=False, aggregators="mean max min std".split(), scalers="identity amplification attenuation".split(),
                    graph_norm=True, batch_norm=True, residual=True, edge_features=False)


@pytest.mark.parametrize("why", ["rows_above_threshold", "hub_row"])
def test_fallbacks_take_the_multi_launch_path(cuda_device, monkeypatch, spy, why):
    V = 600
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 500 if why == "rows_above_threshold" else 1 << 20)
    src, dst, _ = _graph(V, 2500, 3, 0, seed=11, hub=300 if why == "hub_row" else 0)
    layer = _random_layer(FALLBACK_CFG, 40, 40, 0, seed=8).to(cuda_device)
    g = Graph(src, dst, V, [600]).to(cuda_device)
    h = (torch.randn(V, 40, generator=torch.Generator().manual_seed(5)) * 1.5).to(BF).to(cuda_device)
    sn = g.snorm_n().to(BF)
    with torch.no_grad():
        out = layer(g, h, None, sn)
    assert not spy["small"] and len(spy["gather"]) == 1
    f = _figures(layer, FALLBACK_CFG, src, dst, V, h, None, sn, out)
    print(f)
    assert f["rho_gpu"] <= 2 * f["rho_emu"], f


def test_deep_posttrans_keeps_the_multi_launch_path(cuda_device, monkeypatch, spy):
    """posttrans_layers = 2 is not one Linear: the existing route, at the bar of test_deep_posttrans_runs_its_first_linear_on_the_kernel."""
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 1 << 20)
    TL.test_deep_posttrans_runs_its_first_linear_on_the_kernel(cuda_device)
    assert not spy["small"] and len(spy["gather"]) == 1


# ---- capture --------------------------------------------------------------------------------------------------------------------
def _zinc_layer(device, edge_dim=0, seed=1):
    cfg = dict(FALLBACK_CFG, edge_features=edge_dim > 0)
    return _random_layer(cfg, 75, 75, edge_dim, seed=seed).to(device)


@pytest.mark.parametrize("rows", [1 << 20, 0], ids=["one_call", "multi_launch"])
def test_layer_under_hipgraph_capture(cuda_device, monkeypatch, spy, rows):
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", rows)
    V = 900
    src, dst, _ = _graph(V, 3600, 4, 0, seed=21)
    g = Graph(src, dst, V, [400, 500]).to(cuda_device)
    layer = _zinc_layer(cuda_device)
    gen = torch.Generator().manual_seed(2)
    hs = [(torch.randn(V, 75, generator=gen) * 1.5).to(BF).to(cuda_device) for _ in range(2)]
    sn = g.snorm_n().to(BF)
    with torch.no_grad():
        want = [layer(g, h, None, sn).clone() for h in hs]
        gf = GraphedForward(lambda h: layer(g, h, None, sn), hs[0])
        got = [gf(h).clone() for h in hs]
        again = [gf(hs[1]).clone() for _ in range(20)]
    assert bool(spy["small"]) == bool(rows) and bool(spy["gather"]) == (not rows)
    assert not torch.equal(want[0], want[1])
    for w, o in zip(want, got):
        assert torch.equal(w, o)
    assert all(torch.equal(a, want[1]) for a in again)


def test_edge_feature_layer_captured_with_unregistered_edge_features(cuda_device, monkeypatch, spy):
    """`e` is an input of the capture and nobody registered its types: eager calls (and the warm-up) find the 4-row table and take the
    one-call kernel, the capture takes the per-edge multi-launch route, and a replay with OTHER bond types equals eager for them."""
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 1 << 20)
    V, ed = 900, 10
    src, dst, _ = _graph(V, 3600, 4, 0, seed=22)
    g = Graph(src, dst, V, [400, 500]).to(cuda_device)
    layer = _zinc_layer(cuda_device, edge_dim=ed, seed=3)
    gen = torch.Generator().manual_seed(6)
    h = (torch.randn(V, 75, generator=gen) * 1.5).to(BF).to(cuda_device)
    table = torch.randn(4, ed, generator=gen).to(BF)
    es = [table[torch.randint(0, 4, (src.numel(),), generator=gen)].to(cuda_device) for _ in range(2)]
    sn = g.snorm_n().to(BF)
    with torch.no_grad():
        gf = GraphedForward(lambda e: layer(g, h, e, sn), es[0])
        assert spy["small"] and all(k["edge_type"] is not None for k in spy["small"])          # the warm-up calls
        assert len(spy["gather"]) == 1 and spy["gather"][0]["edge_type"] is None               # the capture: per-edge rows
        got = [gf(e).clone() for e in es]
        one_call = [layer(g, h, e, sn).clone() for e in es]
        # eager on the multi-launch kernels: R(W_e ef) per type (the table) or per edge (the capture) are the same bf16 rows, added
        # to the same messages in the same order, so the replay equals it bit for bit
        monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 0)
        want = [layer(g, h, e, sn).clone() for e in es]
    print({"max_diff_replay_to_one_call_eager": [float((o.float() - w.float()).abs().max()) for o, w in zip(got, one_call)]})
    assert not torch.equal(want[0], want[1])
    for w, o in zip(want, got):
        assert torch.equal(w, o)


def _zinc_net(device):
    from pna_amd.nets import PNANet
    torch.manual_seed(3)
    net = PNANet(dict(num_atom_type=28, num_bond_type=4, hidden_dim=75, out_dim=70, in_feat_dropout=0.0, dropout=0.0, L=3, readout="sum",
                      graph_norm=True, batch_norm=True, residual=True, aggregators="mean max min std", scalers="identity amplification attenuation",
                      avg_d={"log": torch.tensor(1.1)}, towers=5, divide_input_first=False, divide_input_last=True, edge_feat=True, edge_dim=50,
                      pretrans_layers=1, posttrans_layers=1, gru=False, device=device)).to(device).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 2:
                p.copy_(torch.randn_like(p) / p.shape[1] ** 0.5)
    return net.to(BF)


def test_molecules_net_in_bf16_under_hipgraph_capture(cuda_device, monkeypatch, spy):
    """test_molecules_net_under_hipgraph_capture_with_varying_bond_types in bf16: atoms AND bond types are inputs, the net registers
    the types from device-side ops, so warm-up and capture both take the one-call kernel with its edge-type table."""
    from pna_amd.synth import molecule_batch
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 1 << 20)
    src, dst, sizes = molecule_batch(64, seed=9)
    V, E = int(sum(sizes)), src.numel()
    g = Graph(src, dst, V, sizes).to(cuda_device)
    net = _zinc_net(cuda_device)
    gen = torch.Generator().manual_seed(1)
    atoms = [torch.randint(0, 28, (V,), generator=gen).to(cuda_device) for _ in range(2)]
    bonds = [torch.randint(0, 4, (E,), generator=gen).to(cuda_device) for _ in range(2)]
    sn = g.snorm_n().to(BF)
    with torch.no_grad():
        want = [net(g, a_, b_, sn, None).clone() for a_, b_ in zip(atoms, bonds)]
        spy["small"].clear()
        gf = GraphedForward(lambda a_, b_: net(g, a_, b_, sn, None), atoms[0], bonds[0])
        assert len(spy["small"]) == 4 * 3 and all(k["edge_type"] is not None for k in spy["small"]) and not spy["gather"]
        got = [gf(a_, b_).clone() for a_, b_ in zip(atoms, bonds)]
    assert want[0].dtype == BF and float((want[0].float() - want[1].float()).abs().max()) > 1e-3
    for w, o in zip(want, got):
        assert torch.equal(w, o)


@pytest.mark.parametrize("edge_feat", [False, True])
def test_superpixels_net_in_bf16_under_hipgraph_capture(cuda_device, monkeypatch, spy, edge_feat):
    """edge_feat=False: the one-call kernel; edge_feat=True: a Linear of a continuous edge value has no table, the per-edge
    multi-launch route is what gets captured."""
    from pna_amd.nets import PNANetSuperpixels
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 1 << 20)
    V, K = 8 * 60, 8
    gen = torch.Generator().manual_seed(12)
    dst = torch.arange(V).repeat_interleave(K)
    src = (dst // 60) * 60 + torch.randint(0, 60, (V * K,), generator=gen)           # K in-edges per node from its own image
    g = Graph(src, dst, V, [60] * 8).to(cuda_device)
    torch.manual_seed(5)
    net = PNANetSuperpixels(dict(in_dim=5, in_dim_edge=1, hidden_dim=60, out_dim=60, n_classes=10, in_feat_dropout=0.0, dropout=0.0, L=2,
                                 readout="mean", graph_norm=True, batch_norm=True, residual=True, aggregators="mean max min std",
                                 scalers="identity amplification attenuation", avg_d={"log": torch.tensor(2.1)}, towers=5,
                                 divide_input_first=True, divide_input_last=True, edge_feat=edge_feat, edge_dim=8, pretrans_layers=1,
                                 posttrans_layers=1, gru=False, device=cuda_device)).to(cuda_device).eval().to(BF)
    xs = [torch.randn(V, 5, generator=gen).to(BF).to(cuda_device) for _ in range(2)]
    es = [torch.rand(V * K, 1, generator=gen).to(BF).to(cuda_device) for _ in range(2)]
    sn = g.snorm_n().to(BF)
    with torch.no_grad():
        want = [net(g, x, e, sn, None).clone() for x, e in zip(xs, es)]
        spy["small"].clear(), spy["gather"].clear()
        gf = GraphedForward(lambda x, e: net(g, x, e, sn, None), xs[0], es[0])
        if edge_feat:
            assert not spy["small"] and len(spy["gather"]) == 4 * 2 and all(k["edge_type"] is None for k in spy["gather"])
        else:
            assert len(spy["small"]) == 4 * 2 and not spy["gather"]
        got = [gf(x, e).clone() for x, e in zip(xs, es)]
    assert want[0].dtype == BF and not torch.equal(want[0], want[1])
    for w, o in zip(want, got):
        assert torch.equal(w, o)


def test_fp32_forward_unchanged_by_one_call_and_captured_bf16_calls(cuda_device, monkeypatch, spy):
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 1 << 20)
    meta, a, sd = load_golden("tower_edgetype")
    layer16 = TL._tower_layer(meta, a, sd, cuda_device)
    layer32 = copy.deepcopy(layer16).float()
    g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
    h, sn, e = a["h"].to(cuda_device), a["snorm_n"].to(cuda_device), a["e"].to(cuda_device)
    with torch.no_grad():
        before = layer32(g, h, e, sn)
        layer16(g, h.to(BF), e.to(BF), sn.to(BF))
        e16 = e.to(BF)
        gf = GraphedForward(lambda x: layer16(g, x, e16, sn.to(BF)), h.to(BF))
        gf(h.to(BF))
        after = layer32(g, h, e, sn)
    assert spy["small"]
    assert before.dtype == torch.float32 and torch.equal(before, after)
