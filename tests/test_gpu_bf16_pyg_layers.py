"""bf16 inference of the PyG front end (PNAConv, PNAConvSimple) against float64 models of the reference's formulas.

The yardstick is the project's (tests/test_gpu_bf16_tower_layers.py): rho(gpu) <= 2 rho(emu), rho(x) = max_j |x_j - ref64_j| / E_j
over EVERY element, emu the float64 model rounded at the contract's points P0-P4 only, E the bound those roundings propagate to the
output (tests/bf16_pyg_ref.py).  Without its roundings the model equals the golden `out` of the reference's own code to 1e-5.
Teeth: the emulation falsified one rule at a time -- the x_i / x_j halves swapped, the empty-row std rule dropped, attenuation's
deg == 0 -> 1 rule dropped, the lin bias dropped -- exceeds 2 rho(emu) on at least one fixture each."""
import numpy as np
import pytest
import torch

import bf16_pyg_ref as R
import bf16_tower_ref as B
from conftest import golden_names, load_golden
from pna_amd import functional as PF, ops
from pna_amd.capture import GraphedForward
from pna_amd.pytorch_geometric import PNAConv, PNAConvSimple
from pna_amd.pytorch_geometric.pna import _graph_of

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FIXTURES = ["pyg_simple_hiv", "pyg_conv_towers", "pyg_conv_edge_divide", "pyg_conv_deep"]
ROUTES = {"multi_launch": 0, "default": 4096}


def _build(meta, a, sd=None):
    if meta["kind"] == "pyg_simple":
        layer = PNAConvSimple(meta["F"], meta["out"], meta["aggregators"], meta["scalers"], a["deg_hist"], post_layers=meta["post_layers"])
    else:
        layer = PNAConv(meta["in_c"], meta["out_c"], meta["aggregators"], meta["scalers"], a["deg_hist"], edge_dim=meta["edge_dim"] or None,
                        towers=meta["towers"], pre_layers=meta["pre_layers"], post_layers=meta["post_layers"], divide_input=meta["divide_input"])
    if sd is not None:
        layer.load_state_dict(sd)
    return layer.eval()


def _models(layer, meta, edge_index, N, x, edge_attr, falsify=None):
    sd = {k: B.f64(v) for k, v in layer.state_dict().items()}
    return R.layer_models(meta["kind"], sd, meta, edge_index.cpu(), N, B.f64(x), None if edge_attr is None else B.f64(edge_attr),
                          layer.avg_deg, falsify=falsify)


def _figures(layer, meta, edge_index, N, x, edge_attr, out):
    ref, emu, E = _models(layer, meta, edge_index, N, x, edge_attr)
    f = {"elements": ref.numel(), "rho_emu": B.rho(emu, ref, E), "rho_gpu": B.rho(B.f64(out), ref, E),
         "rho_zero_output": B.rho(torch.zeros_like(ref), ref, E)}
    for name in R.FALSIFICATIONS:
        f[name] = B.rho(_models(layer, meta, edge_index, N, x, edge_attr, falsify=name)[1], ref, E)
    return f


_CACHE = {}


def _fixture(name, device):
    """The golden fixture cast to bf16 on the device, its float64 figures computed once and shared by the routes."""
    if name not in _CACHE:
        meta, a, sd = load_golden(name)
        layer32 = _build(meta, a, sd)
        ea32 = a["edge_attr"] if meta.get("edge_dim") else None
        ref32 = _models(layer32, meta, a["edge_index"], meta["N"], a["x"], ea32)[0]      # the model without roundings on the fp32 values
        tie = float((ref32 - a["out"].double()).abs().max())
        _CACHE[name] = (meta, a, sd, tie)
    meta, a, sd, tie = _CACHE[name]
    layer = _build(meta, a, sd).to(device).to(BF)
    x = a["x"].to(device).to(BF)
    ea = a["edge_attr"].to(device).to(BF) if meta.get("edge_dim") else None
    return meta, a, layer, x, a["edge_index"].to(device), ea, tie


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_meet_the_contract_on_both_routes(cuda_device, monkeypatch, name, route):
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", ROUTES[route])
    seen = []
    small = ops.tower_layer_bf16
    monkeypatch.setattr(ops, "tower_layer_bf16", lambda *a_, **k: (seen.append(1), small(*a_, **k))[1])
    meta, a, layer, x, ei, ea, tie = _fixture(name, cuda_device)
    assert int((torch.bincount(a["edge_index"][1], minlength=meta["N"]) == 0).sum()) >= 2          # nodes without in-edges
    assert tie <= 1e-5, f"the float64 model is not the reference's layer: {tie}"
    with torch.no_grad():
        out = layer(x, ei, ea)
        again = layer(x, ei, ea)
    assert out.dtype == BF and out.shape == a["out"].shape and torch.equal(out, again)
    # the one-call kernel: a 1-layer pre_nn and post_nn, no per-edge features (pyg_conv_edge_divide's are continuous: no type table)
    one_call = route == "default" and meta.get("pre_layers", 1) == 1 and meta["post_layers"] == 1 and not meta.get("edge_dim")
    assert len(seen) == (2 if one_call else 0), (route, seen)
    f = _figures(layer, meta, ei, meta["N"], x, ea, out)
    print(name, route, f)
    assert f["rho_zero_output"] > 2 * f["rho_emu"]
    assert f["rho_gpu"] <= 2 * f["rho_emu"], f


def test_the_bar_has_teeth_for_every_pyg_rule(cuda_device):
    """Each falsified emulation exceeds 2 rho(emu) on at least one fixture (the table of DESIGN.md 4.14)."""
    table = {}
    for name in FIXTURES:
        meta, a, layer, x, ei, ea, _ = _fixture(name, cuda_device)
        ref, emu, E = _models(layer, meta, ei, meta["N"], x, ea)
        r0 = B.rho(emu, ref, E)
        table[name] = {k: B.rho(_models(layer, meta, ei, meta["N"], x, ea, falsify=k)[1], ref, E) / r0 for k in R.FALSIFICATIONS}
    print(table)
    for k in R.FALSIFICATIONS:
        assert max(table[n][k] for n in FIXTURES) > 2, (k, table)


def _random_graph(V, E, n_empty, seed, hub=0):
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, V, (E,), generator=gen)
    dst = torch.randint(n_empty, V, (E,), generator=gen)            # rows [0, n_empty) have no in-edges
    if hub:
        src = torch.cat([src, torch.randint(0, V, (hub,), generator=gen)])
        dst = torch.cat([dst, torch.full((hub,), n_empty)])
    perm = torch.randperm(src.numel(), generator=gen)
    return torch.stack([src[perm], dst[perm]])


def _random_layer(meta, ei, N, seed, device):
    torch.manual_seed(seed)
    hist = torch.bincount(torch.bincount(ei[1], minlength=N))
    layer = _build(meta, {"deg_hist": hist})
    with torch.no_grad():
        for m in layer.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.5, 0.5)
    return layer.to(device).to(BF)


CONV = dict(kind="pyg_conv", aggregators=["mean", "min", "max", "std"], scalers=["identity", "amplification", "attenuation"],
            divide_input=False, edge_dim=0, pre_layers=1, post_layers=1)
SIX = ["sum", "mean", "min", "max", "var", "std"]
BIG = [
    # a 1003-edge hub (the heavy-row segments) and rows without in-edges, every route of both layers
    ("hub_simple", dict(kind="pyg_simple", F=33, out=20, aggregators=SIX, scalers=["attenuation", "linear", "identity"], post_layers=2), 600, 2400, 1003),
    ("hub_conv", dict(CONV, in_c=24, out_c=32, towers=4, divide_input=True, edge_dim=5, aggregators=SIX, scalers=["inverse_linear", "identity"]), 600, 2400, 1003),
    ("hub_conv_deep", dict(CONV, in_c=20, out_c=10, towers=2, pre_layers=3, edge_dim=4, post_layers=2), 600, 2400, 1003),
    # many workgroups: V = 20 000, E = 100 003, F = 75
    ("wide_simple", dict(kind="pyg_simple", F=75, out=75, aggregators=CONV["aggregators"], scalers=CONV["scalers"], post_layers=1), 20000, 100003, 0),
    ("wide_conv", dict(CONV, in_c=75, out_c=75, towers=1), 20000, 100003, 0),
    ("wide_conv_deep", dict(CONV, in_c=75, out_c=75, towers=1, pre_layers=2), 20000, 100003, 0),
]


@pytest.mark.parametrize("name,meta,V,E,hub", BIG, ids=[b[0] for b in BIG])
def test_hub_rows_and_many_workgroups(cuda_device, name, meta, V, E, hub):
    ei = _random_graph(V, E, 5, seed=len(name), hub=hub)
    layer = _random_layer(meta, ei, V, seed=V + hub, device=cuda_device)
    gen = torch.Generator().manual_seed(E)
    in_c = meta.get("in_c", meta.get("F"))
    x = (torch.randn(V, in_c, generator=gen) * 1.5 + 0.25).to(BF).to(cuda_device)
    ea = (torch.randn(ei.shape[1], meta["edge_dim"], generator=gen)).to(BF).to(cuda_device) if meta.get("edge_dim") else None
    eid = ei.to(cuda_device)
    with torch.no_grad():
        out = layer(x, eid, ea)
    assert (_graph_of(eid, V).heavy_schedule().n_heavy == 1) == bool(hub)
    ref, emu, Eb = _models(layer, meta, ei, V, x, ea)
    f = {"elements": ref.numel(), "rho_emu": B.rho(emu, ref, Eb), "rho_gpu": B.rho(B.f64(out), ref, Eb),
         "rho_zero_output": B.rho(torch.zeros_like(ref), ref, Eb)}
    print(name, f)
    assert f["rho_zero_output"] > 2 * f["rho_emu"]
    assert f["rho_gpu"] <= 2 * f["rho_emu"], f


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("pre_layers", [1, 2])
def test_edge_features_of_four_types_on_both_routes(cuda_device, monkeypatch, route, pre_layers):
    """edge_attr takes 4 distinct rows (bond types): P0 and P1 run over the table's rows, and with pre_layers = 1 the default route is
    the one-call kernel with its edge table."""
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", ROUTES[route])
    seen = []
    small = ops.tower_layer_bf16
    monkeypatch.setattr(ops, "tower_layer_bf16", lambda *a_, **k: (seen.append(k), small(*a_, **k))[1])
    V, ed = 500, 7
    meta = dict(CONV, in_c=27, out_c=12, towers=3, edge_dim=ed, pre_layers=pre_layers, scalers=["attenuation", "identity", "linear"])
    ei = _random_graph(V, 2000, 6, seed=31)
    layer = _random_layer(meta, ei, V, seed=5, device=cuda_device)
    gen = torch.Generator().manual_seed(8)
    x = (torch.randn(V, 27, generator=gen) * 1.5 + 0.25).to(BF).to(cuda_device)
    ea = torch.randn(4, ed, generator=gen).to(BF)[torch.randint(0, 4, (ei.shape[1],), generator=gen)].to(cuda_device)
    eid = ei.to(cuda_device)
    with torch.no_grad():
        out = layer(x, eid, ea)
    assert _graph_of(eid, V).edge_type_table(ea) is not None
    assert len(seen) == (1 if route == "default" and pre_layers == 1 else 0) and all(k["edge_table"] is not None for k in seen)
    ref, emu, Eb = _models(layer, meta, ei, V, x, ea)
    f = {"rho_emu": B.rho(emu, ref, Eb), "rho_gpu": B.rho(B.f64(out), ref, Eb), "rho_zero_output": B.rho(torch.zeros_like(ref), ref, Eb)}
    print(route, pre_layers, f)
    assert f["rho_zero_output"] > 2 * f["rho_emu"]
    assert f["rho_gpu"] <= 2 * f["rho_emu"], f


# ---- capture --------------------------------------------------------------------------------------------------------------------
def _no_host_sync(fn):
    """fn() under torch's sync debug mode: a device-to-host copy, a nonzero() or an .item() raises."""
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("route", list(ROUTES))
def test_simple_conv_under_hipgraph_capture(cuda_device, monkeypatch, route):
    monkeypatch.setattr(PF, "BF16_SMALL_ROWS", ROUTES[route])
    V = 900
    ei = _random_graph(V, 3600, 4, seed=21).to(cuda_device)
    meta = dict(kind="pyg_simple", F=80, out=80, aggregators=CONV["aggregators"], scalers=CONV["scalers"], post_layers=1)
    layer = _random_layer(meta, ei.cpu(), V, seed=1, device=cuda_device)
    gen = torch.Generator().manual_seed(2)
    xs = [(torch.randn(V, 80, generator=gen) * 1.5).to(BF).to(cuda_device) for _ in range(2)]
    with torch.no_grad():
        want = [layer(x, ei).clone() for x in xs]
        _no_host_sync(lambda: layer(xs[1], ei))                       # after its warm-up calls a forward makes no host synchronisation
        gf = GraphedForward(lambda x: layer(x, ei), xs[0])
        got = [gf(x).clone() for x in xs]
        again = [gf(xs[1]).clone() for _ in range(5)]
    assert not torch.equal(want[0], want[1])
    for w, o in zip(want, got):
        assert torch.equal(w, o)
    assert all(torch.equal(o, want[1]) for o in again)


@pytest.mark.parametrize("pre_layers", [1, 2])
def test_conv_with_edge_attr_under_hipgraph_capture(cuda_device, monkeypatch, pre_layers):
    """edge_attr is an input of the capture and nobody registered its types: the capture takes the per-edge multi-launch route, and a
    replay equals the eager call on the multi-launch kernels bit for bit (R(W_e enc) per type or per edge are the same bf16 rows)."""
    V, ed = 900, 6
    ei = _random_graph(V, 3600, 4, seed=22).to(cuda_device)
    meta = dict(CONV, in_c=75, out_c=75, towers=5, edge_dim=ed, pre_layers=pre_layers)
    layer = _random_layer(meta, ei.cpu(), V, seed=3, device=cuda_device)
    gen = torch.Generator().manual_seed(6)
    xs = [(torch.randn(V, 75, generator=gen) * 1.5).to(BF).to(cuda_device) for _ in range(2)]
    table = torch.randn(4, ed, generator=gen).to(BF)
    eas = [table[torch.randint(0, 4, (ei.shape[1],), generator=gen)].to(cuda_device) for _ in range(2)]
    with torch.no_grad():
        gf = GraphedForward(lambda x, e: layer(x, ei, e), xs[0], eas[0])
        got = [gf(x, e).clone() for x, e in zip(xs, eas)]
        monkeypatch.setattr(PF, "BF16_SMALL_ROWS", 0)
        want = [layer(x, ei, e).clone() for x, e in zip(xs, eas)]
        # continuous edge features: no table, the same route eagerly and captured
        cont = (torch.randn(ei.shape[1], ed, generator=gen)).to(BF).to(cuda_device)
        w2 = layer(xs[0], ei, cont).clone()
        _no_host_sync(lambda: layer(xs[0], ei, cont))
    assert not torch.equal(want[0], want[1]) and not torch.equal(w2, want[0])
    for w, o in zip(want, got):
        assert torch.equal(w, o)
    assert torch.equal(gf(xs[0], cont), w2)


# ---- what stays as it was -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names("pyg_simple") + golden_names("pyg_conv"))
def test_fp32_outputs_are_untouched_by_a_bf16_call_on_a_converted_copy(cuda_device, name):
    import copy
    meta, a, sd = load_golden(name)
    layer = _build(meta, a, sd).to(cuda_device)
    x, ei = a["x"].to(cuda_device), a["edge_index"].to(cuda_device)
    ea = a["edge_attr"].to(cuda_device) if meta.get("edge_dim") else None
    with torch.no_grad():
        before = layer(x, ei, ea).clone()
        twin = copy.deepcopy(layer).to(BF)
        try:
            twin(x.to(BF), ei, None if ea is None else ea.to(BF))
        except (TypeError, RuntimeError):
            assert name == "pyg_simple_all"                          # five scalers: outside the predicate
        after = layer(x, ei, ea)
        back = twin.float()(x, ei, ea)                               # ... and a round trip through bf16 leaves no bf16 operand behind
    assert torch.equal(before, after)
    assert before.dtype == torch.float32 and back.dtype == torch.float32 and torch.isfinite(back).all()
    torch.testing.assert_close(after, a["out"].to(cuda_device), rtol=1e-5, atol=1e-5)


def test_five_scalers_in_bf16_raise_as_before(cuda_device):
    meta, a, sd = load_golden("pyg_simple_all")
    assert len(meta["scalers"]) == 5
    layer = _build(meta, a, sd).to(cuda_device).to(BF)
    with torch.no_grad(), pytest.raises((TypeError, RuntimeError)):
        layer(a["x"].to(cuda_device).to(BF), a["edge_index"].to(cuda_device))
    with torch.no_grad(), pytest.raises((TypeError, RuntimeError)):
        layer.aggregate(a["x"].to(cuda_device).to(BF), a["edge_index"].to(cuda_device))      # the materialised tensor stays fp32-only
