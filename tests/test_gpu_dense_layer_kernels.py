"""pna_dense_layer_fwd_f32 / _bwd_f32 through autograd.DenseLayerFn on the GPU: the output and every gradient per element against float64
within 4 x the fp32 oracle's own error + 2^-20 max|ref64| (tests/dense_layer_cases.py; the bar is capped at 1e-4 max|ref64| on the host),
bitwise repeatability, the tie rule and the empty row / column against the existing route, and the scope's refusals."""
import ctypes

import pytest
import torch

import dense_layer_cases as C
from pna_amd import _lib
from pna_amd import autograd as AG
from pna_amd import functional as PF

pytestmark = pytest.mark.gpu


def _run(layer, x, adj, go):
    """One forward + backward through the one-call route: {'out', 'x', <parameter name>} on the CPU."""
    x = x.clone().requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    out = AG.dense_layer(layer, x, adj)
    out.backward(go)
    res = {"out": out.detach().cpu(), "x": x.grad.cpu()}
    res.update({k: p.grad.cpu() for k, p in layer.named_parameters()})
    return res


@pytest.mark.parametrize("name", C.NAMES)
def test_forward_and_every_gradient_against_float64(cuda_device, name):
    c = C.dense_case(name)
    ref64, _, bars = C.references(name)
    layer = C.make_layer(c, cuda_device)
    got = _run(layer, c["x"].to(cuda_device), c["adj"].to(cuda_device), c["go"].to(cuda_device))
    assert set(got) == set(ref64)
    ratios = {k: C.worst_ratio(got[k], ref64[k], bars[k]) for k in ref64}
    worst = max(ratios, key=ratios.get)
    print(f"DENSE_RATIO {name} worst {worst} {ratios[worst]:.3f} out {ratios['out']:.3f} x {ratios['x']:.3f}")
    assert all(torch.isfinite(v).all() for v in got.values())
    assert all(r <= 1.0 for r in ratios.values()), {k: round(r, 3) for k, r in ratios.items() if r > 1.0}


@pytest.mark.parametrize("name", ["n15", "n65", "slab"])
def test_two_calls_give_identical_bits(cuda_device, name):
    c = C.dense_case(name)
    layer = C.make_layer(c, cuda_device)
    args = (c["x"].to(cuda_device), c["adj"].to(cuda_device), c["go"].to(cuda_device))
    a, b = _run(layer, *args), _run(layer, *args)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_without_grad_and_with_unwanted_gradients(cuda_device):
    """no_grad runs the forward alone; a backward that wants grad_x only, or the parameters only, gives the full run's bits."""
    c = C.dense_case("n15")
    layer = C.make_layer(c, cuda_device)
    x, adj, go = c["x"].to(cuda_device), c["adj"].to(cuda_device), c["go"].to(cuda_device)
    full = _run(layer, x, adj, go)
    with torch.no_grad():
        assert torch.equal(AG.dense_layer(layer, x, adj).cpu(), full["out"])
    for p in layer.parameters():
        p.grad = None
    AG.dense_layer(layer, x, adj).backward(go)                                     # x wants no gradient
    for k, p in layer.named_parameters():
        assert torch.equal(p.grad.cpu(), full[k]), k
    layer.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    AG.dense_layer(layer, xg, adj).backward(go)
    assert torch.equal(xg.grad.cpu(), full["x"])


def _both_routes(layer, x, adj, go, monkeypatch):
    """(one-call route, existing route) in this process: {'out', 'x', parameters}."""
    new = _run(layer, x, adj, go)
    monkeypatch.setattr(PF, "DENSE_LAYER_ROWS", 0)
    xo = x.clone().requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    out = layer(xo, adj)
    out.backward(go)
    old = {"out": out.detach().cpu(), "x": xo.grad.cpu()}
    old.update({k: p.grad.cpu() for k, p in layer.named_parameters()})
    return new, old


def test_hand_built_ties_pick_the_existing_routes_winner(cuda_device, monkeypatch):
    """Exactly representable values with every column's maximum and minimum attained several times: the one-call route and the existing
    route (knob off, same process) agree bit for bit -- forward and gradients -- with max / min the only aggregators, where nothing but the
    winner's identity could differ (every sum is over a few small dyadic numbers: exact in any order)."""
    from pna_amd.pytorch.pna.layer import PNALayer
    B, N, T, Fi, Fo = 2, 6, 2, 2, 2
    layer = PNALayer(T * Fi, T * Fo, ["max", "min"], ["identity"], C.AVG_D, towers=T, divide_input=True, device="cpu")
    gen = torch.Generator().manual_seed(5)
    q = lambda *s: torch.randint(-4, 5, s, generator=gen).float() / 4.0            # noqa: E731  (multiples of 1/4)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(q(*p.shape))
    layer.mixing_network.activation.negative_slope = 0.25                           # (0.01 is no dyadic number: its products round)
    layer = layer.to(cuda_device)
    x = q(B, N, T * Fi)
    x[:, 1] = x[:, 0]                                                               # nodes 0, 1 and 4 carry one row: P ties among them
    x[:, 4] = x[:, 0]
    x[:, 5] = x[:, 2]
    adj = torch.ones(B, N, N)
    adj[0, 0, 3] = 0.0
    adj[1, 2, :] = 0.0
    adj[1, 2, 1] = 1.0
    go = q(B, N, T * Fo)
    new, old = _both_routes(layer, x.to(cuda_device), adj.to(cuda_device), go.to(cuda_device), monkeypatch)
    for k in new:
        assert torch.equal(new[k], old[k]), (k, (new[k] - old[k]).abs().max())


def test_isolated_node_matches_the_existing_route(cuda_device, monkeypatch):
    """A node without any edge (an empty row AND an empty column), scalers identity + amplification: 0 in its blocks, as the existing
    route gives.  The oracle has no value for an empty row (0 / 0), so the bar is that of the same layer on the same graphs with the node
    still connected: 4 x the fp32 oracle's error + 2^-20 max|ref64| per tensor."""
    c = dict(C.dense_case("n15"))
    c["scalers"] = ["identity", "amplification"]
    A, S, Fi, Fo = 4, 2, c["Fi"], c["Fo"]
    gen = torch.Generator().manual_seed(77)
    sd = dict(c["sd"])
    for t in range(c["T"]):
        sd[f"towers.{t}.posttrans.fully_connected.0.linear.weight"] = torch.randn(Fo, (1 + A * S) * Fi, generator=gen) / ((1 + A * S) * Fi) ** 0.5
    c["sd"] = sd
    _, _, bars = C.references_of(c)
    adj = c["adj"].clone()
    adj[:, 5, :] = 0.0
    adj[:, :, 5] = 0.0
    layer = C.make_layer(c, cuda_device)
    new, old = _both_routes(layer, c["x"].to(cuda_device), adj.to(cuda_device), c["go"].to(cuda_device), monkeypatch)
    for k in new:
        err = float((new[k] - old[k]).abs().max())
        print(f"DENSE_ISOLATED {k} err {err:.3e} bar {bars[k]:.3e}")
        assert torch.isfinite(new[k]).all()
        assert err <= bars[k], (k, err, bars[k])


def _scope_args(**kw):
    """An args struct inside the scope except for `kw`; the pointers are non-null but never followed: every check precedes a launch."""
    a = _lib.PnaDenseLayerArgs()
    a.B, a.N, a.in_dim, a.n_tower, a.Fi, a.Fo, a.divide_input, a.n_aggr, a.n_scaler = 2, 8, 8, 2, 4, 4, 1, 2, 2
    a.aggr[0], a.aggr[1] = _lib.AGG_CODES["mean"], _lib.AGG_CODES["max"]
    a.scaler[0], a.scaler[1] = 0, 1
    for f in ("x", "adj", "avg_log", "avg_lin", "w_mix", "b_mix", "out"):
        setattr(a, f, 4096)
    for f in ("w_pre", "b_pre", "w_post", "b_post"):
        for t in range(2):
            getattr(a, f)[t] = 4096
    aggr, scaler = kw.pop("aggr", None), kw.pop("scaler", None)
    for k, v in kw.items():
        setattr(a, k, v)
    for k, v in enumerate(aggr or ()):
        a.aggr[k] = v
    for k, v in enumerate(scaler or ()):
        a.scaler[k] = v
    return a


@pytest.mark.parametrize("kw", [
    {"N": 0}, {"N": 129}, {"n_tower": 0}, {"n_tower": 9}, {"Fi": 0}, {"Fi": 33, "in_dim": 66}, {"Fo": 0}, {"Fo": 33}, {"B": 0}, {"B": 2 ** 28},
    {"n_aggr": 0}, {"n_aggr": 5}, {"aggr": (0, 0)}, {"aggr": (0, 1)}, {"aggr": (5, 0)}, {"n_scaler": 0}, {"n_scaler": 4}, {"scaler": (1, 1)},
    {"scaler": (0, 5)}, {"in_dim": 4}, {"x": None}, {"adj": None}, {"avg_log": None}, {"w_mix": None}, {"b_mix": None}, {"out": None},
    {"N": 128, "n_tower": 8, "Fi": 8, "Fo": 8, "in_dim": 64}], ids=str)
def test_every_refusal_outside_the_scope_is_invalid(cuda_device, kw):
    L = _lib.lib()
    assert L.pna_dense_layer_fwd_f32(ctypes.byref(_scope_args(**kw)), None) == -1, L.pna_last_error()
    inside = _scope_args()
    inside.out = None
    inside.grad_out = 4096
    assert L.pna_dense_layer_bwd_f32(ctypes.byref(inside), None) == -1 and b"workspace" in L.pna_last_error()
