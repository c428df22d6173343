"""The one-call route of pna_amd.pytorch.pna.layer.PNALayer behind PNA_AMD_DENSE_LAYER_ROWS on the GPU: the reference's goldens of the
multitask layer and of every PNALayer call of its GNN, the first training step of the multitask benchmark, the routing (knob off, calls
outside the scope) and hipGraph capture.  A spy on autograd.DenseLayerFn.apply counts the calls: without the route these tests fail."""
import pytest
import torch

import dense_layer_cases as C
from conftest import golden_names, load_golden
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd.pytorch.pna.layer import PNALayer, PNATower

pytestmark = pytest.mark.gpu

C1_DENSE = [n for n in golden_names("dense") if n.startswith("c1_dense_")]


@pytest.fixture
def spy(monkeypatch):
    """Knob on; -> the list of (B, N) of every call that went through DenseLayerFn.apply."""
    calls = []
    real = AG.DenseLayerFn.apply

    def apply(x, adj, *rest):
        calls.append(tuple(adj.shape[:2]))
        return real(x, adj, *rest)
    monkeypatch.setattr(AG.DenseLayerFn, "apply", staticmethod(apply))
    monkeypatch.setattr(PF, "DENSE_LAYER_ROWS", 1 << 20)
    return calls


def _ref64(meta, a, sd, x, divide):
    from oracle import torch_oracle as TO
    avg = {"log": a["avg_log"].double(), "lin": a["avg_lin"].double()}
    return TO.dense_layer_forward({k: v.double() for k, v in sd.items()}, x.double(), a["adj"].double(), meta["aggregators"], meta["scalers"], avg,
                                  meta["towers"], divide, meta.get("self_loop", False))


def _assert_golden(out, golden, ref64, what):
    """The plain 1e-5 |ref| + 1e-5 bar plus 4 x the golden's own distance from the float64 oracle, per element."""
    tol = 1e-5 * golden.double().abs() + 1e-5 + 4.0 * (golden.double() - ref64).abs()
    err = (out.double() - golden.double()).abs()
    print(f"DENSE_GOLDEN {what} worst err / tol {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), (what, float((err / tol).max()))


def test_the_goldens_cover_the_three_sizes():
    assert {load_golden(n)[0]["N"] for n in C1_DENSE} == {15, 47, 97} and len(C1_DENSE) == 12


@pytest.mark.parametrize("name", C1_DENSE)
def test_multitask_layer_goldens_on_the_one_call_route(cuda_device, spy, name):
    meta, a, sd = load_golden(name)
    avg_d = {"log": a["avg_log"].to(cuda_device), "lin": a["avg_lin"].to(cuda_device)}
    layer = PNALayer(meta["in_features"], meta["out_features"], meta["aggregators"], meta["scalers"], avg_d, towers=meta["towers"],
                     self_loop=meta["self_loop"], divide_input=meta["divide_input"], device=cuda_device)
    layer.load_state_dict(sd)
    layer = layer.to(cuda_device).eval()
    with torch.no_grad():
        out = layer(a["x"].to(cuda_device), a["adj"].to(cuda_device)).cpu()
    assert spy == [(meta["B"], meta["N"])]
    _assert_golden(out, a["out"], _ref64(meta, a, sd, a["x"], meta["divide_input"]), name)


@pytest.mark.parametrize("name", golden_names("c1_gnn"))
def test_every_conv_call_of_the_multitask_gnn_on_the_one_call_route(cuda_device, spy, name):
    meta, a, sd = load_golden(name)
    avg_d = {"log": a["avg_log"].to(cuda_device), "lin": a["avg_lin"].to(cuda_device)}
    layers, lsds = [], []
    for li, divide in ((0, False), (1, True)):
        lay = PNALayer(2 if li == 0 else meta["hidden"], meta["hidden"], meta["aggregators"], meta["scalers"], avg_d, towers=meta["towers"],
                       divide_input=divide, device=cuda_device)
        lsds.append({k[len(f"conv_layers.{li}."):]: v for k, v in sd.items() if k.startswith(f"conv_layers.{li}.")})
        lay.load_state_dict(lsds[-1], strict=True)
        layers.append(lay.to(cuda_device).eval())
    adj = a["adj"].to(cuda_device)
    with torch.no_grad():
        for k in range(meta["n_calls"]):
            li = int(a["call_layer"][k])
            out = layers[li](a[f"call_in/{k}"].to(cuda_device), adj).cpu()
            _assert_golden(out, a[f"call_out/{k}"], _ref64(meta, a, lsds[li], a[f"call_in/{k}"], li == 1), f"{name} call {k}")
    assert len(spy) == meta["n_calls"] == 7


@pytest.mark.parametrize("name", golden_names("c1_train_trace"))
def test_first_training_step_of_the_multitask_benchmark(cuda_device, spy, name):
    """Step-1 loss to 1e-6 of the reference's and the PNA-layer gradients to 5e-4 of the parameter's largest gradient against fp32 CPU
    autograd through the oracle layer: test_gpu_train_trace.py's network (restated from public pieces there) and its bars (1) and (2).
    The eight-step Adam trace stays with that test."""
    from test_gpu_train_trace import _GNN, _oracle_layer_type, _total_loss
    meta, a, sd = load_golden(name)
    dev = cuda_device
    avg_d = {k: a["avg_" + k].to(dev) for k in ("lin", "log", "exp")}
    torch.manual_seed(0)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                      # (the reference run's CPU summation order)
    try:
        net = _GNN(PNALayer, meta, avg_d, dev)
        net.load_state_dict(sd, strict=True)
        net.conv_layers.to(dev)
        B = meta["B"]
        adj, x, nl, gl = (a[k].split(B) for k in ("adj", "x", "node_labels", "graph_labels"))
        avg32 = {k: a["avg_" + k] for k in ("lin", "log", "exp")}
        ref = _GNN(_oracle_layer_type(meta, avg32), meta, avg32, "cpu")
        ref.load_state_dict(sd, strict=True)
        ref.train()
        _total_loss(ref(x[0], adj[0]), (nl[0], gl[0])).backward()
        net.train()
        loss0 = _total_loss(net(x[0], adj[0]), (nl[0], gl[0]))
        loss0.backward()
    finally:
        torch.set_num_threads(threads)
    assert len(spy) == meta["N"] // 2 and set(spy) == {(B, meta["N"])}
    want = float(a["out"][0])
    print(f"DENSE_TRACE loss rel err {abs(loss0.item() - want) / abs(want):.3e}")
    assert abs(loss0.item() - want) <= 1e-6 * abs(want)
    worst = (0.0, "")
    for (n, p), (_, q) in zip(net.conv_layers.named_parameters(), ref.conv_layers.named_parameters()):
        scale = q.grad.abs().max().item()
        if scale > 0:
            worst = max(worst, ((p.grad.cpu() - q.grad).abs().max().item() / scale, n))
    print("DENSE_TRACE worst gradient", worst)
    assert worst[0] <= 5e-4, worst


def _case_layer(name, dev, **kw):
    c = C.dense_case(name)
    return c, C.make_layer(c, dev), c["x"].to(dev), c["adj"].to(dev)


def test_the_knob_at_its_default_never_calls_the_route(cuda_device, monkeypatch):
    calls = []
    monkeypatch.setattr(AG.DenseLayerFn, "apply", staticmethod(lambda *a: calls.append(1)))
    assert PF.DENSE_LAYER_ROWS == 0
    c, layer, x, adj = _case_layer("n15", cuda_device)
    out = layer(x, adj)
    assert not calls and out.shape == (c["B"], c["N"], c["out_features"])


def _off(layer_fn, monkeypatch):
    with monkeypatch.context() as m:
        m.setattr(PF, "DENSE_LAYER_ROWS", 0)
        return layer_fn()


def test_calls_outside_the_scope_fall_through_to_the_existing_route(cuda_device, spy, monkeypatch):
    dev = cuda_device
    gen = torch.Generator().manual_seed(3)
    c, layer, x, adj = _case_layer("n15", dev)
    with torch.no_grad():
        assert torch.equal(layer(x, adj), AG.dense_layer(layer, x, adj)) and len(spy) == 2          # (inside: the route is taken)
        del spy[:]
        # a two-layer pretrans, an aggregator outside the four, more nodes than the kernel holds
        for kw, n in (({"pretrans_layers": 2}, 15), ({"aggregators": ["mean", "sum"]}, 15), ({}, 129)):
            aggs = kw.pop("aggregators", ["mean", "max", "min", "std"])
            lay = PNALayer(16, 16, aggs, ["identity", "amplification"], C.AVG_D, towers=4, **kw).to(dev)
            xs = torch.randn(2, n, 16, generator=gen).to(dev)
            a = (torch.rand(2, n, n, generator=gen) < 0.3).float()
            a[:, torch.arange(n), (torch.arange(n) + 1) % n] = 1.0
            a = a.to(dev)
            got = lay(xs, a)
            assert not spy and torch.equal(got, _off(lambda: lay(xs, a), monkeypatch)), (kw, n)
        # a non-contiguous input
        xt = x.transpose(0, 1).contiguous().transpose(0, 1)
        assert not xt.is_contiguous()
        got = layer(xt, adj)
        assert not spy and torch.equal(got, _off(lambda: layer(xt, adj), monkeypatch))
        # a bare tower
        tower = layer.towers[0]
        xt0 = x[:, :, :c["Fi"]].contiguous()
        got = tower(xt0, adj)
        assert not spy and isinstance(tower, PNATower) and torch.equal(got, _off(lambda: tower(xt0, adj), monkeypatch))
    # an adjacency that wants a gradient
    ag = adj.clone().requires_grad_(True)
    got = layer(x, ag)
    assert not spy and torch.equal(got, _off(lambda: layer(x, ag), monkeypatch))


def test_graphed_forward_replays_to_the_eager_bits(cuda_device, spy):
    from pna_amd.capture import GraphedForward
    c = C.dense_case("n15")
    avg_d = {k: torch.tensor(v, device=cuda_device) for k, v in C.AVG_D.items()}          # 0-dim device scalars: passed by pointer
    layer = C.make_layer(c, cuda_device, avg_d=avg_d).eval()
    x, adj = c["x"].to(cuda_device), c["adj"].to(cuda_device)
    with torch.no_grad():
        eager = layer(x, adj).clone()
        gf = GraphedForward(layer, x, adj)
        n = len(spy)
        assert n >= 2
        assert torch.equal(gf(x, adj), eager) and len(spy) == n                              # the replay makes no call
        x2 = (x * 0.5 + 0.25).contiguous()
        assert torch.equal(gf(x2, adj), layer(x2, adj))
    # Python floats in avg_d become a device scalar per call: the same bits, and nothing cached on the layer
    floats = C.make_layer(c, cuda_device).eval()
    with torch.no_grad():
        assert torch.equal(floats(x, adj), eager)
        assert not [k for k in floats.__dict__ if str(k).startswith("_pna_amd_dense")]
        gf2 = GraphedForward(floats, x, adj)                                                 # ... and captures as well
        assert torch.equal(gf2(x, adj), eager)
