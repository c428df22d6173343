"""The one-call route of layers.Set2Set behind PNA_AMD_S2S_ROWS on the GPU: Set2Set and S2SReadout in train mode against float64, the
routing (calls outside the scope run the loop over nn.LSTM, bit for bit), and pytorch.gnn_framework.GNN entirely on the GPU with the three
one-call knobs on -- the reference's forward golden, the first loss of its training trace, and hipGraph capture of an eval forward.  A spy
on autograd.set2set counts the calls: without the route these tests fail.  (No multi-step Adam trace here: tests/test_gpu_train_trace.py
documents why that one is unstable.)"""
import types

import pytest
import torch
import torch.nn.functional as F

import set2set_cases as C
from conftest import golden_names, load_golden
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd import layers
from pna_amd.pytorch.gnn_framework import GNN
from pna_amd.pytorch.pna.layer import PNALayer

pytestmark = pytest.mark.gpu


@pytest.fixture
def spy(monkeypatch):
    """Knob on; -> the list of (B, N, steps) of every call that went through autograd.set2set."""
    calls = []
    real = AG.set2set

    def set2set(x, lstm, steps):
        calls.append((x.shape[0], x.shape[1], steps))
        return real(x, lstm, steps)
    monkeypatch.setattr(AG, "set2set", set2set)
    monkeypatch.setattr(PF, "S2S_ROWS", 1 << 20)
    return calls


def _module(c, dev, dtype=torch.float32, **kw):
    m = layers.Set2Set(c["D"], steps=c["steps"], **kw)
    if not kw:
        m.lstm.load_state_dict(C.lstm_state_dict(c), strict=True)
    return m.to(dtype).to(dev)


@pytest.mark.parametrize("name", ["n15", "n97", "steps3", "slab"])
def test_set2set_module_in_train_mode_against_float64(cuda_device, spy, name):
    c = C.s2s_case(name)
    ref64, _, bars = C.references(name)
    m = _module(c, cuda_device).train()
    x = c["x"].to(cuda_device).requires_grad_(True)
    out = m(x)
    out.backward(c["go"].to(cuda_device))
    assert spy == [(c["B"], c["N"], c["steps"])]
    got = {"out": out.detach(), "x": x.grad, "w_ih": m.lstm.weight_ih_l0.grad, "w_hh": m.lstm.weight_hh_l0.grad,
           "b_ih": m.lstm.bias_ih_l0.grad, "b_hh": m.lstm.bias_hh_l0.grad}
    ratios = {k: C.worst_ratio(got[k], ref64[k], bars[k]) for k in C.TENSORS}
    print("S2S_LAYER", name, "worst err / bar", {k: round(v, 3) for k, v in ratios.items()})
    for k in C.TENSORS:
        assert ((got[k].double().cpu() - ref64[k]).abs() <= bars[k]).all(), (name, k, ratios[k])
    with torch.no_grad():                                              # no_grad and eval take the route too, to the same bits
        assert torch.equal(m(x), out) and torch.equal(m.eval()(x), out) and len(spy) == 3


def _readout_run(c, sd, dtype, dev, go):
    """S2SReadout (train mode: batch statistics) on the case's rows: {'out': ..., 'x': grad, <parameter name>: grad}."""
    head = layers.S2SReadout(c["D"], c["D"], 3, fc_layers=3, final_activation="LeakyReLU")
    head.load_state_dict(sd, strict=True)
    head = head.to(dtype).to(dev).train()
    x = c["x"].to(dtype).to(dev).requires_grad_(True)
    out = head(x)
    names = [n for n, _ in head.named_parameters()]
    grads = torch.autograd.grad(out, [x] + list(head.parameters()), go.to(dtype).to(dev))
    res = {"out": out.detach().cpu(), "x": grads[0].cpu()}
    res.update({n: g.cpu() for n, g in zip(names, grads[1:])})
    return res


def test_s2s_readout_in_train_mode_against_float64(cuda_device, spy):
    """The head of the multitask shape (16 x 15 x 16): the bars are the Set2Set cases' convention on the whole module -- 4 x the fp32 CPU
    run's distance from the float64 CPU run + 2^-20 of the tensor's largest value, and never above 1e-4 of it."""
    c = C.s2s_case("n15")
    gen = torch.Generator().manual_seed(77)
    head = layers.S2SReadout(c["D"], c["D"], 3, fc_layers=3, final_activation="LeakyReLU")
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    sd.update({"set2set.lstm." + k: v for k, v in C.lstm_state_dict(c).items()})
    for k in sd:                                                       # biases and batch-norm off their initial 0 / 1
        if k.endswith("linear.bias") or k.endswith("b_norm.bias"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=gen)
        elif k.endswith("b_norm.weight"):
            sd[k] = 1.0 + 0.2 * torch.randn(sd[k].shape, generator=gen)
        elif k.endswith("linear.weight"):
            sd[k] = torch.randn(sd[k].shape, generator=gen) / sd[k].shape[1] ** 0.5
    go = torch.randn(c["B"], 3, generator=gen)
    r64, r32 = _readout_run(c, sd, torch.float64, "cpu", go), _readout_run(c, sd, torch.float32, "cpu", go)
    assert not spy
    got = _readout_run(c, sd, torch.float32, cuda_device, go)
    assert spy == [(c["B"], c["N"], c["N"])]
    worst = (0.0, "")
    for k in r64:
        top = float(r64[k].abs().max())
        bar = 4.0 * float((r32[k].double() - r64[k]).abs().max()) + C.FLOOR * top
        assert bar <= C.CAP * top, (k, bar, top)
        worst = max(worst, (C.worst_ratio(got[k], r64[k], bar), k))
        assert ((got[k].double() - r64[k]).abs() <= bar).all(), (k, C.worst_ratio(got[k], r64[k], bar))
    print("S2S_READOUT worst err / bar", round(worst[0], 3), worst[1])


def _off(fn, monkeypatch):
    with monkeypatch.context() as m:
        m.setattr(PF, "S2S_ROWS", 0)
        return fn()


def test_calls_outside_the_scope_fall_through_to_the_loop(cuda_device, spy, monkeypatch):
    dev = cuda_device
    gen = torch.Generator().manual_seed(5)
    c = C.s2s_case("steps3")
    with torch.no_grad():
        inside = _module(c, dev)
        x = c["x"].to(dev)
        inside(x)
        assert len(spy) == 1                                           # (inside: the route is taken)
        del spy[:]
        for what, m, xs in (
                ("N = 129", layers.Set2Set(16, steps=3, device=dev), torch.randn(2, 129, 16, generator=gen).to(dev)),
                ("D = 33", layers.Set2Set(33, steps=3, device=dev), torch.randn(2, 15, 33, generator=gen).to(dev)),
                ("steps = 129", layers.Set2Set(16, steps=129, device=dev), torch.randn(2, 15, 16, generator=gen).to(dev)),
                ("float64", _module(c, dev, torch.float64), c["x"].double().to(dev)),
                ("not contiguous", inside, c["x"].transpose(0, 1).contiguous().transpose(0, 1).to(dev)),
                ("num_layers = 2", _module(c, dev, num_layers=2), x)):
            if what == "not contiguous":
                assert not xs.is_contiguous()
            got = m(xs)
            assert not spy and torch.equal(got, _off(lambda: m(xs), monkeypatch)), what
            assert got.shape == (xs.shape[0], 2 * xs.shape[2]), what
    monkeypatch.setattr(PF, "S2S_ROWS", c["B"] * c["N"] - 1)              # more rows than the knob covers
    with torch.no_grad():
        assert torch.equal(inside(x), _off(lambda: inside(x), monkeypatch)) and not spy
    monkeypatch.setattr(PF, "S2S_ROWS", 0)
    with torch.no_grad():
        inside(x)
    assert not spy


# ---- the GNN entirely on the GPU -------------------------------------------------------------------------------------------------------
@pytest.fixture
def all_knobs(spy, monkeypatch):
    monkeypatch.setattr(PF, "DENSE_LAYER_ROWS", 1 << 20)
    monkeypatch.setattr(PF, "GRU_ROWS", 1 << 20)
    return spy


def _gnn(meta, a, dev):
    """The README model: hidden 16, 4 towers, fixed, variable N / 2 layers, shared GRU."""
    avg_d = {k: a["avg_" + k].to(dev) for k in ("log", "lin")}
    conv = dict(aggregators=meta["aggregators"], scalers=meta["scalers"], avg_d=avg_d, towers=meta["towers"], self_loop=False,
                pretrans_layers=1, posttrans_layers=1)
    return GNN(nfeat=2, nhid=meta["hidden"], nodes_out=3, graph_out=3, dropout=meta.get("dropout", 0.0), conv_layers=lambda adj: adj.shape[1] // 2,
               fc_layers=3, first_conv_descr=dict(layer_type=PNALayer, args=dict(conv, divide_input=False)),
               middle_conv_descr=types.SimpleNamespace(layer_type=PNALayer, args=dict(conv, divide_input=True)),
               final_activation="LeakyReLU", gru=True, fixed=True, variable=True, device=dev)


def _route_counts(monkeypatch):
    counts = {"dense": 0, "gru": 0}
    dense, gru = AG.DenseLayerFn.apply, AG.GruCellFn.apply
    monkeypatch.setattr(AG.DenseLayerFn, "apply", staticmethod(lambda *a: (counts.__setitem__("dense", counts["dense"] + 1), dense(*a))[1]))
    monkeypatch.setattr(AG.GruCellFn, "apply", staticmethod(lambda *a: (counts.__setitem__("gru", counts["gru"] + 1), gru(*a))[1]))
    return counts


def test_gnn_forward_golden_with_the_three_knobs_on(cuda_device, all_knobs, monkeypatch):
    meta, a, sd = load_golden("c1_gnn_forward_n15")
    counts = _route_counts(monkeypatch)
    net = _gnn(meta, a, cuda_device)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda_device).eval()
    with torch.no_grad():
        nodes, graph = net(a["x"].to(cuda_device), a["adj"].to(cuda_device))
    assert all_knobs == [(meta["B"], meta["N"], meta["N"])] and counts == {"dense": 7, "gru": 7}
    for got, want, what in ((nodes, a["out"], "out"), (graph, a["graph_out"], "graph_out")):
        err = float((got.cpu() - want).abs().max()) / float(want.abs().max())
        print("S2S_GNN_GOLDEN", what, f"{err:.2e}")
        assert err <= 1e-5, (what, err)


def _total_loss(out, target):               # multitask_benchmark/util/util.py:51-66 with loss = 'mse'
    nodes, graph = F.mse_loss(out[0], target[0]), F.mse_loss(out[1], target[1])
    return (nodes * out[0].shape[-1] + graph * out[1].shape[-1]) / (out[0].shape[-1] + out[1].shape[-1])


@pytest.mark.parametrize("name", golden_names("c1_train_trace"))
def test_first_training_loss_with_the_three_knobs_on(cuda_device, all_knobs, name):
    """Train mode (batch statistics in the head), everything on the GPU: the reference's first loss to 1e-6, and a backward through the
    three one-call routes that leaves a finite gradient on every parameter."""
    meta, a, sd = load_golden(name)
    dev = cuda_device
    net = _gnn(meta, a, dev)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    B = meta["B"]
    adj, x, nl, gl = (a[k][:B].to(dev) for k in ("adj", "x", "node_labels", "graph_labels"))
    loss = _total_loss(net(x, adj), (nl, gl))
    loss.backward()
    want = float(a["out"][0])
    print(f"S2S_TRACE loss rel err {abs(loss.item() - want) / abs(want):.3e}")
    assert all_knobs == [(B, meta["N"], meta["N"])]
    assert abs(loss.item() - want) <= 1e-6 * abs(want)
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n


def test_graphed_eval_forward_replays_to_the_eager_bits(cuda_device, all_knobs):
    from pna_amd.capture import GraphedForward
    meta, a, sd = load_golden("c1_gnn_forward_n15")
    net = _gnn(meta, a, cuda_device)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda_device).eval()
    x, adj = a["x"].to(cuda_device), a["adj"].to(cuda_device)
    with torch.no_grad():
        nodes, graph = (t.clone() for t in net(x, adj))
        gf = GraphedForward(net, x, adj)
        n = len(all_knobs)
        assert n >= 2
        got = gf(x, adj)
        assert torch.equal(got[0], nodes) and torch.equal(got[1], graph) and len(all_knobs) == n        # the replay makes no call
        x2 = (x * 0.5 + 0.25).contiguous()
        want = [t.clone() for t in net(x2, adj)]
        got = gf(x2, adj)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
