"""The one-call MLP head route behind PNA_AMD_MLP_HEAD_ROWS on the GPU: nets.MLPReadout and layers.MLP in train mode against float64 within
the bars of tests/mlp_head_cases.py; eval and no_grad to the same bits; the calls outside the scope run the old lines bit for bit; one
training step of PNANetHIV, PNANet and PNANetSuperpixels with the knob on against the knob off; pytorch.gnn_framework.GNN with all four
one-call knobs on against the reference's forward golden; and hipGraph capture of an eval forward.  A spy on autograd.mlp_head counts the
calls: without the route these tests fail."""
import types

import pytest
import torch

import mlp_head_cases as C
from conftest import load_golden
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd import layers, nets
from pna_amd.graph import Graph
from pna_amd.pytorch.gnn_framework import GNN
from pna_amd.pytorch.pna.layer import PNALayer

pytestmark = pytest.mark.gpu


@pytest.fixture
def spy(monkeypatch):
    """Knob on; -> the list of (rows, widths) of every call that went through autograd.mlp_head."""
    calls = []
    real = AG.mlp_head

    def mlp_head(x, linears, acts):
        calls.append((x.shape[0], (x.shape[1],) + tuple(lin.out_features for lin in linears)))
        return real(x, linears, acts)
    monkeypatch.setattr(AG, "mlp_head", mlp_head)
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 1 << 20)
    return calls


def _off(fn, monkeypatch):
    with monkeypatch.context() as m:
        m.setattr(PF, "MLP_HEAD_ROWS", 0)
        return fn()


def _load(linears, c, dev):
    with torch.no_grad():
        for lin, w, b in zip(linears, c["ws"], c["bs"]):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
    return [p for lin in linears for p in (lin.weight, lin.bias)]


def _check(c, tag, y, x, params):
    got = {"y": y.detach().reshape(c["ref"]["y"].shape), "x": x.grad.reshape(c["x"].shape)}
    for l in range(len(c["ws"])):
        got[f"w{l}"], got[f"b{l}"] = params[2 * l].grad, params[2 * l + 1].grad
    worst = {k: C.worst_ratio(got[k].cpu(), c["ref"][k], c["bars"][k]) for k in C.tensors_of(c)}
    print("MLP_LAYER", tag, "worst err / bar", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("name", ["zinc", "cls10"])
def test_mlp_readout_in_train_mode_against_float64(cuda_device, spy, name):
    c = C.mlp_case(name)
    widths = C.CASES[name][1]
    m = nets.MLPReadout(widths[0], widths[-1]).to(cuda_device).train()
    params = _load(list(m.FC_layers), c, cuda_device)
    x = c["x"].to(cuda_device).requires_grad_(True)
    y = m(x)
    y.backward(c["go"].to(cuda_device))
    assert spy == [(c["x"].shape[0], widths)]
    _check(c, name, y, x, params)
    with torch.no_grad():                                              # no_grad and eval take the route too, to the same bits
        assert torch.equal(m(x), y) and torch.equal(m.eval()(x), y) and len(spy) == 3


def test_layers_mlp_in_train_mode_against_float64(cuda_device, spy):
    """The multitask node head: three FCLayers with LeakyReLU(0.01) after each on (16, 15, 16) rows."""
    c = C.mlp_case("mt")
    m = layers.MLP(16, 16, 3, 3, mid_activation="LeakyReLU", last_activation="LeakyReLU", device=cuda_device).train()
    params = _load([fc.linear for fc in m.fully_connected], c, cuda_device)
    x = c["x"].reshape(16, 15, 16).to(cuda_device).requires_grad_(True)
    y = m(x)
    assert y.shape == (16, 15, 3)
    y.backward(c["go"].reshape(16, 15, 3).to(cuda_device))
    assert spy == [(240, (16, 16, 16, 3))]
    _check(c, "mt", y, x, params)
    with torch.no_grad():
        assert torch.equal(m(x), y) and torch.equal(m.eval()(x), y) and len(spy) == 3
        assert torch.equal(m(x.reshape(240, 16)), y.reshape(240, 3)) and len(spy) == 4                  # 2-D rows take it too


def test_calls_outside_the_scope_run_the_old_lines(cuda_device, spy, monkeypatch):
    dev = cuda_device
    gen = torch.Generator().manual_seed(5)
    rows = lambda *s: torch.randn(*s, generator=gen).to(dev)                       # noqa: E731
    mk = lambda **kw: layers.MLP(16, 16, 3, 3, mid_activation="LeakyReLU", last_activation="LeakyReLU", device=dev, **kw)     # noqa: E731
    inside = mk()
    with torch.no_grad():
        inside(rows(4, 15, 16))
        assert len(spy) == 1                                                     # (inside: the route is taken)
        del spy[:]
        for what, m, xs in (
                ("batch-norm (S2SReadout's MLP)", layers.S2SReadout(16, 16, 3, device=dev).train().mlp, rows(8, 32)),
                ("float64", mk().double(), rows(4, 15, 16).double()),
                ("width 129", layers.MLP(129, 16, 3, 3, device=dev), rows(4, 15, 129)),
                ("five layers", layers.MLP(16, 16, 3, 5, device=dev), rows(4, 15, 16)),
                ("five layers (MLPReadout)", nets.MLPReadout(128, 1, L=4).to(dev), rows(9, 128)),
                ("not contiguous", inside, rows(15, 4, 16).transpose(0, 1))):
            keep = {k: v.clone() for k, v in m.state_dict().items()}
            got = m(xs)
            m.load_state_dict(keep)                                              # (batch-norm moved its running statistics)
            assert not spy and torch.equal(got, _off(lambda: m(xs), monkeypatch)), what
    drop = mk(dropout=0.3).train()                                               # an active dropout: torch's ops and torch's mask
    xs = rows(4, 15, 16)
    torch.manual_seed(7)
    got = drop(xs)
    torch.manual_seed(7)
    assert not spy and torch.equal(got, _off(lambda: drop(xs), monkeypatch))
    with torch.no_grad():
        drop.eval()(xs)
    assert len(spy) == 1                                                         # in eval mode the dropout is inactive: routed
    del spy[:]
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 59)                                  # more rows than the knob covers
    with torch.no_grad():
        xs = rows(4, 15, 16)
        assert torch.equal(inside(xs), _off(lambda: inside(xs), monkeypatch)) and not spy
    monkeypatch.setattr(PF, "MLP_HEAD_ROWS", 0)
    with torch.no_grad():
        inside(xs)
    assert not spy


# ---- the nets: one training step with the knob on against the knob off ----------------------------------------------------------------
def _molecules(dev):
    from pna_amd.synth import molecule_batch
    src, dst, sizes = molecule_batch(6, mean_nodes=23, sd_nodes=5, lo=8, hi=40, seed=4)
    V = sum(sizes)
    g = Graph(src, dst, V, sizes).to(dev)
    avg = {"log": torch.log(g.in_degrees().double() + 1).mean().float().cpu()}
    return g, sizes, V, avg


def _zinc(dev):
    g, sizes, V, avg = _molecules(dev)
    torch.manual_seed(0)
    net = nets.PNANet(dict(num_atom_type=28, num_bond_type=4, hidden_dim=32, out_dim=32, in_feat_dropout=0.0, dropout=0.0, L=2, readout="sum",
                           graph_norm=True, batch_norm=True, residual=True, aggregators="mean max min std",
                           scalers="identity amplification attenuation", avg_d=avg, towers=4, divide_input_first=True, divide_input_last=True,
                           edge_feat=False, edge_dim=0, pretrans_layers=1, posttrans_layers=1, gru=True, device=dev)).to(dev)
    gen = torch.Generator().manual_seed(1)
    atoms = torch.randint(0, 28, (V,), generator=gen).to(dev)
    snorm = torch.cat([torch.full((n, 1), n ** -0.5) for n in sizes]).to(dev)
    y = torch.randn(len(sizes), 1, generator=gen).to(dev)
    return net, lambda: net.loss(net(g, atoms, None, snorm), y), [(len(sizes), (32, 16, 8, 1))]


def _hiv(dev):
    g, sizes, V, avg = _molecules(dev)
    torch.manual_seed(0)
    net = nets.PNANetHIV(dict(hidden_dim=32, out_dim=32, in_feat_dropout=0.0, dropout=0.0, L=2, readout="mean", batch_norm=True, residual=True,
                              aggregators="mean max min std", scalers="identity amplification attenuation", avg_d=avg, posttrans_layers=1,
                              device=dev)).to(dev)
    gen = torch.Generator().manual_seed(0)
    x = torch.stack([torch.randint(0, d, (V,), generator=gen) for d in (119, 4, 12, 12, 10, 6, 6, 2, 2)], dim=1).to(dev)
    y = torch.randint(0, 2, (len(sizes),), generator=gen)
    return net, lambda: net.loss(net(g, x), y), [(len(sizes), (32, 16, 8, 1))]


def _superpixels(dev):
    import tower_drop_train_cases as T
    b = T.net_batch()
    torch.manual_seed(T.NET_SEED)
    net = nets.PNANetSuperpixels(T.net_params(0.0, True, b["avg_log"])).to(dev)
    g = Graph(b["src"], b["dst"], b["N"], b["sizes"]).to(dev)
    x, e, snorm, labels = (b[k].to(dev) for k in ("x", "e", "snorm_n", "labels"))
    E = b["src"].numel()
    return net, lambda: net.loss(net(g, x, e, snorm), labels), [(b["N"], (5, 60)), (E, (1, 50)), (4, (60, 30, 15, 10))]


@pytest.mark.parametrize("build", [_hiv, _zinc, _superpixels], ids=["PNANetHIV", "PNANet", "PNANetSuperpixels"])
def test_one_training_step_of_a_net_with_the_knob_on_against_knob_off(cuda_device, spy, monkeypatch, build):
    """Both routes evaluate the same function in fp32, in another summation order.  Under the convention of tests/mlp_head_cases.py the
    bar of one fp32 evaluation never exceeds 1e-4 of a tensor's largest value (the cap the host tests hold every case to), so two of
    them differ by at most twice that: the loss within 2e-4 relative, every gradient tensor within 2e-4 of its largest entry.  One kind
    of tensor has no scale of its own: a Linear bias ahead of a train-mode BatchNorm has a true gradient of exactly 0 (the batch mean
    removes it), and what either route computes is the rounding noise of a sum whose terms are those of the sibling weight's gradient;
    outside the heads a bias is therefore held to 2e-4 of the larger of its own and its sibling weight's largest entry."""
    net, step, want_calls = build(cuda_device)
    net.train()

    def run():
        net.zero_grad(set_to_none=True)
        loss = step()
        loss.backward()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters()}
    loss_off, g_off = _off(run, monkeypatch)
    assert not spy
    loss_on, g_on = run()
    assert all(c in spy for c in want_calls), (spy, want_calls)                  # (the towers' one-layer pretrans / posttrans MLPs may add calls)
    rel = abs(float(loss_on) - float(loss_off)) / abs(float(loss_off))
    head = lambda n: n.startswith("MLP_layer.") or (build is _superpixels and n.startswith("embedding_"))      # noqa: E731

    def scale(n):
        own = float(g_off[n].abs().max())
        sibling = n[:-len("bias")] + "weight"
        return max(own, float(g_off[sibling].abs().max())) if n.endswith(".bias") and not head(n) and sibling in g_off else own
    worst = max((float((g_on[n] - g_off[n]).abs().max()) / scale(n), n) for n in g_off)
    print("MLP_NET", build.__name__, f"loss rel {rel:.2e} worst gradient {worst[0]:.2e} {worst[1]}")
    assert rel <= 2 * C.CAP and worst[0] <= 2 * C.CAP, (rel, worst)
    heads = [n for n in g_on if head(n)]
    assert len(heads) == 6 + (4 if build is _superpixels else 0)
    for n in heads:
        assert bool(torch.isfinite(g_on[n]).all()) and float(g_on[n].abs().max()) > 0, n


# ---- the GNN entirely on the GPU -------------------------------------------------------------------------------------------------------
@pytest.fixture
def all_knobs(spy, monkeypatch):
    monkeypatch.setattr(PF, "DENSE_LAYER_ROWS", 1 << 20)
    monkeypatch.setattr(PF, "GRU_ROWS", 1 << 20)
    monkeypatch.setattr(PF, "S2S_ROWS", 1 << 20)
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


def test_gnn_forward_golden_with_the_four_knobs_on(cuda_device, all_knobs):
    meta, a, sd = load_golden("c1_gnn_forward_n15")
    net = _gnn(meta, a, cuda_device)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda_device).eval()
    with torch.no_grad():
        nodes, graph = net(a["x"].to(cuda_device), a["adj"].to(cuda_device))
    assert (meta["B"] * meta["N"], (16, 16, 16, 3)) in all_knobs                   # the node head
    assert not any(w[0] == 32 for _, w in all_knobs)                               # the graph head (batch-norm) keeps torch's ops
    for got, want, what in ((nodes, a["out"], "out"), (graph, a["graph_out"], "graph_out")):
        err = float((got.cpu() - want).abs().max()) / float(want.abs().max())
        print("MLP_GNN_GOLDEN", what, f"{err:.2e}")
        assert err <= 1e-5, (what, err)


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
