"""PNALayer with another list of aggregators than mean max min std in training through the one-call route
(autograd.TowerLayerAggrSmallTrainFn: pna_tower_aggr_train_fwd_f32 / _bwd_f32) behind the knob functional.SMALL_TOWER_TRAIN_AGGR_ROWS: the
entry pair actually called with the knob on, the step against the float64 oracle and against the knob-off run, the routes a layer takes
when only the other knobs (or only this one, on a standard layer) are on, a two-layer PNANet with `sum` against its knob-off step, and a
planned batch against an unplanned one."""
import copy

import pytest
import torch

import batch_plan_cases as BP
import tower_aggr_train_cases as C
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd import graph as G
from pna_amd.dgl.pna_layer import PNALayer
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu

KNOBS = ("SMALL_TOWER_TRAIN_ROWS", "SMALL_TOWER_TRAIN_EDGE_ROWS", "SMALL_TOWER_TRAIN_DROPOUT_ROWS", "SMALL_TOWER_TRAIN_AGGR_ROWS")


def _calls(monkeypatch):
    """Records the C entry points autograd._tower_train_call runs, by re-deriving the name it forms from its arguments."""
    seen = []
    real = AG._tower_train_call

    def wrapped(which, base, edge, key, dev, aggr=None):
        kind = "aggr" if aggr is not None else "drop" if key is not None else "edge" if edge is not None else "plain"
        seen.append(f"{kind}_{which}")
        return real(which, base, edge, key, dev, aggr)
    monkeypatch.setattr(AG, "_tower_train_call", wrapped)
    return seen


def _setup(name, dev):
    meta, a, sd, ref, key = C.case(name)
    edge = meta["edge_dim"] > 0
    layer = PNALayer(meta["in_dim"], meta["out_dim"], meta["aggregators"], meta["scalers"], {"log": a["avg_log"]}, key[0] if key else 0.0, True, True,
                     towers=meta["towers"], pretrans_layers=1, posttrans_layers=1, divide_input=meta["divide_input"], residual=meta["residual"],
                     edge_features=edge, edge_dim=meta["edge_dim"])
    layer.load_state_dict(sd)
    layer = layer.to(dev).train()
    g = Graph(a["src"], a["dst"], meta["N"]).to(dev)
    return meta, a, ref, key, layer, g


def _step(layer, g, a, meta, dev):
    h = a["h"].to(dev).requires_grad_(True)
    e = a["e"].to(dev).requires_grad_(True) if meta["edge_dim"] else None
    out = layer(g, h, e, a["snorm_n"].to(dev))
    (out * a["R"].to(dev)).sum().backward()
    return (out.detach(), h.grad, None if e is None else e.grad, {k: q.grad for k, q in layer.named_parameters()},
            {k: b.clone() for k, b in layer.named_buffers() if "running" in k})


@pytest.mark.parametrize("name", ["mpnn_sum", "mpnn_max", "sum_var_min", "std_only", "reordered", "edge50_max_var", "drop_mpnn_max", "drop_edge3_sum"])
def test_training_step_takes_the_new_route_and_matches_float64_and_the_generic_route(cuda_device, monkeypatch, name):
    """Output, every gradient and the running statistics against the float64 oracle (under the mask of the key the layer draws, for a
    dropout case) at the bars of tower_train_cases.check_step; without dropout also against the knob-off run of the same layer, whose
    own step passes the same bars (with dropout the generic route draws another mask)."""
    dev = cuda_device
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_AGGR_ROWS", 4096)
    seen = _calls(monkeypatch)
    meta, a, ref, key, layer, g = _setup(name, dev)
    generic = copy.deepcopy(layer)
    if key is not None:
        gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
        gen.manual_seed(key[1])
        gen.set_offset(key[2])
    out, gh, ge, grads, running = _step(layer, g, a, meta, dev)
    assert seen == ["aggr_fwd", "aggr_bwd"]
    C.check_step(meta, ref, out, gh, grads, running)
    if ge is not None:
        C.check_grad_e(ref, ge)
    for t, tower in enumerate(layer.towers):
        assert int(tower.batchnorm_h.num_batches_tracked) == 4
    if key is not None:
        n = meta["N"] * meta["out_dim"]
        assert gen.get_offset() == key[2] + 4 * ((n + 3) // 4)
        return
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_AGGR_ROWS", 0)
    out0, gh0, ge0, grads0, running0 = _step(generic, g, a, meta, dev)
    assert seen == ["aggr_fwd", "aggr_bwd"]                                        # (the knob-off run called none of the four)
    C.check_step(meta, ref, out0, gh0, grads0, running0)
    n_ill = int(ref.ill.sum())
    C.close(out, out0.double().cpu(), "out vs generic", 1e-5, n_ill, ref.ill)
    C.close(gh, gh0.double().cpu(), "grad_h vs generic", 1e-4, n_ill, ref.touched)
    wscale = max(v.abs().max().item() for v in ref.ref32["grads"].values())
    for k in grads:
        pre = "pretrans" in k and k.endswith("weight")
        exact = grads0[k].double().cpu()
        own = exact + (ref.ref32["grads"][k].double() - ref.grads[k])              # (close() adds 4 x max |ref - exact|: the fp32 oracle's own error)
        C.close(grads[k], exact, k + " vs generic", 3e-4 if pre else 1e-5, n_ill, scale=wscale, ref=own)
    for k in running:
        torch.testing.assert_close(running[k], running0[k], rtol=1e-5, atol=1e-6)


def test_a_sum_layer_under_the_other_three_knobs_takes_the_generic_route(cuda_device, monkeypatch):
    for knob in KNOBS[:3]:
        monkeypatch.setattr(PF, knob, 4096)
    assert PF.SMALL_TOWER_TRAIN_AGGR_ROWS == 0
    seen = _calls(monkeypatch)
    for name in ("mpnn_sum", "edge3_sum", "drop_mpnn_max"):
        meta, a, ref, key, layer, g = _setup(name, cuda_device)
        out, gh, *_ = _step(layer, g, a, meta, cuda_device)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gh).all())
    assert seen == []


def test_a_standard_layer_under_this_knob_alone_takes_the_generic_route(cuda_device, monkeypatch):
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_AGGR_ROWS", 4096)
    seen = _calls(monkeypatch)
    for name in ("std_plain", "std_edge", "drop_std_plain"):
        meta, a, ref, key, layer, g = _setup(name, cuda_device)
        out, gh, *_ = _step(layer, g, a, meta, cuda_device)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gh).all())
    assert seen == []
    for knob in KNOBS[:3]:                                                          # ... and with all four on, its own routes
        monkeypatch.setattr(PF, knob, 4096)
    for name, want in (("std_plain", "plain"), ("std_edge", "edge"), ("drop_std_plain", "drop")):
        meta, a, ref, key, layer, g = _setup(name, cuda_device)
        del seen[:]
        _step(layer, g, a, meta, cuda_device)
        assert seen == [want + "_fwd", want + "_bwd"]


def _net(dev, avg):
    from pna_amd.nets import PNANet
    torch.manual_seed(3)
    return PNANet(dict(hidden_dim=40, out_dim=30, L=2, readout="sum", edge_feat=True, gru=False, in_feat_dropout=0.0, dropout=0.0, graph_norm=True,
                       batch_norm=True, residual=True, aggregators="sum", scalers="identity", avg_d=avg, towers=5, edge_dim=6, pretrans_layers=1,
                       posttrans_layers=1, divide_input_first=True, divide_input_last=True, num_atom_type=28, num_bond_type=4, device=dev)).to(dev).train()


def test_two_layer_sum_net_matches_its_knob_off_step(cuda_device, monkeypatch):
    """PNANet(aggregators="sum", scalers="identity", edge_feat=True), two layers (40 -> 40 -> 30, 5 towers, edge_dim 6) on 32 molecules:
    one training step with the knob on (both layers through the new entry pair) against the same step with it off -- the loss at rtol /
    atol 1e-5; parameter gradients at 3e-4 of the largest parameter-gradient entry for pretrans weights, 1e-4 for the bond embedding (a
    sum over all edges of both layers, held like the edge gradients), 1e-5 for the others.  `sum` has no ill-conditioned destinations
    (no std, no extremum), so the bars carry no own-error term."""
    dev = cuda_device
    c = BP.molecules(32, seed=11)
    g = BP.unplanned(c, dev)
    V, E = g.num_nodes, int(g.csr.col.numel())
    avg = {"log": torch.log(g.in_degrees().double() + 1).mean().float().cpu()}
    gen = torch.Generator().manual_seed(4)
    atoms, bonds = torch.randint(0, 28, (V,), generator=gen).to(dev), torch.randint(0, 4, (E,), generator=gen).to(dev)
    targets = torch.randn(len(c["num_nodes"]), 1, generator=gen).to(dev)
    seen = _calls(monkeypatch)
    results = []
    for knob in (4096, 0):
        monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_AGGR_ROWS", knob)
        net = _net(dev, avg)
        loss = net.loss(net(g, atoms, bonds, g.snorm_n()), targets)
        loss.backward()
        results.append((loss.detach(), {k: q.grad.clone() for k, q in net.named_parameters()}))
        if knob:
            assert seen == ["aggr_fwd", "aggr_fwd", "aggr_bwd", "aggr_bwd"]
    assert len(seen) == 4
    (loss1, gr1), (loss0, gr0) = results
    torch.testing.assert_close(loss1, loss0, rtol=1e-5, atol=1e-5)
    wscale = max(v.abs().max().item() for v in gr0.values())
    assert gr1.keys() == gr0.keys()
    for k in gr1:
        base = 3e-4 if ("pretrans" in k and k.endswith("weight")) else 1e-4 if k.startswith("embedding_e") else 1e-5
        C.close(gr1[k], gr0[k].double().cpu(), k, base, 0, scale=wscale)


@pytest.mark.parametrize("kind", ["sum", "max_edge_drop"])
def test_one_training_step_is_bit_identical_on_a_planned_graph(cuda_device, monkeypatch, kind):
    """With graph.BATCH_PLAN_ROWS on, a fresh batch (its transposed CSR and pos_t seated by the batch plan) gives the bits of the same
    batch without the plan."""
    dev = cuda_device
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_AGGR_ROWS", 4096)
    seen = _calls(monkeypatch)
    c = BP.molecules(32, seed=11)
    V, E = sum(c["num_nodes"]), int(c["src"].numel())
    avg = {"log": torch.tensor(1.05)}
    edge = kind != "sum"
    torch.manual_seed(5)
    layer = PNALayer(110, 80, "max" if edge else "sum", "identity", avg, 0.2 if edge else 0.0, True, True, towers=5, pretrans_layers=1, posttrans_layers=1,
                     divide_input=True, residual=True, edge_features=edge, edge_dim=20 if edge else 0).to(dev).train()
    gen = torch.Generator().manual_seed(2)
    h0, e0, R = torch.randn(V, 110, generator=gen).to(dev), torch.randn(E, 20, generator=gen).to(dev), torch.randn(V, 80, generator=gen).to(dev)
    results = []
    for planned in (False, True):
        lay = copy.deepcopy(layer)
        if planned:
            monkeypatch.setattr(G, "BATCH_PLAN_ROWS", 1 << 20)
            g = Graph.collate_flat(c["src"], c["dst"], c["edge_counts"], c["num_nodes"], device=dev, train=True, avg_d=avg)
        else:
            g = BP.unplanned(c, dev)
        assert (g._snorm_n is not None) == planned
        torch.manual_seed(9)                                                        # the mask's key
        h = h0.clone().requires_grad_(True)
        e = e0.clone().requires_grad_(True) if edge else None
        assert lay._small_tower_aggr_train_path(g, h, e, g.snorm_n())
        out = lay(g, h, e, g.snorm_n())
        (out * R).sum().backward()
        results.append([out.detach(), h.grad] + ([e.grad] if edge else []) + [q.grad for q in lay.parameters()] + [b for b in lay.buffers()])
    assert seen == ["aggr_fwd", "aggr_bwd"] * 2
    assert len(results[0]) == len(results[1]) and all(BP.same(x, y) for x, y in zip(*results))
