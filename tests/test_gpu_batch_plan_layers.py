"""Graph.collate_flat behind the knob graph.BATCH_PLAN_ROWS: a planned Graph and an unplanned one hold the same arrays under the same
keys, the one-call training routes give the same bits on either, a captured eval forward runs on a planned graph, a bad id is a
ValueError, and the batches outside the route take the one of today."""
import copy

import pytest
import torch

import batch_plan_cases as C
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd import graph as G
from pna_amd import nets
from pna_amd.dgl.pna_layer import PNALayer, PNASimpleLayer
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu

AGGS, SCALERS = "mean max min std", "identity amplification attenuation"
ITEMS = ("items", G.HEAVY_THRESHOLD, G.SEG_LEN, "natural", 96)
ITEMS_T = ("items", 1 << 30, G.SEG_LEN, "natural", 96)


def _spy(monkeypatch):
    """Counts the pna_batch_plan_i32 calls."""
    seen = {"n": 0}
    real = G._collate_planned

    def wrapped(*a, **k):
        g = real(*a, **k)
        seen["n"] += g is not None
        return g
    monkeypatch.setattr(G, "_collate_planned", wrapped)
    return seen


def _planned(c, dev, monkeypatch, **kw):
    monkeypatch.setattr(G, "BATCH_PLAN_ROWS", 1 << 20)
    return Graph.collate_flat(c["src"], c["dst"], c["edge_counts"], c["num_nodes"], device=dev, **kw)


def _same_csr(a, b):
    return all(C.same(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("name", C.NAMES)
def test_a_planned_graph_holds_the_unplanned_graphs_arrays(cuda_device, monkeypatch, name):
    c = C.case(name)
    seen = _spy(monkeypatch)
    g = _planned(c, cuda_device, monkeypatch, train=True, avg_d={"log": torch.tensor(1.3)})
    assert seen["n"] == 1
    avg_a, avg_b = float(torch.tensor(1.3)), 0.9
    ref = C.reference(c, cuda_device, avg_logs=(avg_a, avg_b))
    g0 = ref["graph"]
    heavy_in, heavy_out = ref["max_in"] > G.HEAVY_THRESHOLD, ref["max_out"] > G.HEAVY_THRESHOLD
    # seated, not rebuilt: the keys the lazy constructions use
    assert g._csr is not None and ("eid32",) in g._heavy and g._snorm_n is not None and avg_a in g._scalers and avg_b not in g._scalers
    assert (ITEMS in g._heavy) == (not heavy_in) and ((G.HEAVY_THRESHOLD, G.SEG_LEN) in g._heavy) == (not heavy_in)
    gT = g._pna_amd_transposed
    assert gT._csr is not None and ITEMS_T in gT._heavy and gT._pna_amd_rank_t is not None and gT._pna_amd_pos_t is not None
    assert (ITEMS in gT._heavy) == (not heavy_out)
    assert g.batch_num_nodes == g0.batch_num_nodes and g.num_nodes == g0.num_nodes
    assert C.same(g.src, g0.src) and C.same(g.dst, g0.dst)
    assert _same_csr(g.csr, g0.csr)
    hs, hs0 = g.heavy_schedule(), g0.heavy_schedule()
    assert all(C.same(x, y) if torch.is_tensor(x) else x == y for x, y in zip(hs, hs0))
    assert C.same(g.work_items(), g0.work_items())
    assert C.same(g.edge_ids32(), g0.edge_ids32())
    assert C.same(g.snorm_n(), g0.snorm_n())
    for v in (avg_a, avg_b):                                                     # one seated from avg_d, one built lazily on the seated CSR
        for x, y in zip(g.degree_scalers(v), ref[("scalers", v)]):
            assert C.same(x, y)
    ro, ro0 = nets._readout_offsets(g, g.src.device), nets._readout_offsets(g0, g0.src.device)
    assert (ro is None) == (ro0 is None) and (ro is None or C.same(ro, ro0))
    for x, y in zip(AG._transposed_whole_rows(g), AG._transposed_whole_rows(g0)):
        assert C.same(x, y)
    assert g._pna_amd_transposed is gT
    assert C.same(gT._pna_amd_pos_t, ref["pos_t"]) and _same_csr(gT.csr, g0._pna_amd_transposed.csr)
    assert C.same(gT.src, ref["row64"]) and C.same(gT.dst, ref["col64"])
    assert C.same(gT.work_items(), g0._pna_amd_transposed.work_items())
    # without train / avg_d: no transposed graph, no scalers, the rest the same
    g1 = _planned(c, cuda_device, monkeypatch, avg_d={"log": torch.tensor(1.3, device=cuda_device)})
    assert seen["n"] == 2 and not hasattr(g1, "_pna_amd_transposed") and not g1._scalers and _same_csr(g1.csr, g0.csr)


def _zinc32():
    return C.molecules(32, seed=11)


def _step(layer, g, args, R):
    out = layer(g, *args)
    (out * R).sum().backward()
    grads = {k: p.grad.clone() for k, p in layer.named_parameters()}
    bufs = {k: b.clone() for k, b in layer.named_buffers()}
    ins = [a.grad.clone() for a in args if torch.is_tensor(a) and a.requires_grad]
    return out.detach(), grads, bufs, ins


@pytest.mark.parametrize("kind", ["tower", "tower_edge", "simple"])
def test_one_training_step_is_bit_identical_on_a_planned_graph(cuda_device, monkeypatch, kind):
    dev = cuda_device
    c = _zinc32()
    V, E = sum(c["num_nodes"]), int(c["src"].numel())
    avg = {"log": torch.tensor(1.05)}
    torch.manual_seed(5)
    if kind == "simple":
        monkeypatch.setattr(PF, "SMALL_TRAIN_ROWS", 4096)
        layer = PNASimpleLayer(75, 75, AGGS, SCALERS, avg, 0.0, True, True)
    else:
        monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_EDGE_ROWS" if kind == "tower_edge" else "SMALL_TOWER_TRAIN_ROWS", 4096)
        edge = kind == "tower_edge"
        layer = PNALayer(75, 75, AGGS, SCALERS, avg, 0.0, True, True, towers=5, pretrans_layers=1, posttrans_layers=1, divide_input=False,
                         residual=True, edge_features=edge, edge_dim=16 if edge else 0)
    layer = layer.to(dev).train()
    gen = torch.Generator().manual_seed(2)
    h0, e0, R = torch.randn(V, 75, generator=gen).to(dev), torch.randn(E, 16, generator=gen).to(dev), torch.randn(V, 75, generator=gen).to(dev)
    results = []
    for planned in (False, True):
        lay = copy.deepcopy(layer)
        g = _planned(c, dev, monkeypatch, train=True, avg_d=avg) if planned else C.unplanned(c, dev)
        assert (g._snorm_n is not None) == planned
        h = h0.clone().requires_grad_(True)
        if kind == "simple":
            assert lay._small_train_path(g, h)
            args = (h,)
        elif kind == "tower":
            assert lay._small_tower_train_path(g, h, g.snorm_n())
            args = (h, None, g.snorm_n())
        else:
            e = e0.clone().requires_grad_(True)
            assert lay._small_tower_train_edge_path(g, h, e, g.snorm_n())
            args = (h, e, g.snorm_n())
        results.append(_step(lay, g, args, R))
    (out0, gr0, bf0, in0), (out1, gr1, bf1, in1) = results
    assert C.same(out0, out1)
    assert len(in0) == len(in1) == (2 if kind == "tower_edge" else 1) and all(C.same(x, y) for x, y in zip(in0, in1))
    assert gr0.keys() == gr1.keys() and all(C.same(gr0[k], gr1[k]) for k in gr0), [k for k in gr0 if not C.same(gr0[k], gr1[k])]
    assert all(C.same(bf0[k], bf1[k]) for k in bf0)


def test_a_captured_eval_forward_runs_on_a_planned_graph(cuda_device, monkeypatch):
    from pna_amd.capture import GraphedForward
    dev = cuda_device
    c = _zinc32()
    V, E = sum(c["num_nodes"]), int(c["src"].numel())
    avg = {"log": torch.tensor(1.1)}
    g = _planned(c, dev, monkeypatch, avg_d=avg)
    torch.manual_seed(3)
    net = nets.PNANet(dict(num_atom_type=28, num_bond_type=4, hidden_dim=75, out_dim=70, in_feat_dropout=0.0, dropout=0.0, L=2, readout="sum",
                           graph_norm=True, batch_norm=True, residual=True, aggregators=AGGS, scalers=SCALERS, avg_d=avg, towers=5,
                           divide_input_first=False, divide_input_last=True, edge_feat=True, edge_dim=50, pretrans_layers=1, posttrans_layers=1,
                           gru=False, device=dev)).to(dev).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 2:
                p.copy_(torch.randn_like(p) / p.shape[1] ** 0.5)
    gen = torch.Generator().manual_seed(1)
    atoms = [torch.randint(0, 28, (V,), generator=gen).to(dev) for _ in range(2)]
    bonds = [torch.randint(0, 4, (E,), generator=gen).to(dev) for _ in range(2)]
    sn = g.snorm_n()
    with torch.no_grad():
        want = [net(g, a_, b_, sn, None).clone() for a_, b_ in zip(atoms, bonds)]
        on_unplanned = net(C.unplanned(c, dev), atoms[0], bonds[0], sn, None)
        gf = GraphedForward(lambda a_, b_: net(g, a_, b_, sn, None), atoms[0], bonds[0])
        got = [gf(a_, b_).clone() for a_, b_ in zip(atoms, bonds)]
    assert C.same(want[0], on_unplanned)
    assert (want[0] - want[1]).abs().max() > 1e-3
    for w, o in zip(want, got):
        assert C.same(o, w)


def test_a_bad_id_is_a_value_error_before_any_layer_sees_the_graph(cuda_device, monkeypatch):
    c = C.case("molecules_300")
    for side, value in (("src", c["num_nodes"][0]), ("dst", -1)):
        bad = dict(c, **{side: c[side].clone()})
        bad[side][3] = value
        with pytest.raises(ValueError, match="outside its member graph"):
            _planned(bad, cuda_device, monkeypatch, train=True)
    with pytest.raises(ValueError, match="do not describe"):
        _planned(dict(c, edge_counts=c["edge_counts"][:-1] + [c["edge_counts"][-1] + 1]), cuda_device, monkeypatch)


def test_batches_outside_the_route_take_the_route_of_today(cuda_device, monkeypatch):
    dev = cuda_device
    seen = _spy(monkeypatch)
    c = C.case("molecules_300")
    V = sum(c["num_nodes"])
    want = C.unplanned(c, dev)

    def old_route(g):
        assert not g._heavy and g._snorm_n is None and not hasattr(g, "_pna_amd_transposed")
        assert C.same(g.src, want.src) and C.same(g.dst, want.dst) and _same_csr(g.csr, want.csr) and g.batch_num_nodes == want.batch_num_nodes
    assert G.BATCH_PLAN_ROWS == 0
    old_route(Graph.collate_flat(c["src"], c["dst"], c["edge_counts"], c["num_nodes"], device=dev, train=True, avg_d=1.2))     # the default
    monkeypatch.setattr(G, "BATCH_PLAN_ROWS", V - 1)                             # a batch over the knob
    old_route(Graph.collate_flat(c["src"], c["dst"], c["edge_counts"], c["num_nodes"], device=dev, train=True))
    monkeypatch.setattr(G, "BATCH_PLAN_ROWS", V)
    counts_dev, sizes_dev = torch.tensor(c["edge_counts"]).to(dev), torch.tensor(c["num_nodes"]).to(dev)
    old_route(Graph.collate_flat(c["src"], c["dst"], counts_dev, c["num_nodes"], device=dev, train=True))                      # device-resident counts
    old_route(Graph.collate_flat(c["src"], c["dst"], c["edge_counts"], sizes_dev, device=dev, train=True))
    assert seen["n"] == 0
    g = Graph.collate_flat(c["src"], c["dst"], torch.tensor(c["edge_counts"]), torch.tensor(c["num_nodes"]), device=dev, train=True)   # host tensors: planned
    assert seen["n"] == 1 and g._snorm_n is not None and _same_csr(g.csr, want.csr)
    g = Graph.collate_flat(c["src"].to(dev), c["dst"].to(dev), c["edge_counts"], c["num_nodes"])                                # device edges, device from them
    assert seen["n"] == 2 and _same_csr(g.csr, want.csr)
    # a member over the limits
    lim_n, lim_e = G.batch_plan_limits()
    big = dict(src=torch.cat([c["src"], torch.zeros(lim_e + 1, dtype=torch.int64)]), dst=torch.cat([c["dst"], torch.arange(lim_e + 1) % 3]),
               edge_counts=c["edge_counts"] + [lim_e + 1], num_nodes=c["num_nodes"] + [3])
    monkeypatch.setattr(G, "BATCH_PLAN_ROWS", 1 << 20)
    g = Graph.collate_flat(big["src"], big["dst"], big["edge_counts"], big["num_nodes"], device=dev, train=True)
    assert seen["n"] == 2 and not g._heavy and _same_csr(g.csr, C.unplanned(big, dev).csr)
