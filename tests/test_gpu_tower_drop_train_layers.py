"""PNALayer with dropout inside its towers in training through the one-call route (autograd.TowerLayerDropSmallTrainFn:
pna_tower_drop_train_fwd_f32 / _bwd_f32) behind the knob functional.SMALL_TOWER_TRAIN_DROPOUT_ROWS: the route actually taken with the knob
on and off, the step against the float64 oracle under the mask of the key the layer drew, reproducibility under torch.manual_seed, the
capture exclusion, and a two-layer PNANetSuperpixels (both published dropout settings) against a masked float64 stack."""
import pytest
import torch

import tower_drop_train_cases as C
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd.dgl.pna_layer import PNALayer
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu


def _spies(monkeypatch):
    seen = {"drop": 0, "edge": 0, "plain": 0}
    for key, fn in (("drop", AG.TowerLayerDropSmallTrainFn), ("edge", AG.TowerLayerEdgeSmallTrainFn), ("plain", AG.TowerLayerSmallTrainFn)):
        real = fn.apply
        monkeypatch.setattr(fn, "apply", staticmethod(lambda *x, _k=key, _r=real: (seen.__setitem__(_k, seen[_k] + 1), _r(*x))[1]))
    return seen


def _setup(name, dev):
    meta, a, sd, _, (p, seed, offset) = C.case(name)
    edge = meta["edge_dim"] > 0
    layer = PNALayer(meta["in_dim"], meta["out_dim"], meta["aggregators"], meta["scalers"], {"log": a["avg_log"]}, p, True, True, towers=meta["towers"],
                     pretrans_layers=1, posttrans_layers=1, divide_input=meta["divide_input"], residual=meta["residual"], edge_features=edge,
                     edge_dim=meta["edge_dim"])
    layer.load_state_dict(sd)
    layer = layer.to(dev).train()
    g = Graph(a["src"], a["dst"], meta["N"]).to(dev)
    h = a["h"].to(dev).requires_grad_(True)
    e = a["e"].to(dev).requires_grad_(True) if edge else None
    return meta, a, sd, layer, g, h, e, a["snorm_n"].to(dev)


def _set_key(dev, seed, offset):
    gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    gen.manual_seed(seed)
    gen.set_offset(offset)
    return gen


@pytest.mark.parametrize("name", ["tower_train_t4_div", "zinc_edge_first"])
def test_training_step_takes_the_new_route_and_matches_the_masked_oracle(cuda_device, monkeypatch, name):
    """The generator state read just before the call is the mask's key; the step matches the float64 oracle under that mask at the bars of
    tower_train_cases.check_step (the case's key was picked on the CPU: tower_drop_train_cases); the generator has moved past the mask."""
    for knob in ("SMALL_TOWER_TRAIN_DROPOUT_ROWS", "SMALL_TOWER_TRAIN_ROWS", "SMALL_TOWER_TRAIN_EDGE_ROWS"):
        monkeypatch.setattr(PF, knob, 4096)
    seen = _spies(monkeypatch)
    meta, a, sd, layer, g, h, e, snorm = _setup(name, cuda_device)
    p, seed, offset = C.case(name)[4]
    gen = _set_key(cuda_device, seed, offset)
    assert layer._small_tower_drop_train_path(g, h, e, snorm)
    assert not layer._small_tower_train_path(g, h, snorm) and not layer._small_tower_train_edge_path(g, h, e, snorm)
    key = (layer.towers[0].dropout, gen.initial_seed(), gen.get_offset())
    assert key == (p, seed, offset)
    out = layer(g, h, e, snorm)
    assert seen == {"drop": 1, "edge": 0, "plain": 0}
    n = meta["N"] * meta["out_dim"]
    assert gen.get_offset() == offset + 4 * ((n + 3) // 4) and gen.initial_seed() == seed
    (out * a["R"].to(cuda_device)).sum().backward()
    ref = C.case(name, *key)[3]
    C.check_step(meta, ref, out.detach(), h.grad, {k: q.grad for k, q in layer.named_parameters()}, {k: b for k, b in layer.named_buffers() if "running" in k})
    if e is not None:
        C.check_grad_e(ref, e.grad)
    for t, tower in enumerate(layer.towers):
        assert int(tower.batchnorm_h.num_batches_tracked) == int(sd[f"towers.{t}.batchnorm_h.num_batches_tracked"]) + 1


def test_knob_at_its_default_keeps_the_generic_route(cuda_device, monkeypatch):
    assert PF.SMALL_TOWER_TRAIN_DROPOUT_ROWS == 0
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_ROWS", 4096)                      # (the other routes' knobs do not serve this layer)
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_EDGE_ROWS", 4096)
    seen = _spies(monkeypatch)
    meta, a, sd, layer, g, h, e, snorm = _setup("tower_train_t4_div", cuda_device)
    out = layer(g, h, e, snorm)
    out.sum().backward()
    assert seen == {"drop": 0, "edge": 0, "plain": 0}
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(h.grad).all())


def test_manual_seed_reproduces_a_step_and_successive_calls_differ(cuda_device, monkeypatch):
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_DROPOUT_ROWS", 4096)
    seen = _spies(monkeypatch)
    meta, a, sd, layer, g, h, e, snorm = _setup("tower_train_t4_div", cuda_device)

    def step():
        h.grad = None
        layer.zero_grad(set_to_none=True)
        out = layer(g, h, e, snorm)
        (out * a["R"].to(cuda_device)).sum().backward()
        return [out.detach().clone(), h.grad.clone()] + [q.grad.clone() for q in layer.parameters()]
    torch.manual_seed(5)
    first = step()
    second = step()                                                               # no re-seeding: the generator moved on, another mask
    torch.manual_seed(5)
    third = step()
    assert seen["drop"] == 3
    for t0, t1 in zip(first, third):
        assert torch.equal(t0, t1)
    assert not torch.equal(first[0], second[0]) and not torch.equal(first[1], second[1])


def test_a_capturing_stream_keeps_the_generic_route(cuda_device, monkeypatch):
    """While a hipGraph is being captured the predicate is false (the key is host state: a replay would repeat the captured mask).  The
    capture records one elementwise kernel and is never replayed."""
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_DROPOUT_ROWS", 4096)
    meta, a, sd, layer, g, h, e, snorm = _setup("tower_train_t4_div", cuda_device)
    assert layer._small_tower_drop_train_path(g, h, e, snorm)                     # (this also builds what the predicate reads of the graph)
    x = torch.ones(64, device=cuda_device)
    torch.cuda.synchronize(cuda_device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        inside = (torch.cuda.is_current_stream_capturing(), layer._small_tower_drop_train_path(g, h, e, snorm))
        y = x * 2.0                                                               # noqa: F841  (a capture is not left empty)
    torch.cuda.synchronize(cuda_device)
    assert inside == (True, False)
    assert layer._small_tower_drop_train_path(g, h, e, snorm)


@pytest.mark.parametrize("name", list(C.NETS))
def test_two_layer_superpixels_net_against_a_masked_float64_stack(cuda_device, monkeypatch, name):
    """PNANetSuperpixels(in_dim 5, hidden = out = 60, 5 towers, both layers over divided inputs, readout sum) at dropout 0.1 without and
    0.3 with edge features (edge_dim 50) on four graphs of 20 to 30 nodes with 8 in-edges per node: every layer goes through the new
    Function; the loss and every parameter gradient against the same net restated from the oracle in float64 under the masks of the
    keys the layers draw (seed = torch.manual_seed's, offsets 0 and 4 ceil(V 60 / 4)).  Bars of the stacked test of
    tests/test_gpu_tower_train_layers.py: the loss at rtol / atol 1e-5; parameter gradients at 3e-4 of the largest parameter-gradient
    entry for pretrans weights, 1e-5 for the others, + 4 x the fp32 stack's own error on the tensor when a layer has an ill-conditioned
    destination.  The seeds (weights, batch, dropout) were picked on the CPU so that the float64 stack has at most 15 % listed
    destinations and no LeakyReLU sign of either layer is decided by rounding under its mask."""
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_DROPOUT_ROWS", 4096)
    seen = _spies(monkeypatch)
    ref, b = C.net_reference(name), C.net_batch()
    n_ill = int(ref.ill.sum())
    print(f"[tower_drop_train] net {name}: {n_ill} ill-conditioned destinations over the two layers; min |p| / max |p| = {ref.pmin:.2e}")
    assert n_ill <= 0.15 * b["N"] and ref.pmin >= 1e-5
    dev = cuda_device
    net = C.net_model(name).to(dev).train()
    g = Graph(b["src"], b["dst"], b["N"], b["sizes"]).to(dev)
    gen = _set_key(dev, ref.seed, 0)
    pred = net(g, b["x"].to(dev), b["e"].to(dev), b["snorm_n"].to(dev), None)
    assert seen == {"drop": 2, "edge": 0, "plain": 0}
    assert gen.get_offset() == 2 * 4 * ((b["N"] * 60 + 3) // 4)
    loss = net.loss(pred, b["labels"].to(dev))
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), ref.loss.float(), rtol=1e-5, atol=1e-5)
    wscale = max(v.grad.abs().max().item() for v in ref.live.values() if v.is_floating_point() and v.grad is not None)
    for k, q in net.named_parameters():
        pre = "pretrans" in k and k.endswith("weight")
        C.close(q.grad, ref.live[k].grad, k, 3e-4 if pre else 1e-5, n_ill, scale=wscale, ref=ref.live32[k].grad)
