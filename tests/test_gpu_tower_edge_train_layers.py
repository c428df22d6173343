"""PNALayer with edge features in training through the one-call route (autograd.TowerLayerEdgeSmallTrainFn:
pna_tower_edge_train_fwd_f32 / _bwd_f32) behind the knob functional.SMALL_TOWER_TRAIN_EDGE_ROWS: the reference's golden training step
with edge features, the route actually taken with the knob on and off, a two-layer ZINC-shaped stack over one shared bond embedding
against a float64 stack, and the calls that fall through."""
import pytest
import torch

import tower_edge_train_cases as C
from oracle import torch_oracle as O
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd.dgl.pna_layer import PNALayer
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu

SEED, GRAPH_SEED = 1, 1          # of the stacked test's embedding / bond types and edge order


def _spies(monkeypatch):
    seen = {"edge": 0, "plain": 0}
    for key, fn in (("edge", AG.TowerLayerEdgeSmallTrainFn), ("plain", AG.TowerLayerSmallTrainFn)):
        real = fn.apply
        monkeypatch.setattr(fn, "apply", staticmethod(lambda *x, _k=key, _r=real: (seen.__setitem__(_k, seen[_k] + 1), _r(*x))[1]))
    return seen


def _layer(meta, a, sd, dev, **kw):
    args = dict(towers=meta["towers"], pretrans_layers=1, posttrans_layers=1, divide_input=meta["divide_input"], residual=meta["residual"],
                edge_features=True, edge_dim=meta["edge_dim"])
    args.update(kw)
    dropout = args.pop("dropout", 0.0)
    layer = PNALayer(meta["in_dim"], meta["out_dim"], meta["aggregators"], meta["scalers"], {"log": a["avg_log"]}, dropout, True, True, **args)
    if sd is not None:
        layer.load_state_dict(sd)
    return layer.to(dev).train()


def _golden(dev):
    meta, a, sd, ref = C.case(C.GOLDEN)
    layer = _layer(meta, a, sd, dev)
    g = Graph(a["src"], a["dst"], meta["N"], meta["sizes"]).to(dev)
    h = a["h"].to(dev).requires_grad_(True)
    e = a["e"].to(dev).requires_grad_(True)
    return meta, a, sd, ref, layer, g, h, e, a["snorm_n"].to(dev)


def test_golden_training_step_through_the_one_call_route(cuda_device, monkeypatch):
    """tower_train_t3_edgefeat (oracle/make_golden_simple_train.py) with the bars of tests/test_gpu_backward.py::
    test_tower_layer_training_step_golden on the output, every gradient (grad_e included) and the running statistics, served by the new
    call and not by the route without edge features, whose knob is on as well."""
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_EDGE_ROWS", 4096)
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_ROWS", 4096)
    seen = _spies(monkeypatch)
    meta, a, sd, ref, layer, g, h, e, snorm = _golden(cuda_device)
    assert layer._small_tower_train_edge_path(g, h, e, snorm) and not layer._small_tower_train_path(g, h, snorm)
    out = layer(g, h, e, snorm)
    assert seen == {"edge": 1, "plain": 0}
    (out * a["R"].to(cuda_device)).sum().backward()
    C.check_step(meta, ref, out.detach(), h.grad, {k: p.grad for k, p in layer.named_parameters()},
                 {k: b for k, b in layer.named_buffers() if "running" in k})
    C.check_grad_e(ref, e.grad)
    for t, tower in enumerate(layer.towers):
        assert int(tower.batchnorm_h.num_batches_tracked) == int(sd[f"towers.{t}.batchnorm_h.num_batches_tracked"]) + 1


def test_knob_at_its_default_keeps_the_existing_route(cuda_device, monkeypatch):
    assert PF.SMALL_TOWER_TRAIN_EDGE_ROWS == 0
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_ROWS", 4096)                      # (the other route's knob does not serve this layer)
    seen = _spies(monkeypatch)
    meta, a, sd, ref, layer, g, h, e, snorm = _golden(cuda_device)
    out = layer(g, h, e, snorm)
    assert seen == {"edge": 0, "plain": 0}
    C.close(out.detach(), ref.out, "out (generic route)", 1e-5, int(ref.ill.sum()), ref.ill)


def stack_inputs():
    """The two-layer stack's inputs (host): zinc_edge_first (70 -> 70, 5 towers, residual) then zinc_edge_last (70 -> 60) on nine complete
    5-node graphs (45 nodes, in-degree 4, the edge order shuffled), e = emb[types] with ONE 4-row embedding shared by both layers."""
    meta1, a, sd1, _ = C.case("zinc_edge_first")
    meta2, _, sd2, _ = C.case("zinc_edge_last")
    gen = torch.Generator().manual_seed(SEED)
    sizes = [5] * 9
    pairs = torch.tensor([(5 * m + u, 5 * m + v) for m in range(9) for u in range(5) for v in range(5) if u != v])
    pairs = pairs[torch.randperm(pairs.shape[0], generator=torch.Generator().manual_seed(GRAPH_SEED))]
    src, dst = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    V = sum(sizes)
    assert V == meta1["N"] == 45
    types = torch.randint(0, 4, (src.numel(),), generator=gen)
    emb = torch.randn(4, meta1["edge_dim"], generator=gen)
    R = torch.randn(V, meta2["out_dim"], generator=gen)
    a = dict(a, src=src, dst=dst, avg_log=torch.log(torch.bincount(dst, minlength=V).double() + 1).mean().float())
    return [meta1, meta2], [sd1, sd2], a, sizes, types, emb, R


def stack_reference(metas, sds, a, types, emb, R, dtype):
    """The stack from the oracle's dgl_layer_forward in `dtype` under torch autograd -> (out, grad_h, grad_emb, live state dicts, the
    layers' inputs)."""
    V = metas[0]["N"]
    src, dst = a["src"].long(), a["dst"].long()
    scalers = metas[0]["scalers"].split()
    live = [{k: (v.to(dtype).clone().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in sd.items()} for sd in sds]
    h0 = a["h"].to(dtype).clone().requires_grad_(True)
    em = emb.to(dtype).clone().requires_grad_(True)
    x, xs = h0, []
    for sd, m in zip(live, metas):
        xs.append(x.detach())
        x = O.dgl_layer_forward(sd, src, dst, V, x, em[types], a["snorm_n"].to(dtype), C.AGGS, scalers, a["avg_log"].to(dtype), m["towers"],
                                m["divide_input"], True, True, True, True, running={})
    (x * R.to(dtype)).sum().backward()
    return x.detach(), h0.grad, em.grad, live, xs


def stack_conditions(metas, sds, a, sizes, types, emb, live64, xs64):
    """(ill destinations of either layer, the rows of the molecules that hold one, the smallest |p| / largest |p| over the layers)."""
    V = metas[0]["N"]
    src, dst = a["src"].long(), a["dst"].long()
    scalers = metas[0]["scalers"].split()
    mol = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ill = torch.zeros(V, dtype=torch.bool)
    pmin = 1.0
    for sd, live, m, x in zip(sds, live64, metas, xs64):
        ill |= C.ill_conditioned(m, dict(a, h=x, e=emb[types]), sd)[0]
        with torch.no_grad():
            y = O.dgl_layer_forward({k: v.detach() for k, v in live.items()}, src, dst, V, x, emb.double()[types], a["snorm_n"].double(), C.AGGS, scalers,
                                    a["avg_log"].double(), m["towers"], m["divide_input"], True, True, False, True, running={})
        p = torch.where(y > 0, y, y / C.SLOPE)
        pmin = min(pmin, (p.abs().min() / p.abs().max()).item())
    return ill, torch.isin(mol, mol[ill]), pmin


def test_two_layer_stack_with_a_shared_embedding_against_a_float64_stack(cuda_device, monkeypatch):
    """Forward + backward of the stack of stack_inputs() against the float64 stack: the bars of tests/test_gpu_tower_train_layers.py's
    stacked test -- the output on EVERY row at rtol / atol 1e-5; grad_h at 1e-4 of the largest entry outside the molecules that hold an
    ill-conditioned destination of either layer, those rows (asserted to be at most a third) at 2e-3; parameter gradients at the golden
    step's bars.  emb.grad is a sum over all edges of both layers, so it is held like a parameter tensor, at the edge gradients' 1e-4 of
    its largest entry + 4 x the fp32 stack's own error when the list is non-empty.  Seeds picked on the CPU so the float64 stack alone
    satisfies the conditions and no LeakyReLU sign is decided by rounding."""
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_EDGE_ROWS", 4096)
    seen = _spies(monkeypatch)
    metas, sds, a, sizes, types, emb, R = stack_inputs()
    out64, gh64, gemb64, live64, xs64 = stack_reference(metas, sds, a, types, emb, R, torch.float64)
    out32, gh32, gemb32, live32, _ = stack_reference(metas, sds, a, types, emb, R, torch.float32)
    ill, loose, pmin = stack_conditions(metas, sds, a, sizes, types, emb, live64, xs64)
    V = metas[0]["N"]
    print(f"[tower_edge_train] stack: {int(ill.sum())} ill-conditioned destinations over the two layers; grad_h rows at the loose bar: {int(loose.sum())} of {V}")
    assert int(loose.sum()) <= V // 3, int(loose.sum())
    assert pmin >= 1e-5, pmin

    dev = cuda_device
    layers = [_layer(m, a, sd, dev) for m, sd in zip(metas, sds)]
    g = Graph(a["src"], a["dst"], V).to(dev)
    h = a["h"].to(dev).requires_grad_(True)
    em = emb.to(dev).requires_grad_(True)
    snorm = a["snorm_n"].to(dev)
    tys = types.to(dev)
    x = h
    for layer in layers:
        x = layer(g, x, em[tys], snorm)
    assert seen == {"edge": 2, "plain": 0}
    (x * R.to(dev)).sum().backward()
    n_ill = int(ill.sum())
    torch.testing.assert_close(x.detach().cpu(), out64.float(), rtol=1e-5, atol=1e-5)
    C.close(h.grad, gh64, "grad_h (stack)", 1e-4, n_ill, loose)
    C.close(em.grad, gemb64, "emb.grad (stack)", 1e-4, n_ill, ref=gemb32)
    wscale = max(v.grad.abs().max().item() for sd in live64 for k, v in sd.items() if v.is_floating_point() and v.grad is not None)
    for i, layer in enumerate(layers):
        for k, p in layer.named_parameters():
            pre = "pretrans" in k and k.endswith("weight")
            C.close(p.grad, live64[i][k].grad, f"layer {i} {k}", 3e-4 if pre else 1e-5, n_ill, scale=wscale, ref=live32[i][k].grad)


def _outcome(layer, g, h, e, snorm):
    """What a call does: the exception type it raises on the host, or "finite" after a forward and backward with finite results."""
    h.grad = None
    try:
        out = layer(g, h, e, snorm)
    except (RuntimeError, TypeError, ValueError) as ex:
        return type(ex)
    out.sum().backward()
    assert bool(torch.isfinite(out).all()) and h.grad is not None and bool(torch.isfinite(h.grad).all())
    return "finite"


@pytest.mark.parametrize("what", ["dropout", "edge_dim_65", "float64_e", "extra_rows", "eval"])
def test_calls_outside_the_scope_fall_through(cuda_device, monkeypatch, what):
    """Each call does with the knob on what it does with the knob off, and the new function is never called.  float64 e and an e with a
    wrong row count do whatever the old route does with them (a dtype error raised on the host; rows past the last edge id are never
    read) -- the row count is wrong by EXTRA rows: with too few the old route's gather of e[eid] would read out of bounds on the
    device, which no test may provoke."""
    seen = _spies(monkeypatch)
    meta, a, sd, _ = C.case(C.GOLDEN)
    torch.manual_seed(0)
    E, ed = a["src"].numel(), meta["edge_dim"]
    if what == "dropout":
        layer = _layer(meta, a, None, cuda_device, dropout=0.3)
    elif what == "edge_dim_65":
        layer, ed = _layer(meta, a, None, cuda_device, edge_dim=65), 65
    elif what == "eval":
        layer = _layer(meta, a, sd, cuda_device).eval()
    else:
        layer = _layer(meta, a, sd, cuda_device)
    g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
    h = a["h"].to(cuda_device).requires_grad_(True)
    snorm = a["snorm_n"].to(cuda_device)
    e = torch.randn(E + (3 if what == "extra_rows" else 0), ed, device=cuda_device, dtype=torch.float64 if what == "float64_e" else torch.float32)
    got = []
    for knob in (0, 4096):
        monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_EDGE_ROWS", knob)
        got.append(_outcome(layer, g, h, e, snorm))
    assert got[0] == got[1] and seen == {"edge": 0, "plain": 0}
    if what != "float64_e":
        assert got[1] == "finite"


def test_a_missing_e_raises_the_existing_value_error(cuda_device, monkeypatch):
    monkeypatch.setattr(PF, "SMALL_TOWER_TRAIN_EDGE_ROWS", 4096)
    seen = _spies(monkeypatch)
    meta, a, sd, _ = C.case(C.GOLDEN)
    layer = _layer(meta, a, sd, cuda_device)
    g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
    h = a["h"].to(cuda_device).requires_grad_(True)
    with pytest.raises(ValueError, match="no edge features were given"):
        layer(g, h, None, a["snorm_n"].to(cuda_device))
    assert seen == {"edge": 0, "plain": 0}
