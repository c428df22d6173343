"""pytorch_geometric.PNAConv in fp32 through the one-call route (autograd.PygConvFn: pna_pyg_conv_train_fwd_f32 / _bwd_f32) behind the knob
functional.PYG_TRAIN_ROWS: the entry pair actually called, the step against the float64 oracle and against the knob-off run of the same
layer, the routes a call takes with the knob off or outside the scope, a reference state_dict, a two-layer stack with BatchNorm1d, the
no-grad forward and its hipGraph replay."""
import copy

import pytest
import torch

import pyg_train_cases as C
from conftest import load_golden
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd.capture import GraphedForward
from pna_amd.pytorch_geometric import PNAConv

pytestmark = pytest.mark.gpu


def _calls(monkeypatch):
    """Records the C entry points autograd.PygConvFn runs (as test_gpu_tower_aggr_train_layers._calls does for the tower routes)."""
    seen = []
    real = AG._pyg_conv_call

    def wrapped(which, y, dev):
        seen.append(which)
        return real(which, y, dev)
    monkeypatch.setattr(AG, "_pyg_conv_call", wrapped)
    return seen


def _layer(meta, a, sd, dev, **kw):
    args = dict(edge_dim=meta["edge_dim"] or None, towers=meta["towers"], divide_input=meta["divide_input"])
    args.update(kw)
    layer = PNAConv(meta["in_c"], meta["out_c"], meta["aggregators"], meta["scalers"], a["deg_hist"], **args)
    if sd is not None:
        layer.load_state_dict(sd, strict=True)
    return layer.to(dev).train()


def _step(layer, a, meta, dev):
    x = a["x"].to(dev).requires_grad_(True)
    e = a["edge_attr"].to(dev).requires_grad_(True) if meta["edge_dim"] else None
    ei = a["edge_index"].to(dev)
    out = layer(x, ei, e)
    (out * a["R"].to(dev)).sum().backward()
    return out.detach(), x.grad, None if e is None else e.grad, {k: p.grad for k, p in layer.named_parameters()}


@pytest.mark.parametrize("name", ["v17_t5", "v33_edge64", "v33_div_edge1", "sum_only", "var_neg", "zinc"])
def test_training_step_takes_the_new_route_and_matches_float64_and_the_generic_route(cuda_device, monkeypatch, name):
    dev = cuda_device
    monkeypatch.setattr(PF, "PYG_TRAIN_ROWS", 4096)
    seen = _calls(monkeypatch)
    meta, a, sd, ref = C.case(name)
    layer = _layer(meta, a, sd, dev)
    assert layer.avg_deg == pytest.approx(meta["avg_deg"], nan_ok=True)
    generic = copy.deepcopy(layer)
    assert layer._one_call_path(a["x"].to(dev), a["edge_attr"].to(dev) if meta["edge_dim"] else None)
    out, gx, ge, grads = _step(layer, a, meta, dev)
    assert seen == ["fwd", "bwd"]
    C.check_step(ref, out, gx, grads, ge)
    monkeypatch.setattr(PF, "PYG_TRAIN_ROWS", 0)
    out0, gx0, ge0, grads0 = _step(generic, a, meta, dev)
    assert seen == ["fwd", "bwd"]                                                # (the knob-off run called neither)
    n_ill = int(ref.ill.sum())
    C.close(out, out0.double().cpu(), "out vs generic", 1e-5, n_ill, ref.ill)
    C.close(gx, gx0.double().cpu(), "grad_x vs generic", 1e-4, n_ill, ref.touched)
    wscale = max(v.abs().max().item() for v in ref.ref32["grads"].values())
    for k, g in grads.items():
        pre = k.startswith("pre_nns") and k.endswith("weight")
        C.close(g, grads0[k].double().cpu(), k + " vs generic", 3e-4 if pre else 1e-5, n_ill, scale=wscale, ref=ref.ref32["grads"][k])
    if ge is not None:
        C.close(ge, ge0.double().cpu(), "grad_edge_attr vs generic", 1e-4, n_ill, scale=max(1.0, ref.grad_e.abs().max().item()), ref=ref.ref32["grad_e"])


def test_knob_off_or_outside_the_scope_takes_the_earlier_route(cuda_device, monkeypatch):
    dev = cuda_device
    seen = _calls(monkeypatch)
    meta, a, sd, _ = C.case("v33_div_edge1")
    monkeypatch.setattr(PF, "PYG_TRAIN_ROWS", 0)
    base = _step(_layer(meta, a, sd, dev), a, meta, dev)
    assert seen == []
    monkeypatch.setattr(PF, "PYG_TRAIN_ROWS", 16)                                # the knob does not cover 33 rows
    small = _step(_layer(meta, a, sd, dev), a, meta, dev)
    assert seen == [] and torch.equal(small[0], base[0])
    monkeypatch.setattr(PF, "PYG_TRAIN_ROWS", 4096)
    x, ei, e = a["x"].to(dev), a["edge_index"].to(dev), a["edge_attr"].to(dev)
    for kw in (dict(pre_layers=2), dict(post_layers=2)):
        layer = _layer(meta, a, None, dev, **kw)
        assert not layer._one_call_path(x, e)
        assert bool(torch.isfinite(layer(x, ei, e)).all()) and seen == []
    m4 = dict(meta, scalers=["identity", "amplification", "attenuation", "linear"])
    layer = _layer(m4, a, None, dev)
    assert not layer._one_call_path(x, e) and bool(torch.isfinite(layer(x, ei, e)).all()) and seen == []
    m3 = dict(meta, in_c=3, towers=1, divide_input=False, out_c=4)                # F_in = 3
    layer = _layer(m3, a, None, dev)
    assert not layer._one_call_path(x[:, :3].contiguous(), e) and bool(torch.isfinite(layer(x[:, :3].contiguous(), ei, e)).all()) and seen == []
    bf = _layer(meta, a, sd, dev).eval().to(torch.bfloat16)
    with torch.no_grad():
        assert not bf._one_call_path(x.to(torch.bfloat16), e.to(torch.bfloat16))
        assert bf(x.to(torch.bfloat16), ei, e.to(torch.bfloat16)).dtype == torch.bfloat16 and seen == []
    with pytest.raises(RuntimeError, match="edge_attr"):                          # the generic route's own error
        _layer(meta, a, sd, dev)(x, ei, None)
    assert seen == []


def test_a_reference_state_dict_loads_strictly_and_trains(cuda_device, monkeypatch):
    """The reference module's own parameters and its own float64 training step (tests/golden/pyg_conv_train_step.npz)."""
    dev = cuda_device
    monkeypatch.setattr(PF, "PYG_TRAIN_ROWS", 4096)
    seen = _calls(monkeypatch)
    gm, a, sd = load_golden("pyg_conv_train_step")
    T = gm["towers"]
    _, avg = C.avg_deg_of(a["edge_index"][1], gm["N"])
    meta = dict(N=gm["N"], in_c=gm["in_c"], out_c=gm["out_c"], towers=T, divide_input=True, F_in=gm["in_c"] // T, F_out=gm["out_c"] // T,
                edge_dim=gm["edge_dim"], aggregators=gm["aggregators"], scalers=gm["scalers"], avg_deg=avg)
    ref = C.reference(meta, a, sd, "golden")
    for k, g in ref.grads.items():                                                # the oracle IS the reference's step (the host test's bar)
        torch.testing.assert_close(g, a["f64/grad/" + k], rtol=1e-10, atol=1e-10)
    layer = _layer(meta, a, sd, dev)
    out, gx, ge, grads = _step(layer, a, meta, dev)
    assert seen == ["fwd", "bwd"]
    C.check_step(ref, out, gx, grads, ge)
    opt = torch.optim.Adam(layer.parameters(), lr=1e-3)
    opt.step()
    out2 = _step(layer, a, meta, dev)[0]
    assert seen == ["fwd", "bwd", "fwd", "bwd"] and not torch.equal(out, out2)     # the call reads the weights as the optimiser left them


class _Stack(torch.nn.Module):
    def __init__(self, meta, a):
        super().__init__()
        kw = dict(edge_dim=meta["edge_dim"] or None, towers=meta["towers"], divide_input=meta["divide_input"])
        self.c1 = PNAConv(meta["in_c"], meta["in_c"], meta["aggregators"], meta["scalers"], a["deg_hist"], **kw)
        self.bn = torch.nn.BatchNorm1d(meta["in_c"])
        self.c2 = PNAConv(meta["in_c"], meta["out_c"], meta["aggregators"], meta["scalers"], a["deg_hist"], **kw)

    def forward(self, x, ei, e):
        return self.c2(torch.relu(self.bn(self.c1(x, ei, e))), ei, e)


def test_two_layer_stack_with_batchnorm_matches_its_knob_off_step(cuda_device, monkeypatch):
    dev = cuda_device
    seen = _calls(monkeypatch)
    meta, a, _, ref = C.case("v33_div_edge1")
    torch.manual_seed(5)
    net = _Stack(meta, a).to(dev).train()
    other = copy.deepcopy(net)
    res = []
    for knob, m in ((4096, net), (0, other)):
        monkeypatch.setattr(PF, "PYG_TRAIN_ROWS", knob)
        out, gx, ge, grads = _step(m, a, meta, dev)
        res.append(((out * a["R"].to(dev)).sum().item(), gx, ge, grads))
    assert seen == ["fwd", "fwd", "bwd", "bwd"]
    (l1, gx1, ge1, g1), (l0, gx0, ge0, g0) = res
    assert abs(l1 - l0) <= 1e-5 * max(1.0, abs(l0)), (l1, l0)
    wscale = max(v.abs().max().item() for v in g0.values())
    C.close(gx1, gx0.double().cpu(), "stack grad_x", 1e-4, 0)
    C.close(ge1, ge0.double().cpu(), "stack grad_edge_attr", 1e-4, 0)
    for k, g in g1.items():
        pre = "pre_nns" in k and k.endswith("weight")
        C.close(g, g0[k].double().cpu(), "stack " + k, 3e-4 if pre else 1e-5, 0, scale=wscale)


def test_no_grad_eval_forward_equals_the_training_forward_and_replays(cuda_device, monkeypatch):
    dev = cuda_device
    monkeypatch.setattr(PF, "PYG_TRAIN_ROWS", 4096)
    seen = _calls(monkeypatch)
    meta, a, sd, _ = C.case("zinc")
    layer = _layer(meta, a, sd, dev)
    x, ei, e = a["x"].to(dev), a["edge_index"].to(dev), a["edge_attr"].to(dev)
    train_out = layer(x, ei, e).detach()
    layer.eval()
    with torch.no_grad():
        eval_out = layer(x, ei, e)
        assert seen == ["fwd", "fwd"] and torch.equal(train_out, eval_out)
        graphed = GraphedForward(layer, x, ei, e)
        n = len(seen)
        x2 = torch.randn_like(x)
        replay = graphed(x2, ei, e).clone()
        assert len(seen) == n                                                    # a replay runs no Python
        assert torch.equal(replay, layer(x2, ei, e))
