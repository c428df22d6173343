"""PNASimpleLayer in training through the one-call route (autograd.SimpleLayerSmallTrainFn: pna_simple_train_fwd_f32 / _bwd_f32) behind
the knob functional.SMALL_TRAIN_ROWS: the reference's golden training steps, the route actually taken with the knob on and off, two
stacked layers against a float64 stack under torch autograd, num_batches_tracked, and eval afterwards."""
import pytest
import torch

import small_train_cases as C
from conftest import golden_names, load_golden
from oracle import torch_oracle as O
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd.dgl.pna_layer import PNASimpleLayer
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu


def _spies(monkeypatch):
    seen = {"small": 0, "tail": 0}
    real_small, real_tail = AG.SimpleLayerSmallTrainFn.apply, AG.bn_relu_residual
    monkeypatch.setattr(AG, "simple_layer_small_train", (lambda real: lambda *x, **k: (seen.__setitem__("small", seen["small"] + 1), real(*x, **k))[1])(AG.simple_layer_small_train))
    monkeypatch.setattr(AG, "bn_relu_residual", lambda *x, **k: (seen.__setitem__("tail", seen["tail"] + 1), real_tail(*x, **k))[1])
    return seen


def _layer(meta, a, sd, dev):
    layer = PNASimpleLayer(meta["F"], meta["out_dim"], meta["aggregators"], meta["scalers"], {"log": a["avg_log"]}, 0.0, True, meta["residual"])
    layer.load_state_dict(sd)
    return layer.to(dev).train()


@pytest.mark.parametrize("name", golden_names("dgl_simple_train"))
def test_golden_training_step_through_the_one_call_route(cuda_device, name, monkeypatch):
    """The reference's own training step (oracle/make_golden_simple_train.py) with the bars of
    tests/test_gpu_backward.py::test_simple_layer_training_step_golden, served by the new call and not by the streaming BatchNorm tail."""
    monkeypatch.setattr(PF, "SMALL_TRAIN_ROWS", 4096)
    seen = _spies(monkeypatch)
    meta, a, sd, ref = C.case(name)
    layer = _layer(meta, a, sd, cuda_device)
    g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
    h = a["h"].to(cuda_device).requires_grad_(True)
    assert layer._small_train_path(g, h)
    out = layer(g, h)
    assert seen == {"small": 1, "tail": 0}
    (out * a["R"].to(cuda_device)).sum().backward()
    torch.testing.assert_close(out.detach().cpu(), a["out"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(layer.batchnorm_h.running_mean.cpu(), a["running_mean_after"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(layer.batchnorm_h.running_var.cpu(), a["running_var_after"], rtol=1e-5, atol=1e-6)
    assert int(layer.batchnorm_h.num_batches_tracked) == int(sd["batchnorm_h.num_batches_tracked"]) + 1
    C.check_gradients(meta, a, ref, h.grad, {k: p.grad for k, p in layer.named_parameters()})
    # eval afterwards: the inference path, unchanged by what the training call left on the graph and the layer
    layer.eval()
    fresh = _layer(meta, a, layer.state_dict(), cuda_device).eval()
    with torch.no_grad():
        got, want = layer(g, h.detach()), fresh(Graph(a["src"], a["dst"], meta["N"]).to(cuda_device), h.detach())
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", golden_names("dgl_simple_train"))
def test_knob_at_zero_keeps_the_existing_route(cuda_device, name, monkeypatch):
    monkeypatch.setattr(PF, "SMALL_TRAIN_ROWS", 0)
    seen = _spies(monkeypatch)
    meta, a, sd, _ = C.case(name)
    layer = _layer(meta, a, sd, cuda_device)
    g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
    h = a["h"].to(cuda_device).requires_grad_(True)
    assert not layer._small_train_path(g, h)
    out = layer(g, h)
    assert seen == {"small": 0, "tail": 1}
    torch.testing.assert_close(out.detach().cpu(), a["out"], rtol=1e-5, atol=1e-5)


def test_two_stacked_layers_against_a_float64_stack(cuda_device, monkeypatch):
    """Two residual layers of width 75 on the simple_train_f75 graph: the second layer's input is the first one's output, so grad_out of
    the first is a real tensor and grad_h flows through both residuals.  Reference: the same stack in float64 from the oracle's
    reduce_bucketed / mlp_forward / batchnorm_train under torch autograd; the fp32 evaluation of that stack measures conditioning."""
    monkeypatch.setattr(PF, "SMALL_TRAIN_ROWS", 4096)
    seen = _spies(monkeypatch)
    meta, a, sd1, _ = C.case("simple_train_f75")
    gen = torch.Generator().manual_seed(7)
    sd2 = {k: (v + 0.05 * torch.randn(v.shape, generator=gen) if v.is_floating_point() and "running" not in k else v.clone()) for k, v in sd1.items()}
    V, scalers = meta["N"], meta["scalers"].split()
    src, dst = a["src"].long(), a["dst"].long()

    def stack(dtype):
        sds = [{k: (v.to(dtype).clone().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in sd.items()} for sd in (sd1, sd2)]
        h0 = a["h"].to(dtype).clone().requires_grad_(True)
        x, pres = h0, []
        for sd in sds:
            agg = O.reduce_bucketed(x[src], src, dst, V, C.AGGS, scalers, a["avg_log"].to(dtype))
            y, _, _ = O.batchnorm_train(sd, "batchnorm_h", O.mlp_forward(sd, "posttrans", agg))
            pres.append(y.detach())
            x = x + torch.relu(y)
        (x * a["R"].to(dtype)).sum().backward()
        return x.detach(), h0.grad, sds, pres
    out64, gh64, sds64, pres = stack(torch.float64)
    out32, gh32, sds32, _ = stack(torch.float32)
    layers = [_layer(meta, a, sd, cuda_device) for sd in (sd1, sd2)]
    g = Graph(src, dst, V).to(cuda_device)
    h = a["h"].to(cuda_device).requires_grad_(True)
    out = layers[1](g, layers[0](g, h))
    assert seen == {"small": 2, "tail": 0}
    (out * a["R"].to(cuda_device)).sum().backward()
    torch.testing.assert_close(out.detach().cpu(), out64.float(), rtol=1e-5, atol=1e-5)
    # the ReLU-flip exclusion over BOTH layers' pre-activations; a flip in layer 2 reaches h through two hops
    risk = [(p.abs() < 1e-5 * max(1.0, p.abs().max().item())) for p in pres]
    n_risk = int(sum(r.sum() for r in risk))
    assert n_risk <= max(2, 2e-4 * sum(r.numel() for r in risk)), n_risk

    def hop(rows):
        nb = torch.zeros(V, dtype=torch.bool)
        nb[src[rows[dst]]] = True
        return rows | nb
    rows_h = hop(risk[0].any(1)) | hop(hop(risk[1].any(1)))
    C.close(h.grad, gh32, gh64, "grad_h (two layers)", rows_h, n_risk)
    for i, layer in enumerate(layers):
        # (a flip in layer 2 moves layer 1's gradients in the columns that feed the flipped node: every column -- layer 1's parameters are
        # excluded as a whole then, which the cap above keeps rare)
        cols = risk[i].any(0) | (risk[1].any() if i == 0 else torch.tensor(False))
        for k, p in layer.named_parameters():
            g64, g32 = sds64[i][k].grad, sds32[i][k].grad
            if k == C.B_KEY:
                assert p.grad.abs().max().item() <= 1e-4 * sds64[i][C.W_KEY].grad.abs().max().item(), (i, k)
                continue
            C.close(p.grad, g32, g64, f"layer {i} {k}", cols if bool(cols.any()) else None, n_risk)
    assert [int(l.batchnorm_h.num_batches_tracked) for l in layers] == [int(sd1["batchnorm_h.num_batches_tracked"]) + 1] * 2


def test_num_batches_tracked_advances_by_one_per_call(cuda_device, monkeypatch):
    monkeypatch.setattr(PF, "SMALL_TRAIN_ROWS", 4096)
    meta, a, sd, _ = C.case("simple_train_f20")
    layer = _layer(meta, a, sd, cuda_device)
    g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
    h = a["h"].to(cuda_device)
    start = int(layer.batchnorm_h.num_batches_tracked)
    for i in range(3):
        layer(g, h).sum().backward()
        assert int(layer.batchnorm_h.num_batches_tracked) == start + i + 1
