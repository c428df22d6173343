"""nets.GRU and layers.GRU through the GRU cell route (autograd.GruCellFn) behind the knob functional.GRU_ROWS: which calls take the
route, outputs and gradients against a float64 CPU nn.GRU carrying the same state_dict within the derived bars of tests/gru_cases.py,
the multitask GNN's SHARED GRU applied three times in a chain (three saved states alive), PNANet(gru=True) with the knob on against the
knob off, and eval under no_grad (nothing saved, the same bits)."""
import pytest
import torch
import torch.nn as nn

import gru_cases as C
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd import layers, nets
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu


def _spy(monkeypatch):
    seen = {"cell": 0, "saved": 0}
    real_c, real_s = AG.gru_cell, AG._gru_saved
    monkeypatch.setattr(AG, "gru_cell", lambda *x, **k: (seen.__setitem__("cell", seen["cell"] + 1), real_c(*x, **k))[1])
    monkeypatch.setattr(AG, "_gru_saved", lambda *x, **k: (seen.__setitem__("saved", seen["saved"] + 1), real_s(*x, **k))[1])
    return seen


def _module(cls, width, dev, seed=0):
    IN, H, I, Hc = C.WIDTHS[width]
    torch.manual_seed(seed)
    return cls(IN, H, dev), (IN, H, I, Hc)


def _case_of(mod, x, h, go):
    sd = {k: v.detach().cpu() for k, v in mod.gru.state_dict().items()}
    return {"x": x.cpu(), "h": h.cpu(), "go": go.cpu(), **{k: sd[C.NN_NAMES[k]] for k in C.PARAMS}}


def test_which_calls_take_the_route(cuda_device, monkeypatch):
    dev = cuda_device
    seen = _spy(monkeypatch)
    g, _ = _module(nets.GRU, "mt_later", dev)
    d, _ = _module(layers.GRU, "mt_later", dev)
    x, y = torch.randn(40, 16, device=dev), torch.randn(40, 16, device=dev)
    xb, yb = torch.randn(4, 10, 2, device=dev), torch.randn(4, 10, 16, device=dev)
    monkeypatch.setattr(PF, "GRU_ROWS", 0)
    off, off_b = g(x, y), d(xb, yb)
    assert seen["cell"] == 0 and off.shape == (40, 16) and off_b.shape == (4, 10, 16)
    monkeypatch.setattr(PF, "GRU_ROWS", 4096)
    on, on_b = g(x, y), d(xb, yb)
    assert seen["cell"] == 2 and on.shape == (40, 16) and on_b.shape == (4, 10, 16)
    torch.testing.assert_close(off, g.gru(x.unsqueeze(0), y.unsqueeze(0))[1].squeeze(), rtol=0, atol=0)    # off: the line it runs today
    # the calls that keep the line they run today, and its result
    seen["cell"] = 0
    assert torch.equal(g(x[:1], y[:1]), g.gru(x[:1].unsqueeze(0), y[:1].unsqueeze(0))[1].squeeze()) and g(x[:1], y[:1]).shape == (16,)   # V == 1
    g64 = nets.GRU(16, 16, dev).double()
    assert g64(x.double(), y.double()).dtype == torch.float64                                              # fp64
    gb = nets.GRU(16, 16, dev).to(torch.bfloat16)
    assert gb(x.bfloat16(), y.bfloat16()).dtype == torch.bfloat16                                          # a bf16 module
    monkeypatch.setattr(PF, "GRU_ROWS", 39)
    assert torch.equal(g(x, y), off)                                                                       # more rows than the knob covers
    assert torch.equal(d(xb, yb), off_b)
    assert seen["cell"] == 0


@pytest.mark.parametrize("cls", [nets.GRU, layers.GRU])
@pytest.mark.parametrize("width", ["mt_first", "h75", "pad_h", "rect"])
def test_module_against_a_float64_cpu_gru_with_the_same_state_dict(cuda_device, monkeypatch, cls, width):
    dev = cuda_device
    monkeypatch.setattr(PF, "GRU_ROWS", 4096)
    seen = _spy(monkeypatch)
    mod, (IN, H, I, Hc) = _module(cls, width, dev)
    B, N = 3, 23
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B * N, I, generator=gen).to(dev).requires_grad_(True)
    h = torch.randn(B * N, Hc, generator=gen).to(dev).requires_grad_(True)
    go = torch.randn(B * N, H, generator=gen).to(dev)
    dense = cls is layers.GRU
    out = mod(x.view(B, N, I), h.view(B, N, Hc)) if dense else mod(x, h)
    assert seen == {"cell": 1, "saved": 1} and out.shape == ((B, N, H) if dense else (B * N, H))
    params = [getattr(mod.gru, C.NN_NAMES[k]) for k in C.PARAMS]
    grads = torch.autograd.grad(out, [x, h] + params, go.view_as(out))
    # the float64 CPU module with the same state_dict
    ref = nn.GRU(IN, H).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in mod.gru.state_dict().items()}, strict=True)
    x64, h64 = x.detach().cpu().double().requires_grad_(True), h.detach().cpu().double().requires_grad_(True)
    out64 = ref(C._pad(x64, IN).unsqueeze(0), C._pad(h64, H).unsqueeze(0))[1][0]
    g64 = torch.autograd.grad(out64, [x64, h64] + [getattr(ref, C.NN_NAMES[k]) for k in C.PARAMS], go.cpu().double())
    c = _case_of(mod, x.detach(), h.detach(), go)
    bars = C.gru_bars(*C.case_params(c), c["go"])
    worst = {"out": C.worst_ratio(out.detach().reshape(B * N, H).cpu(), out64.detach(), bars["out"])}
    for k, got, want in zip(("x", "h") + C.PARAMS, grads, g64):
        worst[k] = C.worst_ratio(got.cpu(), want, bars[k])
    assert all(v <= 1.0 for v in worst.values()), worst


def test_a_shared_gru_applied_three_times_in_a_chain(cuda_device, monkeypatch):
    """models/pytorch/gnn_framework.py:93-95: one GRU after every convolution, first on the 2 input features, then on its own output.
    Three saved states are alive when the backward starts; the parameter gradients accumulate over the three uses.

    The bar against the float64 chain has two parts.  (1) Each use is one call: its output and gradients are within that use's derived
    bars of the float64 formulas evaluated at the inputs and the cotangent the use really got (its fp32 input rows; the cotangent caught
    by a hook) -- `own`.  (2) `own` differs from the float64 CHAIN because a use's inputs carry the earlier uses' rounding; that
    difference is computed in float64, not bounded: |gpu - chain| <= bars + |own - chain|.  The parameter gradients are the fp32 sum of
    three uses: the uses' bars added, and two additions' roundings on the partial sums."""
    dev = cuda_device
    monkeypatch.setattr(PF, "GRU_ROWS", 4096)
    seen = _spy(monkeypatch)
    torch.manual_seed(3)
    mod = layers.GRU(16, 16, dev)
    B, N = 4, 19
    R = B * N
    gen = torch.Generator().manual_seed(9)
    x0 = torch.randn(B, N, 2, generator=gen)
    ys = [torch.randn(B, N, 16, generator=gen) for _ in range(3)]                # what the three convolutions would hand over
    go = torch.randn(B, N, 16, generator=gen)
    xd = x0.to(dev).requires_grad_(True)
    yd = [y.to(dev).requires_grad_(True) for y in ys]
    xs, cots, x = [xd], {}, xd
    for i, y in enumerate(yd):
        x = mod(x, y)
        x.register_hook(lambda gr, i=i: cots.__setitem__(i, gr.detach().cpu()))
        xs.append(x)
    assert seen == {"cell": 3, "saved": 3}
    params = [getattr(mod.gru, C.NN_NAMES[k]) for k in C.PARAMS]
    grads = torch.autograd.grad(xs[-1], [xd] + yd + params, go.to(dev))
    assert sorted(cots) == [0, 1, 2]
    # the float64 chain
    ref = nn.GRU(16, 16).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in mod.gru.state_dict().items()}, strict=True)
    x64 = x0.double().requires_grad_(True)
    y64 = [y.double().requires_grad_(True) for y in ys]
    o64 = x64
    for y in y64:
        o64 = ref(C._pad(o64.reshape(R, -1), 16).unsqueeze(0), y.reshape(1, R, 16))[1].reshape(B, N, 16)
    g64 = torch.autograd.grad(o64, [x64] + y64 + [getattr(ref, C.NN_NAMES[k]) for k in C.PARAMS], go.double())
    # every use against its own float64 reference, then against the chain
    sd = [mod.gru.state_dict()[C.NN_NAMES[k]].detach().cpu() for k in C.PARAMS]
    own_p = {k: 0.0 for k in C.PARAMS}
    bar_p = {k: 0.0 for k in C.PARAMS}
    mass_p = {k: 0.0 for k in C.PARAMS}
    for i in range(3):
        xi, yi, ci = xs[i].detach().cpu().reshape(R, -1), ys[i].reshape(R, 16), cots[i].reshape(R, 16)
        f, g = C.gru_grad_ref64(xi, yi, *sd, ci)
        b = C.gru_bars(xi, yi, *sd, ci)
        assert C.worst_ratio(xs[i + 1].detach().cpu().reshape(R, 16), f["out"], b["out"]) <= 1.0, i
        assert C.worst_ratio(grads[1 + i].cpu().reshape(R, 16), g["h"], b["h"]) <= 1.0, i
        assert C.worst_ratio(grads[1 + i].cpu().reshape(R, 16), g64[1 + i].reshape(R, 16), b["h"] + (g["h"] - g64[1 + i].reshape(R, 16)).abs()) <= 1.0, i
        if i == 0:
            assert C.worst_ratio(grads[0].cpu().reshape(R, 2), g["x"], b["x"]) <= 1.0
            assert C.worst_ratio(grads[0].cpu().reshape(R, 2), g64[0].reshape(R, 2), b["x"] + (g["x"] - g64[0].reshape(R, 2)).abs()) <= 1.0
        for k in C.PARAMS:
            own_p[k], bar_p[k], mass_p[k] = own_p[k] + g[k], bar_p[k] + b[k], mass_p[k] + g[k].abs() + b[k]
    assert C.worst_ratio(xs[3].detach().cpu().reshape(R, 16), o64.detach().reshape(R, 16),
                         C.gru_bars(xs[2].detach().cpu().reshape(R, 16), ys[2].reshape(R, 16), *sd)["out"]
                         + (C.gru_ref64(xs[2].detach().cpu().reshape(R, 16), ys[2].reshape(R, 16), *sd)["out"] - o64.detach().reshape(R, 16)).abs()) <= 1.0
    for j, k in enumerate(C.PARAMS):
        bar = bar_p[k] + 2 * C.U * mass_p[k]
        assert C.worst_ratio(grads[4 + j].cpu(), own_p[k], bar) <= 1.0, k
        assert C.worst_ratio(grads[4 + j].cpu(), g64[4 + j], bar + (own_p[k] - g64[4 + j]).abs()) <= 1.0, k
        assert float((own_p[k] - g64[4 + j]).abs().max()) <= 1e-4 * float(g64[4 + j].abs().max())      # (the chain is well conditioned: part (2) is small)


def _zinc_net(dev, seed=0):
    from pna_amd.synth import molecule_batch
    src, dst, sizes = molecule_batch(6, mean_nodes=23, sd_nodes=5, lo=8, hi=40, seed=4)
    V = sum(sizes)
    g = Graph(src, dst, V, sizes).to(dev)
    avg = {"log": torch.log(g.in_degrees().double() + 1).mean().float().cpu()}
    torch.manual_seed(seed)
    net = nets.PNANet(dict(num_atom_type=28, num_bond_type=4, hidden_dim=32, out_dim=32, in_feat_dropout=0.0, dropout=0.0, L=2, readout="sum",
                           graph_norm=True, batch_norm=True, residual=True, aggregators="mean max min std",
                           scalers="identity amplification attenuation", avg_d=avg, towers=4, divide_input_first=True, divide_input_last=True,
                           edge_feat=False, edge_dim=0, pretrans_layers=1, posttrans_layers=1, gru=True, device=dev)).to(dev)
    gen = torch.Generator().manual_seed(1)
    atoms = torch.randint(0, 28, (V,), generator=gen).to(dev)
    snorm = torch.cat([torch.full((n, 1), n ** -0.5) for n in sizes]).to(dev)
    y = torch.randn(len(sizes), 1, generator=gen).to(dev)
    return net, g, atoms, snorm, y


def test_pnanet_with_gru_knob_on_against_knob_off(cuda_device, monkeypatch):
    net, g, atoms, snorm, y = _zinc_net(cuda_device)
    net.eval()
    seen = _spy(monkeypatch)
    monkeypatch.setattr(PF, "GRU_ROWS", 0)
    with torch.no_grad():
        off = net(g, atoms, None, snorm)
    assert seen["cell"] == 0
    monkeypatch.setattr(PF, "GRU_ROWS", 4096)
    with torch.no_grad():
        on = net(g, atoms, None, snorm)
    assert seen["cell"] == 1                                                      # L = 2: one GRU between the two layers
    assert float((on - off).abs().max()) <= 1e-5 * float(off.abs().max())        # tests/tower_train_cases.py's bar for outputs
    # one training step on the route
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    opt.zero_grad()
    net.loss(net(g, atoms, None, snorm), y).backward()
    assert seen["cell"] == 2
    for name in C.NN_NAMES.values():
        gr = getattr(net.gru.gru, name).grad
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, name
    opt.step()


def test_eval_under_no_grad_saves_nothing_and_returns_the_same_bits(cuda_device, monkeypatch):
    dev = cuda_device
    monkeypatch.setattr(PF, "GRU_ROWS", 4096)
    seen = _spy(monkeypatch)
    mod, _ = _module(nets.GRU, "h75", dev)
    mod.eval()
    x, y = torch.randn(50, 75, device=dev), torch.randn(50, 75, device=dev)
    with_grad = mod(x, y)
    assert seen == {"cell": 1, "saved": 1} and with_grad.requires_grad
    with torch.no_grad():
        without = mod(x, y)
    assert seen == {"cell": 2, "saved": 1} and not without.requires_grad
    assert torch.equal(with_grad.detach(), without)
    for p in mod.parameters():
        p.requires_grad_(False)
    frozen = mod(x, y)                                                            # grad mode on, nothing requires a gradient
    assert seen == {"cell": 3, "saved": 1} and torch.equal(frozen, without)


def test_expanded_cotangent_and_expanded_rows(cuda_device, monkeypatch):
    """The cotangent of `out.sum(0)` is an expand with strides (0, 1), and a broadcast input has row pitch 0: the C calls refuse a pitch
    below the width, so the backward copies such a cotangent and the predicate declines such rows (the helper copies them)."""
    dev = cuda_device
    monkeypatch.setattr(PF, "GRU_ROWS", 4096)
    seen = _spy(monkeypatch)
    mod, _ = _module(nets.GRU, "mt_later", dev)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(40, 16, generator=gen).to(dev).requires_grad_(True)
    h = torch.randn(40, 16, generator=gen).to(dev).requires_grad_(True)
    params = [getattr(mod.gru, C.NN_NAMES[k]) for k in C.PARAMS]
    out = mod(x, h)
    assert seen["cell"] == 1
    grads = torch.autograd.grad(out.sum(0).sum(), [x, h] + params)                # grad_out = ones(16).expand(40, 16)
    c = _case_of(mod, x.detach(), h.detach(), torch.ones(40, 16))
    _, g64 = C.gru_grad_ref64(*C.case_params(c), c["go"])
    bars = C.gru_bars(*C.case_params(c), c["go"])
    for k, got in zip(("x", "h") + C.PARAMS, grads):
        assert C.worst_ratio(got.cpu(), g64[k], bars[k]) <= 1.0, k
    # expanded input rows: the module keeps nn.GRU; the helper itself serves them through a copy
    row = torch.randn(1, 16, generator=gen).to(dev)
    wide = row.expand(40, 16)
    assert wide.stride() == (0, 1)
    via_module = mod(wide, h.detach())
    assert seen["cell"] == 1
    direct = AG.gru_cell(wide, h.detach(), mod.gru)
    ref = C.gru_ref64(wide.cpu(), h.detach().cpu(), *[c[k] for k in C.PARAMS])
    b = C.gru_bars(wide.cpu().contiguous(), h.detach().cpu(), *[c[k] for k in C.PARAMS])
    assert C.worst_ratio(direct.detach().cpu(), ref["out"], b["out"]) <= 1.0 and via_module.shape == (40, 16)


def test_the_workspace_is_one_buffer_per_device_whatever_the_row_counts(cuda_device, monkeypatch):
    """Molecule batches have another row count every step: the cache must not keep a buffer per size."""
    dev = cuda_device
    monkeypatch.setattr(PF, "GRU_ROWS", 4096)
    monkeypatch.setattr(AG, "_gru_ws", {})
    mod, _ = _module(nets.GRU, "mt_later", dev)
    for V in (40, 300, 41, 129, 7):
        x = torch.randn(V, 16, device=dev, requires_grad=True)
        mod(x, torch.randn(V, 16, device=dev)).sum().backward()
    assert list(AG._gru_ws) == [dev]
    assert AG._gru_ws[dev].numel() * 4 >= PF.gru_cell_workspace_bytes(300, 16, 16, 16) + 16
    assert AG._gru_ws[dev].numel() * 4 < 2 * PF.gru_cell_workspace_bytes(300, 16, 16, 16)
