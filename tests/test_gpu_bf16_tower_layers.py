"""bf16 inference of PNALayer / PNATower and of the nets against float64 models of the arithmetic contract (bf16_tower_ref.py).

Layer level (reference-generated tower fixtures, every value cast to bf16 first): four roundings stack, and the propagated
worst-case bound E is far wider than what a faithful implementation does, so the yardstick is the float64 emulation `emu` that
rounds at R1-R4 only.  With rho(x) = max_j |x_j - ref64_j| / E_j the bar is

    rho(gpu) <= 2 rho(emu)       per fixture, no element left out

(GPU and emulation round at the same points and differ in fp32 against float64 accumulation only: two draws of one maximum).
Each test shows on the host that the bar has teeth: an all-zero output and an output without the destination term violate it.

Net level: `emu` is the whole net with the layers and the readout emulated at their rounding points and the embeddings, GRU and
MLPReadout run by the same torch modules on the host in bf16; `ref` is the oracle's net in float64 (float32 for GRU fixtures,
whose GRU the oracle builds in torch's default dtype).  Bar: max |gpu - emu| <= 2 max |emu - ref|."""
import copy

import pytest
import torch

import bf16_tower_ref as B
from conftest import load_golden
from oracle import torch_oracle as O
from pna_amd.dgl.pna_layer import PNALayer, PNATower
from pna_amd.graph import Graph

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TOWER_FIXTURES = ["tower_f75", "tower_zinc_first", "tower_zinc_last", "tower_edgefeat", "tower_edgetype", "tower_edgetype_div",
                  "tower_hiv_t8_div", "tower_groups_t1_f75", "tower_groups_t4_div", "tower_groups_t5_f75"]
NET_FIXTURES = ["net_zinc_max", "net_zinc_mean_gru", "net_zinc_sum_edgefeat", "net_hiv_readme", "net_superpixels_cifar",
                "net_superpixels_edgefeat_gru"]


def _bf64(t):
    return t.to(BF).double()


def _sd64(sd):
    return {k: (_bf64(v) if v.is_floating_point() else v) for k, v in sd.items()}


def _cfg(meta):
    return dict(towers=meta["towers"], divide_input=meta["divide_input"], aggregators=meta["aggregators"].split(),
                scalers=meta["scalers"].split(), graph_norm=meta["graph_norm"], batch_norm=meta["batch_norm"], residual=meta["residual"],
                edge_features=meta["edge_dim"] > 0)


def _tower_layer(meta, a, sd, device):
    layer = PNALayer(meta["in_dim"], meta["out_dim"], meta["aggregators"], meta["scalers"], {"log": a["avg_log"].to(BF).float()}, 0.0,
                     meta["graph_norm"], meta["batch_norm"], towers=meta["towers"], pretrans_layers=meta["pretrans_layers"],
                     posttrans_layers=meta["posttrans_layers"], divide_input=meta["divide_input"], residual=meta["residual"],
                     edge_features=meta["edge_dim"] > 0, edge_dim=meta["edge_dim"])
    layer.load_state_dict(sd, strict=True)
    return layer.to(device).eval().to(BF)


def layer_figures(name, device):
    """One tower fixture in bf16 on the GPU against ref64 / emu / E on the host -> the figures the test asserts on."""
    meta, a, sd = load_golden(name)
    layer = _tower_layer(meta, a, sd, device)
    has_e = meta["edge_dim"] > 0
    g = Graph(a["src"], a["dst"], meta["N"]).to(device)
    h, sn = a["h"].to(BF).to(device), a["snorm_n"].to(BF).to(device)
    e = a["e"].to(BF).to(device) if has_e else None
    with torch.no_grad():
        assert layer._bf16_path(g, h, e)
        out = layer(g, h, e, sn)
    assert out.dtype == BF and out.shape == (meta["N"], meta["out_dim"]) and out.is_contiguous()
    cfg, avg = _cfg(meta), float(a["avg_log"].to(BF))
    args = (_sd64(sd), cfg, a["src"], a["dst"], meta["N"], _bf64(a["h"]), _bf64(a["e"]) if has_e else None, _bf64(a["snorm_n"]), avg)
    ref, emu, E = B.layer_models(*args)
    oracle = O.dgl_layer_forward(args[0], a["src"].long(), a["dst"].long(), meta["N"], args[5], args[6], args[7], cfg["aggregators"],
                                 cfg["scalers"], torch.tensor(avg, dtype=torch.float64), cfg["towers"], cfg["divide_input"],
                                 cfg["graph_norm"], cfg["batch_norm"], cfg["residual"], cfg["edge_features"])
    assert float((oracle - ref).abs().max()) < 1e-9            # the model without roundings IS the oracle's layer in float64
    _, no_dst, _ = B.layer_models(*args, drop_dst_term=True)
    return {"fixture": name, "elements": ref.numel(), "rho_emu": B.rho(emu, ref, E), "rho_gpu": B.rho(B.f64(out), ref, E),
            "rho_zero_output": B.rho(torch.zeros_like(ref), ref, E), "rho_no_destination_term": B.rho(no_dst, ref, E),
            "median_E_over_ref": float((E / ref.abs()).median())}


@pytest.mark.parametrize("name", TOWER_FIXTURES)
def test_tower_fixtures_in_bf16(cuda_device, name):
    f = layer_figures(name, cuda_device)
    print(f)
    assert f["elements"] >= 2000
    assert f["rho_zero_output"] > 2 * f["rho_emu"] and f["rho_no_destination_term"] > 2 * f["rho_emu"], f   # the bar's own teeth
    assert f["rho_gpu"] <= 2 * f["rho_emu"], f


def test_single_tower_in_bf16(cuda_device):
    """PNATower called on its own (no mixing network): towers 0 of tower_groups_t1_f75, against the towers' part of the models."""
    meta, a, sd = load_golden("tower_groups_t1_f75")
    layer = _tower_layer(meta, a, sd, cuda_device)
    tower = layer.towers[0]
    assert isinstance(tower, PNATower)
    g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
    h, sn = a["h"].to(BF).to(cuda_device), a["snorm_n"].to(BF).to(cuda_device)
    with torch.no_grad():
        assert tower._bf16_path(g, h)
        out = tower(g, h, None, sn.float())                      # snorm_n may be fp32 as well
    ref, emu, E = B.layer_models(_sd64(sd), _cfg(meta), a["src"], a["dst"], meta["N"], _bf64(a["h"]), None, _bf64(a["snorm_n"]),
                                 float(a["avg_log"].to(BF)), stop_after_towers=True)
    assert out.dtype == BF and out.shape == ref.shape
    assert B.rho(B.f64(out), ref, E) <= 2 * B.rho(emu, ref, E)


def test_deep_posttrans_runs_its_first_linear_on_the_kernel(cuda_device):
    """posttrans_layers = 2: the kernel's part (first Linear with bias, scalers, self block) followed by the module's own bf16 ops
    equals the same torch ops applied to the kernel's result, and stays close to the layer evaluated in fp32."""
    torch.manual_seed(5)
    layer = PNALayer(24, 24, "mean max min std", "identity amplification attenuation", {"log": torch.tensor(1.25)}, 0.0, True, True,
                     towers=3, posttrans_layers=2, divide_input=False, residual=True)
    layer32 = layer.to(cuda_device).eval()
    layer16 = copy.deepcopy(layer32).to(BF)
    V = 500
    gen = torch.Generator().manual_seed(1)
    src, dst = torch.randint(0, V, (3000,), generator=gen), torch.randint(0, V, (3000,), generator=gen)
    g = Graph(src, dst, V, [200, 300]).to(cuda_device)
    h = torch.randn(V, 24, generator=gen).to(BF).to(cuda_device)
    sn = g.snorm_n().to(BF)
    with torch.no_grad():
        assert layer16._bf16_path(g, h)
        out16 = layer16(g, h, None, sn)
        # fp32 layer on the bf16 VALUES of the parameters and inputs
        for p32, p16 in zip(layer32.parameters(), layer16.parameters()):
            p32.copy_(p16.float())
        for b32, b16 in zip(layer32.buffers(), layer16.buffers()):
            if b32.is_floating_point():
                b32.copy_(b16.float())
        out32 = layer32(g, h.float(), None, sn.float())
    assert out16.dtype == BF and out16.shape == out32.shape
    # six roundings of values of order 1 (u = 2^-8 each, amplified by weights of norm ~ 1): a few percent of the output's scale
    scale = float(out32.abs().mean())
    assert float((out16.float() - out32).abs().max()) <= 0.1 * max(scale, 1.0)
    assert float((out16.float() - out32).abs().mean()) <= 0.02 * max(scale, 1.0)


def test_deep_pretrans_in_bf16_raises_as_before(cuda_device):
    meta, a, sd = load_golden("tower_deep_mlps")
    layer = _tower_layer(meta, a, sd, cuda_device)
    g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
    h, sn = a["h"].to(BF).to(cuda_device), a["snorm_n"].to(BF).to(cuda_device)
    with torch.no_grad():
        assert not layer._bf16_path(g, h)
        with pytest.raises((TypeError, RuntimeError)):
            layer(g, h, None, sn)


def test_fp32_forward_unchanged_by_bf16_calls(cuda_device):
    for name in ("tower_groups_t5_f75", "tower_edgetype"):
        meta, a, sd = load_golden(name)
        layer16 = _tower_layer(meta, a, sd, cuda_device)
        layer32 = copy.deepcopy(layer16).float()
        g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
        h, sn = a["h"].to(cuda_device), a["snorm_n"].to(cuda_device)
        e = a["e"].to(cuda_device) if meta["edge_dim"] > 0 else None
        with torch.no_grad():
            before = layer32(g, h, e, sn)
            for _ in range(2):
                layer16(g, h.to(BF), None if e is None else e.to(BF), sn.to(BF))
            after = layer32(g, h, e, sn)
        assert before.dtype == torch.float32 and torch.equal(before, after)


def test_changing_a_pretrans_weight_in_place_changes_the_next_output(cuda_device):
    """The cached weight images are keyed on every tensor they are built from: the LAST tower's pretrans weight included.  After each
    update the warm layer gives bit for bit what a fresh layer with the same state gives: a half-stale cache -- one
    image rebuilt, another not -- changes the output too, and only the comparison with a fresh layer tells the two apart."""
    meta, a, sd = load_golden("tower_zinc_first")
    layer = _tower_layer(meta, a, sd, cuda_device)
    g = Graph(a["src"], a["dst"], meta["N"]).to(cuda_device)
    h, sn = a["h"].to(BF).to(cuda_device), a["snorm_n"].to(BF).to(cuda_device)

    def fresh():
        other = _tower_layer(meta, a, sd, cuda_device)
        other.load_state_dict(layer.state_dict())
        return other(g, h, None, sn)
    with torch.no_grad():
        first = layer(g, h, None, sn)
        assert torch.equal(layer(g, h, None, sn), first)
        assert torch.equal(fresh(), first)                               # control: a fresh layer, same state, same bits
        layer.towers[-1].pretrans.fully_connected[0].linear.weight.mul_(1.5)
        after = layer(g, h, None, sn)
        assert not torch.equal(after, first)
        assert torch.equal(after, fresh())
        layer.mixing_network.linear.weight.mul_(0.5)
        second = layer(g, h, None, sn)
        assert torch.equal(second, fresh())
        layer.towers[1].batchnorm_h.running_var.mul_(4.0)
        third = layer(g, h, None, sn)
        assert not torch.equal(third, second)
        assert torch.equal(third, fresh())


# ---- nets ---------------------------------------------------------------------------------------------------------------------
def _simple_layer_emu(sd, src, dst, N, h, aggs, scalers, avg):
    """PNASimpleLayer at its two rounding points: the aggregate, then the posttrans epilogue."""
    z = B.rbf(B.aggregate64(h[src], src, dst, N, aggs))
    deg = torch.bincount(dst, minlength=N).numpy()
    W, b = sd["posttrans.fully_connected.0.linear.weight"], sd["posttrans.fully_connected.0.linear.bias"]
    Wz = W.reshape(W.shape[0], len(scalers), -1)
    y = b.expand(N, -1).clone()
    for s, name in enumerate(scalers):
        y = y + torch.from_numpy(B.scale64(name, deg, avg))[:, None] * (z @ Wz[:, s].T)
    cs = sd["batchnorm_h.weight"] / torch.sqrt(sd["batchnorm_h.running_var"] + 1e-5)
    y = torch.relu(y * cs + sd["batchnorm_h.bias"] - sd["batchnorm_h.running_mean"] * cs)
    return B.rbf(h + y)


def _build_net(name):
    from pna_amd.nets import PNANet, PNANetHIV, PNANetSuperpixels
    from test_gpu_layers import _superpixels_params
    from test_host_logic import _net_params
    meta, a, sd = load_golden(name)
    a = dict(a)
    a["avg_log"] = a["avg_log"].to(BF).float()
    if meta["kind"] == "net_hiv":
        net = PNANetHIV(dict(hidden_dim=meta["hidden_dim"], out_dim=meta["out_dim"], in_feat_dropout=0.0, dropout=0.3, L=meta["L"],
                             readout=meta["readout"], batch_norm=True, residual=True, aggregators=meta["aggregators"],
                             scalers=meta["scalers"], avg_d={"log": a["avg_log"]}, posttrans_layers=1, device="cpu"))
    elif meta["kind"] == "net_superpixels":
        net = PNANetSuperpixels(_superpixels_params(meta, a))
    else:
        net = PNANet(_net_params(meta, a))
    net.load_state_dict(sd, strict=True)
    return meta, a, sd, net.eval().to(BF)


def net_figures(name, device):
    meta, a, sd, net = _build_net(name)
    kind, N = meta["kind"], meta["N"]
    src, dst = a["src"].long(), a["dst"].long()
    avg = float(a["avg_log"])
    aggs, scalers = meta["aggregators"].split(), meta["scalers"].split()
    sd16 = {k: (v.to(BF) if v.is_floating_point() else v) for k, v in sd.items()}
    sn16 = a["snorm_n"].to(BF) if "snorm_n" in a else None
    # --- GPU
    gnet = copy.deepcopy(net).to(device)
    g = Graph(a["src"], a["dst"], N, meta["sizes"]).to(device)
    with torch.no_grad():
        if kind == "net_hiv":
            out = gnet(g, a["atoms"].to(device))
        elif kind == "net_superpixels":
            out = gnet(g, a["x"].to(BF).to(device), a["e"].to(BF).to(device), sn16.to(device), None)
        else:
            out = gnet(g, a["atoms"].to(device), a["bonds"].to(device), sn16.to(device), None)
    assert out.dtype == BF
    # --- emulation: layers and readout at their rounding points, the rest by the net's own modules on the host in bf16
    with torch.no_grad():
        e = None
        if kind == "net_hiv":
            h = net.embedding_h(a["atoms"])
        elif kind == "net_superpixels":
            h = net.embedding_h(a["x"].to(BF))
            e = net.embedding_e(a["e"].to(BF)) if meta["edge_feat"] else None
        else:
            h = net.embedding_h(a["atoms"])
            e = net.embedding_e(a["bonds"]) if meta["edge_dim"] > 0 else None
        L = meta["L"]
        for i in range(L):
            lsd = {k[len(f"layers.{i}."):]: v.double() for k, v in sd16.items() if k.startswith(f"layers.{i}.") and v.is_floating_point()}
            if kind == "net_hiv":
                h_t = _simple_layer_emu(lsd, src, dst, N, h.double(), aggs, scalers, avg).to(BF)
            else:
                if kind == "net_superpixels":
                    divide = meta["divide_input_last"] if i == L - 1 else meta["divide_input_first"]
                else:
                    divide = i == L - 1
                cfg = dict(towers=meta["towers"], divide_input=divide, aggregators=aggs, scalers=scalers, graph_norm=True, batch_norm=True,
                           residual=True, edge_features=e is not None)
                _, h_t, _ = B.layer_models(lsd, cfg, src, dst, N, h.double(), None if e is None else e.double(), sn16.double(), avg)
                h_t = h_t.to(BF)
                if meta["gru"] and i != L - 1:
                    h_t = net.gru(h, h_t)
            h = h_t
        parts = torch.split(h.double(), meta["sizes"])
        op = {"sum": lambda p: p.sum(0), "mean": lambda p: p.mean(0), "max": lambda p: p.max(0)[0]}[meta["readout"]]
        emu = net.MLP_layer(B.rbf(torch.stack([op(p) for p in parts])).to(BF)).double()
    # --- the oracle's net on the same bf16 values
    rd = torch.float32 if meta.get("gru") else torch.float64
    sdr = {k: (v.to(rd) if v.is_floating_point() else v) for k, v in sd16.items()}
    avg_t = torch.tensor(avg, dtype=rd)
    with torch.no_grad():
        if kind == "net_hiv":
            ref = O.net_hiv_forward(sdr, meta, src, dst, a["atoms"], avg_t)
        elif kind == "net_superpixels":
            ref = O.net_superpixels_forward(sdr, meta, src, dst, a["x"].to(BF).to(rd), a["e"].to(BF).to(rd), sn16.to(rd), avg_t)
        else:
            ref = O.net_molecules_forward(sdr, meta, src, dst, a["atoms"], a["bonds"], sn16.to(rd), avg_t)
    ref = ref.double()
    return {"fixture": name, "gpu_minus_emu": float((out.cpu().double() - emu).abs().max()), "emu_minus_ref": float((emu - ref).abs().max()),
            "ref_scale": float(ref.abs().max())}


@pytest.mark.parametrize("name", NET_FIXTURES)
def test_nets_in_bf16(cuda_device, name):
    f = net_figures(name, cuda_device)
    print(f)
    assert f["gpu_minus_emu"] <= 2 * f["emu_minus_ref"], f
