"""The molecule nets through the net-ends route (autograd.EmbedSumFn / ReadoutFn) behind the knob functional.NET_ENDS_ROWS: the
reference's golden outputs with both routes seen taken, neither with the knob at 0 or in bf16, the nine table gradients of a PNANetHIV
loss against the same net with the knob off, and a training loop."""
import pytest
import torch

import net_ends_cases as C
from conftest import load_golden
from pna_amd import autograd as AG
from pna_amd import functional as PF
from pna_amd.graph import Graph
from pna_amd.nets import PNANet, PNANetHIV

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-5, atol=1e-5)          # tests/test_gpu_layers.py's, for the same fixtures


def _spies(monkeypatch):
    seen = {"embed": 0, "readout": 0}
    real_e, real_r = AG.embed_sum, AG.readout
    monkeypatch.setattr(AG, "embed_sum", lambda *x, **k: (seen.__setitem__("embed", seen["embed"] + 1), real_e(*x, **k))[1])
    monkeypatch.setattr(AG, "readout", lambda *x, **k: (seen.__setitem__("readout", seen["readout"] + 1), real_r(*x, **k))[1])
    return seen


def _golden_net(name, dev):
    from test_host_logic import _net_params
    meta, a, sd = load_golden(name)
    if meta["kind"] == "net_hiv":
        net = PNANetHIV(dict(hidden_dim=meta["hidden_dim"], out_dim=meta["out_dim"], in_feat_dropout=0.0, dropout=0.3, L=meta["L"],
                             readout=meta["readout"], batch_norm=True, residual=True, aggregators=meta["aggregators"],
                             scalers=meta["scalers"], avg_d={"log": a["avg_log"]}, posttrans_layers=1, device=dev))
    else:
        net = PNANet(_net_params(meta, a))
    net.load_state_dict(sd, strict=True)
    g = Graph(a["src"], a["dst"], meta["N"], meta["sizes"]).to(dev)

    def run(n, dtype=torch.float32):
        if meta["kind"] == "net_hiv":
            return n(g, a["atoms"].to(dev))
        return n(g, a["atoms"].to(dev), a["bonds"].to(dev), a["snorm_n"].to(dtype).to(dev), None)
    return meta, a, net.to(dev).eval(), run


@pytest.mark.parametrize("name", ["net_hiv_readme", "net_zinc_sum_edgefeat"])
def test_golden_nets_through_the_new_route(cuda_device, name, monkeypatch):
    meta, a, net, run = _golden_net(name, cuda_device)
    assert meta["N"] <= 4096
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 4096)
    seen = _spies(monkeypatch)
    with torch.no_grad():
        out = run(net).cpu()
    assert seen["embed"] >= 1 and seen["readout"] == 1, seen
    torch.testing.assert_close(out, a["out"], **TOL)
    # ... and with the knob at 0 neither route is taken, the output the same within the tolerance
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 0)
    seen.update(embed=0, readout=0)
    with torch.no_grad():
        off = run(net).cpu()
    assert seen == {"embed": 0, "readout": 0}
    torch.testing.assert_close(off, a["out"], **TOL)
    torch.testing.assert_close(out, off, **TOL)


@pytest.mark.parametrize("name", ["net_hiv_readme", "net_zinc_sum_edgefeat"])
def test_a_bf16_net_takes_neither_route(cuda_device, name, monkeypatch):
    meta, a, net, run = _golden_net(name, cuda_device)
    net = net.to(torch.bfloat16)
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 4096)
    seen = _spies(monkeypatch)
    with torch.no_grad():
        out = run(net, torch.bfloat16)
    assert out.dtype == torch.bfloat16 and seen == {"embed": 0, "readout": 0}


def _hiv_net(dev, L=3, hidden=32, seed=0):
    from pna_amd.synth import molecule_batch
    src, dst, sizes = molecule_batch(12, mean_nodes=25.5, sd_nodes=12, lo=6, hi=60, seed=2, lognormal=True)
    V = sum(sizes)
    g = Graph(src, dst, V, sizes).to(dev)
    avg = {"log": torch.log(g.in_degrees().double() + 1).mean().float().cpu()}
    torch.manual_seed(seed)
    net = PNANetHIV(dict(hidden_dim=hidden, out_dim=hidden, in_feat_dropout=0.0, dropout=0.0, L=L, readout="mean", batch_norm=True,
                         residual=True, aggregators="mean max min std", scalers="identity amplification attenuation",
                         avg_d=avg, posttrans_layers=1, device=dev)).to(dev)
    gen = torch.Generator().manual_seed(0)
    x = torch.stack([torch.randint(0, d, (V,), generator=gen) for d in C.ATOM_DIMS], dim=1)
    y = torch.randint(0, 2, (len(sizes),), generator=gen)
    return net, g, x, y, sizes


def test_table_gradients_of_a_net_loss_against_the_knob_off(cuda_device, monkeypatch):
    """torch.autograd.grad of a 3-layer PNANetHIV loss with respect to the nine tables, knob on against knob off.  The bar is the
    serial-sum bound applied to the grad_out that REACHES the encoder, caught by a hook on the encoder's output in each run: the new
    route's gradient against the float64 index-sum of its own grad_out within n u sum |g|; the old route's (a one-hot GEMM: an fp32 sum
    of the same n terms in another order) within the same bound of ITS grad_out; the two grad_outs may differ by what the readout's
    two backwards round differently, which the difference of the two float64 sums accounts for."""
    net, g, x, y, sizes = _hiv_net(cuda_device)
    xd = x.to(cuda_device)
    tables = [e.weight for e in net.embedding_h.atom_embedding_list]
    rows = [w.shape[0] for w in tables]
    caught = {}
    net.embedding_h.register_forward_hook(lambda mod, inp, out: out.register_hook(lambda gr: caught.__setitem__("go", gr.detach().cpu())) and None)
    res = {}
    for knob in (4096, 0):
        monkeypatch.setattr(PF, "NET_ENDS_ROWS", knob)
        seen = _spies(monkeypatch)
        net.train()
        grads = torch.autograd.grad(net.loss(net(g, xd), y), tables)
        assert seen == ({"embed": 1, "readout": 1} if knob else {"embed": 0, "readout": 0})
        monkeypatch.undo()
        res[knob] = ([gr.cpu().double() for gr in grads], C.embed_grad_ref64(x, rows, caught["go"]))
    (on, ref_on), (off, ref_off) = res[4096], res[0]
    for j in range(len(rows)):
        r_on, n, m_on = ref_on[j]
        r_off, _, m_off = ref_off[j]
        b_on, b_off = C.serial_sum_bound(n, m_on), C.serial_sum_bound(n, m_off)
        assert bool(((on[j] - r_on).abs() <= b_on).all()), (j, float(((on[j] - r_on).abs() - b_on).max()))
        assert bool(((on[j] - off[j]).abs() <= b_on + b_off + (r_on - r_off).abs()).all()), j
        assert bool((on[j][n == 0] == 0).all())
        assert float(r_on.abs().max()) > 0


def test_hiv_net_trains_with_the_knob_on(cuda_device, monkeypatch):
    """The loop of tests/test_gpu_layers.py::test_hiv_net_runs_and_trains, both ends on the new route."""
    monkeypatch.setattr(PF, "NET_ENDS_ROWS", 4096)
    seen = _spies(monkeypatch)
    net, g, x, y, sizes = _hiv_net(cuda_device)
    x = x.to(cuda_device)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = net.loss(net(g, x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert seen == {"embed": 10, "readout": 10}
    assert losses[-1] < losses[0]
    net.eval()
    with torch.no_grad():
        assert net(g, x).shape == (len(sizes), 1)
