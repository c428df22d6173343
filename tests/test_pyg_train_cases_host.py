"""pyg_train_cases.py's float64 restatement of PNAConv's training step against what the reference's own module computed (the existing
forward goldens and the training-step golden tools/make_golden_pyg_train.py records), the conditions of every case on the float64 oracle
alone, and the identities of the pack / unpack fold (include/pna_amd.h, pna_pyg_conv_train_args) in float64 against autograd."""
import pytest
import torch

import pyg_train_cases as C
from conftest import load_golden


def _meta_of(meta, a):
    T = meta["towers"]
    Fi = meta["in_c"] // T if meta["divide_input"] else meta["in_c"]
    _, avg = C.avg_deg_of(a["edge_index"][1], meta["N"])
    return dict(N=meta["N"], in_c=meta["in_c"], out_c=meta["out_c"], towers=T, divide_input=meta["divide_input"], F_in=Fi, F_out=meta["out_c"] // T,
                edge_dim=meta["edge_dim"], aggregators=meta["aggregators"], scalers=meta["scalers"], avg_deg=avg)


@pytest.mark.parametrize("name", ["pyg_conv_towers", "pyg_conv_edge_divide"])
def test_oracle_forward_reproduces_the_forward_goldens(name):
    """The reference's fp32 output of its own module: the restatement in fp32 agrees to fp32 rounding of a sum in another order, and in
    float64 to the same bar (these graphs repeat edges, so a few std entries sit at sqrt(1e-5) and carry the golden's own fp32 noise)."""
    meta, a, sd = load_golden(name)
    m = _meta_of(meta, a)
    for dt in (torch.float32, torch.float64):
        out = C.forward({k: v.to(dt) for k, v in sd.items()}, m, a["x"].to(dt), a["edge_index"], a["edge_attr"].to(dt))
        torch.testing.assert_close(out.float(), a["out"], rtol=2e-4, atol=2e-4)


def test_oracle_step_reproduces_the_reference_modules_training_step():
    meta, a, sd = load_golden("pyg_conv_train_step")
    assert meta["N"] == 50 and meta["towers"] == 4 and meta["edge_dim"] == 6 and meta["divide_input"]
    assert int((torch.bincount(a["edge_index"][1], minlength=50) == 0).sum()) >= 2
    m = _meta_of(meta, a)
    assert torch.equal(C.avg_deg_of(a["edge_index"][1], 50)[0], a["deg_hist"])
    got = C.step(sd, m, a, torch.float64)
    torch.testing.assert_close(got["out"], a["f64/out"], rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(got["grad_x"], a["f64/grad_x"], rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(got["grad_e"], a["f64/grad_edge_attr"], rtol=1e-10, atol=1e-10)
    assert set(got["grads"]) == {k[9:] for k in a if k.startswith("f64/grad/")}
    for k, g in got["grads"].items():
        torch.testing.assert_close(g, a["f64/grad/" + k], rtol=1e-10, atol=1e-10, msg=k)
    # the reference's fp32 run is within fp32 noise of its float64 run, and so is the restatement's
    got32 = C.step(sd, m, a, torch.float32)
    for k, g in got32["grads"].items():
        scale = a["f64/grad/" + k].abs().max().item()
        assert (g.double() - a["f64/grad/" + k]).abs().max().item() <= 1e-4 * max(scale, 1.0), k
        assert (a["f32/grad/" + k].double() - a["f64/grad/" + k]).abs().max().item() <= 1e-4 * max(scale, 1.0), k


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_case_meets_its_conditions_on_the_float64_oracle(name):
    meta, a, sd, ref = C.case(name)
    assert ref.frac <= 0.15
    deg = torch.bincount(a["edge_index"][1], minlength=meta["N"])
    assert bool((deg[-C.ISOLATED:] == 0).all())                       # rows without in-edges in the last tile
    for v in [ref.out, ref.grad_x, *ref.grads.values()]:
        assert bool(torch.isfinite(v).all())
    if "std" in meta["aggregators"] and a["edge_index"].shape[1]:
        assert ref.grads["post_nns.0.0.weight"].abs().max() > 0


def test_the_var_case_has_three_equal_messages_into_one_destination():
    meta, a, sd, ref = C.case("var_neg")
    ei = a["edge_index"]
    into0 = ei[0][ei[1] == 0]
    assert into0.tolist() == [3, 3, 3]


@pytest.mark.parametrize("ed", [0, 5])
def test_pack_then_unpack_reproduces_autograd(ed):
    """[W_j | W_i | W_e W_enc], b + W_e b_enc is the tower call's image of (W_pre, b_pre, W_enc, b_enc); given the gradient of a loss
    with respect to the image, the unpack formulas give autograd's gradients of the layer's own tensors -- float64, 1e-12."""
    gen = torch.Generator().manual_seed(3 + ed)
    T, Fi = 3, 7
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)      # noqa: E731
    W = [rnd(Fi, (3 if ed else 2) * Fi).requires_grad_(True) for _ in range(T)]
    b = [rnd(Fi).requires_grad_(True) for _ in range(T)]
    Wenc, benc = (rnd(Fi, ed).requires_grad_(True), rnd(Fi).requires_grad_(True)) if ed else (None, None)

    def pack(t):
        Wi, Wj, We = W[t][:, :Fi], W[t][:, Fi:2 * Fi], W[t][:, 2 * Fi:]
        if not ed:
            return torch.cat([Wj, Wi], dim=1), b[t]
        return torch.cat([Wj, Wi, We @ Wenc], dim=1), b[t] + We @ benc

    # any loss of the images: a random linear functional plus a quadratic term
    images = [pack(t) for t in range(T)]
    coef = [(rnd(*im.shape), rnd(Fi)) for im, _ in images]
    loss = sum((im * cw).sum() + 0.5 * (im * im).sum() + (bb * cb).sum() + 0.5 * (bb * bb).sum() for (im, bb), (cw, cb) in zip(images, coef))
    leaves = W + b + ([Wenc, benc] if ed else [])
    auto = torch.autograd.grad(loss, leaves)
    gW, gb = auto[:T], auto[T:2 * T]
    gWenc = torch.zeros(Fi, ed, dtype=torch.float64)
    gbenc = torch.zeros(Fi, dtype=torch.float64)
    for t in range(T):
        im, bb = images[t][0].detach(), images[t][1].detach()
        gim, gbb = coef[t][0] + im, coef[t][1] + bb                       # the tower call's gW'_t = [gA | gB | gM], gb'_t
        gA, gB, gM = gim[:, :Fi], gim[:, Fi:2 * Fi], gim[:, 2 * Fi:]
        blocks = [gB, gA] + ([gM @ Wenc.detach().t() + torch.outer(gbb, benc.detach())] if ed else [])
        assert (torch.cat(blocks, dim=1) - gW[t]).abs().max().item() <= 1e-12
        assert (gbb - gb[t]).abs().max().item() <= 1e-12
        if ed:
            We = W[t].detach()[:, 2 * Fi:]
            gWenc += We.t() @ gM
            gbenc += We.t() @ gbb
    if ed:
        assert (gWenc - auto[2 * T]).abs().max().item() <= 1e-12
        assert (gbenc - auto[2 * T + 1]).abs().max().item() <= 1e-12
