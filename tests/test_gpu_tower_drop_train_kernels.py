"""pna_dropout_mask_f32 and pna_tower_drop_train_fwd_f32 / pna_tower_drop_train_bwd_f32 through ctypes (PNALayer's training forward and
backward with the towers' dropout, one C call each: models/dgl/pna_layer.py:55-76, 130-145 in train mode): the device mask against the
numpy restatement bit for bit, every output per element against the float64 oracle under the same mask
(tower_drop_train_cases.masked_step) at the bars of tower_train_cases / tower_edge_train_cases, p = 0 against the calls without dropout
bit for bit, repeatability for one key, and the dropped positions.

Conditioning: the lists of ill-conditioned rows and their 15 % cap are those of the base cases (the mask does not reach what they are
derived from); the dropout keys of tower_drop_train_cases.CASES were picked on the CPU so that no float64 mixing pre-activation lies
within 1e-5 of the largest of zero under the mask and the fp32 oracle under the same mask passes these bars on its own
(tests/test_tower_drop_train_host.py::test_fp32_oracle_under_the_same_mask_is_inside_the_bars)."""
import ctypes

import numpy as np
import pytest
import torch

import tower_drop_train_cases as C
from pna_amd import _lib, autograd as AG
from pna_amd import functional as PF
from tower_train_run import Run

pytestmark = pytest.mark.gpu

CASES = list(C.CASES)


def _Run(name, dev, key):
    return Run(name, C.case(name), dev, key=key)


_runs = {}


def _run(name, dev, key="case"):
    key = C.case(name)[4] if key == "case" else key
    if (name, key) not in _runs:
        _runs[(name, key)] = _Run(name, dev, key)
    return _runs[(name, key)]


def _device_mask(dev, V, Cc, p, seed, offset, ld=None):
    ld = Cc if ld is None else ld
    buf = torch.full((V, ld), -1.0, device=dev)
    _lib.check(_lib.lib().pna_dropout_mask_f32(buf.data_ptr(), ld, V, Cc, p, seed, offset, _lib.stream_ptr(dev)), "pna_dropout_mask_f32")
    torch.cuda.synchronize(dev)
    return buf.cpu().numpy()


@pytest.mark.parametrize("V,Cc,p,seed,offset,ld", [
    (45, 75, 0.1, 7, 0, None),                                  # C % 4 = 3: quads straddle the row ends
    (16, 16, 0.3, 7, 0, None),
    (33, 70, 0.3, 11, 64, None),                                # a tail tile of one row, C % 4 = 2
    (45, 75, 0.3, 7, (1 << 32) + 12, None),                     # an offset above 2^32: the counter's fourth word
    (45, 75, 0.3, (0xDEADBEEF << 32) | 5, 8, None),             # a seed with a non-zero high word: the second key word
    (33, 70, 0.1, 11, 64, 77),                                  # a padded ld > C: the padding is not written
])
def test_device_mask_equals_the_host_restatement(cuda_device, V, Cc, p, seed, offset, ld):
    got = _device_mask(cuda_device, V, Cc, p, seed, offset, ld)
    want = C.host_mask(V, Cc, p, seed, offset)
    assert np.array_equal(got[:, :Cc], want)
    if ld is not None:
        assert bool((got[:, Cc:] == -1.0).all())
    assert np.array_equal(PF.dropout_mask(V, Cc, p, seed, offset, cuda_device).cpu().numpy(), want)         # the Python entry
    # the high words are read: the same low words with a zero high word give another mask
    if offset >> 32 or seed >> 32:
        assert not np.array_equal(want, C.host_mask(V, Cc, p, seed & C.MASK32, offset & C.MASK32))


@pytest.mark.parametrize("name", CASES)
def test_step_per_element_against_the_masked_float64_oracle(cuda_device, name):
    """Output, grad_h, grad_e where the case has edge features, every parameter gradient and the running statistics with
    tower_train_cases.check_step / tower_edge_train_cases.check_grad_e, the references taken under the case's mask.  z and the batch
    statistics are those of the undropped rows: the bars of test_gpu_tower_train_kernels.py against the base case's float64 values."""
    r = _run(name, cuda_device)
    meta, a, sd, ref, key = C.case(name)
    C.check_step(meta, ref, r.out, r.gh, r.grads, r.running)
    if r.ed:
        C.check_grad_e(ref, r.ge)
    err = (r.z.double().cpu() - ref.z).abs()
    tol = 1e-5 * ref.z.abs() + 2e-6 * ref.mass
    print(f"[tower_drop_train] z: max err / tol = {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all())
    torch.testing.assert_close(r.stats[0].double().cpu(), ref.mean, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(r.stats[1].double().cpu(), ref.invstd, rtol=1e-5, atol=1e-6)
    for k, v in r.running.items():
        torch.testing.assert_close(v.double().cpu(), ref.running[k], rtol=1e-5, atol=1e-6)
    act = torch.where(r.p > 0, r.p, r.p * C.SLOPE)
    assert torch.equal(r.out, a["h"].to(cuda_device) + act if meta["residual"] else act)


@pytest.mark.parametrize("name", CASES)
def test_p_zero_gives_the_bits_of_the_calls_without_dropout(cuda_device, name):
    """thr = 0 keeps every element and the factor is 1.0f: the new entry points compute what the existing ones compute, bit for bit --
    the saved state, the output, every gradient, the running statistics."""
    with_p0, base = _run(name, cuda_device, key=(0.0, 99, 4)), _run(name, cuda_device, key=None)
    assert len(with_p0.everything) == len(base.everything)
    for t0, t1 in zip(with_p0.everything, base.everything):
        assert torch.equal(t0, t1)


@pytest.mark.parametrize("name", ["zinc_first", "zinc_edge_first"])
def test_one_key_repeats_bitwise_and_another_offset_changes_the_mask(cuda_device, name):
    p, seed, offset = C.case(name)[4]
    first, again = _run(name, cuda_device), _Run(name, cuda_device, (p, seed, offset))
    for t0, t1 in zip(first.everything, again.everything):
        assert torch.equal(t0, t1)
    other = _run(name, cuda_device, key=(p, seed, offset + 4))
    assert not torch.equal(first.out, other.out) and not torch.equal(first.grads["mixing_network.linear.weight"], other.grads["mixing_network.linear.weight"])
    assert torch.equal(first.z, other.z) and torch.equal(first.stats, other.stats)          # what lies in front of the mask does not move
    for k in first.running:
        assert torch.equal(first.running[k], other.running[k])


@pytest.mark.parametrize("name", CASES)
def test_dropped_positions_carry_no_gradient(cuda_device, name):
    """The mixing weight's gradient is g_p^T (mask * hcat) and grad_beta is the column sum of mask * (g_p W_mix): computed here in float64
    from the call's own saved p and z and the HOST mask.  A mask applied on one side only, or after the column sums, fails it: a
    dropped element contributes exactly nothing to either."""
    r = _run(name, cuda_device)
    meta, a, sd, ref, key = C.case(name)
    V, Cc = meta["N"], meta["out_dim"]
    mask = ref.mask.double()
    z, p = r.z.double().cpu(), r.p.double().cpu()
    gamma = torch.cat([sd[f"towers.{t}.batchnorm_h.weight"] for t in range(r.T)]).double()
    beta = torch.cat([sd[f"towers.{t}.batchnorm_h.bias"] for t in range(r.T)]).double()
    mean, invstd = r.stats[0].double().cpu(), r.stats[1].double().cpu()
    xhat = (z - mean) * invstd
    hcat = (xhat * gamma + beta) * mask
    gp = torch.where(p > 0, a["R"].double(), a["R"].double() * C.SLOPE)
    W = sd["mixing_network.linear.weight"].double()
    ghc = (gp @ W) * mask
    # bars: the worst-case fp32 bound of a sum of n products, n 2^-24 sum |terms|, with n = the rows + the mixing width + 16 for the
    # few roundings inside a term (the affine expression, the factor, xhat; the weight-gradient kernel's three-term bf16 split of an
    # operand drops products of relative size 3 x 2^-24)
    u = (V + Cc + 16) * 2.0 ** -24
    ghc_mass = (gp.abs() @ W.abs()) * mask
    gmw = r.grads["mixing_network.linear.weight"].double().cpu()
    assert bool(((gmw - gp.t() @ hcat).abs() <= u * (gp.abs().t() @ hcat.abs())).all())
    gb = torch.cat([r.grads[f"towers.{t}.batchnorm_h.bias"] for t in range(r.T)]).double().cpu()
    gg = torch.cat([r.grads[f"towers.{t}.batchnorm_h.weight"] for t in range(r.T)]).double().cpu()
    assert bool(((gb - ghc.sum(0)).abs() <= u * ghc_mass.sum(0)).all())
    assert bool(((gg - (ghc * xhat).sum(0)).abs() <= u * (ghc_mass * xhat.abs()).sum(0)).all())
    dropped = float((mask == 0).double().mean())
    assert abs(dropped - key[0]) < 0.05, dropped                                  # the share the rule promises, at these sizes


def test_out_of_scope_arguments_are_refused_and_write_nothing(cuda_device):
    r = _run("zinc_edge_first", cuda_device)
    towers, grads, go, ge, args, qb = r.keep
    L, st = _lib.lib(), _lib.stream_ptr(cuda_device)
    before = [t.clone() for t in [r.out, r.gh, r.ge] + list(r.grads.values())]
    other = _lib.PnaTowerTrainArgs()
    ctypes.memmove(ctypes.byref(other), ctypes.byref(args), ctypes.sizeof(other))
    for fn in (L.pna_tower_drop_train_fwd_f32, L.pna_tower_drop_train_bwd_f32):
        for p in (1.0, -0.25, float("nan")):
            assert fn(ctypes.byref(AG._tower_drop_args(args, qb, (p, 1, 0))), st) == -1, p
        assert fn(ctypes.byref(AG._tower_drop_args(other, qb, (0.3, 1, 0))), st) == -1                      # edge->base is another struct
        d = AG._tower_drop_args(args, qb, (0.3, 1, 0))
        d.struct_size -= 8
        assert fn(ctypes.byref(d), st) == -1
    torch.cuda.synchronize(cuda_device)
    for t0, t in zip(before, [r.out, r.gh, r.ge] + list(r.grads.values())):
        assert torch.equal(t0, t)
