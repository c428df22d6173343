"""Kernel-level checks of pna_tower_layer_bf16 (pna_bf16_small.hip) through a ctypes caller that owns every pointer and pitch
(bf16_small_ref.py), stage by stage.  Each probe makes the later stages exact, so that ONE rounding separates the kernel from float64
on the exact bf16 operands and the merged contract applies to it alone,

    |got - ref64| <= 2u |ref64| + 4u M_j,      u = 2^-8,  M_j the absolute mass of the element,

or bit equality where the stage is a selection:
  projection   x_cat equals pna_contract_bf16 on the same image bit for bit and meets the bar; padding columns are zero
  gather       post_img selects (weights 0 / 1): y is the LDS aggregate tile.  max / min bit for bit against the fp32 messages rebuilt
               from the call's own x_cat; mean / sum / std / var at the gather bar of test_gpu_bf16_tower_kernels.py
  towers       max / min aggregators, no mixing network: the contraction, scalers, bias, graph norm, BatchNorm fold, activation and
               residual against float64 on the exact A operand
  mixing       the tower stage selects the exact max aggregate: y = R(res + act(W_mix z + b_mix))
Output and x_cat buffers are wider and longer than the call needs and prefilled with a canary: nothing but the V rows of the
output columns may change.  Graphs have prescribed in-degrees (0..5, 7, 8, 9, 11 and one row of a thousand edges), asserted here.

The header says the statistics are those of pna_gather_bf16.  Measured on an MI355X over the 13 gather cases of this file (in-degrees
0..11 and 1003, 1..8 towers, 1..80 features, all six aggregators): the largest difference is 0, the bits ARE equal -- both kernels
fold a row's edges in CSR order with the formulas of pna_bf16_dev.h -- so equality is asserted.  The largest error of any probe is
0.166 of its bar: u / 2 of a value against 2u |ref| + 4u M with M = |ref|, one rounding and nothing else."""
import ctypes

import pytest
import torch

import bf16_small_ref as R
from pna_amd import _lib
from pna_amd import ops

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ok(out):
    assert out["rc"] == 0, out["error"]
    return out


def _check_buffers(c, out):
    """Nothing outside the V rows of the output columns and of the 2 T Fp projection columns was written; no NaN came out."""
    V = c["V"]
    R.assert_untouched(out["y"], V, out["width"], "y")
    assert not torch.isnan(out["y"].float()).any(), "NaN in y"
    if out["x_cat"] is not None:
        R.assert_untouched(out["x_cat"], V, out["xw"], "x_cat")
        assert not torch.isnan(out["x_cat"].float()).any(), "NaN in x_cat"


def _check_projection(dev, c, out, h_dev):
    """Launch 1 as seen in the x_cat the call left behind."""
    V, T, Fi = c["V"], c["T"], c["Fi"]
    Fp, xw = R.rnd(Fi, 8), out["xw"]
    x = out["x_cat"][:V, :xw]
    want = ops.contract_bf16(h_dev, h_dev.shape[1], c["proj_img"].to(dev), xw, (None,), c["proj_bias"].to(dev))
    assert torch.equal(_bits(x), _bits(want.cpu())), "x_cat differs from pna_contract_bf16 on the same image"
    ref, mass = R.project64(c)
    tol = R.contract_tol(ref, mass)
    assert R.outside(x.double(), ref, tol) == 0, "projection: " + R.worst(x.double(), ref, tol)
    assert torch.count_nonzero(x.reshape(V, 2 * T, Fp)[:, :, Fi:]) == 0, "padding columns of x_cat are not zero"


def _h_pitch(c, i):
    """Every other case keeps h in a NaN-padded buffer (16-byte aligned rows), the rest contiguous (any alignment)."""
    return R.rnd(c["h"].shape[1], 8) + 8 if i % 2 else None


# ---- projection + gather probe ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.GATHER)), ids=lambda i: "V{V}_T{T}_Fi{Fi}_types{n_types}_bad{bad_types}".format(**R.GATHER[i]))
def test_gather_probe(cuda_device, i):
    """The aggregate tile against float64, against the fp32 messages (max / min) and against pna_gather_bf16 on the same operands
    (measured: max |one-call - pna_gather_bf16| = 0 in every case, so equal bits are asserted)."""
    c = R.gather_case(i)
    V, T, Fi, aggs = c["V"], c["T"], c["Fi"], c["aggs"]
    A, Fp = len(aggs), R.rnd(Fi, 8)
    R.assert_degree_classes(c["rowptr"], V, c["hub"])
    out = _ok(R.run(cuda_device, c, h_pitch=_h_pitch(c, i), table_pitch=T * Fp + 8 * (i % 2) if c.get("edge_type") is not None else None))
    _check_buffers(c, out)
    _check_projection(cuda_device, c, out, out["h_dev"])
    x, got = out["x_cat"], R.selector_view(out["y"], c)
    # max / min: the fp32 message, a selection, one rounding
    sel = R.selections(c, x)
    for j, name in enumerate(("max", "min")):
        if name in aggs:
            assert torch.equal(got[:, :, aggs.index(name)], sel[:, :, j]), f"{name} not bit-exact"
    ref, tol = R.gather64(c, x), R.gather_tol(c, x)
    print(f"gather probe {R.GATHER[i]}: max err / tol = {float(((got.double() - ref).abs() / tol.clamp_min(1e-300)).max()):.3f}")
    assert R.outside(got.double(), ref, tol) == 0, R.worst(got.double(), ref, tol)
    deg = (c["rowptr"][1:] - c["rowptr"][:-1]).long()
    assert torch.count_nonzero(got[deg == 0]) == 0
    # the multi-launch gather on the same operands: x_src | x_dst of the call's x_cat, the table with the types clamped on the host
    xd = x[:V].to(cuda_device)
    er = et = None
    if c.get("edge_type") is not None:
        er = c["edge_table"].to(cuda_device)
        et = c["edge_type"].clamp(0, c["n_types"] - 1).to(cuda_device)
    multi = ops.gather_bf16(c["rowptr"].to(cuda_device), c["col"].to(cuda_device), xd[:, :T * Fp], T * Fp, aggs, dst_term=xd[:, T * Fp:2 * T * Fp],
                            edge_rows=er, edge_type=et, block_stride=T * Fp)
    multi = multi.cpu()[:, :A * T * Fp].reshape(V, A, T, Fp)[..., :Fi].permute(0, 2, 1, 3)
    diff = float((multi.float() - got.float()).abs().max())
    print(f"gather probe {R.GATHER[i]}: max |one-call - pna_gather_bf16| = {diff:.3e}")
    assert torch.equal(_bits(multi), _bits(got)), f"statistics differ from pna_gather_bf16 by up to {diff:.3e}"


@pytest.mark.parametrize("i", range(len(R.GATHER_SIMPLE)), ids=["V80_aligned", "V75_contiguous_2byte", "V75_in_88_nan_padded_16byte"])
def test_gather_probe_no_self_panel(cuda_device, i):
    """The PNASimpleLayer form: the messages are the raw rows h[u]; the three layouts of h take the 16-byte, the 2-byte and the
    16-byte-with-readable-tail loads, the last one over NaN padding that must not reach y."""
    Fi, pitch, tail = R.GATHER_SIMPLE[i]
    c = R.gather_simple_case(i)
    V, aggs = c["V"], c["aggs"]
    R.assert_degree_classes(c["rowptr"], V, c["hub"])
    out = _ok(R.run(cuda_device, c, h_pitch=pitch, h_tail_readable=tail))
    assert out["h_dev"].stride(0) == (pitch or Fi) and out["x_cat"] is None
    _check_buffers(c, out)
    got = R.selector_view(out["y"], c)
    sel = R.selections(c, None)
    for j, name in enumerate(("max", "min")):
        assert torch.equal(got[:, :, aggs.index(name)], sel[:, :, j]), f"{name} not bit-exact"
    ref, tol = R.gather64(c, None), R.gather_tol(c, None)
    assert R.outside(got.double(), ref, tol) == 0, R.worst(got.double(), ref, tol)
    multi = ops.gather_bf16(c["rowptr"].to(cuda_device), c["col"].to(cuda_device), out["h_dev"], Fi, aggs, block_stride=R.rnd(Fi, 8))
    multi = multi.cpu().reshape(V, len(aggs), 1, R.rnd(Fi, 8))[..., :Fi].permute(0, 2, 1, 3)
    assert torch.equal(_bits(multi), _bits(got)), f"statistics differ from pna_gather_bf16 by up to {float((multi.float() - got.float()).abs().max()):.3e}"


# ---- tower contraction probe -----------------------------------------------------------------------------------------------------
def _towers_probe(dev, c, i):
    Kin, width = c["h"].shape[1], R.width_of(c)
    out = _ok(R.run(dev, c, h_pitch=_h_pitch(c, i + 1), res_pitch=width + 11 if c["residual"] is not None else None,
                    x_extra=16, y_extra=3 + i))
    assert out["h_dev"].stride(0) == (_h_pitch(c, i + 1) or Kin)
    _check_buffers(c, out)
    _check_projection(dev, c, out, out["h_dev"])
    ref, tol = R.towers_expect(c, out["x_cat"])
    got = out["y"][:c["V"], :width].double()
    print(f"towers probe T={c['T']} Fi={c['Fi']} Fo={c['Fo']} S={c['S']}: max err / tol = {float(((got - ref).abs() / tol.clamp_min(1e-300)).max()):.3f}")
    assert R.outside(got, ref, tol) == 0, R.worst(got, ref, tol)


@pytest.mark.parametrize("i", range(len(R.TOWERS)), ids=lambda i: "T{T}_Fi{Fi}_Fo{Fo}_S{S}".format(S=len(R.TOWERS[i]["scales"]), **R.TOWERS[i]))
def test_towers_probe(cuda_device, i):
    c = R.towers_case(i)
    R.assert_degree_classes(c["rowptr"], c["V"], c["hub"])
    _towers_probe(cuda_device, c, i)


def test_towers_probe_largest_tile(cuda_device):
    """The most towers of 33 features and 2 aggregators that fit: a tile beyond 64 KiB, the hipFuncSetAttribute route."""
    T, nbytes = R.largest_tile_shape()
    assert 64 * 1024 < nbytes <= 160 * 1024
    c = R.largest_tile_case()
    assert c["T"] == T and ops.tower_layer_bf16_lds_bytes(T, 33, 3, 2, False) == nbytes
    _towers_probe(cuda_device, c, 0)


# ---- mixing probe ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.MIX)), ids=lambda i: "K{K}_No{No}".format(K=R.MIX[i]["T"] * R.MIX[i]["Fi"], **R.MIX[i]))
def test_mix_probe(cuda_device, i):
    c = R.mix_case(i)
    V, No = c["V"], c["No"]
    R.assert_degree_classes(c["rowptr"], V, c["hub"])
    out = _ok(R.run(cuda_device, c, h_pitch=_h_pitch(c, i), res_pitch=No + 9 if c["residual"] is not None else None, y_extra=7))
    assert out["width"] == No
    _check_buffers(c, out)
    ref, tol = R.mix_expect(c, out["x_cat"])
    got = out["y"][:V, :No].double()
    print(f"mix probe {R.MIX[i]}: max err / tol = {float(((got - ref).abs() / tol.clamp_min(1e-300)).max()):.3f}")
    assert R.outside(got, ref, tol) == 0, R.worst(got, ref, tol)


# ---- the whole call --------------------------------------------------------------------------------------------------------------
def _zinc_case():
    return R.make_case(500, 700, 5, 75, 15, ["mean", "max", "min", "std"], scales=(False, True, True), post_bias=True, row_post=True, bn=True,
                       slope=0.01, residual=True, No=75, mix_bias=True, n_types=4)


def test_direct_caller_is_the_product_route(cuda_device):
    """A ZINC-like layer through the ctypes caller (wider pitches, canaries) equals ops.tower_layer_bf16 bit for bit, twice."""
    dev = cuda_device
    c = _zinc_case()
    first, second = _ok(R.run(dev, c)), _ok(R.run(dev, c, x_extra=24, y_extra=1, res_pitch=88))
    _check_buffers(c, first)
    _check_buffers(c, second)
    V = c["V"]
    d = lambda t: None if t is None else t.to(dev)   # noqa: E731
    want = ops.tower_layer_bf16(d(c["rowptr"]), d(c["col"]), d(c["h"]), n_tower=5, Fi=75, Fo=15, divide_input=False, aggregators=c["aggs"],
                                row_scales=[d(r) for r in c["row_scale"]], post_img=d(c["post_img"]), post_bias=d(c["post_bias"]),
                                proj_img=d(c["proj_img"]), proj_bias=d(c["proj_bias"]), row_post=d(c["row_post"]), col_scale=d(c["col_scale"]),
                                col_shift=d(c["col_shift"]), mix_img=d(c["mix_img"]), mix_bias=d(c["mix_bias"]), No=75, slope=0.01,
                                residual=d(c["residual"]), edge_type=d(c["edge_type"]), edge_table=d(c["edge_table"]))
    assert want.shape == (V, 75) and float(want.float().abs().max()) > 0.5
    assert torch.equal(_bits(first["y"][:V, :75]), _bits(want.cpu()))
    assert torch.equal(_bits(second["y"][:V, :75]), _bits(want.cpu()))
    assert torch.equal(_bits(first["x_cat"][:V, :first["xw"]]), _bits(second["x_cat"][:V, :second["xw"]]))


def test_no_rows_with_null_pointers_is_ok(cuda_device):
    a = _lib.PnaTowerLayerBf16Args()
    a.V, a.n_tower, a.Fi, a.Fo, a.n_scaler, a.n_aggr, a.mix_slope = 0, 5, 75, 15, 3, 4, 0.01
    for i, code in enumerate((0, 2, 3, 4)):
        a.aggr[i] = code
    assert _lib.lib().pna_tower_layer_bf16(ctypes.byref(a), _lib.stream_ptr(cuda_device)) == 0
    torch.cuda.synchronize(cuda_device)
