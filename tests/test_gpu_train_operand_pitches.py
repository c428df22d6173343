"""The five training entry pairs (pna_tower_train_*, pna_tower_edge_train_*, pna_tower_drop_train_*, pna_tower_aggr_train_*,
pna_simple_train_*) through ctypes with PITCHED operands: h, out, grad_out, e and grad_e as [:, :width] views of wider buffers, every pitch
another one and none a multiple of 4 floats.  A pitch changes addresses, never arithmetic or summation order, so every output of the
pitched run has the contiguous run's bits -- the run the entry pairs' own kernel test files hold to float64; one case per entry pair is
held to float64 here as well.  The padding of an output keeps its sentinel, the guard row each side of it too, and no NaN of an input's
padding reaches an output.  Last, the pitches below the width: refused by the argument checks, nothing launched, nothing written."""
import ctypes

import pytest
import torch

import small_train_cases as SC
import tower_aggr_train_cases as TA
import tower_aggr_train_run as AR
import tower_drop_train_cases as TD
import tower_edge_train_cases as TE
import tower_train_cases as TT
import tower_train_run as TR
from pna_amd import _lib, autograd as AG
from test_gpu_small_train_kernels import _Run as SimpleRun

pytestmark = pytest.mark.gpu

PNA_E_INVALID = -1                      # include/pna_amd.h
FILL = 7.0                              # what the outputs hold before a refused call


def pitches_of(widths):
    """{operand: pitch} for {operand: width}: width + 1, + 3, + 5, + 1, + 3 in turn, moved on by 2 until the pitch is no multiple of 4 floats
    (no row but the first 16-byte aligned by accident) and no other operand's pitch (a swapped ld_* cannot cancel)."""
    out = {}
    for (name, width), extra in zip(widths.items(), (1, 3, 5, 1, 3)):
        p = width + extra
        while p % 4 == 0 or p in out.values():
            p += 2
        out[name] = p
    return out


def tower_pitches(meta):
    w = {"h": meta["in_dim"], "out": meta["out_dim"], "go": meta["out_dim"]}
    if meta["edge_dim"]:
        w.update(e=meta["edge_dim"], ge=meta["edge_dim"])
    return pitches_of(w)


def test_the_pitches_are_distinct_and_unaligned():
    for widths in ({"h": 75, "out": 75, "go": 75, "e": 50, "ge": 50}, {"h": 16, "out": 16, "go": 16, "e": 3, "ge": 3}, {"h": 4, "out": 1, "go": 1}):
        p = pitches_of(widths)
        assert len(set(p.values())) == len(p) and all(v % 4 and v > widths[k] for k, v in p.items()), p


def _same_bits(pitched, plain, names=None):
    assert len(pitched) == len(plain)
    for i, (x, y) in enumerate(zip(pitched, plain)):
        what = names[i] if names else i
        assert x.shape == y.shape and not bool(torch.isnan(x).any()), what         # (no NaN of an input's padding reached an output)
        assert torch.equal(x, y), (what, float((x - y).abs().max()))


def _padding_kept(run, widths):
    for name, buf in run.buffers.items():
        assert TR.padding_untouched(buf, widths[name]), name


# ---- pna_tower_train_* / pna_tower_edge_train_* / pna_tower_drop_train_* (tower_train_run.Run) ----------------------------------------------
#            id: (cases module, case, key, want_grad_e, float64 check)
TOWER_RUNS = {
    "plain-two_scalers": (TT, "two_scalers", False, True, False),
    "plain-hand_res": (TT, "hand_res", False, True, True),
    "plain-zinc_last": (TT, "zinc_last", False, True, False),
    "edge3-hand": (TE, "hand", False, True, True),
    "edge3-hand-no_grad_e": (TE, "hand", False, False, False),
    "edge50-zinc_edge_first": (TE, "zinc_edge_first", False, True, False),
    "edge50-zinc_edge_first-no_grad_e": (TE, "zinc_edge_first", False, False, False),
    "drop-zinc_edge_first": (TD, "zinc_edge_first", True, True, True),
}


@pytest.mark.parametrize("rid", list(TOWER_RUNS))
def test_tower_entries_with_pitched_operands_give_the_contiguous_bits(cuda_device, rid):
    cases, name, keyed, want_ge, f64 = TOWER_RUNS[rid]
    case = cases.case(name)
    meta, ref = case[0], case[3]
    key = case[4] if keyed else None
    plain = TR.Run(name, case, cuda_device, key=key, want_grad_e=want_ge)
    pitches = tower_pitches(meta)
    r = TR.Run(name, case, cuda_device, key=key, want_grad_e=want_ge, pitches=pitches)
    assert r.args.ldh == pitches["h"] and r.args.ld_out == pitches["out"] and r.args.ld_go == pitches["go"]
    if meta["edge_dim"]:
        assert r.q.ld_e == pitches["e"] and (not want_ge or r.q.ld_ge == pitches["ge"])
    assert sorted(r.buffers) == (["ge", "out"] if meta["edge_dim"] and want_ge else ["out"])
    _same_bits(r.everything, plain.everything)
    _padding_kept(r, {"out": meta["out_dim"], "ge": meta["edge_dim"]})
    if f64:
        cases.check_step(meta, ref, r.out, r.gh, r.grads, r.running)
        if r.ge is not None:
            cases.check_grad_e(ref, r.ge)


# ---- pna_tower_aggr_train_* (tower_aggr_train_run.Run) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,f64", [("hand", True), ("edge50_max_var", False), ("no_edges_edge", False), ("drop_edge3_sum", False)])
def test_aggr_entries_with_pitched_operands_give_the_contiguous_bits(cuda_device, name, f64):
    case = TA.case(name)
    meta, ref = case[0], case[3]
    plain = AR.Run(case, cuda_device)
    pitches = tower_pitches(meta)
    r = AR.Run(case, cuda_device, pitches=pitches)
    base, q = r.keep[4], r.keep[5]
    assert base.ldh == pitches["h"] and base.ld_out == pitches["out"] and base.ld_go == pitches["go"]
    if meta["edge_dim"] and r.plan.E:
        assert q.ld_e == pitches["e"] and q.ld_ge == pitches["ge"]
    names = sorted(plain.history[-1])
    assert sorted(r.history[-1]) == names
    _same_bits([r.history[-1][k] for k in names], [plain.history[-1][k] for k in names], names)
    _padding_kept(r, {"out": meta["out_dim"], "ge": meta["edge_dim"]})
    if f64:
        TA.check_step(meta, ref, r.out, r.gh, r.grads)
        if r.ge is not None and r.ge.numel():
            TA.check_grad_e(ref, r.ge)


# ---- pna_simple_train_* (test_gpu_small_train_kernels._Run) ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,f64", [("hand_res", True), ("narrow", False)])
def test_simple_entries_with_pitched_operands_give_the_contiguous_bits(cuda_device, name, f64):
    meta, a, sd, ref = SC.case(name)
    plain = SimpleRun(name, cuda_device)
    pitches = pitches_of({"h": meta["F"], "out": meta["out_dim"], "go": meta["out_dim"]})
    r = SimpleRun(name, cuda_device, pitches=pitches)
    assert r.args.ldh == pitches["h"] and r.args.ld_out == pitches["out"] and r.args.ld_go == pitches["go"]
    _same_bits(r.history[-1], plain.history[-1])
    _padding_kept(r, {"out": meta["out_dim"]})
    if f64:
        torch.testing.assert_close(r.out.cpu(), ref.out.float(), rtol=1e-5, atol=1e-5)      # test_z_and_batch_statistics_against_float64's bar
        SC.check_gradients(meta, a, ref, r.gh, {SC.W_KEY: r.gw, SC.B_KEY: r.gv[0], "batchnorm_h.weight": r.gv[1], "batchnorm_h.bias": r.gv[2]})


# ---- pitches below the width: refused on the host, nothing launched ------------------------------------------------------------------------
def _copy(block):
    c = type(block)()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(block), ctypes.sizeof(c))
    return c


def _filled(tensors):
    for t in tensors:
        t.fill_(FILL)
    return tensors


def _still_filled(tensors, dev):
    torch.cuda.synchronize(dev)
    return all(bool((t == FILL).all()) for t in tensors)


def _tower_refusals(dev, base, q, outputs, call):
    """call(which, base', q') -> return code of the entry pair under test on copies of the argument blocks with one pitch set one below
    its operand's width."""
    C, in_dim = base.n_tower * base.Fo, (base.n_tower * base.Fi if base.divide_input else base.Fi)
    bad = [("fwd", "ldh", in_dim - 1), ("bwd", "ldh", in_dim - 1), ("fwd", "ld_out", C - 1), ("bwd", "ld_go", C - 1)]
    if q is not None:
        bad += [("fwd", "ld_e", q.edge_dim - 1), ("bwd", "ld_e", q.edge_dim - 1), ("bwd", "ld_ge", q.edge_dim - 1)]
    for which, field, value in bad:
        b2 = _copy(base)
        q2 = None
        if q is not None:
            q2 = _copy(q)
            q2.base = ctypes.cast(ctypes.pointer(b2), ctypes.c_void_p)
        setattr(q2 if field in ("ld_e", "ld_ge") else b2, field, value)
        _filled(outputs)
        assert call(which, b2, q2) == PNA_E_INVALID, (which, field)
        assert _still_filled(outputs, dev), (which, field)
    b2 = _copy(base)                                                                 # (the unchanged copies are accepted)
    q2 = None
    if q is not None:
        q2 = _copy(q)
        q2.base = ctypes.cast(ctypes.pointer(b2), ctypes.c_void_p)
    assert call("bwd", b2, q2) == 0
    torch.cuda.synchronize(dev)


@pytest.mark.parametrize("rid", ["plain-hand_res", "edge3-hand", "drop-zinc_edge_first"])
def test_tower_entries_refuse_a_pitch_below_the_width(cuda_device, rid):
    cases, name, keyed, want_ge, _ = TOWER_RUNS[rid]
    case = cases.case(name)
    key = case[4] if keyed else None
    r = TR.Run(name, case, cuda_device, key=key)
    L, st = _lib.lib(), _lib.stream_ptr(cuda_device)

    def call(which, base, q):
        if key is not None:
            return getattr(L, f"pna_tower_drop_train_{which}_f32")(ctypes.byref(AG._tower_drop_args(base, q, key)), st)
        if q is not None:
            return getattr(L, f"pna_tower_edge_train_{which}_f32")(ctypes.byref(q), st)
        return getattr(L, f"pna_tower_train_{which}_f32")(ctypes.byref(base), st)
    outputs = [r.out, r.gh] + ([r.ge] if r.ge is not None else []) + list(r.grads.values())
    _tower_refusals(cuda_device, r.args, r.q, outputs, call)


def test_aggr_entries_refuse_a_pitch_below_the_width(cuda_device):
    case = TA.case("edge50_max_var")
    r = AR.Run(case, cuda_device)
    base, q = r.keep[4], r.keep[5]
    L, st = _lib.lib(), _lib.stream_ptr(cuda_device)

    def call(which, b2, q2):
        block = r.plan.aggr_args(b2, q2, r.key, r.saved, backward=which == "bwd")
        return getattr(L, f"pna_tower_aggr_train_{which}_f32")(ctypes.byref(block), st)
    outputs = [r.out, r.gh, r.ge] + list(r.grads.values())
    _tower_refusals(cuda_device, base, q, outputs, call)


def test_simple_entries_refuse_a_pitch_below_the_width(cuda_device):
    r = SimpleRun("hand_res", cuda_device)
    L, st = _lib.lib(), _lib.stream_ptr(cuda_device)
    F, N = r.meta["F"], r.meta["out_dim"]
    outputs = [r.out, r.gh, r.gw, r.gv]
    for which, field, value in (("fwd", "ldh", F - 1), ("bwd", "ldh", F - 1), ("fwd", "ld_out", N - 1), ("bwd", "ld_go", N - 1)):
        a2 = _copy(r.args)
        setattr(a2, field, value)
        _filled(outputs)
        assert getattr(L, f"pna_simple_train_{which}_f32")(ctypes.byref(a2), st) == PNA_E_INVALID, (which, field)
        assert _still_filled(outputs, cuda_device), (which, field)
    assert L.pna_simple_train_bwd_f32(ctypes.byref(_copy(r.args)), st) == 0
    torch.cuda.synchronize(cuda_device)
