"""Kernel-level float64 checks of pna_fused_degree_f32 (pna_amd/csrc/pna_fused_degree.hip) on HAND-BUILT degree plans (fused_plan_cases.py)
through a ctypes caller that owns every pointer and pitch.  The plans use the whole of the header's contract, not the production builder's
subset: one in-degree per aligned 16-row block (tiles that mix four degrees), D on both sides of the ring's groups of four (0, 1, 3 | 4 |
5, 7 | 8 | 9 ..), D above the production hub threshold (129, 300), padding rows inside blocks, all-padding blocks and tiles, D = 0 blocks
whose placeholder records feed the id prefetch of the live block behind them.  A plan of a few tiles gives every workgroup ONE tile; the
loop-carried state (ids fetched by the previous tile's last packets, descriptors two tiles ahead, the claim counter) is exercised by
listing the same tiles again and again in chain order (fused_plan_cases.chain_order) -- several virtual tiles then name the same nodes and
write the same values.

  agg_out (the H2 verification instantiation)   the BITS of the C oracle's sequential fp32 fold for every live row; zeros for D = 0
  y under PNA_FD_ARITH_X3 / _H2 / _GUARDED      |got - ref64| <= 1e-5 |ref64| + 2e-6 mass |row_post col_scale| + 2^-22 E  per element, ref64
                                                the float64 contraction of the ORACLE's statistics (a gather error is visible)
  GUARDED on benign inputs                      H2's bits, guard words 0 / 1 zero, word 2 unchanged
y, agg_out and the guard workspace are prefilled with a canary: nothing but the named rows' N (or y_cols_writable) columns may change.

Measured on an MI355X, worst err / bar over every case of this module: bf16 x 3 0.113, fp16 x 2 0.113, fp16 x 2 guarded
0.113 -- the same element in all three (ladder, F = 49, N = 16): what is left at that level is common to the arithmetics (W_D formed in fp32, the
epilogue's fp32 roundings), not the operand split; tower mode 0.072 / 0.055 / 0.055; the 75 776-row claim-counter plans 0.106.  Every test
asserts err / bar <= 1."""
import ctypes

import numpy as np
import pytest
import torch

import fused_plan_cases as C
from pna_amd import _lib

pytestmark = pytest.mark.gpu

X3, H2, GUARDED = _lib.FD_ARITH_X3, _lib.FD_ARITH_H2, _lib.FD_ARITH_GUARDED
WORD2 = 1000                                                            # what guard word 2 holds before a call
_worst = {}


def _note(arith, ratio, what):
    name = _lib.FD_ARITH_NAMES[arith]
    _worst[name] = max(_worst.get(name, 0.0), ratio)
    print(f"[fused plans] {what}: {name} worst err / bar = {ratio:.4f} (module so far: {_worst[name]:.4f})")


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _pitched(a, dev, pitch, fill=float("nan"), tail_rows=0):
    """(rows, cols) view of a (rows + tail_rows, pitch) device buffer filled with `fill` around the data."""
    buf = torch.full((a.shape[0] + tail_rows, pitch), fill, dtype=torch.float32, device=dev)
    buf[:a.shape[0], :a.shape[1]] = _t(a, dev)
    return buf[:a.shape[0], :a.shape[1]], buf


def _images(dev, c, x3):
    key = ("img", x3)
    if key not in c:
        L = _lib.lib()
        F, N, S, n_img, tower = c["F"], c["N"], c["S"], c["n_img"], 1 if c["tower"] else 0
        stride = L.pna_fused_image_bytes(F, N, tower, x3)
        assert stride > 0 and stride % 4 == 0
        w = _t(c["w_ref"], dev)
        sc = None if c["scale"] is None else _t(c["scale"], dev)
        img = torch.zeros(n_img * stride // 4, dtype=torch.float32, device=dev)
        sp, st = (None if sc is None else ctypes.c_void_p(sc.data_ptr())), _lib.stream_ptr(dev)
        if tower and not x3:
            rc = L.pna_fused_tower_pack_f32(ctypes.c_void_p(w.data_ptr()), w.stride(0), N, F, S, sp, n_img, ctypes.c_void_p(img.data_ptr()), st)
        else:
            rc = L.pna_fused_pack_f32(ctypes.c_void_p(w.data_ptr()), w.stride(0), N, F, S, sp, n_img, ctypes.c_void_p(img.data_ptr()), tower, x3, st)
        _lib.check(rc, "pna_fused_pack_f32")
        torch.cuda.synchronize(dev)
        c[key] = (img, stride)
    return c[key]


def _source(dev, c, mode):
    """The source table in one of the layouts the header admits: `pitched` rows of round_up(F, 8) + 8 floats with NaN in the padding
    columns, `contiguous` rows at ldx = F (4-byte aligned only when F is odd), `tail` contiguous rows followed by NaN in the same allocation."""
    key = ("x", mode)
    if key not in c:
        F = c["F"]
        if mode == "pitched":
            c[key] = _pitched(c["x"], dev, C.round_up(F, 8) + 8)
        else:
            flat = torch.full((c["x"].size + (64 if mode == "tail" else 0),), float("nan"), dtype=torch.float32, device=dev)
            flat[:c["x"].size] = _t(c["x"], dev).reshape(-1)
            c[key] = (flat[:c["x"].size].view(-1, F), flat)
    return c[key][0]


class Call:
    """One pna_fused_degree_f32 call over a case: owns every device buffer; run() launches and synchronises, y_host() reads back."""

    def __init__(self, dev, c, arith, plan=None, dump=False, x_mode="pitched", ycw=0, dynamic=False, spare=0, ldy=None, ld_res=None):
        L = _lib.lib()
        p = c["plan"] if plan is None else plan
        F, N = c["F"], c["N"]
        self.dev, self.c, self.p, self.arith, self.dump = dev, c, p, arith, dump
        self.keep = []
        a = self.a = _lib.PnaFusedDegreeArgs()

        def ptr(t):
            self.keep.append(t)
            return ctypes.c_void_p(t.data_ptr())
        assert 0 <= p["tile_desc"][:, 2].min() and p["tile_desc"][:, 2].max() < c["n_img"] and p["tile_ids"].max() < c["x"].shape[0]
        assert p["perm"].max() < p["n_nodes"] and p["tile_desc"].shape[0] * 16 == p["M"] and p["tile_ids"].shape == (p["n_records"], 16)
        a.tile_desc, a.tile_ids, a.n_records = ptr(_t(p["tile_desc"], dev)), ptr(_t(p["tile_ids"], dev)), p["n_records"]
        x = _source(dev, c, x_mode)
        a.x, a.ldx, a.x_rows, a.F, a.N = ptr(x), x.stride(0), x.shape[0], F, N
        self.perm = _t(p["perm"], dev)
        a.row_perm, a.M, a.n_nodes = ptr(self.perm), p["M"], p["n_nodes"]
        if arith != X3:
            img, a.image_stride = _images(dev, c, 0)
            a.w_img = ptr(img)
        if arith != H2:
            img3, a.image_stride_x3 = _images(dev, c, 1)
            a.w_img_x3 = ptr(img3)
        for name in ("bias", "col_scale", "col_shift"):
            if c[name] is not None:
                setattr(a, name, ptr(_t(c[name], dev)))
        tw = c["tower"]
        ldy = (N + 5 if ycw == 0 else max(ycw, N + 5)) if ldy is None else ldy
        self.y = torch.full((p["n_nodes"], ldy), float(C.CANARY), dtype=torch.float32, device=dev)
        a.y, a.ldy, a.relu, a.act_slope, a.y_cols_writable = ptr(self.y), ldy, c["relu"], c["slope"], ycw
        if c["residual"] is not None:
            ld_res = (C.round_up(N, 4) + 8 if tw else N + 9) if ld_res is None else ld_res       # (tower mode: 16-byte aligned rows)
            res, _ = _pitched(c["residual"], dev, ld_res)
            assert ld_res != ldy
            a.residual, a.ld_res = ptr(res), ld_res
        if tw:
            for field, ld, name in (("x_dst", "ld_xdst", "x_dst"), ("h_self", "ld_h", "h_self")):
                t, _ = _pitched(tw[name], dev, C.round_up(F, 8) + (8 if name == "x_dst" else 16))
                setattr(a, field, ptr(t))
                setattr(a, ld, t.stride(0))
            rp = tw["row_post"]
            if "tile_of" in p:
                rp = rp.reshape(-1, p["tile"])[p["tile_of"]].reshape(-1)
            a.row_post = ptr(_t(rp, dev))
            if tw.get("pre_add") is not None:
                t, _ = _pitched(tw["pre_add"], dev, N + 3)
                a.pre_add, a.ld_pre_add = ptr(t), t.stride(0)
        self.agg = None
        if dump:
            self.ld_agg = 4 * F + 3
            self.agg = torch.full((p["M"], self.ld_agg), float(C.CANARY), dtype=torch.float32, device=dev)
            a.agg_out, a.ld_agg = ptr(self.agg), self.ld_agg
        self.ws = None
        if arith == GUARDED:
            nb = L.pna_fused_degree_guard_bytes(p["M"])
            self.ws_words = (nb + 3) // 4
            self.ws = torch.full((self.ws_words + 16,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            self.ws[:4] = torch.tensor([0, 0, WORD2, 0], dtype=torch.int32, device=dev)
            a.guard_ws, a.guard_ws_bytes = ptr(self.ws), nb
        self.counter = None
        if dynamic:
            self.counter = torch.zeros(2, dtype=torch.int32, device=dev)
            a.tile_counter = ptr(self.counter)
        a.arith, a.spare_workgroups = arith, spare

    def run(self, times=1):
        for _ in range(times):
            rc = _lib.lib().pna_fused_degree_f32(ctypes.byref(self.a), _lib.stream_ptr(self.dev))
            assert rc == 0, _lib.lib().pna_last_error().decode()
        torch.cuda.synchronize(self.dev)
        return self

    def y_host(self):
        return self.y.cpu().numpy()

    def guard_words(self):
        assert bool((self.ws[self.ws_words:] == 0x5A5A5A5A).all()), "the guard workspace was written past pna_fused_degree_guard_bytes(M)"
        return self.ws[:4].tolist()


class Judge:
    """The oracle's statistics and the float64 reference of a case's base plan: computed once, shared, never written to."""

    def __init__(self, c):
        self.c = c
        self.stats = C.oracle_stats(c["plan"], c["x"], c["F"])
        self.ref = C.layer_ref(c, self.stats)

    def check_stats(self, call):
        """agg_out: the oracle's bits on every live row (D = 0: zeros), canary behind the 4F columns."""
        p, F = call.p, self.c["F"]
        base = _t(self.stats, call.dev).view(torch.int32).view(-1, p["tile"], 4 * F)
        want = (base if "tile_of" not in p else base[_t(p["tile_of"], call.dev)]).reshape(-1, 4 * F)
        got = call.agg.view(torch.int32)
        live = call.perm >= 0
        diff = (got[:, :4 * F] != want)[live]
        if bool(diff.any()):
            rows = torch.nonzero(live).flatten()[diff.any(dim=1)]
            raise AssertionError(f"statistics differ from the oracle's bits in {rows.numel()} live rows, first: virtual row {int(rows[0])}")
        D = _t(np.repeat(p["block_D"], 16), call.dev)
        assert not bool(call.agg[live & (D == 0)][:, :4 * F].any()), "rows without in-edges must have zero statistics"
        assert bool((got[:, 4 * F:] == int(C.CANARY.view(np.int32))).all()), "agg_out was written behind its 4F columns"

    def check_y(self, call, what, cols_written=None, expect_pass=True):
        ratio, msg = C.compare_y(call.y_host(), self.c, self.ref, cols_written=cols_written)
        if expect_pass:
            _note(call.arith, ratio, what)
            assert ratio <= 1.0, f"{what} [{_lib.FD_ARITH_NAMES[call.arith]}]: {msg}"
        return ratio


def _all_arithmetics(dev, c, judge, what, plan=None, dump=True, benign=True, **kw):
    """The assertions every benign case shares; returns the H2 call's output."""
    if dump:
        d = Call(dev, c, H2, plan=plan, dump=True, **kw).run()
        judge.check_stats(d)
        judge.check_y(d, what + " (verification instantiation)")
    calls = {ar: Call(dev, c, ar, plan=plan, **kw).run() for ar in (X3, H2, GUARDED)}
    for ar, call in calls.items():
        judge.check_y(call, what, cols_written=kw.get("ycw") or None)
    words = calls[GUARDED].guard_words()
    assert words[:2] == [0, 0], f"{what}: guard words after the call: {words}"
    if benign:
        assert torch.equal(calls[GUARDED].y.view(torch.int32), calls[H2].y.view(torch.int32)), f"{what}: GUARDED on benign inputs differs from H2"
        assert words[2] == WORD2, f"{what}: tiles handed over on benign inputs: {words}"
    return calls


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


_cache = {}


def _case(key, make):
    if key not in _cache:
        c = make()
        assert C.check_contract(c["plan"], x_rows=c["plan"]["x_rows"])
        _cache[key] = (c, Judge(c))
    return _cache[key]


# ---- the degree ladder at every instantiation edge -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,N", C.LADDER_SHAPES, ids=lambda v: str(v))
def test_degree_ladder(cuda_device, F, N):
    assert _lib.lib().pna_fused_degree_image_bytes(F, N) > 0 and _lib.lib().pna_fused_degree_tile_rows(F, N) == C.TILE
    k = C.LADDER_SHAPES.index((F, N))
    c, judge = _case(("ladder", F, N), lambda: C.make_case(F, N, C.ladder_blocks(), seed=k, S=1 + k % 3, relu=k % 3, slope=0.01, residual=k % 2 == 0))
    _all_arithmetics(cuda_device, c, judge, f"ladder F={F} N={N}")


@pytest.mark.parametrize("F,N", [(75, 75), (64, 64), (33, 40), (20, 16), (128, 128), (64, 100), (112, 17)], ids=lambda v: str(v))
def test_degree_ladder_across_tile_boundaries(cuda_device, F, N):
    """The ladder's tiles listed three rounds deep in chain order for a grid of one workgroup per CU: every workgroup walks three tiles
    that follow one another in the ladder, so the ids fetched by a tile's last packets and the descriptors fetched two tiles ahead cross
    every boundary of the list -- D = 0 placeholders in front of a live block, 300 edges in front of 1, mixed degrees per wavefront."""
    dev = cuda_device
    c, judge = _case(("ladder", F, N, "chain"), lambda: C.make_case(F, N, C.ladder_blocks(), seed=50 + F, relu=1))
    base = c["plan"]
    G = _cus(dev)
    plan = C.retile(base, C.chain_order(base["M"] // C.TILE, G, 3))
    assert C.check_contract(plan, x_rows=base["x_rows"])
    _all_arithmetics(dev, c, judge, f"chained ladder F={F} N={N}", plan=plan, spare=G)


# ---- padding and stores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,N,relu,residual,bias,bn", [(75, 75, 1, True, True, True), (64, 20, 2, False, True, False), (40, 13, 0, True, False, True),
                                                       (128, 100, 2, True, False, False), (33, 4, 1, False, False, False)])
def test_padding_rows_and_stores(cuda_device, F, N, relu, residual, bias, bn):
    """Live rows at {0, 7, 15} only, an all-padding block between live ones, an all-padding tile: nothing is written for perm = -1, rows no
    virtual row names and columns >= N keep the canary; with y_cols_writable = 16 ceil(N / 16) the columns behind N are zero and the
    N columns hold the same bits."""
    dev = cuda_device
    c, judge = _case(("padding", F, N), lambda: C.make_case(F, N, C.padding_blocks(), seed=F + N, n_img=2, relu=relu, slope=0.2,
                                                           residual=residual, bias=bias, bn=bn))
    calls = _all_arithmetics(dev, c, judge, f"padding F={F} N={N}")
    ycw = C.round_up(N, 16)
    for ar in (X3, H2, GUARDED):
        wide = Call(dev, c, ar, ycw=ycw).run()
        judge.check_y(wide, f"padding F={F} N={N} y_cols_writable={ycw}", cols_written=ycw)
        assert torch.equal(wide.y[:, :N].view(torch.int32), calls[ar].y[:, :N].view(torch.int32))


# ---- source-row addressing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,N,mode", [(75, 75, "contiguous"), (33, 40, "contiguous"), (75, 75, "tail"), (33, 40, "tail"), (65, 16, "tail"),
                                      (113, 128, "tail"), (49, 80, "contiguous"), (17, 5, "tail")])
def test_source_rows_of_any_pitch(cuda_device, F, N, mode):
    """x contiguous at ldx = F (rows 4-byte aligned only) and as a view whose last row is followed by NaN in the same allocation (the
    pitched layout with NaN padding columns is every other test's): a read past a row's F-th float poisons a statistic."""
    c, judge = _case(("ladder", F, N, "addr"), lambda: C.make_case(F, N, C.ladder_blocks(C.LADDER[:12]), seed=3 * F))
    assert c["plan"]["x_rows"] - 1 in c["plan"]["col"]
    _all_arithmetics(cuda_device, c, judge, f"x {mode} F={F} N={N}", x_mode=mode)


# ---- pack edges ----------------------------------------------------------------------------------------------------------------------------
def _pack_edge_case(F, N, S, n_img, zero_x):
    c = C.make_case(F, N, [(D, (i // 4) % n_img, C.ALL16) for i, D in enumerate((1, 2, 3, 4, 5, 6, 9, 0) * (2 if n_img < 5 else 4))][:max(8, 4 * n_img)],
                    seed=7 * S + n_img, S=S, n_img=n_img, relu=0, x_scale=0.0 if zero_x else 1.0)
    w = c["w_ref"]
    K = 4 * F
    w[N // 2, :] = 0.0                                               # an all-zero output column
    for s in range(S):
        w[:, s * K + 5:(s + 1) * K:F] = 0.0                          # an all-zero feature column (feature 5 of every aggregator and scaler)
    w[1, :] *= 1e4                                                   # columns eight decades apart
    w[3, :] *= 1e-4
    if S > 1:
        c["scale"][n_img - 1, S - 1] = 0.0                           # a scale of 0 on one scaler
    return c


@pytest.mark.parametrize("F,N,S,n_img,zero_x", [(75, 75, 1, 1, False), (75, 75, 2, 7, False), (40, 16, 3, 7, False), (64, 100, 3, 1, False),
                                                (128, 128, 2, 2, False), (75, 75, 3, 2, True), (33, 5, 1, 2, True)])
def test_pack_edges(cuda_device, F, N, S, n_img, zero_x):
    """Zero output / feature columns, columns eight decades apart, 1..3 scalers with arbitrary positive values and a zero, 1 and 7
    images; an all-zero source table (std = sqrt(1e-5) exactly, the row-scale bound at its floor)."""
    c, judge = _case(("pack", F, N, S, n_img, zero_x), lambda: _pack_edge_case(F, N, S, n_img, zero_x))
    if zero_x:
        live = np.repeat(c["plan"]["block_D"], 16) > 0
        assert np.array_equal(judge.stats[live][:, 3 * F:], np.full((int(live.sum()), F), np.sqrt(np.float32(1e-5)), np.float32))
    dev = cuda_device
    d = Call(dev, c, H2, dump=True).run()
    judge.check_stats(d)
    for ar in (X3, H2, GUARDED):
        call = Call(dev, c, ar).run()
        judge.check_y(call, f"pack edges F={F} N={N} S={S} images={n_img}")
        if ar == GUARDED:
            assert call.guard_words()[:2] == [0, 0]


# ---- schedules give the same bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,N", [(75, 75), (128, 128), (40, 72)])
def test_schedules_give_the_same_bits(cuda_device, F, N):
    dev = cuda_device
    c, judge = _case(("ladder", F, N, "chain"), lambda: C.make_case(F, N, C.ladder_blocks(), seed=50 + F, relu=1))
    base = c["plan"]
    nt = base["M"] // C.TILE
    cus = _cus(dev)
    for ar in (X3, H2, GUARDED):
        ref = Call(dev, c, ar).run()
        judge.check_y(ref, f"schedules F={F} N={N}")
        bits = ref.y.view(torch.int32)
        dyn = Call(dev, c, ar, dynamic=True).run()
        assert torch.equal(dyn.y.view(torch.int32), bits) and dyn.counter.tolist() == [0, 0], "dynamic schedule"
        assert torch.equal(Call(dev, c, ar, spare=2 * cus + 3).run().y.view(torch.int32), bits), "spare_workgroups >= 2 x CU count"
        order = np.random.default_rng(5).permutation(nt)
        assert torch.equal(Call(dev, c, ar, plan=C.retile(base, order)).run().y.view(torch.int32), bits), "tiles in a permuted order"
        again = Call(dev, c, ar, dynamic=True)
        for _ in range(20):
            again.y.fill_(float(C.CANARY))
            again.run()
            assert torch.equal(again.y.view(torch.int32), bits), "the same call twenty times"
        assert again.counter.tolist() == [0, 0]
    # a plan of a single tile (M = one tile): the ladder's mixed tile with the D = 0 block
    t1 = int(np.nonzero((base["block_D"].reshape(-1, 4) == 0).any(axis=1) & (base["block_D"].reshape(-1, 4) > 0).any(axis=1))[0][0])
    one = C.retile(base, [t1])
    for ar in (X3, H2, GUARDED):
        full, single = Call(dev, c, ar).run(), Call(dev, c, ar, plan=one).run()
        rows = _t(base["perm"].reshape(-1, C.TILE)[t1], dev).long()
        rows = rows[rows >= 0]
        assert torch.equal(single.y[rows].view(torch.int32), full.y[rows].view(torch.int32)), "a plan of a single tile"
        untouched = torch.ones(base["n_nodes"], dtype=torch.bool, device=dev)
        untouched[rows] = False
        assert bool((single.y[untouched].view(torch.int32) == int(C.CANARY.view(np.int32))).all())


@pytest.mark.parametrize("F,N", [(75, 75), (64, 128)])
def test_claim_counter_over_thousands_of_cheap_tiles(cuda_device, F, N):
    """More than 4 G + G / 2 tiles of D in 0 .. 5 for a grid of G = CU count workgroups: every workgroup goes through its four static tiles
    and then takes claims.  All outputs meet the bar, both counter words are zero afterwards, and a second launch without any memset
    gives the same bits."""
    dev = cuda_device
    c, judge = _case(("claim", F, N), lambda: C.make_case(F, N, C.claim_blocks(), seed=F, n_img=2))
    base = c["plan"]
    G = _cus(dev)
    n_tiles = 4 * G + G // 2 + 32
    plan = C.retile(base, C.chain_order(base["M"] // C.TILE, G, (n_tiles + G - 1) // G)[:n_tiles])
    assert plan["M"] // C.TILE > 4 * G + G // 2 and plan["block_D"].max() <= 5
    d = Call(dev, c, H2, plan=plan, dump=True, dynamic=True, spare=G).run()
    judge.check_stats(d)
    assert d.counter.tolist() == [0, 0]
    for ar in (X3, H2, GUARDED):
        call = Call(dev, c, ar, plan=plan, dynamic=True, spare=G).run()
        judge.check_y(call, f"claim counter F={F} N={N}, {plan['M']} virtual rows")
        assert call.counter.tolist() == [0, 0], call.counter.tolist()
        first = call.y.clone()
        call.y.fill_(float(C.CANARY))
        call.run()                                                   # (no memset of the counter or of the guard words in between)
        assert torch.equal(call.y.view(torch.int32), first.view(torch.int32)) and call.counter.tolist() == [0, 0]
        static = Call(dev, c, ar, plan=plan, spare=G).run()
        assert torch.equal(static.y.view(torch.int32), first.view(torch.int32)), "static against dynamic"
        if ar == GUARDED:
            assert call.guard_words()[:3] == [0, 0, WORD2]


# ---- the guard's hand-over at tile edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,N", [(75, 75), (128, 128), (40, 72)])
def test_guard_hands_over_exactly_the_tiles_with_an_adversarial_row(cuda_device, F, N):
    """Feature 7 of ONE source row is 1e8 x the rest, with zero weights on that feature's statistics; three virtual rows in two tiles have
    that source among their in-edges -- tiles that also hold a D = 0 block, padding rows and mixed degrees."""
    dev = cuda_device
    BAD_SRC, f0 = 17, 7

    def make():
        c = C.make_case(F, N, C.ladder_blocks(), seed=90 + F, relu=1)
        p = c["plan"]
        col = p["col"].copy()
        col[col == BAD_SRC] = BAD_SRC + 1
        Dm = p["block_D"].reshape(-1, 4)
        mixed = np.nonzero((np.array([len(set(t)) for t in Dm]) >= 3) & (Dm == 0).any(axis=1))[0]
        victims = []
        for t in (mixed[0], mixed[-1]):                               # a mixed tile with a D = 0 block; the list's last tile (padding, D = 0)
            rows = np.nonzero((p["perm"][t * C.TILE:(t + 1) * C.TILE] >= 0) & (np.repeat(Dm[t], 16) > 0))[0] + t * C.TILE
            victims += [int(rows[0]), int(rows[-1])][:2 if t == mixed[0] else 1]
        for v in victims:
            col[p["rowptr"][v] + (p["rowptr"][v + 1] - p["rowptr"][v]) // 2] = BAD_SRC
        c["plan"] = C.with_edges(p, col)
        c["x"][BAD_SRC, f0] = 1e8
        K = 4 * F
        for s in range(c["S"]):
            for a in range(4):
                c["w_ref"][:, s * K + a * F + f0] = 0.0
        c["victim_tiles"] = sorted({v // C.TILE for v in victims})
        return c
    c, judge = _case(("guard", F, N), make)
    assert len(c["victim_tiles"]) == 2
    base = c["plan"]
    x3, h2, gd = (Call(dev, c, ar).run() for ar in (X3, H2, GUARDED))
    judge.check_y(x3, f"guard hand-over F={F} N={N}")
    judge.check_y(gd, f"guard hand-over F={F} N={N}")
    assert judge.check_y(h2, "", expect_pass=False) > 1.0, "the unguarded form was expected to leave the bar on the adversarial rows"
    words = gd.guard_words()
    assert words[:2] == [0, 0] and words[2] == WORD2 + 2, words
    others = np.ones(base["M"] // C.TILE, bool)
    others[c["victim_tiles"]] = False
    rows = base["perm"].reshape(-1, C.TILE)[others].reshape(-1)
    rows = _t(rows[rows >= 0], dev).long()
    assert torch.equal(gd.y[rows].view(torch.int32), h2.y[rows].view(torch.int32)), "tiles that were not handed over keep H2's bits"


# ---- tower mode ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,N", C.TOWER_SHAPES, ids=lambda v: str(v))
def test_tower_mode(cuda_device, F, N):
    """x_dst / h_self / row_post (+ pre_add in its own buffer) on the ladder up to D = 33: the [deg > 0] mask of the x_dst term on live
    rows without in-edges, a row_post of 0, one row whose h_self is 1e6 x its statistics (the mid-row rescale), both list layouts and
    the chained list."""
    dev = cuda_device
    k = C.TOWER_SHAPES.index((F, N))

    def make():
        c = C.make_case(F, N, C.ladder_blocks(C.LADDER[:16]), seed=70 + k, tower=True, pre_add=k % 2 == 0, relu=2, slope=0.01, residual=k % 3 != 1)
        p = c["plan"]
        live = np.nonzero(p["perm"] >= 0)[0]
        c["tower"]["row_post"][live[3]] = 0.0
        c["tower"]["h_self"][p["perm"][live[len(live) // 2]]] *= 1e6
        return c
    c, judge = _case(("tower", F, N), make)
    D = np.repeat(c["plan"]["block_D"], 16)
    assert ((D == 0) & (c["plan"]["perm"] >= 0)).any()
    _all_arithmetics(dev, c, judge, f"tower F={F} N={N}", dump=False, benign=False)   # (the 1e6 row may be the guard's: not a benign input)
    G = _cus(dev)
    plan = C.retile(c["plan"], C.chain_order(c["plan"]["M"] // C.TILE, G, 3))
    _all_arithmetics(dev, c, judge, f"tower, chained list F={F} N={N}", plan=plan, dump=False, benign=False, spare=G)
