"""The one-kernel layer (pna_amd/csrc/pna_fused_degree.hip) on plans whose rows ALL have one in-degree D, for every residue of D mod 4
on both sides of ceil(D / 4) = 1 | 2 and one D of three groups: a tile owns max(4, round_up(D, 4)) id records, the ones past D repeat
edge D - 1, and from two groups on the kernel requests such a record's rows for lane 0 only (ld_packet_masked) -- the other lanes of
the ring slot keep the edge the slot held a round earlier, edge D - 5 + j, and the drain folds the slot all the same.  That fold must
be invisible: max / min see an edge a second time, the sums take zero.  The plans are hand-built (fused_plan_cases.py) with

  group A   the LAST real edge of every row carries every column's maximum (and, negated in half the columns, the minimum)
  group B   the edge FOUR positions before the last carries it (D >= 5): the edge a padding slot keeps -- a stale fold that was not
            idempotent, or that reached the sums, shows here
  group C   random sources with multi-edges and self loops, one of them a source row of magnitude 1e4

of 64 rows each (one full tile) or 80 (a second tile with 16 live rows, 48 padding), through the half-block instantiation (F = N = 75),
the wide one (F = N = 128: two gather passes) and tower mode (F = 75).

  agg_out (verification instantiation)   the BITS of pna_segreduce_fwd_f32 over the same rows and of the C oracle's sequential fold;
                                         conftest.check_blocks against oracle/torch_oracle.py in fp32 and float64
  y, every arithmetic                    |got - ref64| within the per-element bar of fused_plan_cases.layer_ref (err / bar <= 1)"""
import numpy as np
import pytest
import torch

import fused_plan_cases as C
from conftest import check_blocks, mass_stats
from test_gpu_fused_degree_plans import H2, Call, Judge, _all_arithmetics, _t

pytestmark = pytest.mark.gpu

DEGREES = (0, 1, 3, 4, 5, 6, 7, 8, 9, 13)
AGGS = ["mean", "max", "min", "std"]
BIG, HUGE = 11, 23                                                    # source rows: every column's extreme | magnitude 1e4


def _blocks(R):
    live = [ALL for ALL in [C.ALL16] * (R // 16)]
    pad = (-R // 16) % (C.TILE // 16)
    return live, pad


def _make(F, N, D, R, tower):
    live, pad = _blocks(R)
    blocks = []
    for _ in range(3):                                                # groups A, B, C: R rows each, whole tiles
        blocks += [(D, 0, m) for m in live] + [(0, 0, 0)] * pad
    c = C.make_case(F, N, blocks, seed=7 * D + R + F, S=3, n_img=1, residual=True, relu=1, tower=tower, pre_add=False)
    p = c["plan"]
    x = c["x"]
    rng = np.random.default_rng(D + R)
    x[BIG] = 60.0 + rng.random(F).astype(np.float32)
    x[BIG, 1::2] *= -1.0                                              # (odd columns: the minimum)
    x[HUGE] = (1e4 * rng.standard_normal(F)).astype(np.float32)
    col, rp, perm = p["col"].copy(), p["rowptr"], p["perm"]
    col[(col == BIG) | (col == HUGE)] = 0
    Mg = (len(live) + pad) * 16                                       # virtual rows of one group
    if D > 0:
        for v in np.nonzero(perm >= 0)[0]:
            grp = v // Mg
            if grp == 0:
                col[rp[v] + D - 1] = BIG
            elif grp == 1 and D >= 5:
                col[rp[v] + D - 5] = BIG
            elif grp == 2:
                k = v % Mg
                if k % 3 == 0:
                    col[rp[v]] = perm[v]                              # a self loop
                if k % 4 == 1 and D >= 2:
                    col[rp[v] + D - 1] = col[rp[v] + D - 2]           # a multi-edge ending the row
                if k == 5:
                    col[rp[v] + D // 2] = HUGE
    c["plan"] = C.with_edges(p, col)
    assert C.check_contract(c["plan"], x_rows=p["x_rows"])
    assert set(c["plan"]["block_D"][np.repeat(perm.reshape(-1, 16)[:, 0] >= 0, 1)]) == {D}
    return c


def _check_statistics(dev, c, call):
    """agg_out against pna_segreduce_fwd_f32 (bits) and against the torch oracle (conftest.check_blocks)."""
    from oracle import torch_oracle as O
    from pna_amd import ops
    p, F = c["plan"], c["F"]
    live = p["perm"] >= 0
    got = call.agg[:, :4 * F]
    if p["col"].size:
        xd = _t(np.ascontiguousarray(c["x"]), dev)
        ref = ops.segreduce(_t(p["rowptr"], dev, torch.int32), _t(p["col"], dev, torch.int32), xd, F, AGGS)
        lv = _t(live, dev)
        assert torch.equal(got[lv].view(torch.int32), ref[lv].view(torch.int32)), "statistics differ from pna_segreduce_fwd_f32's bits"
    M = p["M"]
    deg = np.diff(p["rowptr"])
    dst = torch.from_numpy(np.repeat(np.arange(M), deg))
    src = torch.from_numpy(p["col"])
    msg = torch.from_numpy(c["x"])[src]
    o32 = O.reduce_bucketed(msg, src, dst, M, AGGS, ["identity"], torch.tensor(2.3)).numpy()
    o64 = O.reduce_bucketed(msg.double(), src, dst, M, AGGS, ["identity"], torch.tensor(2.3)).numpy()
    check_blocks(got.cpu().numpy()[live], o32[live], o64[live], AGGS, 1, F, f"D={int(deg.max())}",
                 tuple(m[live] for m in mass_stats(p["rowptr"], msg.numpy())))


@pytest.mark.parametrize("F,N,tower,R", [(75, 75, False, 64), (75, 75, False, 80), (128, 128, False, 64), (128, 128, False, 80), (75, 75, True, 80)],
                         ids=lambda v: str(v))
def test_rows_of_one_degree_through_the_padding_slots(cuda_device, F, N, tower, R):
    dev = cuda_device
    for D in DEGREES:
        c = _make(F, N, D, R, tower)
        judge = Judge(c)
        what = f"one degree D={D} rows={R} F={F}{' tower' if tower else ''}"
        if not tower:
            d = Call(dev, c, H2, dump=True).run()
            judge.check_stats(d)
            _check_statistics(dev, c, d)
        # (the 1e4 row may be the guard's to hand over: not a benign input)
        _all_arithmetics(dev, c, judge, what, dump=not tower, benign=False)
