"""pna_batch_plan_i32 through ctypes on the hand-built batches of tests/batch_plan_cases.py: every output against the route of today
(collate_flat with the knob off, the lazy properties, autograd._transposed_whole_rows) -- integers for equality, fp32 tables bit for
bit -- with and without the transposed arrays, with and without scalers, with outputs skipped; bad ids; the scope; repeatability."""
import ctypes

import pytest
import torch

import batch_plan_cases as C
from pna_amd import _lib
from pna_amd import graph as G

pytestmark = pytest.mark.gpu

I32 = ("rowptr", "col", "row", "eid", "items", "readout_offsets", "rowptr_t", "col_t", "row_t", "pos_t", "rank_t", "items_t")
I64 = ("src", "dst", "eid64", "pos_t64", "row64", "col64")
F32 = ("snorm_n", "amp", "att")
TRANSPOSED = ("rowptr_t", "col_t", "row_t", "pos_t", "pos_t64", "rank_t", "items_t", "row64", "col64")
SENTINEL = -7


def _sizes(B, E, V):
    return dict(rowptr=V + 1, col=E, row=E, eid=E, items=4 * V, readout_offsets=B + 1, rowptr_t=V + 1, col_t=E, row_t=E, pos_t=E, rank_t=E,
                items_t=4 * V, src=E, dst=E, eid64=E, pos_t64=E, row64=E, col64=E, snorm_n=V, amp=V, att=V)


def plan(c, dev, want_transposed=1, avg_log=0.0, skip=(), src=None, dst=None, member_max=None):
    """One call.  Every output is its own tensor filled with SENTINEL first; the names in `skip` are passed as NULL.  Returns (rc, outputs,
    record as a list)."""
    B, V = len(c["num_nodes"]), sum(c["num_nodes"])
    src = c["src"] if src is None else src
    dst = c["dst"] if dst is None else dst
    E = int(src.numel())
    s32, d32 = src.to(torch.int32).to(dev), dst.to(torch.int32).to(dev)
    counts = torch.tensor([c["edge_counts"], c["num_nodes"]], dtype=torch.int32).to(dev)
    out = {}
    for name, n in _sizes(B, E, V).items():
        dtype = torch.int32 if name in I32 else torch.int64 if name in I64 else torch.float32
        out[name] = torch.full((n,), SENTINEL, dtype=dtype, device=dev)
    record = torch.full((4,), SENTINEL, dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = L.pna_batch_plan_workspace_bytes(B, E, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a = _lib.PnaBatchPlanArgs()
    a.src_local, a.dst_local = (s32.data_ptr(), d32.data_ptr()) if E else (None, None)
    a.edge_count, a.node_count = counts[0].data_ptr(), counts[1].data_ptr()
    a.B, a.E, a.V, a.want_transposed, a.avg_log = B, E, V, want_transposed, avg_log
    a.member_nodes_max, a.member_edges_max = member_max if member_max is not None else (max(c["num_nodes"]), max(c["edge_counts"]))
    for name, t in out.items():
        setattr(a, name, None if name in skip else t.data_ptr())
    a.record, a.workspace, a.workspace_bytes = record.data_ptr(), ws.data_ptr(), nbytes
    rc = L.pna_batch_plan_i32(ctypes.byref(a), _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return rc, out, record.tolist()


def _expected(ref, name, avg_log):
    if name in ("amp", "att"):
        return ref[("scalers", avg_log)][0 if name == "amp" else 1]
    t = ref[name]
    return t.reshape(-1) if name in ("items", "items_t") else t


def check(c, ref, out, record, want_transposed, avg_log, skip=()):
    """Every output that the call was asked for equals the reference; every other one still holds the sentinel."""
    assert record == [ref["max_in"], ref["max_out"] if want_transposed else 0, 0, 0], record
    heavy_in = ref["max_in"] > G.HEAVY_THRESHOLD
    for name, got in out.items():
        wanted = name not in skip and (want_transposed or name not in TRANSPOSED) and (avg_log > 0 or name not in ("amp", "att"))
        if not wanted:
            assert bool((got == SENTINEL).all()), f"{name}: written although not asked for"
            continue
        if name == "items" and heavy_in:
            # the reference list has hub segments; the call's whole-row records are what work_items(threshold=1 << 30) gives
            want = ref["graph"].work_items(threshold=1 << 30).reshape(-1)
        else:
            want = _expected(ref, name, avg_log)
        assert C.same(got, want), f"{name}: {int((got != want).sum()) if got.shape == want.shape else 'shape'} entries differ"


@pytest.mark.parametrize("name", C.NAMES)
def test_every_output_equals_the_route_of_today(cuda_device, name):
    c = C.case(name)
    ref = C.reference(c, cuda_device, avg_logs=(1.3,))
    for want_transposed, avg_log, skip in ((1, 1.3, ()), (0, 0.0, ()), (1, 0.0, ("col", "eid64", "items", "snorm_n", "pos_t", "row64", "dst")),
                                           (0, 1.3, ("att", "rowptr", "src"))):
        rc, out, record = plan(c, cuda_device, want_transposed, avg_log, skip)
        assert rc == 0, _lib.lib().pna_last_error()
        check(c, ref, out, record, want_transposed, avg_log, skip)


def test_snorm_is_one_ieee_division_and_one_ieee_square_root(cuda_device):
    """Member sizes from 1 to the limit: sqrt(1 / n) is numpy's fp32 division and fp32 square root (both correctly rounded; the square
    root checked against the float64 one rounded once) and the bits Graph.snorm_n() gives on the device."""
    import numpy as np
    lim_n, _ = G.batch_plan_limits()
    sizes = list(range(1, 130)) + [255, 256, 257, 511, 513, 1000, lim_n]
    z = torch.zeros(len(sizes), dtype=torch.int64)                                # one self-loop on node 0 of every member
    c = dict(src=z, dst=z, edge_counts=[1] * len(sizes), num_nodes=sizes)
    rc, out, record = plan(c, cuda_device, 0, 0.0)
    assert rc == 0 and record == [1, 0, 0, 0]
    r = np.float32(1.0) / np.asarray(sizes, dtype=np.float32)
    s = np.sqrt(r)
    assert s.dtype == np.float32 and np.array_equal(s, np.sqrt(r.astype(np.float64)).astype(np.float32))
    want = torch.repeat_interleave(torch.from_numpy(s), torch.tensor(sizes))
    assert C.same(out["snorm_n"].cpu(), want)
    assert C.same(out["snorm_n"], C.unplanned(c, cuda_device).snorm_n().reshape(-1))


@pytest.mark.parametrize("bad_value", ["n_g", -1])
@pytest.mark.parametrize("side", ["src", "dst"])
def test_a_bad_id_sets_the_status_and_leaves_every_other_member_alone(cuda_device, bad_value, side):
    c = C.case("alternating_1_200")
    ref = C.reference(c, cuda_device, avg_logs=(1.3,))
    member = 5                                                                   # a 200-node member between two one-node members
    noff = torch.tensor([0] + c["num_nodes"]).cumsum(0)
    eoff = torch.tensor([0] + c["edge_counts"]).cumsum(0)
    k = int(eoff[member]) + 17
    src, dst = c["src"].clone(), c["dst"].clone()
    (src if side == "src" else dst)[k] = c["num_nodes"][member] if bad_value == "n_g" else -1
    rc, out, record = plan(c, cuda_device, 1, 1.3, src=src, dst=dst)
    assert rc == 0 and record[2] == 1 and record[3] == 0
    nodes = torch.ones(sum(c["num_nodes"]), dtype=torch.bool)
    nodes[noff[member]:noff[member + 1]] = False
    edges = torch.ones(int(c["src"].numel()), dtype=torch.bool)
    edges[eoff[member]:eoff[member + 1]] = False
    nodes, edges = nodes.to(cuda_device), edges.to(cuda_device)
    for name, got in out.items():
        want = _expected(ref, name, 1.3)
        if name == "readout_offsets":
            assert C.same(got, want)
        elif name in ("items", "items_t"):
            assert C.same(got.view(-1, 4)[nodes], want.view(-1, 4)[nodes]), name
        elif name in ("rowptr", "rowptr_t"):
            assert C.same(got[:-1][nodes], want[:-1][nodes]) and int(got[-1]) == int(want[-1]), name
        elif got.numel() == nodes.numel() and name in ("snorm_n", "amp", "att"):
            assert C.same(got[nodes], want[nodes]), name
        else:
            assert C.same(got[edges], want[edges]), name
    # the refused edge is written nowhere: its own slot of src / dst and the last CSR slot of its member keep what they held
    assert int(out["src"][k]) == SENTINEL and int(out["dst"][k]) == SENTINEL
    last = int(eoff[member + 1]) - 1
    for name in ("col", "row", "eid", "eid64", "col_t", "row_t", "pos_t", "rank_t"):
        assert int(out[name][last]) == SENTINEL, name
        inside = out[name][int(eoff[member]):last]
        assert bool((inside != SENTINEL).all()), name


def test_a_member_above_the_limits_is_outside_the_scope(cuda_device):
    lim_n, lim_e = G.batch_plan_limits()
    c = dict(src=torch.zeros(lim_e + 1, dtype=torch.int64), dst=torch.zeros(lim_e + 1, dtype=torch.int64), edge_counts=[lim_e + 1], num_nodes=[4])
    rc, out, record = plan(c, cuda_device)
    assert rc == -1 and b"scope" in _lib.lib().pna_last_error()
    assert record == [SENTINEL] * 4 and all(bool((t == SENTINEL).all()) for t in out.values())          # nothing was launched
    # a member larger than the caller declared: no fault, bit 1 of the status, that member's group is skipped
    c = C.case("at_max_member_edges")
    rc, out, record = plan(c, cuda_device, member_max=(600, 4096))
    assert rc == 0 and record[2] == 2
    e0 = c["edge_counts"][0]
    assert bool((out["col"][e0:e0 + c["edge_counts"][1]] == SENTINEL).all())


def test_two_calls_on_one_input_give_identical_bytes(cuda_device):
    for name in ("molecules_300", "interleaved", "at_max_member_edges"):
        c = C.case(name)
        _, first, rec1 = plan(c, cuda_device, 1, 1.3)
        _, second, rec2 = plan(c, cuda_device, 1, 1.3)
        assert rec1 == rec2
        for key in first:
            assert C.same(first[key], second[key]), (name, key)
