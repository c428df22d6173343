"""The batch plan without a GPU: the library's exports and limits, the ctypes mirror against the header, the knob, the consistency of
what the GPU tests compare with (tests/batch_plan_cases.py), and collate_flat's new keywords on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

import batch_plan_cases as C
from pna_amd import _lib
from pna_amd import graph as G
from pna_amd.graph import Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_three_symbols():
    L = _lib.lib()
    for name in ("pna_batch_plan_i32", "pna_batch_plan_limits", "pna_batch_plan_workspace_bytes"):
        assert hasattr(L, name), name
    assert L.pna_abi_version() == _lib.PNA_ABI_VERSION == 23
    assert "23, additive: + pna_batch_plan_i32 / pna_batch_plan_limits" in open(os.path.join(ROOT, "include", "pna_amd.h")).read()


def test_limits_admit_superpixel_members_and_are_a_host_call():
    n, e = G.batch_plan_limits()
    assert n >= 512 and e >= 4096
    L = _lib.lib()
    assert L.pna_batch_plan_limits(None, None) == 0                                   # either pointer may be NULL
    assert L.pna_batch_plan_workspace_bytes(1, 0, 0) > 0
    assert L.pna_batch_plan_workspace_bytes(2048, 120000, 52000) >= 4 * 3 * 2049
    for bad in ((0, 1, 1), (1, -1, 1), (1, 1, -1), (1, 1 << 31, 1), (1, 1, 1 << 31)):
        assert L.pna_batch_plan_workspace_bytes(*bad) == -1, bad


def test_the_ctypes_struct_follows_the_headers_field_order():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pna_amd.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+pna_batch_plan_args\s*\{(.*?)\}\s*pna_batch_plan_args\s*;", text, flags=re.S).group(1)
    fields = [re.match(r".*?(\w+)$", d.strip(), flags=re.S).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f for f, *_ in _lib.PnaBatchPlanArgs._fields_]
    assert fields[0] == "struct_size" and _lib.PnaBatchPlanArgs().struct_size == ctypes.sizeof(_lib.PnaBatchPlanArgs)


def test_the_call_checks_its_struct_and_its_scope_before_any_launch():
    L = _lib.lib()
    cls = _lib.PnaBatchPlanArgs
    a = cls()
    for short in (0, ctypes.sizeof(cls) - 8):
        a.struct_size = short
        assert L.pna_batch_plan_i32(ctypes.byref(a), None) == -1 and b"struct_size" in L.pna_last_error()
    a = cls()
    assert L.pna_batch_plan_i32(ctypes.byref(a), None) == -1 and b"scope" in L.pna_last_error()       # B = 0
    assert L.pna_batch_plan_i32(None, None) == -1
    lim_n, lim_e = G.batch_plan_limits()
    for n, e in ((lim_n + 1, 0), (0, lim_e + 1), (-1, 0)):
        a = cls()
        a.B, a.E, a.V, a.member_nodes_max, a.member_edges_max = 1, 1, 1, n, e
        assert L.pna_batch_plan_i32(ctypes.byref(a), None) == -1 and b"pna_batch_plan_limits" in L.pna_last_error(), (n, e)


def test_knob_is_off_by_default_and_read_from_the_environment(monkeypatch):
    """The module's own assignment evaluated under two environments (not a reload: other modules hold graph.Graph by identity)."""
    line = re.search(r"^BATCH_PLAN_ROWS = (.+)$", open(G.__file__).read(), flags=re.M).group(1)
    monkeypatch.delenv("PNA_AMD_BATCH_PLAN_ROWS", raising=False)
    assert eval(line, {"os": os, "int": int}) == 0
    monkeypatch.setenv("PNA_AMD_BATCH_PLAN_ROWS", "65536")
    assert eval(line, {"os": os, "int": int}) == 65536
    assert isinstance(G.BATCH_PLAN_ROWS, int)


@pytest.mark.parametrize("name", C.NAMES)
def test_the_expected_arrays_of_a_case_are_consistent(name):
    c = C.case(name)
    r = C.reference(c, "cpu")
    V, E = sum(c["num_nodes"]), int(c["src"].numel())
    lim_n, lim_e = G.batch_plan_limits()
    assert max(c["num_nodes"]) <= lim_n and max(c["edge_counts"]) <= lim_e
    for rp in (r["rowptr"], r["rowptr_t"]):
        assert rp.shape == (V + 1,) and int(rp[0]) == 0 and int(rp[V]) == E and bool((rp[1:] >= rp[:-1]).all())
    for perm in (r["eid64"], r["pos_t64"]):
        assert torch.equal(torch.sort(perm).values, torch.arange(E))
    # a member's rows lie inside its own edge range, forward and transposed: what lets a workgroup plan it alone
    noff = r["readout_offsets"].long()
    eoff = torch.tensor([0] + c["edge_counts"]).cumsum(0)
    for rp in (r["rowptr"].long(), r["rowptr_t"].long()):
        assert torch.equal(rp[noff], eoff)
    # rank_t: the position of a transposed edge inside its destination's in-edge list; col_t at that place is the same edge
    pos = r["rank_t"].long() + r["rowptr"].long()[r["col_t"].long()]
    assert torch.equal(pos, r["pos_t64"])
    assert torch.equal(r["row"][pos], r["col_t"]) and torch.equal(r["col"][pos], r["row_t"])
    assert torch.equal(r["src"][r["eid64"]], r["col"].long()) and torch.equal(r["dst"][r["eid64"]], r["row"].long())
    deg = r["rowptr"][1:] - r["rowptr"][:-1]
    assert r["max_in"] == (int(deg.max()) if E else 0)
    if name == "in_star_128":
        assert r["max_in"] == 128
    if name == "in_star_129":
        assert r["max_in"] == 129 and r["items"].shape[0] > V                       # heavy segments: the plan leaves this list lazy
    if name == "out_star_129":
        assert r["max_out"] == 129 and r["items_t"].shape[0] == V


def test_collate_flat_with_the_new_keywords_on_cpu_tensors_returns_todays_graph(monkeypatch):
    c = C.case("molecules_300")
    want = Graph.collate_flat(c["src"], c["dst"], c["edge_counts"], c["num_nodes"])
    monkeypatch.setattr(G, "BATCH_PLAN_ROWS", 1 << 20)
    for kw in (dict(), dict(train=True), dict(train=True, avg_d=1.2), dict(avg_d={"log": torch.tensor(1.2)})):
        got = Graph.collate_flat(c["src"], c["dst"], torch.tensor(c["edge_counts"]), c["num_nodes"], **kw)
        assert got.device.type == "cpu" and got.batch_num_nodes == want.batch_num_nodes
        assert torch.equal(got.src, want.src) and torch.equal(got.dst, want.dst)
        for x, y in zip(got.csr, want.csr):
            assert torch.equal(x, y) if torch.is_tensor(x) else x == y
        assert not got._heavy and got._snorm_n is None and not hasattr(got, "_pna_amd_transposed")
    srcs = list(torch.split(c["src"], c["edge_counts"]))
    dsts = list(torch.split(c["dst"], c["edge_counts"]))
    got = Graph.collate(srcs, dsts, c["num_nodes"], train=True, avg_d=1.2)
    assert torch.equal(got.src, want.src) and torch.equal(got.csr.eid, want.csr.eid)
    with pytest.raises(ValueError):
        Graph.collate_flat(c["src"], c["dst"][:-1], c["edge_counts"], c["num_nodes"])
