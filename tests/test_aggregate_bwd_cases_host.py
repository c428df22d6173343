"""The cases and the comparison of test_gpu_aggregate_backward_edges.py are sound (no GPU): every case builds and meets the builder's two
conditions, the graphs and the planted values are what the GPU tests rely on, the oracle's tie rule is "the first index", and the
comparison SEES the bugs it is there for -- a plain float64 model of the ranked pull meets the bar on every case, and fails on the cases
written for it as soon as one of three classic bugs is planted (aggregate_bwd_cases.pull_model)."""
import pytest
import torch

import aggregate_bwd_cases as C
from oracle import torch_oracle as O
from pna_amd.graph import HEAVY_THRESHOLD, SEG_LEN, Graph

KEYS = C.all_case_keys()
_id = lambda k: "-".join(str(v) for v in k)           # noqa: E731


@pytest.mark.parametrize("key", KEYS, ids=_id)
def test_case_builds_and_the_float64_model_of_the_pull_meets_the_bar(key):
    c = C.case(*key)                                       # (asserts: ill <= 15 % of the nodes, the fp32 oracle within a quarter of the bar)
    print(f"[aggregate_bwd] {_id(key)}: ill share {c.ill_share:.4f}, fp32 oracle err / bar = {c.oracle32_err / C.BAR:.4f}")
    assert c.ill_share <= C.MAX_ILL and c.oracle32_err <= C.BAR / 4
    A = len(c.aggs)
    R5 = c.R.view(c.V, c.T, 3, A, c.F)
    stat = [i for i, a in enumerate(c.aggs) if a in ("std", "var")]
    assert not bool(R5[c.ill][:, :, :, stat].any())        # the mask: std / var blocks of the ill destinations ...
    rest = torch.cat([R5[~c.ill].flatten(), R5[c.ill][:, :, :, [i for i in range(A) if i not in stat]].flatten()])
    assert float((rest != 0).double().mean()) > 0.9999     # ... and nothing else (a normal deviate is exactly 0 once in millions)
    gx, gd = C.pull_model(c)
    assert C.check(c, gx, gd, "float64 model") <= 0.01     # (the same formulas in the same precision: far inside the bar)


def test_the_parametrisation_covers_every_route_at_every_width_class():
    cases = C.width_cases()
    assert 140 <= len(cases) + len(C.outside_cases()) + len(C.DETERMINISTIC_INSIDE) <= 180
    classes = {"F%4==0": lambda T, F: F % 4 == 0, "F%4==1": lambda T, F: F % 4 == 1, "F%4==3": lambda T, F: F % 4 == 3,
               "F>=64": lambda T, F: F >= 64, "T>1": lambda T, F: T > 1}
    for route in C.ROUTES:
        mine = [k for k in cases if k[2] == route]
        assert {(T, F) for T, F, *_ in mine} == set(C.WIDTHS)
        for T, F in C.WIDTHS:                              # both aggregator sets, with and without a destination term, at every width
            here = [(a, d) for t, f, _, a, d in mine if (t, f) == (T, F)]
            assert {a for a, _ in here} == {"A", "B"} and {d for _, d in here} == {False, True}
        for name, pred in classes.items():
            assert any(pred(T, F) for T, F, *_ in mine), (route, name)
    # the per-edge-rows pull serves T = 1, set A, no destination term: the default route and its switch both get that at every T = 1 width
    for route in C.ROUTES[:2]:
        assert all((T, F, route, "A", False) in cases for T, F in C.WIDTHS if T == 1)
    assert all(F < 4 or F > 256 for _, F in C.WIDTHS_OUTSIDE) and all(4 <= F <= 256 for _, F in C.WIDTHS)
    assert {F for _, F in C.WIDTHS} >= {4, 256} and {F for _, F in C.WIDTHS_OUTSIDE} >= {3, 257}      # both sides of both boundaries


@pytest.mark.parametrize("hub_sources", [True, False])
def test_general_graph_has_the_rows_the_gpu_tests_rely_on(hub_sources):
    V = 600
    src, dst = C.graph(1, V, hub_sources)
    g = Graph(src, dst, V)
    csr, tcsr = g.csr, Graph(dst, src, V).csr
    din, dout = torch.bincount(dst, minlength=V), torch.bincount(src, minlength=V)
    assert int(din[0]) > 2 * SEG_LEN and int(din[1]) > HEAVY_THRESHOLD                      # hub destinations: two and more forward segments
    assert g.heavy_schedule().n_heavy == 2
    if hub_sources:
        assert int(dout[2]) > HEAVY_THRESHOLD and int(dout[3]) > HEAVY_THRESHOLD and tcsr.max_degree > HEAVY_THRESHOLD
    else:
        assert tcsr.max_degree <= HEAVY_THRESHOLD                                           # no atomics in the pull: bit-identical runs
    assert int(din[-4:].sum()) == 0 and int(dout[-1]) == 0 and int((dout == 0).sum()) >= 3
    assert int(tcsr.rowptr[V - 1]) == int(tcsr.rowptr[V]) == src.numel()                    # the last record: beg == the end of the arrays
    assert torch.unique(src * V + dst).numel() == src.numel()                               # no repeated edge
    eid = csr.eid
    assert not torch.equal(eid, torch.arange(eid.numel())) and torch.equal(torch.sort(eid).values, torch.arange(eid.numel()))
    same_row = csr.row[1:] == csr.row[:-1]
    assert bool((eid[1:] > eid[:-1])[same_row].all())                                       # mailbox order == CSR order: one "first"
    assert 3200 <= src.numel() <= 3400 if hub_sources else 2800 <= src.numel() <= 2900


def test_oracle_sends_a_tied_max_or_min_to_the_first_index():
    for dtype in (torch.float64, torch.float32):
        h = torch.tensor([[[1.0], [3.0], [3.0], [0.0], [0.0]], [[2.0], [2.0], [2.0], [2.0], [2.0]]], dtype=dtype, requires_grad=True)
        (O.MAILBOX_AGGREGATORS["max"](h).sum() + 10 * O.MAILBOX_AGGREGATORS["min"](h).sum()).backward()
        assert h.grad[:, :, 0].tolist() == [[0.0, 1.0, 0.0, 10.0, 0.0], [11.0, 0.0, 0.0, 0.0, 0.0]]
    # ... and through reduce_bucketed on a graph: three equal messages into node 0, edges in the order of sources 2, 0, 1
    src, dst = torch.tensor([2, 0, 1]), torch.tensor([0, 0, 0])
    x = torch.ones(3, 1, dtype=torch.float64, requires_grad=True)
    O.reduce_bucketed(x[src], src, dst, 3, ["max"], ["identity"], torch.tensor(1.0)).sum().backward()
    assert x.grad.flatten().tolist() == [0.0, 0.0, 1.0]                                     # the first EDGE (source 2), not the first node


@pytest.mark.parametrize("D", C.RANK_DEGREES)
@pytest.mark.parametrize("terms", [False, True])
def test_rank_cases_plant_the_extrema_at_the_ranks_they_name(D, terms):
    c = C.case(f"rank{D}", 1, 8, "A", terms)
    rowptr, col, row, pos = C.csr_order(c.src, c.dst, c.V)
    assert int(rowptr[0]) == 0 and int(rowptr[1]) == D and c.V == D + 40
    m = c.x[col[:D]] + (c.dt[0] if terms else 0)
    assert all(torch.unique(m[:, f]).numel() == D for f in range(8))                         # no ties in the hub row
    assert m.argmax(0).tolist() == [D - 1] * 4 + [32767] * 4 and m[:, 4:].argmin(0).tolist() == [32768] * 4
    assert Graph(c.src, c.dst, c.V).csr.max_degree == D
    _, support = C.support_case(f"rank{D}", 1, 8, "A", terms)
    assert bool(support[col[D - 1], :4].all()) and bool(support[col[32767], 4:].all()) and bool(support[col[32768], 4:].all())


def test_mirror_case_is_one_hub_source():
    c = C.case("mirror", 1, 8, "A", False)
    assert int(torch.bincount(c.src, minlength=c.V)[0]) == C.MIRROR_DEGREE and int(torch.bincount(c.dst, minlength=c.V)[1:C.MIRROR_DEGREE].max()) == 1


@pytest.mark.parametrize("T,F", C.TIES)
def test_tie_cases_plant_their_ties_at_the_hub_destination(T, F):
    c = C.case("ties", T, F, "B", True)
    rowptr, col, _, _ = C.csr_order(c.src, c.dst, c.V)
    m = c.x[col[:int(rowptr[1])]] + c.dt[0]
    TF = T * F
    assert bool((c.x * 4 == (c.x * 4).round()).all()) and bool((c.dt * 4 == (c.dt * 4).round()).all()) and float(c.x.abs().max()) <= 1
    assert torch.unique(m[:, 0]).numel() == 1                                               # constant: max and min belong to the first edge
    for col_, sign in ((1, 1.0), (TF - 1, -1.0)):
        top = (sign * m[:, col_]).max()
        assert torch.nonzero(sign * m[:, col_] == top).flatten().tolist() == [127, 128]     # the last edge of one segment, the first of the next
    assert SEG_LEN == 128
    # the oracle on node 0's in-edges alone (same edge order): the row's whole max / min gradient in those columns goes to CSR position 0 / 127
    keep = c.dst == 0
    s0 = col[:int(rowptr[1])]
    for which, col_, first in ((("max", "min"), 0, 0), (("max",), 1, 127), (("min",), TF - 1, 127)):
        R = C.only_max_min(c.R, c.aggs, T, F, keep=which)
        _, gx, _ = C.oracle(c.x, c.dt, c.src[keep], c.dst[keep], c.V, c.aggs, T, F, R, torch.float64)
        assert torch.nonzero(gx[:, col_]).flatten().tolist() == [int(s0[first])]


# ---- falsifiers: each planted bug must fail the comparison on the cases written for it ------------------------------------------------
def _fails(fn):
    with pytest.raises(AssertionError):
        fn()


@pytest.mark.parametrize("D", C.RANK_DEGREES)
@pytest.mark.parametrize("terms", [False, True])
def test_falsifier_signed_16_bit_ranks_fail_the_rank_boundary_cases(D, terms):
    c = C.case(f"rank{D}", 1, 8, "A", terms)
    R, support = C.support_case(f"rank{D}", 1, 8, "A", terms)
    C.same_support(C.pull_model(c, R)[0], support, "model")                                  # sound with the switch off ...
    bad = C.pull_model(c, signed_ranks=True)
    _fails(lambda: C.check(c, *bad, "signed ranks"))                                         # ... and both checks see the planted bug
    _fails(lambda: C.same_support(C.pull_model(c, R, signed_ranks=True)[0], support, "signed ranks"))
    assert torch.equal(bad[1], C.pull_model(c)[1])                                           # (grad_dst does not go through the ranks)


@pytest.mark.parametrize("T,F", C.TIES)
@pytest.mark.parametrize("aggs_key,terms", [("A", False), ("B", True)])
def test_falsifier_last_tied_edge_fails_the_tie_cases(T, F, aggs_key, terms):
    c = C.case("ties", T, F, aggs_key, terms)
    R, support = C.support_case("ties", T, F, aggs_key, terms)
    C.same_support(C.pull_model(c, R)[0], support, "model")
    _fails(lambda: C.check(c, *C.pull_model(c, last_tie=True), "last tie"))
    _fails(lambda: C.same_support(C.pull_model(c, R, last_tie=True)[0], support, "last tie"))


@pytest.mark.parametrize("T,F", [(T, F) for T, F in C.WIDTHS])
def test_falsifier_dropped_tail_window_fails_every_width_that_has_one(T, F):
    c = C.case("general", T, F, "A", False)
    if F % 4:
        _fails(lambda: C.check(c, *C.pull_model(c, drop_tail=True), "dropped tail"))
    else:                                                                                     # (no partial window: the switch changes nothing)
        assert torch.equal(C.pull_model(c, drop_tail=True)[0], C.pull_model(c)[0])


def test_comparison_helpers_at_their_edges():
    z = torch.zeros(3, 2, dtype=torch.float64)
    assert C.rel_err(z.float(), z) == 0.0 and C.rel_err(z.float() + 1e-30, z) == float("inf")
    ref = torch.tensor([[100.0, 0.0]], dtype=torch.float64)
    assert C.close(ref.float() + torch.tensor([[0.0, 0.99e-2]]), ref, "inside") <= 1.0       # per element against the LARGEST entry
    _fails(lambda: C.close(ref.float() + torch.tensor([[0.0, 1.01e-2]]), ref, "outside"))
    _fails(lambda: C.same_support(torch.tensor([[1.0, 0.0]]), torch.tensor([[True, True]]), "missing"))
