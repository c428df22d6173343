"""The backward of the segment-reduce aggregation at its width, degree and tie edges: pna_segreduce_bwd_f32, _rowprep_f32, _argscatter_f32,
_pull_f32 (per-edge rows, packed ranked rows, separate ranks) and the router autograd._backward_pull against float64 CPU autograd through
the oracle (aggregate_bwd_cases.py: the cases, the bar |got - ref64| <= 1e-4 max|ref64| per element with no carve-out, and why the
upstream gradient is zero on the std / var blocks of the ill-conditioned destinations).  Every case asserts WHICH entry points ran -- a
test that silently took another route fails --, and which of the three ranked pulls the pull entry ran as.

Worst |got - ref64| as a fraction of the bar, measured on an MI355X on the first run (a record, not a bar derived from the code):
  1. widths: default 0.037 (T=3 F=4), packed rows 0.026, separate ranks 0.037, sums-only pull + argscatter 0.048 (T=1 F=4), scatter 0.035;
     outside the ranked pull 0.100 (T=3 F=2); the sorted max / min sum at F >= 4 0.026
  2. bit identity (no hub sources): 0.085 on each of the three ranked pulls (T=1 F=128) -- the same bits
  3. row pitch 0.034 (default) / 0.033 (scatter); extra columns 0.034 / 0.033 (T=1 F=75 with a destination term)
  4. rank boundary 0.019 (D = 65534, all three ranked pulls), the fall-back at D = 65535 0.012; hub source of 65534 out-edges 0.004
  5. ties: 0.004 (ranked pulls), 0.005 (argscatter), 0.006 (scatter); the support of grad_x equals the oracle's on every route
  6. degenerate graphs 0.001.  The graph without edges raised on the default route (pna_segreduce_bwd_pull_f32 refuses null index arrays)
     until autograd._backward_pull returned its zero gradients without a launch.
"""
import pytest
import torch

import aggregate_bwd_cases as C
from pna_amd import Graph, autograd as AG, functional as PF

pytestmark = pytest.mark.gpu

PULL, ROWPREP, ARGSCATTER, SCATTER = C.ENTRIES
RANKED = ("default", "packed_rows", "separate_rows")
_id = lambda k: "-".join(str(v) for v in k)           # noqa: E731


class _Recorder:
    """Which backward entry points ran (autograd._lib.check receives each one's name), how the pull entry was called, and whether the
    sorted (deterministic) max / min sum ran."""

    def __init__(self, monkeypatch):
        self.names, self.pulls, self.sorted = [], [], 0
        AG._lib.lib()                                          # (loaded, its prototypes bound to the real struct classes, before one is wrapped)
        real_check, real_args, real_sorted = AG._lib.check, AG._lib.PnaSegreduceBwdPullArgs, AG._argscatter_sorted

        def check(rc, what):
            self.names.append(what)
            return real_check(rc, what)

        def pull_args():
            q = real_args()
            self.pulls.append(q)
            return q

        def sorted_sum(*a, **k):
            self.sorted += 1
            return real_sorted(*a, **k)
        monkeypatch.setattr(AG._lib, "check", check)
        monkeypatch.setattr(AG._lib, "PnaSegreduceBwdPullArgs", pull_args)
        monkeypatch.setattr(AG, "_argscatter_sorted", sorted_sum)

    def entries(self):
        return {n for n in self.names if n in C.ENTRIES}

    def pull_kind(self, TF):
        assert len(self.pulls) == 1, len(self.pulls)
        q = self.pulls[0]
        if q.edge_rows:
            return "edge_rows"
        packed = q.run_rowprep and q.ld_table >= 5 * TF and q.ranks == q.table + 16 * TF
        return "packed_rows" if packed else "separate_rows"


def _select(monkeypatch, route, deterministic=False):
    for k in ("PNA_AMD_BWD", "PNA_AMD_BWD_ARGS", "PNA_AMD_BWD_DETERMINISTIC"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(AG, "PULL_EDGE_ROWS", route not in ("packed_rows", "separate_rows"))
    monkeypatch.setattr(AG, "PULL_PACKED", route != "separate_rows")
    if route == "args_scatter":
        monkeypatch.setenv("PNA_AMD_BWD_ARGS", "scatter")
    if route == "scatter":
        monkeypatch.setenv("PNA_AMD_BWD", "scatter")
    if deterministic:
        monkeypatch.setenv("PNA_AMD_BWD_DETERMINISTIC", "1")


def _expect(rec, c, route, deterministic=False, ranked_applies=True):
    """The entry points of `route` for case c, and nothing else of the family."""
    edge_rows = c.T == 1 and not c.terms and set(c.aggs) == {"mean", "max", "min", "std"}
    if route == "scatter":
        want = {SCATTER}
    elif route in RANKED and ranked_applies:
        want = {PULL}
        kind = rec.pull_kind(c.T * c.F)
        assert kind == ("edge_rows" if route == "default" and edge_rows else "separate_rows" if route == "separate_rows" else "packed_rows"), kind
    else:                                                     # the sums-only pull: rowprep, then the max / min terms by atomics or by the sorted sum
        by_sort = c.F < 4 or deterministic
        want = {ROWPREP} if by_sort else {ROWPREP, ARGSCATTER}
        assert rec.sorted == (1 if by_sort else 0), rec.sorted
    assert rec.entries() == want, (rec.entries(), want)
    if PULL not in want:
        assert not rec.pulls


def _run(dev, monkeypatch, c, route, R=None, deterministic=False, layout="plain", graph=None):
    """-> (grad_x, grad_dst, recorder, graph) of the device route on case c."""
    _select(monkeypatch, route, deterministic)
    rec = _Recorder(monkeypatch)
    g = Graph(c.src, c.dst, c.V).to(dev) if graph is None else graph
    TF = c.T * c.F
    if layout == "pitch":                                     # a row pitch with stride(1) == 1
        xg = torch.full((c.V, TF + 5), float("nan"), device=dev)[:, :TF]
        xg.copy_(c.x)
        assert xg.stride() == (TF + 5, 1)
    elif layout == "extra":                                   # x wider than T F: the gradient of the extra columns is zero
        xg = torch.cat([c.x, torch.randn(c.V, 3, generator=torch.Generator().manual_seed(5))], dim=1).to(dev)
    else:
        xg = c.x.to(dev)
    xg.requires_grad_(True)
    dg = c.dt.to(dev).requires_grad_(True) if c.terms else None
    amp, att = g.degree_scalers(C.AVG_LOG)
    out = PF.aggregate(g, xg, c.F, c.aggs, n_tower=c.T, dst_term=dg, row_scales=[None, amp, att])
    (out * (c.R if R is None else R).to(dev)).sum().backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    return xg.grad, (dg.grad if c.terms else None), rec, g


# ---- 1. widths, every route, against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,F,route,aggs_key,terms", C.width_cases(), ids=list(map(_id, C.width_cases())))
def test_widths_on_every_route_against_float64(cuda_device, monkeypatch, T, F, route, aggs_key, terms):
    c = C.case("general", T, F, aggs_key, terms)
    gx, gd, rec, _ = _run(cuda_device, monkeypatch, c, route)
    _expect(rec, c, route)
    C.check(c, gx, gd, f"widths {route} T={T} F={F} {aggs_key} terms={terms}")
    assert torch.equal(gx[-3:], torch.zeros_like(gx[-3:]))    # no out-edges: no gradient


@pytest.mark.parametrize("T,F,deterministic,aggs_key,terms", C.outside_cases(), ids=list(map(_id, C.outside_cases())))
def test_widths_outside_the_ranked_pull_fall_back_and_match_float64(cuda_device, monkeypatch, T, F, deterministic, aggs_key, terms):
    c = C.case("general", T, F, aggs_key, terms)
    gx, gd, rec, _ = _run(cuda_device, monkeypatch, c, "default", deterministic=deterministic)
    _expect(rec, c, "default", deterministic, ranked_applies=False)                            # (asserts that the pull entry was NOT called)
    C.check(c, gx, gd, f"outside T={T} F={F} {aggs_key} terms={terms} deterministic={deterministic}")


@pytest.mark.parametrize("T,F,aggs_key,terms", C.DETERMINISTIC_INSIDE, ids=list(map(_id, C.DETERMINISTIC_INSIDE)))
def test_sorted_max_min_sum_inside_the_ranked_widths(cuda_device, monkeypatch, T, F, aggs_key, terms):
    """PNA_AMD_BWD_DETERMINISTIC=1 at F >= 4: autograd._argscatter_sorted behind the sums-only pull (which PNA_AMD_BWD_ARGS=scatter selects;
    with the ranked pull in charge there are no atomics to order and the switch has nothing to do)."""
    c = C.case("general", T, F, aggs_key, terms)
    gx, gd, rec, _ = _run(cuda_device, monkeypatch, c, "args_scatter", deterministic=True)
    _expect(rec, c, "args_scatter", deterministic=True)
    C.check(c, gx, gd, f"sorted T={T} F={F} {aggs_key} terms={terms}")
    gx2, gd2, rec2, _ = _run(cuda_device, monkeypatch, c, "default", deterministic=True)     # the switch alone leaves the ranked pull in charge
    _expect(rec2, c, "default", deterministic=True)
    C.check(c, gx2, gd2, f"sorted (ranked pull) T={T} F={F} {aggs_key} terms={terms}")


# ---- 2. bit identity between the ranked routes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,F", C.IDENTITY, ids=list(map(_id, C.IDENTITY)))
def test_ranked_routes_are_bit_identical_without_hub_sources(cuda_device, monkeypatch, T, F):
    """pna_segreduce_bwd.hip: the per-edge-rows pull does "the same additions in the same order as the ranked pull: bit-identical
    gradients".  On a graph whose out-degrees stay below the heavy threshold nothing is added atomically, so the three ranked pulls must
    agree bit for bit, and each with itself from run to run."""
    res = {}
    for terms in (False, True):
        c = C.case("nohub", T, F, "A", terms)
        for route in RANKED:
            for rep in range(2):
                gx, gd, rec, g = _run(cuda_device, monkeypatch, c, route)
                _expect(rec, c, route)
                assert g._pna_amd_transposed.heavy_schedule().n_heavy == 0
                C.check(c, gx, gd, f"identity {route} T={T} F={F} terms={terms}")
                res[terms, route, rep] = (gx, gd)
            assert torch.equal(res[terms, route, 0][0], res[terms, route, 1][0]), (route, terms, "grad_x differs between two runs")
        for route in RANKED[1:]:
            assert torch.equal(res[terms, route, 0][0], res[terms, "default", 0][0]), (route, terms, "grad_x differs between the ranked routes")
        if terms:
            assert torch.equal(res[terms, "packed_rows", 0][1], res[terms, "separate_rows", 0][1]) and torch.equal(res[terms, "packed_rows", 0][1], res[terms, "default", 1][1])


# ---- 3. pitches and extra columns ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["default", "scatter"])
@pytest.mark.parametrize("terms", [False, True])
@pytest.mark.parametrize("T,F", C.PITCH, ids=list(map(_id, C.PITCH)))
def test_row_pitch_and_extra_columns_of_x(cuda_device, monkeypatch, T, F, terms, route):
    c = C.case("general", T, F, "A", terms)
    gx, gd, rec, _ = _run(cuda_device, monkeypatch, c, route, layout="pitch")
    _expect(rec, c, route)
    C.check(c, gx, gd, f"pitch {route} T={T} F={F} terms={terms}")
    gx, gd, rec, _ = _run(cuda_device, monkeypatch, c, route, layout="extra")
    _expect(rec, c, route)
    assert tuple(gx.shape) == (c.V, T * F + 3) and torch.equal(gx[:, T * F:], torch.zeros_like(gx[:, T * F:]))
    C.check(c, gx[:, :T * F], gd, f"extra columns {route} T={T} F={F} terms={terms}")


# ---- 4. the 16-bit rank boundary ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,terms", [("default", False), ("packed_rows", False), ("separate_rows", False), ("default", True)])
@pytest.mark.parametrize("D", C.RANK_DEGREES)
def test_rank_boundary(cuda_device, monkeypatch, D, route, terms):
    """The max at the hub row's LAST position (rank D - 1; columns 0-3), the min at rank 32768 = 0x8000 and the max at 32767 (columns 4-7);
    D = 65534 is the last in-degree the 16-bit ranks admit (0xFFFF: none), at D = 65535 the router must leave the ranked pull and still be
    right."""
    c = C.case(f"rank{D}", 1, 8, "A", terms)
    R_mm, support = C.support_case(f"rank{D}", 1, 8, "A", terms)
    g = None
    for R, what in ((None, "full R"), (R_mm, "R on max / min")):
        gx, gd, rec, g = _run(cuda_device, monkeypatch, c, route, R=R, graph=g)
        assert g.csr.max_degree == D
        _expect(rec, c, route, ranked_applies=D < 65535)
        if R is None:
            C.check(c, gx, gd, f"rank D={D} {route} terms={terms}")
        else:
            C.same_support(gx, support, f"rank D={D} {route} terms={terms}")                  # exact: needs no tolerance


def test_rank_boundary_mirror_hub_source(cuda_device, monkeypatch):
    """Node 0 SENDS to 65534 distinct destinations: one source row of the ranked pull cut into 512 segments that add atomically."""
    c = C.case("mirror", 1, 8, "A", False)
    for route in RANKED:
        gx, gd, rec, g = _run(cuda_device, monkeypatch, c, route)
        _expect(rec, c, route)
        assert g._pna_amd_transposed.csr.max_degree == C.MIRROR_DEGREE
        C.check(c, gx, gd, f"mirror {route}")


# ---- 5. ties: the first extremal edge wins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", C.ROUTES)
@pytest.mark.parametrize("aggs_key,terms", [("A", False), ("B", True)])
@pytest.mark.parametrize("T,F", C.TIES, ids=list(map(_id, C.TIES)))
def test_ties_go_to_the_first_extremal_edge(cuda_device, monkeypatch, T, F, aggs_key, terms, route):
    """Features on the grid of multiples of 1/4 (ties are exact in fp32 and float64), a constant column and an extremum shared by CSR positions
    127 | 128 (two forward segments) at hub destination 0: the float64 oracle sends a tied max / min to the first index of the mailbox, which
    is the CSR order once csr.eid increases inside every row."""
    c = C.case("ties", T, F, aggs_key, terms)
    R_mm, support = C.support_case("ties", T, F, aggs_key, terms)
    g = None
    for R, what in ((None, "full R"), (R_mm, "R on max / min")):
        gx, gd, rec, g = _run(cuda_device, monkeypatch, c, route, R=R, graph=g)
        if R is None:
            csr = g.csr
            assert bool((csr.eid[1:] > csr.eid[:-1])[csr.row[1:] == csr.row[:-1]].all())
            assert torch.equal(csr.col.cpu().long(), C.csr_order(c.src, c.dst, c.V)[1])
        _expect(rec, c, route)
        if R is None:
            C.check(c, gx, gd, f"ties {route} T={T} F={F} {aggs_key} terms={terms}")
        else:
            C.same_support(gx, support, f"ties {route} T={T} F={F} {aggs_key} terms={terms}")


# ---- 6. degenerate graphs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["default", "scatter"])
@pytest.mark.parametrize("kind", ["empty", "selfloop", "degree1"])
def test_degenerate_graphs(cuda_device, monkeypatch, kind, route):
    """V = 5 without edges, one node with a self-loop, every node of in-degree 1 (variance 0: the std gradient is 0 in both precisions):
    ordinary inputs -- no route may raise or refuse a launch on them."""
    c = C.case(kind, 1, 8, "A", False)
    gx, gd, rec, _ = _run(cuda_device, monkeypatch, c, route)
    if kind == "empty":
        assert rec.entries() == (set() if route == "default" else {SCATTER})                   # (the router has nothing to pull without an edge)
    else:
        _expect(rec, c, route)
    C.check(c, gx, gd, f"degenerate {kind} {route}")
    assert torch.equal(gx.cpu() == 0, c.gx64 == 0)                                             # zeros exactly where the oracle has zeros
