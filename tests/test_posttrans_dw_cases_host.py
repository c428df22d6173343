"""Host half of the weight-gradient edge cases (posttrans_dw_cases.py): the tables hit every edge they claim, the builder's asserts hold,
the clean numpy model of the kernels' data path is inside the bar on every case (the inputs were chosen so that the reference alone
passes) and equals float64 bit for bit on the integer cases, and the bar and the bit comparison BITE -- the model with one defect at a
time leaves them on a case named here."""
import numpy as np
import pytest

import posttrans_dw_cases as C


@pytest.fixture(scope="module")
def plain():
    return C.plain_cases(host_only=True)


@pytest.fixture(scope="module")
def grouped():
    return C.grouped_cases()


def _ratio(got, r):
    gw, gb = got
    worst = C.worst_ratio(gw, r["gw"], r["floor_w"])[0]
    if gb is not None:
        worst = max(worst, C.worst_ratio(gb, r["gb"], r["floor_b"])[0])
    return worst


def _bits(got, r):
    gw, gb = got
    return C.same_bits(gw, r["gw"]) and (gb is None or C.same_bits(gb, r["gb"]))


def _fails(c, got, r):
    """The check the GPU module applies to the case: the bar, and for an integer case the bit comparison."""
    return _ratio(got, r) > 1.0 or (c["variant"] == "int" and not _bits(got, r))


def test_every_edge_is_hit_by_a_case(plain, grouped):
    hit = C.edges_hit(plain, grouped)
    # every edge but the wide ones by a case the kernel RUNS; (240, 1) and N = 129, 200, 240 with one scaler are the refused shapes
    assert set(C.EDGES_N) <= hit["N"] and set(C.EDGES_N_S1_WIDE) == hit["N_wide"]
    assert set(C.EDGES_SN240) - {(240, 1)} <= hit["SN240"] and hit["SN240_refused"] == {(240, 1)} and hit["slabs"] == {1, 2, 3}
    only_gpu = C.edges_hit(C.plain_cases(), grouped)               # the GPU module's own case set reaches the same edges
    assert all(only_gpu[k] == hit[k] for k in ("N", "SN240", "SN240_refused", "N_wide", "R", "M", "slabs", "scalers"))
    assert set(C.EDGES_R) <= hit["R"] and set(C.EDGES_M) <= hit["M"] and set(C.EDGES_SCALERS) <= hit["scalers"]
    assert set(C.EDGES_GROUPED_N) <= hit["gN"] and set(C.EDGES_GROUPED_R) <= hit["gR"] and hit["gS"] == {1, 2, 3}
    assert set(C.EDGES_ENTRIES) <= hit["entries"] and set(C.EDGES_WORKGROUPS) <= hit["wgs"]
    assert {"pow2", "int", "h panel across a third boundary", "h panel behind a K that is no multiple of 64", "one tile in one group",
            "group order A, B, A", "a run cut across two workgroups", "a workgroup range with three group changes", "empty workgroup ranges",
            "a tile whose first row is padding", "padding in the middle of a tile", "a tile that is all padding",
            "nodes that no virtual row names"} <= hit["flags"]
    # R = 2 is K = 1 without an h panel; the ones column is the last slot of a third (R = 128, 256, 384) and the first of the next (129, 257)
    assert any(c["K"] == 1 and c["Kh"] == 0 for c in plain.values())
    assert max(c["M"] for c in plain.values()) <= 600
    assert all(len(c["tiles"]) <= 12 or c["n_entries"] == 17 for c in grouped.values())      # (17 entries cannot come from 12 tiles)


def test_builder_asserts(plain, grouped):
    for name, c in plain.items():
        assert c["slabs"] == (c["M"] + C.SLAB_ROWS - 1) // C.SLAB_ROWS, name
        assert c["refused"] == (c["N"] > 128), name
        assert (c["scales"][0] is None) == c["bias"], name
    assert {c["slabs"] for c in plain.values() if not c["refused"]} == {1, 2, 3}
    assert {n for n, c in plain.items() if c["refused"]} - set(C.plain_cases()) == {"m40_n129/int", "m40_n240_s1/int"}      # host only
    for name, c in grouped.items():
        lit = C.tables_literal(c["tile_group"], c["n_wg"])
        der = C.tables_derived(c["tile_group"], c["n_wg"])
        on = lit[0][:, 1] > lit[0][:, 0]
        assert np.array_equal(lit[0], der[0]) and np.array_equal(lit[2], der[2]) and np.array_equal(lit[1][on], der[1][on]), name
        assert c["n_entries"] == lit[2].size and c["row_perm"].size == C.TILE * c["tile_group"].size, name
        live = c["row_perm"][c["row_perm"] >= 0]
        assert np.unique(live).size == live.size and live.min() >= 1 and live.max() < c["n_nodes"], name
        assert np.isnan(c["gy"][~c["named"]]).all() and np.isfinite(c["gy"][c["named"]]).all(), name
        assert np.isnan(C.a_in_plan_order(c)[c["row_perm"] < 0]).all(), name
    for c in list(plain.values()) + list(grouped.values()):         # (make_plain / make_grouped assert it while they build)
        if c["variant"] == "int":
            r = C.ref_plain(c) if "M" in c else C.ref_grouped(c)
            assert max(r["floor_w"].max(), r["floor_b"].max()) < 2.0 ** 24, c["name"]


def test_derived_tables_are_the_plan_builders():
    """tables_derived() is DegreePlan.dw_tables: the same arrays on a tile list with runs, for every grid of the table."""
    torch = pytest.importorskip("torch")
    from pna_amd import degree_groups as DG
    tg = np.array([0, 0, 1, 1, 1, 2, 0, 0, 3, 3, 3, 3], np.int32)
    plan = DG.DegreePlan.__new__(DG.DegreePlan)
    plan.perm = torch.zeros(C.TILE * tg.size, dtype=torch.int32)
    plan.NV = C.TILE * tg.size
    plan.tile_image = torch.from_numpy(tg)
    assert DG.TILE == C.TILE
    for n_wg in (1, 2, 3, 5, 7, 12, 20):
        plan.__dict__.pop("_dw_tables", None)
        t, wr, we, eg, ne = plan.dw_tables(n_wg)
        d = C.tables_derived(tg, n_wg)
        assert np.array_equal(wr.numpy(), d[0]) and np.array_equal(we.numpy(), d[1]) and np.array_equal(eg.numpy(), d[2]) and ne == d[2].size


def test_clean_model_is_inside_the_bar_on_every_case(plain, grouped):
    for name, c in plain.items():
        r = C.ref_plain(c)
        got = C.model_dw(c)
        ratio = _ratio(got, r)
        print(f"[dw cases] plain {name}: clean model worst err / bar = {ratio:.4f}")
        assert ratio <= 1.0, name
        assert c["variant"] != "int" or (_bits(got, r) and ratio == 0.0), name
    for name, c in grouped.items():
        r = C.ref_grouped(c)
        for a_plan in (False, True):
            got = C.model_dw_grouped(c, a_plan=a_plan)
            ratio = _ratio(got, r)
            print(f"[dw cases] grouped {name} a_plan_order={int(a_plan)}: clean model worst err / bar = {ratio:.4f}")
            assert ratio <= 1.0, name
            assert c["variant"] != "int" or (_bits(got, r) and ratio == 0.0), name


# the case on which each defect must be caught
PLAIN_CAUGHT_ON = {"gy_columns_from_128_not_staged": "m40_n240_s1/int", "last_partial_step_dropped": "m33_n65_r383/int",
                   "third_split_term_dropped": "m255_n127_r384", "padding_rows_not_masked": "m257_n80_s3/int",
                   "ones_column_off_by_one": "m8_n16_r128/int"}
GROUPED_CAUGHT_ON = {"third_split_term_dropped": "three_changes", "no_flush_on_group_change": "aba/int",
                     "entry_scaled_by_wrong_group": "aba/int", "padding_rows_not_masked": "mixed7_wg3/int",
                     "ones_column_off_by_one": "alt9/int"}


@pytest.mark.parametrize("defect", C.PLAIN_DEFECTS)
def test_each_defect_of_the_plain_model_is_caught(plain, defect):
    caught = [name for name, c in plain.items() if _fails(c, C.model_dw(c, defect), C.ref_plain(c))]
    print(f"[dw cases] plain defect {defect}: caught on {caught}")
    assert PLAIN_CAUGHT_ON[defect] in caught, (defect, caught)
    if defect == "gy_columns_from_128_not_staged":                   # exactly the cases wider than the two staged column blocks
        assert set(caught) == {n for n, c in plain.items() if c["N"] > 128}
        gw, gb = C.model_dw(plain["m40_n240_s1"], defect)
        assert not gw[128:].any() and not gb[128:].any() and gw[:128].any()


@pytest.mark.parametrize("defect", C.GROUPED_DEFECTS)
def test_each_defect_of_the_grouped_model_is_caught(grouped, defect):
    caught = []
    for name, c in grouped.items():
        r = C.ref_grouped(c)
        # workspace at 0: the bar itself must catch the defect, not only the NaN of an entry nobody wrote
        if any(_fails(c, C.model_dw_grouped(c, a_plan=ap, defect=defect, workspace_fill=0.0), r) for ap in (False, True)):
            caught.append(name)
    print(f"[dw cases] grouped defect {defect}: caught on {caught}")
    assert GROUPED_CAUGHT_ON[defect] in caught, (defect, caught)


def test_split_is_exact_and_truncating():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(4096) * np.exp2(rng.integers(-30, 30, 4096))).astype(np.float32)
    t0, t1, t2 = C.split3(x)
    assert np.array_equal(t0.astype(np.float64) + t1.astype(np.float64) + t2.astype(np.float64), x.astype(np.float64))
    for t in (t0, t1, t2):
        assert not (t.view(np.uint32) & 0xFFFF).any()
    assert (np.abs(t0) <= np.abs(x)).all() and (np.sign(t1) * np.sign(x) >= 0).all()
