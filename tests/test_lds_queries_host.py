"""CPU-side checks of the two host-only tile queries behind the one-call tower layers, pna_tower_layer_lds_bytes (pna_tower_fused.hip) and
pna_tower_layer_bf16_lds_bytes (pna_bf16_small.hip): each answers with the code its entry point sizes the tile with, the Python
predicates (functional.small_tower_fits, ops.tower_layer_bf16_lds_bytes) only ask them, and the formulas below are the tests' own."""
import os

from pna_amd import _lib, functional as PF, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 160 * 1024


def _tower_tile_bytes(T, Fi, Fo, divided, No=None):
    """The fp32 tile at one tower per pass: 16 rows of the aggregates, of the own features (per tower when the input is divided) and of
    the concatenated outputs on pitches of 16 quads + 4, 16 work items of 256 floats, three per-column vectors, the mixing bias and 64
    row scalars."""
    quads = lambda k: (k + 15) // 16   # noqa: E731
    No = T * Fo if No is None else No
    floats = 16 * (quads(4 * Fi) * 16 + 4) + (T if divided else 1) * 16 * (quads(Fi) * 16 + 4) + 16 * (quads(T * Fo) * 16 + 4) + \
        16 * 256 + 3 * quads(T * Fo) * 16 + quads(No) * 16 + 64
    return floats * 4


def _bf16_tile_bytes(T, Fi, Fo, A, divided, No=None, no_self_panel=False):
    """The bf16 tile: 16 rows of the aggregates of every tower, the own features, and the concatenated outputs with a mixing network."""
    r = lambda x, m: (x + m - 1) // m * m   # noqa: E731
    la = T * r(A * r(Fi, 8), 32) + 8
    lh = 0 if no_self_panel else (T if divided else 1) * r(Fi, 32) + 8
    lc = 0 if No is None else r(T * Fo, 32) + 8
    return 16 * (la + lh + lc) * 2


def test_symbols_are_exported_and_declared():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "pna_amd.h")).read()
    assert "23, additive: + pna_gru_cell_in_scope, pna_tower_layer_lds_bytes, pna_tower_layer_bf16_lds_bytes" in header
    for name in ("pna_tower_layer_lds_bytes", "pna_tower_layer_bf16_lds_bytes"):
        assert hasattr(L, name) and f"int64_t {name}(" in header, name


def test_small_tower_fits_is_the_fp32_tile_within_the_budget():
    L = _lib.lib()
    seen = set()
    for T in range(1, 9):
        for Fi in (1, 4, 16, 75, 128, 129, 300):
            for Fo in (1, 15, 16, 128):
                for divided in (False, True):
                    for No in (None, 75):
                        want = _tower_tile_bytes(T, Fi, Fo, divided, No)
                        assert L.pna_tower_layer_lds_bytes(T, Fi, Fo, No or 0, divided) == want, (T, Fi, Fo, divided, No)
                        assert PF.small_tower_fits(T, Fi, Fo, divided, No) == (want <= BUDGET), (T, Fi, Fo, divided, No)
                        seen.add(want <= BUDGET)
    assert seen == {True, False}


def test_bf16_tile_bytes_are_the_entry_points():
    L = _lib.lib()
    for T, Fi, Fo, A in ((1, 1, 1, 1), (5, 75, 15, 4), (5, 300, 15, 4), (8, 64, 16, 6), (3, 33, 3, 2), (1, 512, 128, 4), (4, 20, 20, 8)):
        for divided in (False, True):
            for No in (None, 75):
                want = _bf16_tile_bytes(T, Fi, Fo, A, divided, No)
                assert L.pna_tower_layer_bf16_lds_bytes(T, Fi, Fo, A, divided, No or 0, 0) == want, (T, Fi, Fo, A, divided, No)
                assert ops.tower_layer_bf16_lds_bytes(T, Fi, Fo, A, divided, No=No) == want
        want = _bf16_tile_bytes(1, Fi, Fo, A, False, no_self_panel=True)
        assert ops.tower_layer_bf16_lds_bytes(1, Fi, Fo, A, False, no_self_panel=True) == want


def test_widths_below_one_have_no_tile():
    L = _lib.lib()
    assert L.pna_tower_layer_lds_bytes(5, 75, 15, 75, 0) > 0 and L.pna_tower_layer_bf16_lds_bytes(5, 75, 15, 4, 0, 75, 0) > 0
    for bad in ((0, 75, 15, 75), (-1, 75, 15, 75), (5, 0, 15, 75), (5, -4, 15, 75), (5, 75, 0, 75), (5, 75, -15, 75), (5, 75, 15, -1)):
        assert L.pna_tower_layer_lds_bytes(*bad, 0) == -1 == L.pna_tower_layer_lds_bytes(*bad, 1), bad
        assert not PF.small_tower_fits(*bad[:3], False, bad[3])
    for bad in ((0, 75, 15, 4, 0, 75), (5, 0, 15, 4, 0, 75), (5, -8, 15, 4, 1, 75), (5, 75, 0, 4, 0, 75), (5, 75, 15, 0, 0, 75), (5, 75, 15, -2, 0, 0),
                (5, 75, 15, 4, 0, -1)):
        assert L.pna_tower_layer_bf16_lds_bytes(*bad, 0) == -1, bad
