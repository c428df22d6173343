"""Cases, float64 references, the per-element bar and a numpy model of pna_posttrans_dw_f32 / pna_posttrans_dw_grouped_f32
(include/pna_amd.h, pna_amd/csrc/pna_posttrans_dw.hip) -- no GPU needed.

Reference: the header's three formulas in float64 from the fp32 operands,
    grad_w[n, Kh + s K + k] = sum_m scale_s[m] gy[m, n] a[m, k]     grad_w[n, j < Kh] = sum_m gy[m, n] h[m, j]     grad_b[n] = sum_m gy[m, n]
(grouped form: m runs over the LIVE virtual rows, scale_s[m] = group_scale[tile_group[m / 128]][s] on the scaler blocks only).
Bar: the project's own (test_gpu_backward.py::test_posttrans_weight_gradient_kernel), per element, for grad_w and grad_b alike:
    |got - ref64| <= 1e-5 |ref64| + 2^-22 sum_m |terms|
PLAIN_TABLE holds one case per edge of the plain kernel's shapes (N against the 16-column tiles and the two 64-column conversion blocks,
R = K + Kh + 1 against the thirds of 128, M against the 8-row groups, the 32-row steps and the 256-row slabs, every scaler layout) with
the smallest M that reaches the edge; `variants` repeats a few shapes with every column on its own power of two and with small integers,
where every sum is exact in fp32 and the result must equal the float64 one BIT FOR BIT.  GROUPED_PLANS spells the degree plan out tile by
tile -- (group, live-row pattern) per 128-row tile and a grid size -- and tables_literal() builds the five tables after the header's text;
tables_derived() is DegreePlan.dw_tables in numpy, and every plan asserts that the two agree.
model_dw() / model_dw_grouped() follow the kernels' data path over the TABLES (truncating three-term bf16 split, six partial products,
fp32 sum per slab / entry, float64 across them, scatter into the weight layout) with one switchable defect at a time: the host module
proves with them that the bar and the bit comparison bite."""
import numpy as np

CANARY = np.array([0xCAFEBABE], dtype=np.uint32).view(np.float32)[0]
SLAB_ROWS = 256                       # plan() of the kernel file: rows per slab at every M of this table, whatever the CU count
SLAB_BYTES = 240 * 384 * 4            # one partial product [240][384] fp32 per slab
ENTRY_BYTES = 80 * 384 * 4            # grouped form: one [80][384] fp32 per workspace entry
TILE = 128                            # rows of a degree-plan tile
MAX_N_PLAIN = 128                     # widest gy the plain kernel stages (two conversion blocks of 64 columns): wider shapes are refused

# ---- the edges every table below must hit (test_posttrans_dw_cases_host.py asserts it) --------------------------------------------------
EDGES_N = (1, 15, 16, 17, 63, 64, 65, 127, 128)
EDGES_SN240 = ((80, 3), (120, 2), (240, 1))
EDGES_N_S1_WIDE = (129, 200, 240)
EDGES_R = (2, 127, 128, 129, 256, 257, 383, 384)
EDGES_M = (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 288, 513)
EDGES_SCALERS = ("x", "x1", "x12", "12", "1")
EDGES_GROUPED_N = (1, 16, 17, 64, 65, 80)
EDGES_GROUPED_R = (2, 65, 321, 384)
EDGES_ENTRIES = (1, 7, 8, 9, 17)
EDGES_WORKGROUPS = (1, 2, 3, 5)

#             name                  M    N    K   Kh  scalers  slabs
PLAIN_TABLE = [("m1_n1_r2",          1,   1,   1,   0, "x",   1),
               ("m7_n15_r127",       7,  15, 126,   0, "x",   1),
               ("m8_n16_r128",       8,  16, 100,  27, "x1",  1),      # h panel with K no multiple of 64; the ones column ends a third
               ("m9_n17_r129",       9,  17, 128,   0, "x12", 1),      # ... and opens the next one
               ("m31_n63_r256",     31,  63, 200,  55, "x",   1),
               ("m32_n64_r257",     32,  64, 256,   0, "12",  1),
               ("m33_n65_r383",     33,  65, 300,  82, "x1",  1),
               ("m255_n127_r384",  255, 127, 383,   0, "1",   1),
               ("m256_n128_h_straddles", 256, 128, 120, 20, "x", 1),   # the h panel lies across the boundary of the first two thirds
               ("m257_n80_s3",     257,  80,  64,  16, "x12", 2),      # S N = 240; a second slab of ONE row
               ("m288_n120_s2",    288, 120,  40,   7, "x1",  2),      # S N = 240; a second slab of exactly one 32-row step
               ("m513_n100_three_slabs", 513, 100, 33, 5, "x", 3),     # two full slabs and a third of ONE row
               # one scaler, N > 128: wider than the two 64-column blocks the kernel stages.  REFUSED by the library: the GPU module asserts
               # the refusal and runs no kernel on them, so they count for no edge but their own (edges_hit)
               ("m40_n129",         40, 129,  20,   4, "x",   1),
               ("m40_n200",         40, 200,  17,   0, "x",   1),
               ("m40_n240_s1",      40, 240,  33,   5, "x",   1)]      # S N = 240 the third way
PLAIN_VARIANTS = {"pow2": ("m33_n65_r383", "m256_n128_h_straddles", "m257_n80_s3"),
                  "int": ("m8_n16_r128", "m33_n65_r383", "m255_n127_r384", "m256_n128_h_straddles", "m257_n80_s3", "m288_n120_s2",
                          "m513_n100_three_slabs")}
# integer operands at the refused widths: HOST ONLY -- the model shows on them that unstaged columns 128 .. of gy cannot pass the bit
# comparison; on the GPU there is nothing to compare (plain_cases(host_only=True))
PLAIN_HOST_ONLY_VARIANTS = {"int": ("m40_n129", "m40_n240_s1")}


def bar_of(ref, floor):
    return 1e-5 * np.abs(ref) + 2.0 ** -22 * floor


def worst_ratio(got, ref, floor):
    """(worst |got - ref| / bar, flat index of it); inf for a non-finite entry or an error where the bar is zero."""
    got = np.asarray(got, np.float64)
    err, bar = np.abs(got - ref), bar_of(ref, floor)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bar)
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    if ratio.size == 0:
        return 0.0, 0
    k = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[k]), k


def same_bits(got, ref64):
    """got (fp32) holds exactly the float64 values (integer cases; -0 and +0 are the same value and no integer case can tell them apart)."""
    got = np.asarray(got)
    return got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref64)


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def _operands(rng, rows, N, K, Kh, variant):
    f32 = np.float32
    if variant == "int":
        gy, a = rng.integers(-3, 4, (rows, N)).astype(f32), rng.integers(-3, 4, (rows, K)).astype(f32)
        h = rng.integers(-3, 4, (rows, Kh)).astype(f32) if Kh else None
    else:
        gy = rng.standard_normal((rows, N)).astype(f32)
        a = (rng.standard_normal((rows, K)) * 3.0 + 0.5).astype(f32)
        h = rng.standard_normal((rows, Kh)).astype(f32) if Kh else None
    if variant == "pow2":                                            # every column on its own power of two: the bar is per element
        gy = gy * np.exp2(rng.integers(-20, 21, N)).astype(f32)
        a = a * np.exp2(rng.integers(-20, 21, K)).astype(f32)
        if Kh:
            h = h * np.exp2(rng.integers(-20, 21, Kh)).astype(f32)
    return gy, a, h


def make_plain(name, M, N, K, Kh, scal, slabs, variant="randn", seed=0):
    rng = np.random.default_rng([seed, M, N, K])
    gy, a, h = _operands(rng, M, N, K, Kh, variant)
    if variant == "int":
        amp, att = np.exp2(rng.integers(-1, 2, M)).astype(np.float32), np.exp2(rng.integers(-2, 1, M)).astype(np.float32)
    else:
        amp = (rng.random(M) + 0.5).astype(np.float32)
        att = (np.float32(1.0) / amp).astype(np.float32)
    scales = [{"x": None, "1": amp, "2": att}[ch] for ch in scal]
    c = dict(name=name + ("" if variant == "randn" else "/" + variant), M=M, N=N, S=len(scal), K=K, Kh=Kh, scal=scal, slabs=slabs, variant=variant,
             gy=gy, a=a, h=h, scales=scales, bias=scales[0] is None, refused=N > MAX_N_PLAIN)
    assert c["bias"] or Kh == 0, "the h panel and grad_b need an unscaled first copy of gy"
    assert (M + SLAB_ROWS - 1) // SLAB_ROWS == slabs and M <= 600
    assert c["S"] * N <= 240 and K + Kh + 1 <= 384
    if variant == "int":
        r = ref_plain(c)
        assert max(r["floor_w"].max(), r["floor_b"].max()) < 2.0 ** 24, "every partial sum of an integer case is exact in fp32"
        assert (r["gw"] == np.round(r["gw"] * 4) / 4).all()
    return c


def plain_cases(host_only=False):
    out = {}
    rows = {r[0]: r for r in PLAIN_TABLE}
    for i, r in enumerate(PLAIN_TABLE):
        out[r[0]] = make_plain(*r, seed=i)
    for variant, names in PLAIN_VARIANTS.items():
        assert all(rows[n][2] <= MAX_N_PLAIN for n in names), "a variant of a refused shape belongs to PLAIN_HOST_ONLY_VARIANTS"
        for name in names + (PLAIN_HOST_ONLY_VARIANTS.get(variant, ()) if host_only else ()):
            c = make_plain(*rows[name], variant=variant, seed=100)
            out[c["name"]] = c
    return out


def ref_plain(c):
    g, a = c["gy"].astype(np.float64), c["a"].astype(np.float64)
    blocks, floors = [], []
    if c["Kh"]:
        h = c["h"].astype(np.float64)
        blocks.append(g.T @ h); floors.append(np.abs(g).T @ np.abs(h))
    for rs in c["scales"]:
        gs = g if rs is None else g * rs.astype(np.float64)[:, None]
        blocks.append(gs.T @ a); floors.append(np.abs(gs).T @ np.abs(a))
    return dict(gw=np.concatenate(blocks, axis=1), floor_w=np.concatenate(floors, axis=1), gb=g.sum(0), floor_b=np.abs(g).sum(0))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
PLAIN_DEFECTS = ("gy_columns_from_128_not_staged", "last_partial_step_dropped", "third_split_term_dropped", "padding_rows_not_masked",
                 "ones_column_off_by_one")
GROUPED_DEFECTS = ("third_split_term_dropped", "no_flush_on_group_change", "entry_scaled_by_wrong_group", "padding_rows_not_masked",
                   "ones_column_off_by_one")
_TA, _TB = (2, 1, 0, 1, 0, 0), (0, 1, 2, 0, 1, 0)                    # the six partial products, small ones first


def _top16(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(x):
    """x = t0 + t1 + t2, each the top 16 bits (a bf16) of what the terms before left: by truncation, exact for finite x."""
    with np.errstate(invalid="ignore"):
        x = np.ascontiguousarray(x, np.float32)
        t0 = _top16(x)
        r = x - t0
        t1 = _top16(r)
        t2 = _top16(r - t1)
    return t0, t1, t2


def _step(acc, L, R, defect):
    """acc (fp32) += L^T R over one 32-row step through the six partial products."""
    Lt, Rt = [t.astype(np.float64) for t in split3(L)], [t.astype(np.float64) for t in split3(R)]
    with np.errstate(invalid="ignore", over="ignore"):
        for pa, pb in zip(_TA, _TB):
            if defect == "third_split_term_dropped" and 2 in (pa, pb):
                continue
            acc = (acc.astype(np.float64) + Lt[pa].T @ Rt[pb]).astype(np.float32)
    return acc


def _right(a, h, K, Kh, rows, defect):
    """[a | h | 1 | one spare column] of `rows` rows, fp32: the ones column sits at K + Kh."""
    R = np.zeros((rows, K + Kh + 2), np.float32)
    R[:, :K] = a
    if Kh:
        R[:, K:K + Kh] = h
    R[:, K + Kh + (1 if defect == "ones_column_off_by_one" else 0)] = 1.0
    return R


def _scatter(total, N, S, K, Kh, bias):
    """total (S N, K + Kh + 2) float64 -> grad_w (N, Kh + S K), grad_b (N) in fp32."""
    gw = np.zeros((N, Kh + S * K), np.float32)
    for s in range(S):
        gw[:, Kh + s * K:Kh + (s + 1) * K] = total[s * N:(s + 1) * N, :K].astype(np.float32)
    gw[:, :Kh] = total[:N, K:K + Kh].astype(np.float32)
    return gw, (total[:N, K + Kh].astype(np.float32) if bias else None)


def model_dw(c, defect=None):
    M, N, S, K, Kh = c["M"], c["N"], c["S"], c["K"], c["Kh"]
    assert defect is None or defect in PLAIN_DEFECTS
    L = np.zeros((M, S * N), np.float32)
    for s, rs in enumerate(c["scales"]):
        L[:, s * N:(s + 1) * N] = c["gy"] if rs is None else c["gy"] * rs[:, None]          # (an fp32 product, like the kernel's)
        if defect == "gy_columns_from_128_not_staged":
            L[:, s * N + 128:(s + 1) * N] = 0
    R = _right(c["a"], c["h"], K, Kh, M, defect)
    total = np.zeros((S * N, K + Kh + 2))
    for r_beg in range(0, M, SLAB_ROWS):
        r_end = min(M, r_beg + SLAB_ROWS)
        acc = np.zeros((S * N, K + Kh + 2), np.float32)
        for row0 in range(r_beg, r_end, 32):
            n = min(32, r_end - row0)
            if n < 32 and defect == "last_partial_step_dropped":
                continue
            Ls, Rs = np.zeros((32, S * N), np.float32), np.zeros((32, K + Kh + 2), np.float32)
            Ls[:n], Rs[:n] = L[row0:row0 + n], R[row0:row0 + n]
            if defect == "padding_rows_not_masked":                  # a row past the slab's end re-reads the last row
                Ls[n:], Rs[n:] = L[r_end - 1], R[r_end - 1]
            acc = _step(acc, Ls, Rs, defect)
        total += acc.astype(np.float64)                              # float64 across the slabs, ascending
    return _scatter(total, N, S, K, Kh, c["bias"])


# ---- hand-built plans of the grouped form --------------------------------------------------------------------------------------------
def live_rows(pattern):
    m = np.zeros(TILE, bool)
    if pattern == "full":
        m[:] = True
    elif pattern == "first_pad":                                     # the tile's first row is padding
        m[1:] = True
    elif pattern == "mid_pad":                                       # padding in the middle, across the boundary of two 32-row steps
        m[:] = True
        m[27:71] = False
    elif pattern == "step_pad":                                      # one whole 32-row step of padding
        m[:] = True
        m[32:64] = False
    elif pattern == "sparse":
        m[::3] = True
    elif pattern.startswith("head:"):
        m[:int(pattern[5:])] = True
    else:
        assert pattern == "none", pattern
    return m


def _alt(n):
    return [(i % 2, "full" if i % 3 else "head:90") for i in range(n)]


_MIXED7 = [(0, "first_pad"), (0, "mid_pad"), (1, "none"), (1, "full"), (1, "head:5"), (2, "sparse"), (0, "step_pad")]
#                name            tiles                                              n_wg  N   K   Kh  S
GROUPED_PLANS = [("one_tile",     [(0, "full")],                                       1,  1,   1,  0, 1),
                 ("aba",          [(0, "full"), (1, "head:100"), (0, "full")],         1, 16,  48, 16, 2),
                 ("run_cut",      [(2, "full"), (2, "head:77"), (2, "full"), (2, "full")], 2, 17, 320, 0, 3),
                 ("three_changes", [(0, "full"), (1, "full"), (2, "mid_pad"), (1, "full"), (1, "full"), (1, "sparse"), (3, "full"), (3, "head:1")],
                  2, 64, 300, 83, 3),
                 ("more_wgs_than_tiles", [(1, "full"), (0, "first_pad"), (0, "full")],  5, 65,  60,  4, 1),
                 ("mixed7_wg1",   _MIXED7,                                             1, 80, 304, 79, 3),
                 ("mixed7_wg2",   _MIXED7,                                             2, 80, 304, 79, 3),
                 ("mixed7_wg3",   _MIXED7,                                             3, 80, 304, 79, 3),
                 ("mixed7_wg5",   _MIXED7,                                             5, 80, 304, 79, 3),
                 ("alt7",         _alt(7),                                             1, 17,  20,  3, 2),
                 ("alt8",         _alt(8),                                             2, 16,  60,  4, 2),
                 ("alt9",         _alt(9),                                             3, 17,  20,  3, 3),
                 ("alt17",        _alt(17),                                            2, 16,  20,  3, 2)]      # (17 entries need 17 tiles)
GROUPED_VARIANTS = {"int": ("aba", "three_changes", "mixed7_wg3", "alt9")}


def wg_ranges(n_tiles, n_wg):
    """Equally long contiguous tile ranges, workgroup by workgroup."""
    return [(w * n_tiles // n_wg, (w + 1) * n_tiles // n_wg) for w in range(n_wg)]


def tables_literal(tile_group, n_wg):
    """(wg_range, wg_entry, entry_group) after the header: workgroup w walks its tiles and writes one partial product per degree run it
    meets into entries wg_entry[w], wg_entry[w] + 1, ...; entry_group[e] = the degree group of entry e."""
    ranges = wg_ranges(len(tile_group), n_wg)
    wg_entry, entry_group = [], []
    for lo, hi in ranges:
        wg_entry.append(len(entry_group))
        for t in range(lo, hi):
            if t == lo or tile_group[t] != tile_group[t - 1]:
                entry_group.append(int(tile_group[t]))
    return np.array(ranges, np.int32).reshape(n_wg, 2), np.array(wg_entry, np.int32), np.array(entry_group, np.int32)


def tables_derived(tile_group, n_wg):
    """The same three tables the way DegreePlan.dw_tables (pna_amd/degree_groups.py) derives them from tile_group and the grid."""
    tg = np.asarray(tile_group, np.int64)
    nt = tg.size
    b = (np.arange(n_wg + 1, dtype=np.int64) * nt) // n_wg
    lo, hi = b[:-1], b[1:]
    change = np.zeros(nt, bool)
    change[1:] = tg[1:] != tg[:-1]
    starts = np.unique(np.concatenate([lo[hi > lo], np.nonzero(change)[0]]))
    wg_entry = np.searchsorted(starts, np.minimum(lo, max(nt - 1, 0)))
    return np.stack([lo, hi], axis=1).astype(np.int32), wg_entry.astype(np.int32), tg[starts].astype(np.int32)


def make_grouped(name, tiles, n_wg, N, K, Kh, S, variant="randn", seed=0, spare=3):
    """One call's operands in NODE order.  Live rows name distinct nodes 1 .. ; node 0 and `spare` more nodes are named by no virtual row
    and hold NaN: a padding row reads node 0 and must mask it, an unnamed node must not contribute."""
    rng = np.random.default_rng([seed, len(tiles), N, K])
    tile_group = np.array([g for g, _ in tiles], np.int32)
    live = np.concatenate([live_rows(p) for _, p in tiles])
    n_live = int(live.sum())
    n_nodes = n_live + spare + 1
    perm = np.full(live.size, -1, np.int32)
    perm[live] = 1 + rng.permutation(n_live + spare)[:n_live]
    wg_range, wg_entry, entry_group = tables_literal(tile_group, n_wg)
    d = tables_derived(tile_group, n_wg)
    on = wg_range[:, 1] > wg_range[:, 0]
    assert np.array_equal(wg_range, d[0]) and np.array_equal(entry_group, d[2]) and np.array_equal(wg_entry[on], d[1][on]), \
        f"{name}: the literal tables and DegreePlan.dw_tables' rule disagree"
    gy, a, h = _operands(rng, n_nodes, N, K, Kh, variant)
    G = int(tile_group.max()) + 1
    if variant == "int":
        scale = np.exp2(rng.integers(-2, 3, (G, S))).astype(np.float32) * rng.choice([-1.0, 1.0], (G, S)).astype(np.float32)
    else:                                                            # arbitrary values: the C contract does not ask for degree functions
        scale = (rng.standard_normal((G, S)) * 2.0).astype(np.float32)
    named = np.zeros(n_nodes, bool)
    named[perm[live]] = True
    for t in (gy, a, h):
        if t is not None:
            t[~named] = np.nan
    c = dict(name=name + ("" if variant == "randn" else "/" + variant), N=N, K=K, Kh=Kh, S=S, variant=variant, tiles=tiles, n_wg=n_wg,
             gy=gy, a=a, h=h, group_scale=scale, row_perm=perm, tile_group=tile_group, wg_range=wg_range, wg_entry=wg_entry,
             entry_group=entry_group, n_entries=int(entry_group.size), n_nodes=n_nodes, named=named)
    assert not named[0] and (~named).sum() == spare + 1 and N <= 80 and K + Kh + 1 <= 384
    if variant == "int":
        r = ref_grouped(c)
        assert max(r["floor_w"].max(), r["floor_b"].max()) < 2.0 ** 24, "every partial sum of an integer case is exact in fp32"
    return c


def grouped_cases():
    out = {}
    rows = {r[0]: r for r in GROUPED_PLANS}
    for r in GROUPED_PLANS:                                          # (the same tile list under another grid: the same operands)
        out[r[0]] = make_grouped(*r, seed=next(j for j, q in enumerate(GROUPED_PLANS) if q[1] is r[1]))
    for variant, names in GROUPED_VARIANTS.items():
        for name in names:
            c = make_grouped(*rows[name], variant=variant, seed=200)
            out[c["name"]] = c
    return out


def a_in_plan_order(c):
    """`a` as a forward that gathered in plan order leaves it: row r = the aggregate of virtual row r, NaN in the padding rows."""
    out = np.full((c["row_perm"].size, c["K"]), np.nan, np.float32)
    lv = c["row_perm"] >= 0
    out[lv] = c["a"][c["row_perm"][lv]]
    return out


def ref_grouped(c):
    perm = c["row_perm"].astype(np.int64)
    v = np.nonzero(perm >= 0)[0]
    node = perm[v]
    g, a = c["gy"].astype(np.float64)[node], c["a"].astype(np.float64)[node]
    w = c["group_scale"].astype(np.float64)[c["tile_group"][v // TILE]]                      # (live rows, S)
    blocks, floors = [], []
    if c["Kh"]:
        h = c["h"].astype(np.float64)[node]
        blocks.append(g.T @ h); floors.append(np.abs(g).T @ np.abs(h))
    for s in range(c["S"]):
        gs = g * w[:, s:s + 1]
        blocks.append(gs.T @ a); floors.append(np.abs(gs).T @ np.abs(a))
    return dict(gw=np.concatenate(blocks, axis=1), floor_w=np.concatenate(floors, axis=1), gb=g.sum(0), floor_b=np.abs(g).sum(0))


def model_dw_grouped(c, a_plan=False, defect=None, workspace_fill=np.nan):
    """The workspace starts at `workspace_fill` (the header: no initialisation needed -- the GPU tests fill it with NaN; 0 shows that a
    defect is caught by the bar itself and not only by an entry nobody wrote)."""
    assert defect is None or defect in GROUPED_DEFECTS
    N, K, Kh, S = c["N"], c["K"], c["Kh"], c["S"]
    perm, tg = c["row_perm"].astype(np.int64), c["tile_group"]
    a_rows = a_in_plan_order(c) if a_plan else None
    part = np.full((c["n_entries"], N, K + Kh + 2), workspace_fill, np.float32)
    for w in range(c["n_wg"]):
        t0, t1 = (int(x) for x in c["wg_range"][w])
        if t0 >= t1:
            continue
        entry, cur = int(c["wg_entry"][w]), tg[t0]
        acc = np.zeros((N, K + Kh + 2), np.float32)
        for t in range(t0, t1):
            if tg[t] != cur and defect != "no_flush_on_group_change":
                part[entry] = acc
                entry, cur, acc = entry + 1, tg[t], np.zeros_like(acc)
            for ks in range(4):
                vr = np.arange(TILE * t + 32 * ks, TILE * t + 32 * ks + 32)
                ids = perm[vr]
                keep, idc = ids >= 0, np.maximum(ids, 0)
                L = c["gy"][idc].copy()
                R = _right(a_rows[vr] if a_plan else c["a"][idc], c["h"][idc] if Kh else None, K, Kh, 32, defect)
                if defect != "padding_rows_not_masked":              # a padding row reads node 0 and is masked to +0 bits
                    L[~keep], R[~keep] = 0, 0
                acc = _step(acc, L, R, defect)
        part[entry] = acc
    eg = c["entry_group"].astype(np.int64)
    if defect == "entry_scaled_by_wrong_group":
        eg = eg[np.maximum(np.arange(eg.size) - 1, 0)]
    sc = c["group_scale"].astype(np.float64)[eg]                                             # (entries, S)
    total = np.zeros((S * N, K + Kh + 2))
    p64 = part.astype(np.float64)
    with np.errstate(invalid="ignore"):
        for y in range(8):                                           # entry lane y adds entries y, y + 8, ...; the eight sums in a fixed order
            lane_w, lane_1 = np.zeros((S, N, K + Kh + 2)), np.zeros((N, K + Kh + 2))
            for e in range(y, c["n_entries"], 8):
                lane_1 += p64[e]
                for s in range(S):
                    lane_w[s] += p64[e] * sc[e, s]
            for s in range(S):
                total[s * N:(s + 1) * N, :K] += lane_w[s][:, :K]
            total[:N, K:] += lane_1[:, K:]
    return _scatter(total, N, S, K, Kh, True)


# ---- which edges a set of cases hits ---------------------------------------------------------------------------------------------------
def edges_hit(plain, grouped):
    """Edges of the lists above that some case reaches WITH A KERNEL RUN: a refused case (the GPU module only asserts -1 on it) counts for
    `N_wide` and `SN240_refused` and nothing else."""
    hit = dict(N=set(), SN240=set(), SN240_refused=set(), N_wide=set(), R=set(), M=set(), slabs=set(), scalers=set(), gN=set(), gR=set(),
               gS=set(), entries=set(), wgs=set(), flags=set())
    for c in plain.values():
        if c["refused"]:
            hit["N_wide"].add(c["N"])
            if c["S"] * c["N"] == 240:
                hit["SN240_refused"].add((c["N"], c["S"]))
            continue
        hit["N"].add(c["N"]); hit["R"].add(c["K"] + c["Kh"] + 1); hit["M"].add(c["M"]); hit["scalers"].add(c["scal"]); hit["slabs"].add(c["slabs"])
        if c["S"] * c["N"] == 240:
            hit["SN240"].add((c["N"], c["S"]))
        if c["Kh"] and c["K"] < 128 < c["K"] + c["Kh"]:
            hit["flags"].add("h panel across a third boundary")
        if c["Kh"] and c["K"] % 64:
            hit["flags"].add("h panel behind a K that is no multiple of 64")
        if c["variant"] != "randn":
            hit["flags"].add(c["variant"])
    for c in grouped.values():
        hit["gN"].add(c["N"]); hit["gR"].add(c["K"] + c["Kh"] + 1); hit["gS"].add(c["S"]); hit["entries"].add(c["n_entries"])
        tg, rng_ = c["tile_group"], c["wg_range"]
        live = (c["row_perm"] >= 0).reshape(-1, TILE)
        if tg.size == 1:
            hit["flags"].add("one tile in one group")
        if tg.size >= 3 and any(tg[i] == tg[i + 2] != tg[i + 1] for i in range(tg.size - 2)):
            hit["flags"].add("group order A, B, A")
        for w in range(1, c["n_wg"]):
            lo = int(rng_[w, 0])
            if rng_[w, 1] > lo and 0 < lo and tg[lo] == tg[lo - 1] and c["entry_group"][c["wg_entry"][w]] == c["entry_group"][c["wg_entry"][w] - 1]:
                hit["flags"].add("a run cut across two workgroups")
        for lo, hi in rng_:
            if sum(tg[t] != tg[t - 1] for t in range(lo + 1, hi)) >= 3:
                hit["flags"].add("a workgroup range with three group changes")
        if (rng_[:, 1] == rng_[:, 0]).any():
            hit["flags"].add("empty workgroup ranges")
        if (~live[:, 0] & live.any(1)).any():
            hit["flags"].add("a tile whose first row is padding")
        if any((~row[np.argmax(row):TILE - np.argmax(row[::-1])]).any() for row in live if row.any()):
            hit["flags"].add("padding in the middle of a tile")
        if (~live.any(1)).any():
            hit["flags"].add("a tile that is all padding")
        if (~c["named"]).any():
            hit["flags"].add("nodes that no virtual row names")
        if c["name"].startswith("mixed7_wg"):
            hit["wgs"].add(c["n_wg"])
    return hit
