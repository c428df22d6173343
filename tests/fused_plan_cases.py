"""Hand-built degree plans for pna_fused_degree_f32 (include/pna_amd.h), their float64 references and the per-element bar -- no GPU needed.

The production plan builder (pna_amd/degree_groups.py::DegreePlan.fused_tables) emits a narrow subset of the header's contract: groups of
at least 128 rows of one in-degree, padding only behind a group, the few low degrees a power-law graph repeats.  Here a plan is spelled
out block by block -- (in-degree, weight image, live rows) per aligned 16-row block -- and built LITERALLY after the header:
    max(4, round_up(D, 4)) records per block, the ones past D copies of record D - 1; a padding row repeats the block's first row's ids;
    an all-padding block has D = 0 and the ids of a valid row; one in-degree per 16-row block, one image per workgroup tile.
References: the statistics are oracle.c_oracle.segreduce with fp32 accumulation over the plan's implied CSR (the sequential edge-order fold
the kernel claims to reproduce bit for bit); the layer is the float64 contraction of THOSE statistics with W_i = sum_s scale[i, s] W_s formed
in float64, epilogue after the header's formula.  The bar is the project's own (test_guarded_contraction_is_componentwise_accurate_on_
adversarial_rows) with an explicit term for the epilogue's O(1) operands:
    |got - ref64| <= 1e-5 |ref64| + 2e-6 mass |row_post col_scale| + 2^-22 E
mass = sum_k |a_k| |W_i[n][k]| (+ the tower terms' magnitudes), E = (|bias| + |pre_add|) |row_post col_scale| + |col_shift| + |residual|.
model_stats() / model_layer() are a plain numpy model of the kernel's data path over the TABLES (not the CSR) with switchable defects: the
host module proves with it that the bar and the bit comparison bite.  A plan of a few tiles gives every workgroup of the persistent kernel ONE
tile: retile() + chain_order() list the same tiles again so that the state carried from tile to tile crosses every boundary of the list."""
import numpy as np

TILE = 64                      # rows of a workgroup tile (pna_fused_degree_tile_rows: 64 for every shape the library builds)
CANARY = np.array([0xCAFEBABE], dtype=np.uint32).view(np.float32)[0]
LADDER = (0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 31, 32, 33, 127, 128, 129, 300)
ALL16 = 0xFFFF
# instantiation edges of the shape rules: every F with a narrow and a wide N, every N with a half-block and a full-block F
LADDER_SHAPES = [(17, 4), (17, 80), (20, 5), (20, 75), (32, 16), (32, 80), (33, 17), (33, 75), (40, 4), (40, 80), (48, 5), (48, 75),
                 (49, 16), (49, 81), (64, 17), (64, 128), (65, 4), (65, 80), (75, 5), (75, 75), (80, 16), (80, 80), (97, 17), (97, 81),
                 (112, 4), (112, 128), (113, 5), (113, 128), (128, 16), (128, 75), (128, 81), (128, 128)]
TOWER_SHAPES = [(49, 4), (64, 75), (65, 80), (75, 75), (80, 4), (80, 80)]


def round_up(a, b):
    return (a + b - 1) // b * b


def n_records_of(D):
    return max(4, round_up(int(D), 4))


def mask_of(positions):
    return sum(1 << p for p in positions)


# ---- the builder ---------------------------------------------------------------------------------------------------------------------
def tables(perm, block_image, rowptr, col, placeholder=0):
    """(tile_desc [M / 16, 4], tile_ids [n_records, 16], n_records) from the virtual rows' nodes `perm` (-1: padding), the image of every
    16-row block and the rows' in-edges (`rowptr` / `col` over the VIRTUAL rows, edge order), after the header, clause by clause."""
    perm, rowptr, col = np.asarray(perm, np.int64), np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    M = perm.size
    assert M % 16 == 0 and len(block_image) == M // 16
    desc = np.zeros((M // 16, 4), np.int32)
    recs = []
    first = 0
    for b in range(M // 16):
        v0 = 16 * b
        live = perm[v0] >= 0                                       # (an all-padding block: D = 0, ids of a valid row)
        D = int(rowptr[v0 + 1] - rowptr[v0]) if live else 0
        n = n_records_of(D)
        rec = np.full((n, 16), placeholder, np.int64)
        if D > 0:
            for i in range(16):
                v = v0 + i if perm[v0 + i] >= 0 else v0             # a padding row repeats the block's first row
                e = np.minimum(np.arange(n), D - 1)                 # records past D: copies of record D - 1
                rec[:, i] = col[rowptr[v] + e]
        desc[b] = (first, D, block_image[b], 0)
        recs.append(rec)
        first += n
    return desc, np.concatenate(recs).astype(np.int32), first


def plan_from_spec(blocks, x_rows, seed=0, tile=TILE, spare_nodes=5, placeholder=None):
    """A plan from [(D, image, live-row mask)] per 16-row block.  Live rows get distinct nodes out of a shuffled range that is
    `spare_nodes` longer than needed (rows of y no virtual row names); the sources are drawn with a seeded generator and include the
    table's row 0 and its last row; D = 0 blocks carry `placeholder` (default: the table's LAST row) in their four records."""
    rng = np.random.default_rng(seed)
    blocks = list(blocks)
    while len(blocks) % (tile // 16):
        blocks.append((0, blocks[-1][1], 0))
    M = 16 * len(blocks)
    live = np.zeros(M, bool)
    deg = np.zeros(M, np.int64)
    for b, (D, _, mask) in enumerate(blocks):
        assert mask == 0 or mask & 1, "a block with live rows has a live first row"
        assert mask != 0 or D == 0, "an all-padding block has D = 0"
        for i in range(16):
            if mask >> i & 1:
                live[16 * b + i], deg[16 * b + i] = True, D
    n_nodes = int(live.sum()) + spare_nodes
    nodes = rng.permutation(n_nodes)[:int(live.sum())]
    perm = np.full(M, -1, np.int64)
    perm[live] = nodes
    rowptr = np.zeros(M + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = rng.integers(0, x_rows, int(rowptr[-1]))
    if col.size >= 2:
        a, b_ = rng.choice(col.size, 2, replace=False)
        col[a], col[b_] = 0, x_rows - 1
    image = np.array([im for _, im, _ in blocks], np.int64)
    for t in range(M // tile):
        assert len(set(image[t * tile // 16:(t + 1) * tile // 16])) == 1, "one weight image per workgroup tile"
    desc, ids, n_rec = tables(perm, image, rowptr, col, placeholder=x_rows - 1 if placeholder is None else placeholder)
    return dict(perm=perm.astype(np.int32), tile_desc=desc, tile_ids=ids, n_records=n_rec, rowptr=rowptr, col=col, M=M, n_nodes=n_nodes,
                x_rows=x_rows, tile=tile, block_D=np.array([D for D, _, _ in blocks]), block_image=image)


def with_edges(plan, col):
    """The plan with the in-edges' sources replaced by `col` (same degrees): its tables built again."""
    out = dict(plan, col=np.asarray(col, np.int64))
    out["tile_desc"], out["tile_ids"], out["n_records"] = tables(plan["perm"], plan["block_image"], plan["rowptr"], out["col"],
                                                                 placeholder=plan["x_rows"] - 1)
    return out


def retile(plan, order):
    """The plan with its workgroup tiles listed as `order` (a permutation, or a longer list with repeats: several virtual tiles then
    name the SAME nodes and records, and write the same values)."""
    order = np.asarray(order, np.int64)
    w = plan["tile"] // 16
    out = dict(plan)
    out["perm"] = plan["perm"].reshape(-1, plan["tile"])[order].reshape(-1).copy()
    out["tile_desc"] = plan["tile_desc"].reshape(-1, w, 4)[order].reshape(-1, 4).copy()
    out["block_D"] = plan["block_D"].reshape(-1, w)[order].reshape(-1)
    out["block_image"] = plan["block_image"].reshape(-1, w)[order].reshape(-1)
    out["M"] = order.size * plan["tile"]
    out["tile_of"] = order                                        # virtual tile -> tile of the base plan (whose rowptr / col still apply)
    return out


def chain_order(n_base, G, rounds):
    """rounds x G tiles such that the tile a workgroup of a static grid of G takes next (j + G) is the base plan's NEXT tile, cyclically:
    every tile boundary of the base list is crossed by the loop-carried state (ids prefetched by the previous tile's last packets,
    descriptors two tiles ahead)."""
    j = np.arange(rounds * G)
    return (j // G + j % G) % n_base


def check_contract(t, x_rows=None, strict_layout=True):
    """The header's clauses on a set of tables (dict with perm, tile_desc, tile_ids, n_records, tile; rowptr / col of the virtual rows
    when present and not retiled): raises AssertionError naming the clause."""
    perm, desc, ids = np.asarray(t["perm"], np.int64), np.asarray(t["tile_desc"], np.int64), np.asarray(t["tile_ids"], np.int64)
    M, tile = perm.size, t.get("tile", TILE)
    assert M % tile == 0, "M is a multiple of the tile"
    assert desc.shape == (M // 16, 4) and ids.shape == (t["n_records"], 16) and t["n_records"] >= 4
    assert (desc[:, 3] == 0).all(), "fourth descriptor word is 0"
    assert (desc[:, 1] >= 0).all() and (desc[:, 0] >= 0).all() and (desc[:, 2] >= 0).all()
    assert (ids >= 0).all() and (x_rows is None or (ids < x_rows).all()), "every id names a valid row of x"
    img = desc[:, 2].reshape(-1, tile // 16)
    assert (img == img[:, :1]).all(), "one weight image per workgroup tile"
    has_csr = "rowptr" in t and "tile_of" not in t
    nxt = 0
    for b in range(M // 16):
        first, D = int(desc[b, 0]), int(desc[b, 1])
        n = n_records_of(D)
        assert first + n <= t["n_records"], "a block owns max(4, round_up(D, 4)) records inside the table"
        if strict_layout and "tile_of" not in t:
            assert first == nxt, "blocks own consecutive, disjoint record ranges"
            nxt = first + n
        rec, p = ids[first:first + n], perm[16 * b:16 * b + 16]
        if p[0] < 0:
            assert (p < 0).all() and D == 0, "a block whose first row is padding is all padding and has D = 0"
        if D > 0:
            assert (rec[D:] == rec[D - 1]).all(), "records past D are copies of record D - 1"
            assert (rec[:, p < 0] == rec[:, :1]).all(), "a padding row repeats the block's first row"
        if has_csr:
            rp, col = np.asarray(t["rowptr"], np.int64), np.asarray(t["col"], np.int64)
            for i in np.nonzero(p >= 0)[0]:
                v = 16 * b + i
                assert rp[v + 1] - rp[v] == D, "one in-degree per 16-row block"
                assert (rec[:D, i] == col[rp[v]:rp[v + 1]]).all(), "record e holds the row's e-th in-edge"
    if strict_layout and "tile_of" not in t:
        assert nxt == t["n_records"]
    return True


# ---- references ----------------------------------------------------------------------------------------------------------------------
def oracle_stats(plan, x, F):
    """(M_base, 4F) fp32 [mean | max | min | std] of every virtual row of the BASE plan: the C oracle's sequential fp32 fold in edge order."""
    from oracle import c_oracle
    return c_oracle.segreduce(plan["rowptr"], plan["col"], np.ascontiguousarray(x[:, :F]), F, ["mean", "max", "min", "std"])


def combined_weights(c):
    """W_i = sum_s scale[i, s] W_s in float64 from the fp32 operands: (n_img, N, K), K = 4F (tower: 5F, the self panel behind)."""
    K = (5 if c.get("tower") else 4) * c["F"]
    w = c["w_ref"].astype(np.float64)
    S = c["S"]
    scale = np.ones((c["n_img"], 1)) if c["scale"] is None else c["scale"].astype(np.float64)
    return sum(scale[:, s, None, None] * w[None, :, s * K:(s + 1) * K] for s in range(S))


def layer_ref(c, stats):
    """float64 reference of the layer on the case's BASE plan from the fp32 statistics `stats` (M, 4F): dict of per-virtual-row (M, N)
    arrays ref, bar and the node of every row.  Follows the header's formula, tower terms included."""
    p, F, N = c["plan"], c["F"], c["N"]
    W = combined_weights(c)
    perm = p["perm"].astype(np.int64)
    node = np.maximum(perm, 0)
    img = np.repeat(p["block_image"], 16)
    D = np.repeat(p["block_D"], 16)
    a = stats.astype(np.float64)
    M = p["M"]
    z, mass = np.zeros((M, N)), np.zeros((M, N))
    tw = c.get("tower")
    rp = np.ones(M)
    pre = np.zeros((M, N))
    if tw:
        xd, hs = tw["x_dst"].astype(np.float64)[node], tw["h_self"].astype(np.float64)[node]
        rp = tw["row_post"].astype(np.float64)
        if tw.get("pre_add") is not None:
            pre = tw["pre_add"].astype(np.float64)[node]
    for i in np.unique(img):
        rows = img == i
        Wi = W[i]                                                                  # (N, K)
        z[rows] = a[rows] @ Wi[:, :4 * F].T
        mass[rows] = np.abs(a[rows]) @ np.abs(Wi[:, :4 * F]).T
        if tw:
            Wsum = Wi[:, :F] + Wi[:, F:2 * F] + Wi[:, 2 * F:3 * F]
            on = (D[rows] > 0).astype(np.float64)[:, None]                        # DGL leaves rows without in-edges at zero: no x_dst term
            z[rows] += on * (xd[rows] @ Wsum.T) + hs[rows] @ Wi[:, 4 * F:].T
            mass[rows] += on * (np.abs(xd[rows]) @ np.abs(Wsum).T) + np.abs(hs[rows]) @ np.abs(Wi[:, 4 * F:]).T
    bias = np.zeros(N) if c["bias"] is None else c["bias"].astype(np.float64)
    cs = np.ones(N) if c["col_scale"] is None else c["col_scale"].astype(np.float64)
    ct = np.zeros(N) if c["col_shift"] is None else c["col_shift"].astype(np.float64)
    res = np.zeros((p["M"], N)) if c["residual"] is None else c["residual"].astype(np.float64)[node]
    v = ((bias + z + pre) * rp[:, None]) * cs + ct
    if c["relu"] == 1:
        v = np.maximum(v, 0.0)
    elif c["relu"] == 2:
        v = np.where(v < 0, v * float(c["slope"]), v)
    ref = res + v
    rc = np.abs(rp[:, None] * cs)
    E = (np.abs(bias) + np.abs(pre)) * rc + np.abs(ct) + np.abs(res)
    bar = 1e-5 * np.abs(ref) + 2e-6 * mass * rc + 2.0 ** -22 * E
    return dict(ref=ref, bar=bar, mass=mass, perm=perm)


def expected_y(c, r):
    """(want, bar, named) full (n_nodes, N) arrays: the reference scattered to node order, and which rows a virtual row names."""
    n_nodes, N = c["plan"]["n_nodes"], c["N"]
    want, bar, named = np.zeros((n_nodes, N)), np.zeros((n_nodes, N)), np.zeros(n_nodes, bool)
    lv = r["perm"] >= 0
    want[r["perm"][lv]], bar[r["perm"][lv]], named[r["perm"][lv]] = r["ref"][lv], r["bar"][lv], True
    return want, bar, named


def compare_y(y, c, r, cols_written=None):
    """Worst err / bar of an output buffer `y` (n_nodes, >= N) float32 that was prefilled with CANARY: rows no virtual row names and the
    columns behind the written ones must still hold it.  Returns (worst ratio, message); ratio = inf for a damaged canary / NaN."""
    N = c["N"]
    ncw = N if cols_written is None else cols_written
    want, bar, named = expected_y(c, r)
    canary = CANARY.view(np.uint32)
    raw = np.ascontiguousarray(y).view(np.uint32)
    if (raw[~named] != canary).any():
        return np.inf, "a row that no virtual row names was written"
    if (raw[:, ncw:] != canary).any():
        return np.inf, "columns behind the writable ones were written"
    if ncw > N and (raw[named][:, N:ncw] != 0).any():
        return np.inf, "writable columns behind N are not zero"
    got = y[named][:, :N].astype(np.float64)
    if not np.isfinite(got).all():
        return np.inf, "non-finite output"
    ratio = np.abs(got - want[named]) / np.maximum(bar[named], 1e-300)
    k = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio.max()), f"worst err / bar {ratio.max():.3f} at live row {k[0]}, column {k[1]}: got {got[k]:.9g}, ref {want[named][k]:.9g}, bar {bar[named][k]:.3g}"


# ---- a numpy model of the kernel's data path over the TABLES, with switchable defects -----------------------------------------------------
MUTATIONS = ("dup_records_in_sums", "ring_slot3_dropped", "first_ids_of_previous_tile", "empty_std_is_eps", "padding_stored_to_node0",
             "second_fp16_term_dropped", "mean_by_reciprocal")


def _round_bits(a, bits):
    m, e = np.frexp(a)
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def model_stats(p, x, F, mut=None):
    """(M, 4F) fp32 statistics as the kernel forms them from tile_desc / tile_ids: the sequential fp32 fold of records 0 .. D - 1."""
    f32 = np.float32
    desc, ids = p["tile_desc"], p["tile_ids"].astype(np.int64)
    w = p["tile"] // 16
    out = np.zeros((p["M"], 4 * F), f32)
    for b in range(p["M"] // 16):
        first, D = int(desc[b, 0]), int(desc[b, 1])
        n, ng = n_records_of(D), max((D + 3) // 4, 1)
        rec = ids[first:first + n].copy()
        if mut == "first_ids_of_previous_tile" and b >= w:
            rec[:4] = ids[int(desc[b - w, 0]):int(desc[b - w, 0]) + 4]
        s, q = np.zeros((16, F), f32), np.zeros((16, F), f32)
        mx, mn = np.full((16, F), -np.inf, f32), np.full((16, F), np.inf, f32)
        for e in range(n):
            on = e < D or (mut == "dup_records_in_sums" and D > 0)
            if mut == "ring_slot3_dropped" and e >= 4 * (ng - 1) and e % 4 == 3:
                continue
            m = x[rec[e], :F].astype(f32)
            if on:
                s, q = s + m, q + m * m
            if D > 0:
                mx, mn = np.maximum(mx, m), np.minimum(mn, m)
        if D > 0:
            Df = f32(D)
            mean = s * (f32(1.0) / Df) if mut == "mean_by_reciprocal" else s / Df
            msq = q * (f32(1.0) / Df) if mut == "mean_by_reciprocal" else q / Df
            var = np.maximum(msq - mean * mean, f32(0))
            out[16 * b:16 * b + 16] = np.concatenate([mean, mx, mn, np.sqrt(var + f32(1e-5))], axis=1)
        elif mut == "empty_std_is_eps":
            out[16 * b:16 * b + 16, 3 * F:] = np.sqrt(f32(1e-5))
    return out


def model_layer(c, mut=None):
    """(y (n_nodes, N) float32 over a CANARY prefill, statistics): the contraction in float64 over model_stats, stored through perm."""
    p, N = c["plan"], c["N"]
    stats = model_stats(p, c["x"], c["F"], mut)
    cc = dict(c)
    a = stats
    if mut == "second_fp16_term_dropped":
        a = _round_bits(stats.astype(np.float64), 11).astype(np.float32)
        cc["w_ref"] = _round_bits(c["w_ref"].astype(np.float64), 11)
    r = layer_ref(cc, a)
    y = np.full((p["n_nodes"], N), CANARY, np.float32)
    for v in range(p["M"]):
        node = int(p["perm"][v])
        if node < 0 and mut != "padding_stored_to_node0":
            continue
        if node < 0:                                               # the padding row computes its block's first row (its ids) and stores it to node 0
            y[0] = r["ref"][v - v % 16].astype(np.float32)
        else:
            y[node] = r["ref"][v].astype(np.float32)
    return y, stats


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def ladder_blocks(degrees=LADDER, n_img=3):
    """Both layouts of the degree ladder in one block list: a tile per degree (its four blocks live, the last one with padding), then tiles
    that mix four different degrees under one image; a D = 0 block sits directly in front of a live block and one ends the list."""
    blocks = []
    for k, D in enumerate(degrees):
        blocks += [(D, k % n_img, ALL16)] * 3 + [(D, k % n_img, mask_of(range(11)))]      # (D = 0: live rows without in-edges)
    mixed = list(degrees)
    while len(mixed) % 4:
        mixed.append(degrees[1])
    mixed = mixed[1:] + mixed[:1]                                   # ... so that the D = 0 block ends a tile and the list goes on behind it
    for t in range(0, len(mixed), 4):
        blocks += [(D, (t // 4) % n_img, ALL16 if (t + j) % 3 else mask_of((0, 7, 15))) for j, D in enumerate(mixed[t:t + 4])]
    blocks += [(9, 0, ALL16), (0, 0, 0), (5, 0, mask_of(range(9))), (0, 0, 0)]     # D = 0 in front of a live block, and as the last block
    return blocks


def padding_blocks():
    """Live rows only at {0, 7, 15}; an all-padding block between live ones; an all-padding tile in the middle."""
    s = mask_of((0, 7, 15))
    return [(3, 0, s), (0, 0, 0), (6, 0, ALL16), (1, 0, s),
            (0, 1, 0), (0, 1, 0), (0, 1, 0), (0, 1, 0),
            (4, 1, ALL16), (0, 1, 0), (0, 1, 0), (11, 1, s),
            (2, 0, mask_of((0,))), (8, 0, ALL16), (5, 0, s), (0, 0, 0)]


def claim_blocks(n_tiles=8):
    """D in 0 .. 5, mixed inside the tiles (the dynamic schedule's plan: thousands of cheap tiles)."""
    return [((3 * t + 5 * j) % 6, t % 2, 0 if (t + j) % 7 == 0 and (3 * t + 5 * j) % 6 == 0 else (ALL16 if j != 3 else mask_of(range(13))))
            for t in range(n_tiles) for j in range(4)]


def make_case(F, N, blocks, seed=0, S=3, n_img=3, x_rows=301, bias=True, bn=True, residual=True, relu=1, slope=0.0, tower=False, pre_add=False,
              x_scale=1.0):
    """Operands of one call (numpy, fp32): Gaussian features and weights, positive scaler values, BatchNorm-like column factors."""
    rng = np.random.default_rng(1000 + seed)
    f32 = np.float32
    plan = plan_from_spec(blocks, x_rows, seed=seed)
    K = (5 if tower else 4) * F
    w = (rng.standard_normal((N, S * K)) / np.sqrt(4 * F)).astype(f32)
    scale = None if S == 1 and n_img == 1 else (0.3 + 1.5 * rng.random((n_img, S))).astype(f32)
    if tower:
        for s in range(1, S):
            w[:, s * K + 4 * F:(s + 1) * K] = 0                   # the self panel lives in block 0 alone ...
        scale[:, 0] = 1.0                                         # ... whose scaler is the identity
    n = plan["n_nodes"]
    x = (x_scale * rng.standard_normal((x_rows, F))).astype(f32)
    if x_scale == 0.0:
        x = np.zeros((x_rows, F), f32)      # (+0 everywhere: over zeros of BOTH signs v_max_f32 / v_min_f32 return +0 / -0, the oracle the first it saw)
    c = dict(F=F, N=N, S=S, n_img=n_img, plan=plan, x=x, w_ref=w, scale=scale,
             bias=rng.standard_normal(N).astype(f32) if bias else None,
             col_scale=(0.5 + rng.random(N)).astype(f32) if bn else None, col_shift=(0.3 * rng.standard_normal(N)).astype(f32) if bn else None,
             residual=rng.standard_normal((n, N)).astype(f32) if residual else None, relu=relu, slope=slope, tower=None)
    if tower:
        c["tower"] = dict(x_dst=rng.standard_normal((n, F)).astype(f32), h_self=rng.standard_normal((n, F)).astype(f32),
                          row_post=(0.5 + rng.random(plan["M"])).astype(f32),
                          pre_add=rng.standard_normal((n, N)).astype(f32) if pre_add else None)
    return c
