"""Cases and float64 references of the net-ends calls (pna_embed_sum_*_f32, pna_readout_*_f32): a plain index-and-sum and a plain
per-segment reduction with their gradients, written without autograd (tests/test_net_ends_host.py checks them against torch autograd),
the error bar of a serial fp32 sum, and the case lists the GPU tests walk.  Everything here runs on the host."""
import torch

ATOM_DIMS = (119, 4, 12, 12, 10, 6, 6, 2, 2)          # nets.AtomEncoderStandIn.DIMS
SLAB = 64                                             # _lib.PNA_EMBED_SLAB_ROWS (tests/test_net_ends_host.py pins the two together)
MAX_SLABS = 256
U = 2.0 ** -24                                        # unit roundoff of fp32


# ---- references ---------------------------------------------------------------------------------------------------------------------
def embed_ref64(idx, tables):
    """sum_j tables[j][idx[:, j]] in float64; idx (V, T) int64."""
    out = torch.zeros(idx.shape[0], tables[0].shape[1], dtype=torch.float64)
    for j, w in enumerate(tables):
        out = out + w.double()[idx[:, j]]
    return out


def embed_grad_ref64(idx, rows, go):
    """Per table: (gradient (rows_j, F) in float64, n = how many rows select each table row, sum of |grad_out| over those rows)."""
    res = []
    g64 = go.double()
    for j, r in enumerate(rows):
        grad = torch.zeros(r, go.shape[1], dtype=torch.float64).index_add_(0, idx[:, j], g64)
        mass = torch.zeros(r, go.shape[1], dtype=torch.float64).index_add_(0, idx[:, j], g64.abs())
        n = torch.zeros(r, dtype=torch.float64).index_add_(0, idx[:, j], torch.ones(idx.shape[0], dtype=torch.float64))
        res.append((grad, n, mass))
    return res


def serial_sum_bound(n, mass):
    """|fp32 sum of n terms, in any fixed order, with or without float64 stages, rounded to fp32 once - exact sum| <= n u sum |terms|:
    a serial sum commits at most (n - 1) roundings of partial sums bounded by the mass, the final store one more.  Derived, not measured.
    n = 0: the bound is 0 (the element must be exactly 0)."""
    n = n if n.dim() == mass.dim() else n.unsqueeze(-1)
    return n * U * mass


def readout_ref64(h, sizes, op):
    """(G, F) float64 values, and for max the (G, F) row of the FIRST maximum (absolute row index)."""
    vals, args, at = [], [], 0
    for n in sizes:
        blk = h[at:at + n].double()
        if op == "max":
            m = blk.max(0).values
            first = (blk == m).to(torch.int64).argmax(0)                    # the first row that attains it
            vals.append(m)
            args.append(first + at)
        else:
            s = blk.sum(0)
            vals.append(s / n if op == "mean" else s)
        at += n
    return torch.stack(vals), (torch.stack(args) if op == "max" else None)


def readout_grad_ref64(h, sizes, op, go):
    """grad_h (V, F) float64 of sum(readout * go)."""
    out, at = torch.zeros(h.shape[0], h.shape[1], dtype=torch.float64), 0
    _, args = readout_ref64(h, sizes, op)
    for g, n in enumerate(sizes):
        if op == "max":
            out[args[g], torch.arange(h.shape[1])] = go[g].double()
        else:
            out[at:at + n] = go[g].double() / (n if op == "mean" else 1)
        at += n
    return out


# ---- embedding cases ------------------------------------------------------------------------------------------------------------------
def _idx(V, dims, seed, mode="random"):
    gen = torch.Generator().manual_seed(seed)
    if mode == "one_row":                                                   # every node selects the same row of every table
        return torch.stack([torch.full((V,), d - 1, dtype=torch.int64) for d in dims], dim=1)
    cols = [torch.randint(0, d, (V,), generator=gen) for d in dims]
    if mode == "skip_row":                                                  # row 3 of table 0 is selected by nobody
        cols[0] = torch.where(cols[0] == 3, torch.zeros_like(cols[0]), cols[0])
    return torch.stack(cols, dim=1)


# name -> (V, F, table rows, index mode).  V walks {1, 2, slab - 1, slab, slab + 1, 3 slab + 17}, F {1, 4, 70, 75, 80, 128}, the table
# count {1, 9, 16}; then the shapes at which the kernels take another path or meet a limit
EMBED_CASES = {
    "v1_f1_t1": (1, 1, (3,), "random"),
    "v2_f4_t9": (2, 4, ATOM_DIMS, "random"),
    "slab_minus_1_f70_t16": (SLAB - 1, 70, (3, 5, 2, 7, 4, 3, 2, 6, 5, 4, 3, 2, 9, 2, 3, 4), "random"),
    "slab_f75_t9": (SLAB, 75, ATOM_DIMS, "random"),
    "slab_plus_1_f80_t1": (SLAB + 1, 80, (5,), "random"),
    "three_slabs_17_f128_t9": (3 * SLAB + 17, 128, ATOM_DIMS, "random"),
    "one_row_table": (SLAB + 1, 4, (1, 3, 1), "random"),
    "unselected_row": (3 * SLAB + 17, 70, (7, 5), "skip_row"),
    "every_node_one_row": (3 * SLAB + 17, 80, (4, 2), "one_row"),
    "lds_limit_f128_t16": (2 * SLAB + 2, 128, (16,) * 16, "random"),        # 256 rows x 128 columns x 4 bytes = 128 KiB exactly
    "lds_limit_f256_t1": (SLAB + 3, 256, (128,), "random"),
    "slab_count_bounded": (SLAB * MAX_SLABS + 300, 4, (5, 3), "random"),    # slabs of 66 rows: 253 of them, not 261
}


def embed_case(name):
    """-> V, F, rows, idx (V, T) int64, tables [(rows_j, F) fp32], grad_out (V, F) fp32 -- all on the host, the same for every caller."""
    V, F, rows, mode = EMBED_CASES[name]
    seed = sorted(EMBED_CASES).index(name)
    gen = torch.Generator().manual_seed(100 + seed)
    tables = [torch.randn(r, F, generator=gen) for r in rows]
    go = torch.randn(V, F, generator=gen)
    return V, F, rows, _idx(V, rows, seed, mode), tables, go


# ---- readout cases --------------------------------------------------------------------------------------------------------------------
READOUT_SIZES = {"one_graph": [37], "mixed": [1, 63, 64, 65, 129, 300]}
READOUT_F = (1, 70, 80, 128)
READOUT_OPS = ("sum", "mean", "max")


def readout_case(sizes_name, F, tie=False):
    """-> sizes, h (V, F) fp32, grad_out (G, F) fp32.  tie: in the second-largest graph two rows share a value above every other one
    in every column (the later row a copy of the earlier), so the maximum is attained twice there."""
    sizes = READOUT_SIZES[sizes_name]
    V = sum(sizes)
    gen = torch.Generator().manual_seed(7 * F + len(sizes))
    h = torch.randn(V, F, generator=gen)
    go = torch.randn(len(sizes), F, generator=gen)
    if tie:
        g = sorted(range(len(sizes)), key=lambda i: sizes[i])[-2] if len(sizes) > 1 else 0
        at = sum(sizes[:g])
        h[at + 5] = 9.0
        h[at + 11] = 9.0
    return sizes, h, go
