"""Backward passes of the fused operators.

`AggregateFn`  : forward = pna_segreduce_fwd_f32 (with argmax/argmin recorded), backward =
                 pna_segreduce_bwd_f32 (re-gather + fp32 atomic scatter; see include/pna_amd.h).
`PosttransFn`  : forward = pna_posttrans_f32; its backward is three plain GEMMs (grad_agg, grad_weight,
                 grad_h) -- library matmuls through torch (rocBLAS/hipBLASLt), like the other non-hot
                 linears of the path.
`BnTailFn`     : forward = pna_bn_tail_fwd_f32 (batch-statistics BatchNorm1d + ReLU + residual of PNASimpleLayer's
                 training forward, models/dgl/pna_layer.py:207-213), backward = pna_bn_tail_bwd_f32: two streaming
                 passes each instead of the library's ~10.
No CPU or eager fallback for the forward; gradients of the degree scalers themselves are not needed
(they depend on the graph only).
"""
import ctypes
import os

import torch

from . import _lib, ops

_STAT_AGGS = ("std", "var")


class AggregateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, graph, x, dst_term, edge_term, F, aggregators, n_tower, row_scales, edge_resident,
                edge_weight, col_override):
        if len(set(aggregators)) != len(aggregators):
            raise NotImplementedError("pna_amd: backward needs distinct aggregators")
        csr = graph.csr
        col = None if edge_resident else (csr.col if col_override is None else col_override)
        aggs = list(aggregators)
        # the backward of std / var needs the forward mean (and std): make sure they are computed
        extra = []
        if any(a in _STAT_AGGS for a in aggs):
            if "mean" not in aggs:
                extra.append("mean")
            if "std" not in aggs:
                extra.append("std")
        elif "var_raw" in aggs and "mean" not in aggs:
            extra.append("mean")
        all_aggs = aggs + extra
        want_arg = any(a in ("max", "min") for a in aggs)
        res = ops.segreduce(csr.rowptr, col, x, F, all_aggs, [None], n_tower=n_tower, tower_stride_in=F,
                            dst_term=dst_term, edge_term=edge_term, edge_weight=edge_weight, want_arg=want_arg,
                            heavy=graph.heavy_schedule(), workspace=graph.workspace, items=graph.work_items())
        ident, amx, amn = res if want_arg else (res, None, None)       # (V, T*A'*F) identity-scaled
        V, T, A, A2, S = ident.shape[0], max(1, n_tower), len(aggs), len(all_aggs), len(row_scales)
        iv = ident.view(V, T, A2, F)
        if S == 1 and row_scales[0] is None and not extra:
            out = ident
        else:
            blocks = [iv[:, :, :A] if rs is None else iv[:, :, :A] * rs.view(V, 1, 1, 1) for rs in row_scales]
            out = torch.stack(blocks, dim=2).reshape(V, T * S * A * F)  # tower-major, scaler-major, aggregator-major
        ctx.graph, ctx.F, ctx.aggs, ctx.all_aggs, ctx.T, ctx.col = graph, F, aggs, all_aggs, T, col
        ctx.row_scales = row_scales
        ctx.needs = (x.requires_grad, dst_term is not None and dst_term.requires_grad,
                     edge_term is not None and edge_term.requires_grad)
        ctx.save_for_backward(x, dst_term, edge_term, ident, amx, amn, edge_weight)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, dst_term, edge_term, ident, amx, amn, edge_weight = ctx.saved_tensors
        graph, F, aggs, all_aggs, T = ctx.graph, ctx.F, ctx.aggs, ctx.all_aggs, ctx.T
        V, A, A2, S = ident.shape[0], len(aggs), len(all_aggs), len(ctx.row_scales)
        go = grad_out.reshape(V, T, S, A, F)
        # fold the degree scalers into the gradient of the unscaled aggregates: G_a = sum_s scale_s * dOut[s, a]
        gagg = None
        for s, rs in enumerate(ctx.row_scales):
            term = go[:, :, s] if rs is None else go[:, :, s] * rs.view(V, 1, 1, 1)
            gagg = term if gagg is None else gagg + term
        gagg = gagg.contiguous().view(V, T * A * F)
        csr = graph.csr
        dev = x.device
        need_x, need_d, need_e = ctx.needs
        if edge_weight is not None or "var_raw" in aggs:
            gx, gd, ge = _backward_edges_torch(graph, ctx.col, x, dst_term, edge_term, edge_weight, ident, amx, amn, gagg, aggs,
                                               all_aggs, T, F, need_x, need_d, need_e)
            return (None, gx, gd, ge, None, None, None, None, None, None, None)
        if ctx.col is not None and edge_term is None and ctx.col is csr.col and os.environ.get("PNA_AMD_BWD", "pull") == "pull":
            gx, gd = _backward_pull(graph, x, dst_term, ident, amx, amn, gagg, aggs, all_aggs, T, F, need_x, need_d)
            return (None, gx, gd, None, None, None, None, None, None, None, None)
        b = _lib.PnaSegreduceBwdArgs()
        b.rowptr = _lib.dev_ptr(csr.rowptr, torch.int32, "rowptr")
        b.col = _lib.dev_ptr(ctx.col, torch.int32, "col")
        b.V, b.F = V, F
        b.x, b.ldx = _lib.dev_ptr(x, torch.float32, "x"), x.stride(0)
        if dst_term is not None:
            b.dst_term, b.ld_dst = _lib.dev_ptr(dst_term, torch.float32, "dst_term"), dst_term.stride(0)
        if edge_term is not None:
            b.edge_term, b.ld_edge = _lib.dev_ptr(edge_term, torch.float32, "edge_term"), edge_term.stride(0)
        b.n_tower, b.n_aggr, b.tower_stride_in = T, A, F
        for i, name in enumerate(aggs):
            b.aggr[i] = _lib.AGG_CODES[name]
        b.gagg, b.ld_g, b.tower_stride_g = _lib.dev_ptr(gagg, torch.float32, "gagg"), gagg.stride(0), A * F
        if any(a in _STAT_AGGS for a in aggs):
            base = ident.data_ptr()
            b.mean = ctypes.c_void_p(base + 4 * all_aggs.index("mean") * F)
            b.stdv = ctypes.c_void_p(base + 4 * all_aggs.index("std") * F)
            if "var" in all_aggs:
                b.var = ctypes.c_void_p(base + 4 * all_aggs.index("var") * F)
            b.ld_stat, b.tower_stride_stat = ident.stride(0), A2 * F
        if amx is not None:
            b.argmax, b.argmin, b.ld_arg = (_lib.dev_ptr(amx, torch.int32, "argmax"),
                                            _lib.dev_ptr(amn, torch.int32, "argmin"), amx.stride(0))
        gx = gd = ge = None
        if need_x:
            gx = torch.zeros(x.shape[0], T * F, dtype=torch.float32, device=dev) if ctx.col is not None else \
                torch.empty(x.shape[0], T * F, dtype=torch.float32, device=dev)
            b.grad_x, b.ld_gx = _lib.dev_ptr(gx, torch.float32, "grad_x"), gx.stride(0)
        if need_d:
            gd = torch.zeros(V, T * F, dtype=torch.float32, device=dev)
            b.grad_dst, b.ld_gd = _lib.dev_ptr(gd, torch.float32, "grad_dst"), gd.stride(0)
        if need_e:
            ge = torch.empty(edge_term.shape[0], T * F, dtype=torch.float32, device=dev)
            b.grad_edge, b.ld_ge = _lib.dev_ptr(ge, torch.float32, "grad_edge"), ge.stride(0)
        hs = graph.heavy_schedule()
        if hs.n_heavy > 0:
            b.heavy_threshold, b.seg_len, b.n_heavy, b.n_seg = hs.threshold, hs.seg_len, hs.n_heavy, hs.n_seg
            b.heavy_rows = _lib.dev_ptr(hs.heavy_rows, torch.int32, "heavy_rows")
            b.heavy_segptr = _lib.dev_ptr(hs.heavy_segptr, torch.int32, "heavy_segptr")
            b.seg_heavy = _lib.dev_ptr(hs.seg_heavy, torch.int32, "seg_heavy")
        if need_x or need_d or need_e:
            rc = _lib.lib().pna_segreduce_bwd_f32(ctypes.byref(b), _lib.stream_ptr(dev))
            _lib.check(rc, "pna_segreduce_bwd_f32")
        if gx is not None and x.shape[1] != T * F:
            full = torch.zeros_like(x)
            full[:, :T * F] = gx
            gx = full
        return (None, gx, gd, ge, None, None, None, None, None, None, None)


def _backward_edges_torch(graph, col, x, dst_term, edge_term, w, ident, amx, amn, gagg, aggs, all_aggs, T, F, need_x, need_d, need_e):
    """Backward of the aggregation with per-edge WEIGHTS (the dense variant's adjacency used as a weight,
    models/pytorch/pna/aggregators.py:25,:69: D = sum_k w_k, s = sum_k w_k m_k, q = sum_k w_k m_k^2; max / min over the edges
    with w_k > 0) and of the unclamped PyG variance (`var_raw`, pytorch_geometric/aggregators.py:25-28), as torch tensor ops
    over the edge list:

        dL/dm_k = w_k [ G_sum + G_mean / D + (G_var [var > 0] + G_var_raw + G_std [var > 0] / (2 std)) (2 / D) (m_k - mean) ]
                  + [k = argmax] G_max + [k = argmin] G_min

    The forward is the HIP kernel; these configurations (small dense graphs, the exotic registry entries) are off the hot path,
    so their backward does not have a kernel of its own -- like the GEMMs of the posttrans backward it runs on the GPU
    through library ops."""
    csr = graph.csr
    V, TF = ident.shape[0], T * F
    A, A2 = len(aggs), len(all_aggs)
    E = int(csr.rowptr[-1].item())
    dev = x.device
    row = csr.row.long()
    cx = col.long() if col is not None else torch.arange(E, device=dev)
    m = x[cx][:, :TF]
    if dst_term is not None:
        m = m + dst_term[row][:, :TF]
    if edge_term is not None:
        m = m + edge_term[:, :TF]
    ww = torch.ones(E, device=dev) if w is None else w.reshape(-1).to(torch.float32)
    D = torch.zeros(V, device=dev).index_add_(0, row, ww).clamp_min(1e-30).unsqueeze(1)
    g4 = gagg.view(V, T, A, F)
    iv = ident.view(V, T, A2, F)

    def G(name):
        return g4[:, :, aggs.index(name)].reshape(V, TF) if name in aggs else None

    base = torch.zeros(V, TF, device=dev)
    if G("sum") is not None:
        base = base + G("sum")
    if G("mean") is not None:
        base = base + G("mean") / D
    r2 = None
    if any(a in aggs for a in ("std", "var", "var_raw")):
        mean = iv[:, :, all_aggs.index("mean")].reshape(V, TF) if "mean" in all_aggs else \
            torch.zeros(V, TF, device=dev).index_add_(0, row, m * ww.unsqueeze(1)) / D
        r2 = torch.zeros(V, TF, device=dev)
        if "std" in aggs or "var" in aggs:
            std = iv[:, :, all_aggs.index("std")].reshape(V, TF)
            pos = (std * std - 1e-5) > 0                      # var > 0  <=>  std > sqrt(eps): the relu mask of the forward
            if G("var") is not None:
                r2 = r2 + G("var") * pos
            if G("std") is not None:
                r2 = r2 + G("std") / (2 * std) * pos
        if G("var_raw") is not None:
            r2 = r2 + G("var_raw")
        r2 = r2 * (2.0 / D)
    dm = base[row]
    if r2 is not None:
        dm = dm + r2[row] * (m - mean[row])
    dm = dm * ww.unsqueeze(1)
    for name, arg in (("max", amx), ("min", amn)):
        g_ = G(name)
        if g_ is None:
            continue
        a_ = arg[:, :TF].long()
        ok = a_ >= 0
        cols = torch.arange(TF, device=dev).unsqueeze(0).expand(V, TF)
        dm.index_put_((a_[ok], cols[ok]), g_[ok], accumulate=True)
    gx = gd = ge = None
    if need_x:
        gx = torch.zeros_like(x)
        gx[:, :TF].index_add_(0, cx, dm)
    if need_d:
        gd = torch.zeros_like(dst_term)
        gd[:, :TF].index_add_(0, row, dm)
    if need_e:
        ge = torch.zeros_like(edge_term)
        ge[:, :TF] = dm
    return gx, gd, ge


def _column_sums(t):
    """t.sum(0) for a tall (M, N) tensor.  torch's reduction over the long outer dimension of a (1e6, 75) tensor takes
    15 ms on this stack (rocBLAS gemv: 10 ms, ones @ t: 1.5 ms); folding 64 rows into one (M/64, 64*N) row first gives the
    reduce kernel a wide inner dimension: 0.07 ms."""
    M, N = t.shape
    t = t.contiguous()
    main = (M // 64) * 64
    out = t[:main].view(-1, 64 * N).sum(0).view(64, N).sum(0) if main else torch.zeros(N, dtype=t.dtype, device=t.device)
    return out + t[main:].sum(0) if main < M else out


def _tall_tn(p, q, chunks=256):
    """p^T q for tall (M, a), (M, b) operands: the reduction runs over M.  As ONE library GEMM the 1e6-long reduction of the C3
    weight gradient ((225 x 1e6)(1e6 x 300)) runs at 44 TF/s -- the output has only 24 tiles; cut into 256 row slabs as a batched
    GEMM + a sum over the slabs it takes 1.27 instead of 3.06 ms (tools/exp_dw_gemm.py [removed in round 5: git history]), and the slab-wise summation is the more
    accurate order."""
    M = p.shape[0]
    if not p.is_cuda or M < 64 * chunks:
        return p.t() @ q
    Mc = M // chunks * chunks
    pc = p if p.is_contiguous() else p.contiguous()
    qc = q if q.is_contiguous() else q.contiguous()
    out = torch.bmm(pc[:Mc].view(chunks, Mc // chunks, -1).transpose(1, 2), qc[:Mc].view(chunks, Mc // chunks, -1)).sum(0)
    if Mc < M:
        out = out + pc[Mc:].t() @ qc[Mc:]
    return out


def _argscatter_sorted(gx, col, amx, amn, gagg, aggs, T, F):
    """grad_x[col[argmax[v, c]], c] += G_max[v, c] (and the min term) without atomics: deterministic, for small graphs."""
    V, TF, A = amx.shape[0], T * F, len(aggs)
    g4 = gagg[:, :T * A * F].reshape(V, T, A, F)
    cols = torch.arange(TF, device=gx.device)
    keys, vals = [], []
    for name, arg in (("max", amx), ("min", amn)):
        if name in aggs and arg is not None:
            G = g4[:, :, aggs.index(name), :].reshape(V, TF)
            e = arg[:, :TF].long()
            ok = e >= 0
            key = col[e.clamp(min=0)].long() * TF + cols
            keys.append(key[ok])
            vals.append(G[ok])
    if not keys:
        return
    key, val = torch.cat(keys), torch.cat(vals)
    order = torch.sort(key, stable=True).indices
    key, val = key[order], val[order].contiguous()
    uniq, counts = torch.unique_consecutive(key, return_counts=True)
    sums = torch.segment_reduce(val, "sum", lengths=counts)
    flat = gx.view(-1)                                       # (contiguous (rows, TF) by construction)
    flat[uniq] = flat[uniq] + sums


def _backward_pull(graph, x, dst_term, ident, amx, amn, gagg, aggs, all_aggs, T, F, need_x, need_d, row_of=None, packed_rows=None, node_of=None):
    """Gradient of the aggregation w.r.t. the source table / destination term WITHOUT one atomic per edge and feature
    (the scatter kernel: 750 M atomics = 11.4 ms on the roofline workload).  With messages m_k = x[u_k] + dst_term[v]:

        dL/dm_k = R1[v] + R2[v] x[u_k] + [k = argmax] G_max[v] + [k = argmin] G_min[v]      (see include/pna_amd.h)

    so  grad_x[u] = sum_{out-edges (u,v)} R1[v]  +  x[u] * sum_{out-edges} R2[v]  +  (max / min terms):
    pna_segreduce_bwd_rowprep_f32 writes the (V, 2TF) table [R1|R2] (and grad_dst), the two sums are a PULL over the
    TRANSPOSED graph with the forward kernel ("sum", 2T towers), pna_segreduce_bwd_argscatter_f32 adds the max / min
    terms with V*T*F atomics each."""
    from . import functional as PF
    from .graph import Graph
    csr = graph.csr
    dev = x.device
    V, TF = gagg.shape[0], T * F                            # (row_of: ident / amx / amn hold node v's row at row_of[v] -- plan order)
    A, A2 = len(aggs), len(all_aggs)
    has_var = any(a in _STAT_AGGS for a in aggs)
    if csr.col.numel() == 0:
        # a graph without edges: no message, so both gradients are zero -- and there is no index array (col, col_t, rank_t) to hand to a
        # kernel (pna_segreduce_bwd_pull_f32 and _argscatter_f32 refuse null pointers)
        return (torch.zeros_like(x) if need_x else None), (torch.zeros(V, TF, dtype=torch.float32, device=dev) if need_d else None)
    b = _lib.PnaSegreduceBwdArgs()
    if row_of is not None:
        b.stat_row_of = _lib.dev_ptr(row_of, torch.int32, "stat_row_of")
    if node_of is not None:                                 # (the inverse map: rowprep walks ident's rows in sequence)
        b.stat_node_of, b.stat_rows = _lib.dev_ptr(node_of, torch.int32, "stat_node_of"), node_of.numel()
    b.rowptr = _lib.dev_ptr(csr.rowptr, torch.int32, "rowptr")
    b.col = _lib.dev_ptr(csr.col, torch.int32, "col")
    b.V, b.F = V, F
    if dst_term is not None:
        b.dst_term, b.ld_dst = _lib.dev_ptr(dst_term, torch.float32, "dst_term"), dst_term.stride(0)
    b.n_tower, b.n_aggr, b.tower_stride_in = T, A, F
    for i, name in enumerate(aggs):
        b.aggr[i] = _lib.AGG_CODES[name]
    b.gagg, b.ld_g, b.tower_stride_g = _lib.dev_ptr(gagg, torch.float32, "gagg"), gagg.stride(0), A * F
    if has_var:
        base = ident.data_ptr()
        b.mean = ctypes.c_void_p(base + 4 * all_aggs.index("mean") * F)
        b.stdv = ctypes.c_void_p(base + 4 * all_aggs.index("std") * F)
        if "var" in all_aggs:
            b.var = ctypes.c_void_p(base + 4 * all_aggs.index("var") * F)
        b.ld_stat, b.tower_stride_stat = ident.stride(0), A2 * F
    if amx is not None:
        b.argmax, b.argmin, b.ld_arg = (_lib.dev_ptr(amx, torch.int32, "argmax"), _lib.dev_ptr(amn, torch.int32, "argmin"),
                                        amx.stride(0))
    gd = None
    if need_d:
        gd = torch.empty(V, TF, dtype=torch.float32, device=dev)
        b.grad_dst, b.ld_gd = _lib.dev_ptr(gd, torch.float32, "grad_dst"), gd.stride(0)
    if row_of is not None and not (need_x and amx is not None and has_var and "max" in aggs and "min" in aggs and 4 <= F <= 256
                                   and csr.max_degree < 65535 and x.stride(1) == 1):
        raise RuntimeError("_backward_pull: row_of needs the ranked pull (mean, max, min, std; 4 <= F <= 256; degrees < 65535)")
    ranked = (need_x and amx is not None and has_var and "max" in aggs and "min" in aggs and 4 <= F <= 256 and csr.max_degree < 65535
              and x.stride(1) == 1 and os.environ.get("PNA_AMD_BWD_ARGS", "pull") == "pull")
    if packed_rows is not None and not ranked:
        raise RuntimeError("_backward_pull: packed_rows (in place) needs the ranked pull")
    # round 6: the pull over PER-EDGE rows (pna_segreduce_bwd_pull_args.edge_rows): one tower, no destination term, the four standard
    # aggregators -- PNASimpleLayer's backward.  2 x 4F bytes per out-edge instead of 20F + ranks; bit-identical gradients.
    edge_mode = (ranked and PULL_EDGE_ROWS and T == 1 and dst_term is None and set(aggs) == {"mean", "std", "max", "min"} and not need_d
                 and csr.col.numel() * ((F + 15) // 16 * 16) * 4 < (1 << 36))
    if edge_mode:
        b.stat_node_of, b.stat_rows = None, 0               # (the per-edge pass walks the FORWARD work list: a node's statistics through row_of)
        # rows at a 64-byte aligned pitch (F = 75: 80 floats): a 300-byte row then lies on exactly three 128-byte lines wherever it starts
        # (at the packed pitch of 76 floats: 3.4 on average, and the writer's last sector of a row is shared with the next row's first)
        Fp = (F + 15) // 16 * 16
        E_ = csr.col.numel()
        flat = graph.__dict__.get("_pna_amd_edge_rows")     # (3.2 GB at C3: kept on the graph like the packed pull rows, sized for the widest layer seen)
        if flat is None or flat.numel() < (E_ + V) * Fp or flat.device != dev:
            flat = graph.__dict__["_pna_amd_edge_rows"] = torch.empty(max((E_ + V) * Fp, 1), dtype=torch.float32, device=dev)
        P = flat[:E_ * Fp].view(E_, Fp)
        table = flat[E_ * Fp:(E_ + V) * Fp].view(V, Fp)       # R2: its own (V, Fp) table behind the edge rows
        ranks = None
    elif ranked and (PULL_PACKED or packed_rows is not None):
        # one row [R1 | R2 | G_max | G_min | 16-bit ranks] per node at a 128-byte aligned pitch: an out-edge of the pull reads 12 cache
        # lines at F = 75 instead of ~14.7 for three separate pieces (pna_segreduce_bwd_pull_f32, packed rows).  packed_rows: the
        # caller's buffer, whose first 4 T F columns ARE gagg (aggs = mean, std, max, min): rowprep works in place
        pitch = (5 * TF + 31) // 32 * 32
        packed = torch.empty(V, pitch, dtype=torch.float32, device=dev) if packed_rows is None else packed_rows
        table = packed[:, :2 * TF]
        ranks = packed.view(torch.int16)[:, 8 * TF:10 * TF]
    else:
        table = torch.empty(V, TF * (2 if has_var else 1), dtype=torch.float32, device=dev)
        ranks = None
    if not ranked:                                          # (the ranked pull below runs this pass itself, with the ranks)
        rc = _lib.lib().pna_segreduce_bwd_rowprep_f32(ctypes.byref(b), _lib.dev_ptr(table, torch.float32, "table"), table.stride(0),
                                                      _lib.stream_ptr(dev))
        _lib.check(rc, "pna_segreduce_bwd_rowprep_f32")
    gx = None
    if need_x:
        gT = getattr(graph, "_pna_amd_transposed", None)
        if gT is None or gT.num_nodes != x.shape[0]:
            gT = Graph(csr.row.long(), csr.col.long(), x.shape[0])        # edge (v -> u): pulls row v of the table into u
            graph._pna_amd_transposed = gT
        if ranked:
            # round 3: the max / min terms inside the SAME pull (pna_segreduce_bwd_pull_f32): per out-edge the rank of the edge in its
            # destination's list is compared with the 16-bit ranks of argmax / argmin -- no scattered atomics (3.8 ms at C3)
            tcsr = gT.csr
            rank_t = getattr(gT, "_pna_amd_rank_t", None)
            if rank_t is None:                                # position of every transposed edge in its destination's in-edge list
                rank_t = (tcsr.eid.to(torch.int64) - csr.rowptr.to(torch.int64)[tcsr.col.long()]).to(torch.int32).contiguous()
                gT._pna_amd_rank_t = rank_t
            items = gT.work_items()
            hs = gT.heavy_schedule()
            gx = torch.empty(x.shape[0], TF, dtype=torch.float32, device=dev)
            if hs.n_heavy > 0:
                gx.index_fill_(0, hs.heavy_rows.long(), 0.0)  # hub sources: their segments add atomically
            if ranks is None and not edge_mode:
                ranks = torch.empty(V, 2 * TF, dtype=torch.int16, device=dev)
            b.x, b.ldx = _lib.dev_ptr(x, torch.float32, "x"), x.stride(0)
            b.grad_x, b.ld_gx = _lib.dev_ptr(gx, torch.float32, "grad_x"), gx.stride(0)
            q = _lib.PnaSegreduceBwdPullArgs()
            q.base = ctypes.cast(ctypes.pointer(b), ctypes.c_void_p)
            q.table, q.ld_table = _lib.dev_ptr(table, torch.float32, "table"), table.stride(0)
            q.col_t, q.rank_t = _lib.dev_ptr(tcsr.col, torch.int32, "col_t"), _lib.dev_ptr(rank_t, torch.int32, "rank_t")
            q.items_t, q.n_items_t, q.run_rowprep = _lib.dev_ptr(items, torch.int32, "items_t"), items.shape[0], 1
            if edge_mode:
                pos_t = getattr(gT, "_pna_amd_pos_t", None)       # position of every transposed edge in the forward CSR
                if pos_t is None:
                    pos_t = gT._pna_amd_pos_t = tcsr.eid.to(torch.int32).contiguous()
                fitems = graph.work_items()
                q.edge_rows, q.ld_edge = _lib.dev_ptr(P, torch.float32, "edge_rows"), P.stride(0)
                q.pos_t = _lib.dev_ptr(pos_t, torch.int32, "pos_t")
                q.items, q.n_items = _lib.dev_ptr(fitems, torch.int32, "items"), fitems.shape[0]
            else:
                q.ranks, q.ld_rank = _lib.dev_ptr(ranks, torch.int16, "ranks"), ranks.stride(0)
            rc = _lib.lib().pna_segreduce_bwd_pull_f32(ctypes.byref(q), _lib.stream_ptr(dev))
            _lib.check(rc, "pna_segreduce_bwd_pull_f32")
            if x.shape[1] != TF:
                full = torch.zeros_like(x)
                full[:, :TF] = gx
                gx = full
            return gx, gd
        S = PF.aggregate(gT, table, F, ["sum"], n_tower=table.shape[1] // F)
        gx = (S[:, :TF] + x[:, :TF] * S[:, TF:]) if has_var else S
        gx = gx.contiguous()
        if amx is not None:
            if F < 4 or os.environ.get("PNA_AMD_BWD_DETERMINISTIC", "0") == "1":
                # Narrow towers (the dense variant's multitask nets: F = 2 or 4 per tower, a few thousand nodes) do not qualify for
                # the ranked pull (4 features per lane); the atomic scatter's order varies from run to run, which Adam amplifies over
                # a training trace (tests/test_gpu_train_trace.py: 2.8e-3 in 2 of 31 runs).  Here the max / min terms are summed in a
                # FIXED order: stable sort of (source, feature) keys, one sequential sum per key.
                _argscatter_sorted(gx, csr.col, amx, amn, gagg, aggs, T, F)
            else:
                b.grad_x, b.ld_gx = _lib.dev_ptr(gx, torch.float32, "grad_x"), gx.stride(0)
                rc = _lib.lib().pna_segreduce_bwd_argscatter_f32(ctypes.byref(b), _lib.stream_ptr(dev))
                _lib.check(rc, "pna_segreduce_bwd_argscatter_f32")
        if x.shape[1] != TF:
            full = torch.zeros_like(x)
            full[:, :TF] = gx
            gx = full
    return gx, gd


def M_rows(t):
    return t.shape[0]


def _rows(t):
    """t as rows the one-call routes take: unit column stride and a row pitch of at least the width, anything else copied once (an
    expanded tensor has pitch 0, and every C entry refuses a pitch below the width).  A tensor that qualifies comes back as it is, no
    copy; so does one of at most one row with unit column stride, whose pitch nothing reads.  The copy is a clone in row-major strides:
    `contiguous()` returns a tensor of width 1 with column stride != 1 as it is."""
    if t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]):
        return t
    return t.clone(memory_format=torch.contiguous_format)


DAGG_GROUPED = os.environ.get("PNA_AMD_DAGG_GROUPED", "1") != "0"     # 0: d agg = gy W^T as the three-block bf16 x 3 contraction (rounds 3-5)
PULL_EDGE_ROWS = os.environ.get("PNA_AMD_PULL_EDGE_ROWS", "1") != "0"   # 0: the ranked pull of rounds 3-5 (R1 | R2 | G_max | G_min | ranks per out-edge)
PULL_PACKED = os.environ.get("PNA_AMD_PULL_PACKED", "1") != "0"   # 0: table, aggregate gradient and ranks as three separate rows (round 3)
DW_KERNEL = os.environ.get("PNA_AMD_DW_KERNEL", "1") != "0"    # 0: the library route (slab-batched GEMM) for the weight gradient
DW_GROUPED = os.environ.get("PNA_AMD_DW_GROUPED", "1") != "0"  # 0: per-row scalers (three scaled copies of gy inside the kernel)
DW_MIN_ROWS = int(os.environ.get("PNA_AMD_DW_MIN_ROWS", "4096"))  # below: a molecule batch's product is one small library GEMM


class SimpleLayerPlanFn(torch.autograd.Function):
    """Gather + posttrans contraction of PNASimpleLayer in TRAINING on a large whole graph, in the graph's DEGREE-PLAN row order
    (models/dgl/pna_layer.py:197-206; round 4).  Forward: the arg-tracking gather writes the aggregate and the arg indices in plan
    order (the work list's rows), so the contraction is the grouped one -- ONE combined block W_D per degree tile instead of three
    scaler blocks (a third of the multiply-adds: 0.72 -> ~0.3 ms at C3) -- and scatters y to node order.  Backward: the weight
    gradient reads the aggregate in sequence (pna_posttrans_dw_grouped_f32, a_plan_order), d agg is the three-block contraction in
    node order as before, rowprep finds a node's mean / std / arg indices through the plan's row map (stat_row_of), the pull is
    unchanged.  Same arithmetic per row as the node-order route up to the combined weight's rounding (the inference paths' relation)."""

    @staticmethod
    def forward(ctx, h, weight, bias, layer, graph):
        from . import degree_groups as DG, functional as PF
        from .dgl.pna_layer import _row_scales, _avg_log_value
        plan = DG.plan_of(graph)
        F, N = layer.in_dim, layer.out_dim
        K = 4 * F
        aggs = list(layer.aggregators)
        x = _rows(h)
        csr = graph.csr
        dev = h.device
        agg = torch.empty(plan.rows, DG.agg_pitch(K), dtype=torch.float32, device=dev)[:, :K]
        agg, amx, amn = ops.segreduce(csr.rowptr, csr.col, x, F, aggs, (None,), tower_stride_in=F, out=agg, want_arg=True, arg_rows=plan.rows,
                                      heavy=graph.heavy_schedule(), workspace=graph.workspace, items=plan.items, heavy_out=plan.heavy_out,
                                      tune=dict(generic=2))
        scales = _row_scales(graph, layer.scalers, layer.avg_d, dev)
        w = weight if weight.stride(-1) == 1 else weight.contiguous()
        y = torch.empty(h.shape[0], N, dtype=torch.float32, device=dev)
        if plan.G:
            img, stride = DG.combined_images(w, K, scales, plan)
            ops.posttrans(agg[:plan.NV], K, w, [None], bias, out=y, row_perm=plan.perm, tile_image=plan.tile_image, w_img=img,
                          image_stride=stride, n_out=N)
        if plan.NR:
            rest_scales = plan.rest_scales(tuple(layer.scalers) + (_avg_log_value(layer.avg_d),), scales)
            ops.posttrans(agg[plan.NV:], K, w, rest_scales, bias, out=y, row_perm=plan.perm_rest, n_out=N)
        ctx.graph, ctx.plan, ctx.scales, ctx.aggs, ctx.F, ctx.N = graph, plan, scales, aggs, F, N
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, agg, amx, amn)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, agg, amx, amn = ctx.saved_tensors
        graph, plan, scales, aggs, F, N = ctx.graph, ctx.plan, ctx.scales, ctx.aggs, ctx.F, ctx.N
        K, S = 4 * F, len(scales)
        gy = _rows(gy)
        g_w = g_b = g_h = None
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            res = ops.posttrans_dw_grouped(gy, agg, K, None, scales, plan, want_bias=want_b, a_plan_order=True)
            if res is None:
                raise RuntimeError("SimpleLayerPlanFn: shape outside pna_posttrans_dw_grouped_f32 (the layer checks it before taking this path)")
            g_w, g_b = res
        if ctx.needs_input_grad[0]:
            # d agg = sum_s scale_s (.) (gy W_s), node order, written STRAIGHT into the pull's packed table rows with the aggregator
            # blocks in the order [mean | std | max | min]: rowprep then turns the first two blocks into R1 | R2 in place -- no
            # separate (V, 4F) gradient tensor, no copy of G_max | G_min (rowprep 0.95 -> ~0.65 ms at C3)
            V = gy.shape[0]
            order = plan.__dict__.get("_dagg_order")                                                           # rows of W^T: mean, std, max, min
            if order is None or order.numel() != K or order.device != gy.device:
                order = plan.__dict__["_dagg_order"] = torch.cat([torch.arange(a * F, (a + 1) * F, device=gy.device) for a in (0, 3, 1, 2)])
            wt = torch.cat([weight[:, s * K:(s + 1) * K].t().index_select(0, order) for s in range(S)], dim=1).contiguous()     # (K, S*N)
            pitch = (5 * F + 31) // 32 * 32
            # (1.5 GB at C3, live only inside this call: kept on the plan -- allocated per step it makes the caching allocator split and
            # re-grow its largest block as soon as the training loop frees its gradients every iteration: +1.8 ms per step measured)
            # One flat buffer sized for the widest layer seen on this graph, viewed at this layer's pitch: a net whose layers differ
            # in F does not reallocate it in every layer's backward.  One backward at a time per Graph (the buffer, the
            # plan's weight-gradient workspace and graph.workspace are shared: the one-caller-per-Graph rule of functional.py).
            flat = plan.__dict__.get("_pull_rows")
            if flat is None or flat.numel() < V * pitch or flat.device != gy.device:
                flat = plan.__dict__["_pull_rows"] = torch.empty(V * pitch, dtype=torch.float32, device=gy.device)
            packed = flat[:V * pitch].view(V, pitch)
            if DAGG_GROUPED and plan.G and ops.project_applies(gy, N, K) and plan.NV % 128 == 0:
                # rows of the degree groups: ONE combined 4F x N weight per group (W_D^T = sum_s scale_s(D) W_s^T: a third of the
                # multiply-adds), resident in LDS, exact fp32 products (pna_project_grouped_f32); the three-block contraction took 1.11 ms
                # at C3.  The few rows no group holds: the three-block contraction over their compact list.
                with torch.no_grad():
                    sc = plan.group_scaler_values(scales)                                                  # (G, S)
                    wb = weight.reshape(N, S, K).index_select(2, order)                                     # (N, S, 4F) in the packed order
                    wg = torch.einsum("gs,nsk->gkn", sc, wb).contiguous()                                  # (G, 4F, N) = W_D^T per group
                perm_g, group_g = plan.tiles_by_group()
                g_agg = ops.project_grouped(gy, N, wg, perm_g, group_g, out=packed[:, :K])
                if plan.NR:
                    rest = plan.rest_rows
                    g_rest = ops.posttrans(gy.index_select(0, rest), N, wt, [None if r is None else r.index_select(0, rest) for r in scales], None,
                                           arith="bf16x3")
                    g_agg.index_copy_(0, rest, g_rest)
            else:
                g_agg = ops.posttrans(gy, N, wt, scales, None, arith="bf16x3", out=packed[:, :K])
            g_h, _ = _backward_pull(graph, x, None, agg, amx, amn, g_agg, ["mean", "std", "max", "min"], aggs, 1, F, True, False,
                                    row_of=plan.vmap32(), packed_rows=packed, node_of=plan.node_of_rows())
        return g_h, g_w, g_b, None, None


def simple_layer_plan_applies(layer, graph, h):
    """Whether SimpleLayerPlanFn serves this training forward: a large whole graph with a degree plan, the four standard aggregators,
    three scalers, one-layer posttrans, out_dim <= 80 (the grouped contraction and the weight-gradient kernel)."""
    from . import degree_groups as DG
    from .graph import Graph
    F, N = layer.in_dim, layer.out_dim
    if not (PLAN_TRAIN and h.is_cuda and h.dtype == torch.float32 and type(graph) is Graph and h.shape[1] == F and 4 <= F and N <= 80
            and len(layer.scalers) == 3 and tuple(layer.aggregators) == ("mean", "max", "min", "std") and layer.posttrans.is_affine
            and ops.POSTTRANS_ARITH != "f32" and graph.csr.max_degree < 65535 and 4 * F + 1 <= 384):
        return False
    V = h.shape[0]
    if not DG.applies(graph, V, N, 3, layer.aggregators, F=F, n_edges=graph.csr.col.numel(), x_rows=V):
        return False
    plan = DG.plan_of(graph)
    return plan.NV % 128 == 0 and plan.NRp % 192 == 0 and plan.items is not None


PLAN_TRAIN = os.environ.get("PNA_AMD_PLAN_TRAIN", "1") != "0"   # 0: the node-order training route (AggregateFn + PosttransFn)


class PosttransFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, agg, K, weight, bias, row_scales, h_self, degree_graph=None):
        w = weight if weight.stride(-1) == 1 else weight.contiguous()
        agg, h_self = _rows(agg), None if h_self is None else _rows(h_self)
        y = ops.posttrans(agg, K, w, row_scales, bias, h_self)
        ctx.K, ctx.row_scales = K, row_scales
        ctx.degree_graph = degree_graph                   # the graph whose DEGREE scalers row_scales are (or None): see backward
        ctx.save_for_backward(agg, weight, h_self)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        agg, weight, h_self = ctx.saved_tensors
        K, scales = ctx.K, ctx.row_scales
        S = len(scales)
        gy = _rows(gy)                                    # (the weight-gradient kernels take a row pitch: an expand has none)
        Kh = 0 if h_self is None else h_self.shape[1]
        a = agg[:, :K]
        # G = [scale_0 (.) gy | scale_1 (.) gy | ...]  (M, S*N): one operand for both big products, so that each is ONE
        # library GEMM (three (N x M)(M x K) products with M = 1e6 ran at 20 TF/s; the fused (S*N x M)(M x K) one tiles better)
        N = gy.shape[1]
        _G = []

        def scaled_blocks():                              # (only the library routes below need the scaled copies of gy)
            if not _G:
                if S == 1 and scales[0] is None:
                    _G.append(gy)
                else:                                     # written block by block into place (mul + cat cost a second pass: 0.65 ms at C3)
                    G3 = gy.new_empty(gy.shape[0], S, N)
                    for s, rs in enumerate(scales):
                        if rs is None:
                            G3[:, s].copy_(gy)
                        else:
                            torch.mul(gy, rs.unsqueeze(1), out=G3[:, s])
                    _G.append(G3.view(gy.shape[0], S * N))
            return _G[0]
        g_agg = g_w = g_b = g_h = None
        if ctx.needs_input_grad[0]:
            # d agg = sum_s scale_s (.) (gy W_s) is the forward contraction with the roles of K and N swapped: input gy (M, N),
            # "weight" W_s^T (K, N) per scaler, per-row scalers applied to the accumulators.  On large batches it runs on the
            # same bf16x3 kernel as the forward (fp32-level accuracy) instead of a library fp32 GEMM: 3.0 -> ~0.9 ms at C3
            if gy.is_cuda and S <= 3 and N >= 4 and M_rows(gy) >= ops.X3_MIN_ROWS and ops.POSTTRANS_ARITH in ("auto", "bf16x3"):
                wt = torch.cat([weight[:, Kh + s * K:Kh + (s + 1) * K].t() for s in range(S)], dim=1).contiguous()   # (K, S*N)
                g_agg = ops.posttrans(gy.contiguous(), N, wt, scales, None, arith="bf16x3")
            else:
                g_agg = scaled_blocks() @ torch.cat([weight[:, Kh + s * K:Kh + (s + 1) * K] for s in range(S)], dim=0)
            if agg.shape[1] != K:
                full = torch.zeros_like(agg)
                full[:, :K] = g_agg
                g_agg = full
        want_b = ctx.has_bias and ctx.needs_input_grad[3]
        if ctx.needs_input_grad[2]:
            # round 4: weight (and bias) gradient on the hand-written bf16x3 kernel (pna_posttrans_dw_f32: no scaled copies of gy, no
            # vendor GEMM on the training step; deterministic); shapes outside it keep the slab-batched library route
            res = None
            if DW_KERNEL and gy.is_cuda and M_rows(gy) >= DW_MIN_ROWS:
                dg = ctx.degree_graph
                if dg is not None and DW_GROUPED and dg.num_nodes == M_rows(gy):
                    # the rows in the graph's degree-plan order: 32 consecutive rows share their scaler values (ops.posttrans_dw_grouped).
                    # Only for a graph that HAS a plan or is large enough for the forward to build one (DG.MIN_ROWS): a per-batch graph
                    # of a few thousand nodes -- a fresh Graph every training step -- must not pay the plan's sorts and host syncs inside
                    # every backward and then throw it away; it takes pna_posttrans_dw_f32 below, which needs no plan
                    from . import degree_groups as DG
                    plan = dg.__dict__.get("_pna_amd_degree_plan")
                    if plan is None and dg.num_nodes >= DG.MIN_ROWS:
                        plan = DG.plan_of(dg)
                    if plan is not None and plan.G > 0 and plan.NR <= DG.MAX_REST_FRACTION * dg.num_nodes:
                        res = ops.posttrans_dw_grouped(gy, a, K, h_self, scales, plan, want_bias=want_b)
                if res is None:
                    res = ops.posttrans_dw(gy, a, K, h_self, scales, want_bias=want_b)
            if res is not None:
                g_w, g_b = res
            else:
                gw = _tall_tn(scaled_blocks(), a)                                  # (S*N, K): block s = (scale_s gy)^T a
                parts = ([_tall_tn(gy, h_self)] if Kh else []) + [gw[s * N:(s + 1) * N] for s in range(S)]
                g_w = torch.cat(parts, dim=1)
        if want_b and g_b is None:
            g_b = _column_sums(gy)
        if Kh and ctx.needs_input_grad[5]:
            g_h = gy @ weight[:, :Kh]
        return g_agg, None, g_w, g_b, None, g_h, None


def bn_tail_applies(bn, y, residual):
    """Whether BnTailFn serves nn.BatchNorm1d `bn` in training mode on `y` (+ residual): fp32 rows on a GPU, batch statistics
    with an exponential running average (momentum=None, the cumulative average, and M < 2 -- where torch raises -- stay torch's)."""
    return (BN_TAIL and bn.training and y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1
            and 2 <= y.shape[0] and 1 <= y.shape[1] <= 128 and bn.track_running_stats and bn.momentum is not None
            and bn.running_mean is not None
            and (residual is None or (residual.shape == y.shape and residual.dtype == torch.float32 and residual.is_cuda)))


BN_TAIL = os.environ.get("PNA_AMD_BN_TAIL", "1") != "0"


def bn_relu_residual(bn, y, residual=None, relu=True):
    """residual + relu(bn(y)) for nn.BatchNorm1d `bn` in TRAINING mode: updates the running statistics and
    num_batches_tracked like the module's own forward."""
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return BnTailFn.apply(y, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, float(bn.momentum), float(bn.eps), bool(relu))


class BnTailFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, gamma, beta, residual, running_mean, running_var, momentum, eps, relu):
        y = _rows(y)
        M, N = y.shape
        dev = y.device
        res = None if residual is None else _rows(residual)
        out = torch.empty(M, N, dtype=torch.float32, device=dev)
        stats = torch.empty(2, N, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.lib().pna_bn_tail_workspace_bytes(M, N) // 4, dtype=torch.float32, device=dev)
        a = _lib.PnaBnTailArgs()
        a.y, a.ldy, a.M, a.N, a.relu = _lib.dev_ptr(y, torch.float32, "y"), y.stride(0), M, N, int(relu)
        if gamma is not None:
            a.gamma, a.beta = _lib.dev_ptr(gamma, torch.float32, "gamma"), _lib.dev_ptr(beta, torch.float32, "beta")
        a.eps, a.momentum = eps, momentum
        a.running_mean, a.running_var = _lib.dev_ptr(running_mean, torch.float32, "running_mean"), _lib.dev_ptr(running_var, torch.float32, "running_var")
        if res is not None:
            a.residual, a.ld_res = _lib.dev_ptr(res, torch.float32, "residual"), res.stride(0)
        a.out, a.ld_out = _lib.dev_ptr(out, torch.float32, "out"), out.stride(0)
        a.save_mean, a.save_invstd = _lib.dev_ptr(stats[0], torch.float32, "save_mean"), _lib.dev_ptr(stats[1], torch.float32, "save_invstd")
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        _lib.check(_lib.lib().pna_bn_tail_fwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_bn_tail_fwd_f32")
        ctx.save_for_backward(y, gamma, beta, stats)
        ctx.relu, ctx.has_res, ctx.eps = relu, residual is not None, eps
        return out

    @staticmethod
    def backward(ctx, go):
        y, gamma, beta, stats = ctx.saved_tensors
        M, N = y.shape
        dev = y.device
        go = _rows(go)
        gy = torch.empty(M, N, dtype=torch.float32, device=dev)
        gwb = torch.empty(2, N, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.lib().pna_bn_tail_workspace_bytes(M, N) // 4, dtype=torch.float32, device=dev)
        a = _lib.PnaBnTailArgs()
        a.y, a.ldy, a.M, a.N, a.relu = _lib.dev_ptr(y, torch.float32, "y"), y.stride(0), M, N, int(ctx.relu)
        if gamma is not None:
            a.gamma, a.beta = _lib.dev_ptr(gamma, torch.float32, "gamma"), _lib.dev_ptr(beta, torch.float32, "beta")
        a.eps, a.momentum = ctx.eps, -1.0
        a.save_mean, a.save_invstd = _lib.dev_ptr(stats[0], torch.float32, "save_mean"), _lib.dev_ptr(stats[1], torch.float32, "save_invstd")
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        a.grad_out, a.ld_go = _lib.dev_ptr(go, torch.float32, "grad_out"), go.stride(0)
        a.grad_y, a.ld_gy = _lib.dev_ptr(gy, torch.float32, "grad_y"), gy.stride(0)
        a.grad_gamma, a.grad_beta = _lib.dev_ptr(gwb[0], torch.float32, "grad_gamma"), _lib.dev_ptr(gwb[1], torch.float32, "grad_beta")
        _lib.check(_lib.lib().pna_bn_tail_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_bn_tail_bwd_f32")
        has_affine = gamma is not None
        return (gy, gwb[0] if has_affine and ctx.needs_input_grad[1] else None, gwb[1] if has_affine and ctx.needs_input_grad[2] else None,
                go if ctx.has_res else None, None, None, None, None, None)


def _transposed_whole_rows(graph):
    """(col_t, rank_t, items_t) of the one-call training backwards' pull: the transposed graph's destinations, the position of every
    transposed edge in its destination's in-edge list, and one whole-row record per source row (no hub segments: no atomics).  Kept on
    the graph, like the pull of the generic route keeps them."""
    from .graph import Graph
    csr = graph.csr
    V = graph.num_nodes
    gT = getattr(graph, "_pna_amd_transposed", None)
    if gT is None or gT.num_nodes != V:
        gT = graph._pna_amd_transposed = Graph(csr.row.long(), csr.col.long(), V)     # edge (v -> u): pulls row v into u
    tcsr = gT.csr
    rank_t = getattr(gT, "_pna_amd_rank_t", None)
    if rank_t is None:
        rank_t = (tcsr.eid.to(torch.int64) - csr.rowptr.to(torch.int64)[tcsr.col.long()]).to(torch.int32).contiguous()
        gT._pna_amd_rank_t = rank_t
    return tcsr.col, rank_t, gT.work_items(threshold=1 << 30)


class _GraphScratchPlan:
    """What the one-call training plans share: the call's workspace out of the graph's reusable scratch (Graph.workspace: allocated once
    per graph, grown to the widest layer seen; every launch writes what it reads, nothing is carried from the forward to the backward).
    One caller at a time per Graph (functional.py's rule for the shared scratch)."""

    def take_workspace(self, graph, nbytes):
        ws = graph.workspace(nbytes + 256)
        self.ws = ws[(-ws.data_ptr() // 4) % 64:][:nbytes // 4]                 # 256-byte aligned
        self.nbytes = nbytes


class _SmallTrainPlan(_GraphScratchPlan):
    """What one call of SimpleLayerSmallTrainFn needs besides the layer's tensors: the transposed graph's arrays (kept on the graph, like
    the pull of the generic route keeps them) and the call's workspace.  Nothing here depends on weight values."""

    def __init__(self, graph, F, N, S, dev):
        csr = graph.csr
        V, E = graph.num_nodes, int(csr.col.numel())
        self.V, self.E, self.F, self.N, self.S, self.dev = V, E, F, N, S, dev
        self.col_t, self.rank_t, self.items_t = _transposed_whole_rows(graph)
        nbytes = _lib.lib().pna_simple_train_workspace_bytes(V, E, F, N, S)
        if nbytes < 0:
            raise RuntimeError("SimpleLayerSmallTrainFn: shape outside pna_simple_train_*_f32 (the layer checks it before taking this path)")
        self.take_workspace(graph, nbytes)

    def new_saved(self):
        """The state one forward leaves for its backward -- a (V, 4F) | z (V, N) | save_mean, save_invstd [N] in one buffer, argmax |
        argmin (V, F) in another.  Per CALL, not per plan: two layers of one shape on one graph are both alive until their backwards."""
        V, F, N = self.V, self.F, self.N
        fbuf = torch.empty(V * 4 * F + V * N + 2 * N, dtype=torch.float32, device=self.dev)
        ibuf = torch.empty(2, V, F, dtype=torch.int32, device=self.dev)
        return fbuf, ibuf

    def args(self, graph, h, w, bias, bn, scales, residual, saved):
        csr = graph.csr
        a = _lib.PnaSimpleTrainArgs()
        a.rowptr = _lib.dev_ptr(csr.rowptr, torch.int32, "rowptr")
        a.col = _lib.dev_ptr(csr.col, torch.int32, "col") if self.E else None
        a.V, a.E, a.F, a.N, a.n_scaler, a.residual = self.V, self.E, self.F, self.N, self.S, int(residual)
        a.h, a.ldh = _lib.dev_ptr(h, torch.float32, "h"), h.stride(0)
        for s, rs in enumerate(scales):
            if rs is not None:
                a.row_scale[s] = _lib.dev_ptr(rs, torch.float32, "row_scale").value
        a.w, a.ldw = _lib.dev_ptr(w, torch.float32, "weight"), w.stride(0)
        a.bias = _lib.dev_ptr(bias, torch.float32, "bias")
        if bn.weight is not None:
            a.gamma, a.beta = _lib.dev_ptr(bn.weight, torch.float32, "gamma"), _lib.dev_ptr(bn.bias, torch.float32, "beta")
        a.eps, a.momentum = float(bn.eps), float(bn.momentum)
        a.running_mean = _lib.dev_ptr(bn.running_mean, torch.float32, "running_mean")
        a.running_var = _lib.dev_ptr(bn.running_var, torch.float32, "running_var")
        fbuf, ibuf = saved
        V, F, N = self.V, self.F, self.N
        base = fbuf.data_ptr()
        a.a, a.z = base, base + 4 * V * 4 * F
        a.save_mean, a.save_invstd = base + 4 * (V * 4 * F + V * N), base + 4 * (V * 4 * F + V * N + N)
        a.argmax, a.argmin = ibuf.data_ptr(), ibuf.data_ptr() + 4 * V * F
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.nbytes
        return a


class SimpleLayerSmallTrainFn(torch.autograd.Function):
    """PNASimpleLayer's training forward (gather, scalers, posttrans Linear, batch-statistics BatchNorm, ReLU, residual:
    models/dgl/pna_layer.py:197-213) on a molecule-sized batch as ONE C call (pna_simple_train_fwd_f32) and its backward as one
    (pna_simple_train_bwd_f32).  The workspace is the graph's scratch; nothing is cached on weight versions.  The output and the
    gradients are fresh tensors per call (autograd and the optimiser keep them), and so is the state a forward saves for its backward."""

    @staticmethod
    def forward(ctx, h, weight, bias, gamma, beta, layer, graph, scales):
        bn = layer.batchnorm_h
        F, N, S = layer.in_dim, layer.out_dim, len(scales)
        dev = h.device
        x = _rows(h)
        w = weight if weight.is_contiguous() else weight.contiguous()
        plan = _SmallTrainPlan(graph, F, N, S, dev)
        out = torch.empty(plan.V, N, dtype=torch.float32, device=dev)
        saved = plan.new_saved()
        a = plan.args(graph, x, w, bias, bn, scales, layer.residual, saved)
        a.out, a.ld_out = _lib.dev_ptr(out, torch.float32, "out"), out.stride(0)
        _lib.check(_lib.lib().pna_simple_train_fwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_simple_train_fwd_f32")
        ctx.plan, ctx.graph, ctx.layer, ctx.scales, ctx.state = plan, graph, layer, scales, saved
        ctx.save_for_backward(x, w, bias, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, go):
        x, w, bias, gamma, beta = ctx.saved_tensors
        plan, layer = ctx.plan, ctx.layer
        F, N, S = plan.F, plan.N, plan.S
        dev = x.device
        go = _rows(go)
        g_h = torch.empty(plan.V, F, dtype=torch.float32, device=dev)
        g_w = torch.empty(N, S * 4 * F, dtype=torch.float32, device=dev)
        g_vec = torch.empty(3, N, dtype=torch.float32, device=dev)          # grad_b | grad_gamma | grad_beta
        a = plan.args(ctx.graph, x, w, bias, layer.batchnorm_h, ctx.scales, layer.residual, ctx.state)
        a.momentum = -1.0
        a.grad_out, a.ld_go = _lib.dev_ptr(go, torch.float32, "grad_out"), go.stride(0)
        a.col_t, a.rank_t = _lib.dev_ptr(plan.col_t, torch.int32, "col_t"), _lib.dev_ptr(plan.rank_t, torch.int32, "rank_t")
        a.items_t, a.n_items_t = _lib.dev_ptr(plan.items_t, torch.int32, "items_t"), plan.items_t.shape[0]
        a.grad_h, a.grad_w = _lib.dev_ptr(g_h, torch.float32, "grad_h"), _lib.dev_ptr(g_w, torch.float32, "grad_w")
        a.grad_b = _lib.dev_ptr(g_vec[0], torch.float32, "grad_b")
        a.grad_gamma, a.grad_beta = _lib.dev_ptr(g_vec[1], torch.float32, "grad_gamma"), _lib.dev_ptr(g_vec[2], torch.float32, "grad_beta")
        _lib.check(_lib.lib().pna_simple_train_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_simple_train_bwd_f32")
        need = ctx.needs_input_grad
        return (g_h if need[0] else None, g_w if need[1] else None, g_vec[0] if bias is not None and need[2] else None,
                g_vec[1] if gamma is not None and need[3] else None, g_vec[2] if beta is not None and need[4] else None, None, None, None)


def simple_layer_small_train(layer, graph, h, scales):
    """residual + relu(bn(posttrans(aggregate))) of a training PNASimpleLayer through SimpleLayerSmallTrainFn; num_batches_tracked advances
    like the module's own forward."""
    bn = layer.batchnorm_h
    lin = layer.posttrans.fully_connected[0].linear
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return SimpleLayerSmallTrainFn.apply(h, lin.weight, lin.bias, bn.weight, bn.bias, layer, graph, tuple(scales))


class _TowerTrainPlan(_GraphScratchPlan):
    """What one call of the three tower training Functions needs besides the layer's tensors: the transposed graph's arrays and the
    call's workspace.  Nothing here depends on weight values.  edge_dim > 0: the plan of a layer with edge features
    (pna_tower_edge_train_*_f32) -- its larger workspace, the int32 edge ids and the transposed edges' CSR positions (both kept on the
    graph), x_edge in the saved state.  aggr: the plan of pna_tower_aggr_train_*_f32 -- the layer's aggregator codes in its order (A of
    them: a, the posttrans weight's gradient and the workspace are sized by A; None = mean max min std, A = 4); its backward is the
    per-edge one, so it holds pos_t also without edge features, and the saved state ends with row_mean (V, T Fi)."""

    def __init__(self, graph, T, Fi, Fo, S, divide_input, dev, edge_dim=0, aggr=None, pyg=False):
        V, E = graph.num_nodes, int(graph.csr.col.numel())
        self.pyg = bool(pyg)                                      # the plan of pna_pyg_conv_train_*_f32: its workspace, `packed` last in the saved state
        self.V, self.E, self.T, self.Fi, self.Fo, self.S, self.div, self.dev = V, E, T, Fi, Fo, S, bool(divide_input), dev
        self.edge_dim = int(edge_dim)
        self.aggr = None if aggr is None else tuple(int(c) for c in aggr)
        self.A = 4 if aggr is None else len(self.aggr)
        self.col_t, self.rank_t, self.items_t = _transposed_whole_rows(graph)
        if self.edge_dim:
            self.eid = graph.edge_ids32()
        if self.pyg:
            nbytes = _lib.lib().pna_pyg_conv_train_workspace_bytes(V, E, T, Fi, Fo, S, int(self.div), self.edge_dim, self.A,
                                                                   (ctypes.c_int32 * self.A)(*self.aggr))
        elif self.aggr is not None:
            nbytes = _lib.lib().pna_tower_aggr_train_workspace_bytes(V, E, T, Fi, Fo, S, int(self.div), self.edge_dim, self.A,
                                                                     (ctypes.c_int32 * self.A)(*self.aggr))
        elif self.edge_dim:
            nbytes = _lib.lib().pna_tower_edge_train_workspace_bytes(V, E, T, Fi, Fo, S, int(self.div), self.edge_dim)
        else:
            nbytes = _lib.lib().pna_tower_train_workspace_bytes(V, E, T, Fi, Fo, S, int(self.div))
        if self.edge_dim or self.aggr is not None:                # the per-edge backward
            gT = graph._pna_amd_transposed
            self.pos_t = getattr(gT, "_pna_amd_pos_t", None)      # position of every transposed edge in the forward CSR
            if self.pos_t is None:
                self.pos_t = gT._pna_amd_pos_t = gT.csr.eid.to(torch.int32).contiguous()
        if nbytes < 0:
            raise RuntimeError("TowerLayerSmallTrainFn: shape outside pna_tower_train_*_f32 (the layer checks it before taking this path)")
        self.take_workspace(graph, nbytes)

    def new_saved(self):
        """The state one forward leaves for its backward -- x_cat (V, 2 T Fi) | a (V, T A Fi) | z (V, C) | p (V, C) | save_mean,
        save_invstd [C] [| x_edge (E, T Fi)] [| row_mean (V, T Fi)] in one buffer, argmax | argmin (V, T Fi) in another.  Per CALL, not
        per plan: two layers of one shape on one graph are both alive until their backwards."""
        V, TFi, C = self.V, self.T * self.Fi, self.T * self.Fo
        fbuf = torch.empty(self._float_end() + (V * TFi if self.aggr is not None else 0) + (self.packed_floats() if self.pyg else 0),
                           dtype=torch.float32, device=self.dev)
        ibuf = torch.empty(2, V, TFi, dtype=torch.int32, device=self.dev)
        return fbuf, ibuf

    def views(self, saved):
        """(x_cat, a, z, p, stats (2, C), argmax, argmin) of a saved state."""
        fbuf, ibuf = saved
        V, TFi, C = self.V, self.T * self.Fi, self.T * self.Fo
        cuts = [V * 2 * TFi, V * self.A * TFi, V * C, V * C, 2 * C]
        parts, o = [], 0
        for n in cuts:
            parts.append(fbuf[o:o + n])
            o += n
        return (parts[0].view(V, 2 * TFi), parts[1].view(V, self.A * TFi), parts[2].view(V, C), parts[3].view(V, C), parts[4].view(2, C), ibuf[0], ibuf[1])

    def x_edge(self, saved):
        """The (E, T Fi) x_edge of an edge plan's saved state (behind the pieces views() returns)."""
        V, TFi, C = self.V, self.T * self.Fi, self.T * self.Fo
        o = V * (2 + self.A) * TFi + 2 * V * C + 2 * C
        return saved[0][o:o + self.E * TFi].view(self.E, TFi)

    def _float_end(self):
        """Where the pieces views() and x_edge() return end in the float buffer of a saved state."""
        V, TFi, C = self.V, self.T * self.Fi, self.T * self.Fo
        return V * (2 + self.A) * TFi + 2 * V * C + 2 * C + (self.E * TFi if self.edge_dim else 0)

    def row_mean(self, saved):
        """The (V, T Fi) row_mean of an aggregator-list plan's saved state (the last piece)."""
        o, n = self._float_end(), self.V * self.T * self.Fi
        return saved[0][o:o + n].view(self.V, self.T * self.Fi)

    def packed_floats(self):
        """The floats of a PyG plan's packed pretrans image: per tower (Fi, 2 Fi + edge_dim) and a bias."""
        return self.T * self.Fi * (2 * self.Fi + self.edge_dim + 1)

    def packed(self, saved):
        """The packed image of a PyG plan's saved state (the last piece, behind row_mean)."""
        o = self._float_end() + self.V * self.T * self.Fi
        return saved[0][o:o + self.packed_floats()]

    def aggr_args(self, base, edge, key, saved, backward=False):
        """The pna_tower_aggr_train_args around `base`, `edge` (or None) and the mask key (p, seed, offset) (or None)."""
        r = _lib.PnaTowerAggrTrainArgs()
        r.base = ctypes.cast(ctypes.pointer(base), ctypes.c_void_p)
        drop = None
        if edge is not None:
            r.edge = ctypes.cast(ctypes.pointer(edge), ctypes.c_void_p)
        if key is not None:
            drop = _tower_drop_args(base, edge, key)
            r.drop = ctypes.cast(ctypes.pointer(drop), ctypes.c_void_p)
        r.n_aggr = self.A
        for i, c in enumerate(self.aggr):
            r.aggr[i] = c
        r.row_mean = self.row_mean(saved).data_ptr()
        if backward and edge is None and self.E:
            r.pos_t = _lib.dev_ptr(self.pos_t, torch.int32, "pos_t")
        r._keep = (base, edge, drop)
        return r

    def edge_args(self, base, e, saved, grad_e=None, backward=False):
        """The pna_tower_edge_train_args around `base` (args() of this plan, set_backward() applied for a backward)."""
        q = _lib.PnaTowerEdgeTrainArgs()
        q.base = ctypes.cast(ctypes.pointer(base), ctypes.c_void_p)
        q.edge_dim = self.edge_dim
        if self.E:
            q.e, q.ld_e = _lib.dev_ptr(e, torch.float32, "e"), e.stride(0)
            q.eid = _lib.dev_ptr(self.eid, torch.int32, "eid")
            q.x_edge = self.x_edge(saved).data_ptr()
            if backward:
                q.pos_t = _lib.dev_ptr(self.pos_t, torch.int32, "pos_t")
        if grad_e is not None:
            q.grad_e, q.ld_ge = _lib.dev_ptr(grad_e, torch.float32, "grad_e"), max(grad_e.stride(0), self.edge_dim)
        return q

    def args(self, graph, h, snorm, scales, towers, mix_w, mix_b, slope, residual, saved):
        """towers: per tower (w_pre, b_pre, w_post, b_post, gamma, beta, running_mean, running_var, eps, momentum)."""
        csr = graph.csr
        a = _lib.PnaTowerTrainArgs()
        a.rowptr = _lib.dev_ptr(csr.rowptr, torch.int32, "rowptr")
        a.col = _lib.dev_ptr(csr.col, torch.int32, "col") if self.E else None
        a.V, a.E, a.n_tower, a.Fi, a.Fo, a.n_scaler = self.V, self.E, self.T, self.Fi, self.Fo, self.S
        a.divide_input, a.residual = int(self.div), int(residual)
        a.h, a.ldh = _lib.dev_ptr(h, torch.float32, "h"), h.stride(0)
        if snorm is not None:
            a.snorm_n = _lib.dev_ptr(snorm, torch.float32, "snorm_n")
        for s, rs in enumerate(scales):
            if rs is not None:
                a.row_scale[s] = _lib.dev_ptr(rs, torch.float32, "row_scale").value
        for t, (w_pre, b_pre, w_post, b_post, gamma, beta, rm, rv, eps, mom) in enumerate(towers):
            a.w_pre[t], a.b_pre[t] = w_pre.data_ptr(), b_pre.data_ptr()
            a.w_post[t], a.b_post[t] = w_post.data_ptr(), b_post.data_ptr()
            if gamma is not None:
                a.gamma[t], a.beta[t] = gamma.data_ptr(), beta.data_ptr()
            if rm is not None:
                a.running_mean[t], a.running_var[t] = rm.data_ptr(), rv.data_ptr()
            a.eps, a.momentum = float(eps), float(mom)
        a.w_mix = _lib.dev_ptr(mix_w, torch.float32, "w_mix")
        a.b_mix = _lib.dev_ptr(mix_b, torch.float32, "b_mix")
        a.slope = float(slope)
        x_cat, agg, z, p, stats, amx, amn = self.views(saved)
        a.x_cat, a.a, a.z, a.p = x_cat.data_ptr(), agg.data_ptr(), z.data_ptr(), p.data_ptr()
        a.save_mean, a.save_invstd = stats[0].data_ptr(), stats[1].data_ptr()
        a.argmax, a.argmin = amx.data_ptr(), amn.data_ptr()
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.nbytes
        return a

    def set_backward(self, a, go, g_h, grads, g_mix_w, g_mix_b):
        """grads: per tower (grad_w_pre, grad_b_pre, grad_w_post, grad_b_post, grad_gamma, grad_beta)."""
        a.momentum = -1.0
        a.grad_out, a.ld_go = _lib.dev_ptr(go, torch.float32, "grad_out"), go.stride(0)
        a.col_t, a.rank_t = _lib.dev_ptr(self.col_t, torch.int32, "col_t"), _lib.dev_ptr(self.rank_t, torch.int32, "rank_t")
        a.items_t, a.n_items_t = _lib.dev_ptr(self.items_t, torch.int32, "items_t"), self.items_t.shape[0]
        a.grad_h = _lib.dev_ptr(g_h, torch.float32, "grad_h")
        for t, (gwp, gbp, gwo, gbo, gg, gb) in enumerate(grads):
            a.grad_w_pre[t], a.grad_b_pre[t], a.grad_w_post[t], a.grad_b_post[t] = gwp.data_ptr(), gbp.data_ptr(), gwo.data_ptr(), gbo.data_ptr()
            if gg is not None:
                a.grad_gamma[t], a.grad_beta[t] = gg.data_ptr(), gb.data_ptr()
        a.grad_w_mix, a.grad_b_mix = _lib.dev_ptr(g_mix_w, torch.float32, "grad_w_mix"), _lib.dev_ptr(g_mix_b, torch.float32, "grad_b_mix")
        return a


def _tower_train_tensors(layer, params):
    """Per tower (w_pre, b_pre, w_post, b_post, gamma, beta, running_mean, running_var, eps, momentum) for _TowerTrainPlan.args: the six
    tensors out of `params` (the modules' own in a forward, the saved ones in a backward), the rest from the layer's modules."""
    out = []
    for t, tower in enumerate(layer.towers):
        bn = tower.batchnorm_h
        out.append((*params[6 * t:6 * t + 6], bn.running_mean, bn.running_var, bn.eps, bn.momentum))
    return out


def _tower_drop_args(base, edge, key):
    """The pna_tower_drop_args around `base` (and `edge`, or None) under the mask key (p, seed, offset)."""
    d = _lib.PnaTowerDropArgs()
    d.base = ctypes.cast(ctypes.pointer(base), ctypes.c_void_p)
    if edge is not None:
        d.edge = ctypes.cast(ctypes.pointer(edge), ctypes.c_void_p)
    d.p, d.seed, d.offset = key
    d._keep = (base, edge)
    return d


def _tower_train_call(which, base, edge, key, dev, aggr=None):
    """One of the four C entry pairs, `which` = "fwd" or "bwd": with an aggregator-list block (_TowerTrainPlan.aggr_args, which holds the
    edge block and the mask key) pna_tower_aggr_train_*_f32, else with a mask key pna_tower_drop_train_*_f32, else with an edge block
    pna_tower_edge_train_*_f32, else pna_tower_train_*_f32."""
    if aggr is not None:
        name, block = f"pna_tower_aggr_train_{which}_f32", aggr
    elif key is not None:
        name, block = f"pna_tower_drop_train_{which}_f32", _tower_drop_args(base, edge, key)
    elif edge is not None:
        name, block = f"pna_tower_edge_train_{which}_f32", edge
    else:
        name, block = f"pna_tower_train_{which}_f32", base
    _lib.check(getattr(_lib.lib(), name)(ctypes.byref(block), _lib.stream_ptr(dev)), name)


def _row_major(params):
    """The tower calls take every parameter as a bare pointer to row-major storage, without a pitch: one that is stored otherwise (a weight
    re-stored as p.data.t().contiguous().t()) goes in as a contiguous copy, and autograd hands the copy's gradient to the parameter; a
    row-major one is passed as it is."""
    return tuple(None if p is None else p.contiguous() for p in params)


def _tower_train_forward(ctx, h, e, layer, graph, scales, snorm, key, params, aggr=None):
    """The forward of the four tower training Functions.  e None or a layer without edge features: no edge block; key None: no dropout;
    aggr None: mean max min std through the three older entry pairs, else the layer's aggregator codes."""
    T, Fi, Fo, S = len(layer.towers), layer.input_tower, layer.output_tower, len(scales)
    dev = h.device
    x = _rows(h)
    ed = layer.towers[0].edge_dim if e is not None else 0
    ef = None if not ed else _rows(e)
    params = _row_major(params)
    plan = _TowerTrainPlan(graph, T, Fi, Fo, S, layer.divide_input, dev, edge_dim=ed, aggr=aggr)
    out = torch.empty(plan.V, T * Fo, dtype=torch.float32, device=dev)
    saved = plan.new_saved()
    slope = layer.mixing_network.activation.negative_slope
    a = plan.args(graph, x, snorm, scales, _tower_train_tensors(layer, params), params[6 * T], params[6 * T + 1], slope, layer.residual, saved)
    a.out, a.ld_out = _lib.dev_ptr(out, torch.float32, "out"), out.stride(0)
    q = plan.edge_args(a, ef, saved) if ed else None
    _tower_train_call("fwd", a, q, key, dev, plan.aggr_args(a, q, key, saved) if aggr is not None else None)
    ctx.plan, ctx.graph, ctx.layer, ctx.scales, ctx.snorm, ctx.state, ctx.slope, ctx.key = plan, graph, layer, scales, snorm, saved, slope, key
    ctx.save_for_backward(x, *([ef] if ed else []), *params)
    return out


def _tower_train_backward(ctx, go, lead):
    """The backward of the three tower training Functions; `lead`: how many inputs the Function has in front of `params` (h first, e
    second where there is one).  The C call reads the SAVED tensors (autograd's version check covers them), the running statistics, eps
    and momentum come from the modules."""
    x, *params = ctx.saved_tensors
    plan, layer = ctx.plan, ctx.layer
    T, Fi, Fo, S, ed = plan.T, plan.Fi, plan.Fo, plan.S, plan.edge_dim
    ef = params.pop(0) if ed else None
    C = T * Fo
    dev = x.device
    go = _rows(go)
    need = ctx.needs_input_grad
    g_h = torch.empty(plan.V, x.shape[1], dtype=torch.float32, device=dev)
    g_e = torch.empty(plan.E, ed, dtype=torch.float32, device=dev) if (ed and need[1]) else None
    # one buffer per kind of parameter: (T, ...) blocks the towers' gradients are views of
    g_wpre = torch.empty(T, Fi, 2 * Fi + ed, dtype=torch.float32, device=dev)
    g_wpost = torch.empty(T, Fo, (1 + plan.A * S) * Fi, dtype=torch.float32, device=dev)
    g_bpre = torch.empty(T, Fi, dtype=torch.float32, device=dev)
    g_vec = torch.empty(3, T, Fo, dtype=torch.float32, device=dev)       # grad_b_post | grad_gamma | grad_beta
    g_mix = torch.empty(C + 1, C, dtype=torch.float32, device=dev)       # grad_w_mix | grad_b_mix
    mix_w, mix_b = params[6 * T], params[6 * T + 1]
    a = plan.args(ctx.graph, x, ctx.snorm, ctx.scales, _tower_train_tensors(layer, params), mix_w, mix_b, ctx.slope, layer.residual, ctx.state)
    has_affine = params[4] is not None
    grads = [(g_wpre[t], g_bpre[t], g_wpost[t], g_vec[0, t], g_vec[1, t] if has_affine else None, g_vec[2, t] if has_affine else None)
             for t in range(T)]
    plan.set_backward(a, go, g_h, grads, g_mix[:C], g_mix[C])
    q = plan.edge_args(a, ef, ctx.state, grad_e=g_e, backward=True) if ed else None
    _tower_train_call("bwd", a, q, ctx.key, dev, plan.aggr_args(a, q, ctx.key, ctx.state, backward=True) if plan.aggr is not None else None)
    res = [g_h if need[0] else None, g_e] + [None] * (lead - 2)
    for t in range(T):
        res += grads[t]
    res += [g_mix[:C], g_mix[C] if mix_b is not None else None]
    return tuple(r if (r is None or need[i]) else None for i, r in enumerate(res))


class TowerLayerSmallTrainFn(torch.autograd.Function):
    """PNALayer's training forward (per tower: pretrans, gather, scalers, posttrans, graph norm, batch-statistics BatchNorm; the mixing
    Linear + LeakyReLU, the residual: models/dgl/pna_layer.py:55-76, 130-145) on a molecule-sized batch as ONE C call
    (pna_tower_train_fwd_f32) and its backward as one (pna_tower_train_bwd_f32).  The weights are the modules' own tensors (no stack, no
    packed image); the output, the gradients and the state a forward saves for its backward are fresh tensors per call.  `params`: per
    tower w_pre, b_pre, w_post, b_post, gamma, beta; then the mixing weight and bias.  This and the two Functions below are one forward
    and one backward (_tower_train_forward, _tower_train_backward) behind three signatures."""

    @staticmethod
    def forward(ctx, h, layer, graph, scales, snorm, *params):
        return _tower_train_forward(ctx, h, None, layer, graph, scales, snorm, None, params)

    @staticmethod
    def backward(ctx, go):
        return _tower_train_backward(ctx, go, 5)


class TowerLayerEdgeSmallTrainFn(torch.autograd.Function):
    """TowerLayerSmallTrainFn for a PNALayer with edge features (models/dgl/pna_layer.py:35-40: the pretrans on [h_u | h_v | ef]), through
    pna_tower_edge_train_fwd_f32 / pna_tower_edge_train_bwd_f32.  `e` (E, edge_dim), in the graph's original edge order, is an input: its
    gradient comes back when it needs one.  A tower's pretrans weight is (Fi, 2 Fi + edge_dim)."""

    @staticmethod
    def forward(ctx, h, e, layer, graph, scales, snorm, *params):
        return _tower_train_forward(ctx, h, e, layer, graph, scales, snorm, None, params)

    @staticmethod
    def backward(ctx, go):
        return _tower_train_backward(ctx, go, 6)


class TowerLayerDropSmallTrainFn(torch.autograd.Function):
    """TowerLayerSmallTrainFn / TowerLayerEdgeSmallTrainFn for a PNALayer whose towers have dropout (models/dgl/pna_layer.py:75, in front
    of the mixing network of :134-141), through pna_tower_drop_train_fwd_f32 / pna_tower_drop_train_bwd_f32.  `e` is None for a layer
    without edge features.  `key` = (p, seed, offset), Python numbers: the backward regenerates the forward's mask from them, no mask is
    saved."""

    @staticmethod
    def forward(ctx, h, e, layer, graph, scales, snorm, key, *params):
        return _tower_train_forward(ctx, h, e, layer, graph, scales, snorm, key, params)

    @staticmethod
    def backward(ctx, go):
        return _tower_train_backward(ctx, go, 7)


class TowerLayerAggrSmallTrainFn(torch.autograd.Function):
    """The three Functions above for a PNALayer whose towers aggregate with any 1-4 distinct aggregators out of mean sum max min std var
    (models/dgl/aggregators.py:6-26, 50-51), through pna_tower_aggr_train_fwd_f32 / pna_tower_aggr_train_bwd_f32.  `e` is None for a layer
    without edge features, `key` = (p, seed, offset) or None for towers without dropout, `aggr` the tuple of aggregator codes in the
    layer's order.  A tower's posttrans weight is (Fo, (1 + len(aggr) n_scaler) Fi)."""

    @staticmethod
    def forward(ctx, h, e, layer, graph, scales, snorm, key, aggr, *params):
        return _tower_train_forward(ctx, h, e, layer, graph, scales, snorm, key, params, aggr=aggr)

    @staticmethod
    def backward(ctx, go):
        return _tower_train_backward(ctx, go, 8)


def _tower_train_inputs(layer, snorm_n):
    """(snorm, *params) as the three Functions take them -- the graph norm's factor flattened (None for a layer without graph norm), per
    tower w_pre, b_pre, w_post, b_post, gamma, beta, then the mixing weight and bias -- after advancing every tower's num_batches_tracked
    like the module's own forward."""
    params = []
    for t in layer.towers:
        pre, post, bn = t.pretrans.fully_connected[0].linear, t.posttrans.fully_connected[0].linear, t.batchnorm_h
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        params += [pre.weight, pre.bias, post.weight, post.bias, bn.weight, bn.bias]
    mix = layer.mixing_network.linear
    snorm = None
    if layer.towers[0].graph_norm:
        snorm = snorm_n.reshape(-1)
        snorm = snorm if snorm.is_contiguous() else snorm.contiguous()
    return (snorm, *params, mix.weight, mix.bias)


def tower_layer_small_train(layer, graph, h, snorm_n, scales):
    """[h +] leaky(mixing(cat_t bn_t(graph_norm(posttrans_t(...))))) of a training PNALayer through TowerLayerSmallTrainFn."""
    return TowerLayerSmallTrainFn.apply(h, layer, graph, tuple(scales), *_tower_train_inputs(layer, snorm_n))


def tower_layer_edge_small_train(layer, graph, h, e, snorm_n, scales):
    """tower_layer_small_train for a layer with edge features, through TowerLayerEdgeSmallTrainFn."""
    return TowerLayerEdgeSmallTrainFn.apply(h, e, layer, graph, tuple(scales), *_tower_train_inputs(layer, snorm_n))


def tower_layer_drop_small_train(layer, graph, h, e, snorm_n, scales):
    """tower_layer_small_train / tower_layer_edge_small_train for a layer whose towers have dropout, through TowerLayerDropSmallTrainFn;
    the mask's key comes from the device's default generator (functional.tower_dropout_key), one per call, drawn after the counters
    have advanced."""
    from . import functional as PF
    snorm, *params = _tower_train_inputs(layer, snorm_n)
    seed, offset = PF.tower_dropout_key(h.device, h.shape[0] * layer.out_dim)
    key = (float(layer.towers[0].dropout), seed, offset)
    return TowerLayerDropSmallTrainFn.apply(h, e if layer.edge_features else None, layer, graph, tuple(scales), snorm, key, *params)


# ---- the routes below have no graph at hand: their backwards' workspaces are cached per device ----------------------------------------
def _device_workspace(cache, dev, nbytes):
    """(buffer, pointer): `cache`'s fp32 buffer on `dev`, ONE per device and route, grown when a larger call arrives (molecule batches
    have another row count every step, so a buffer per size would never stop growing), and the address of `nbytes` bytes in it from a
    16-byte boundary on.  Every launch writes what it reads and nothing is carried in it between calls; one caller at a time per device
    and stream, like a graph's scratch."""
    n = (nbytes + 16 + 3) // 4
    buf = cache.get(dev)
    if buf is None or buf.numel() < n:
        buf = cache[dev] = torch.empty(n, dtype=torch.float32, device=dev)
    return buf, buf.data_ptr() + (-buf.data_ptr()) % 16


# ---- the two ends of the molecule nets: the sum of embedding tables and the per-graph readout (pna_net_ends.hip) -----------------
_embed_ws = {}      # device -> the embedding backward's reusable workspace (no graph is at hand where the encoder runs)


def _embed_args(idx, tables):
    a = _lib.PnaEmbedSumArgs()
    T, F = len(tables), tables[0].shape[1]
    a.V, a.n_table, a.F = idx.shape[0], T, F
    if idx.dtype != torch.int64 or not idx.is_cuda:
        raise TypeError("pna_amd: the embedding index must be an int64 tensor on the GPU")
    a.idx, a.ld_idx = ctypes.c_void_p(idx.data_ptr()), idx.stride(0)
    for j, w in enumerate(tables):
        a.table[j], a.rows[j], a.ld_table[j] = _lib.dev_ptr(w, torch.float32, "table").value, w.shape[0], w.stride(0)
    return a


class EmbedSumFn(torch.autograd.Function):
    """out[v] = sum_j table_j[idx[v, j]] (ogb's AtomEncoder; one table: nn.Embedding) as ONE C call (pna_embed_sum_fwd_f32) and the
    gradient of every table as one (pna_embed_sum_bwd_f32: no atomics, bitwise repeatable).  idx: int64 (V, n_table) with unit column
    stride, or 1-D of any stride for one table.  The backward's workspace is a cached buffer; nothing is carried in it."""

    @staticmethod
    def forward(ctx, idx, *tables):
        if idx.dim() == 2:
            idx = _rows(idx)
        tables = tuple(_rows(w) for w in tables)
        dev = tables[0].device
        out = torch.empty(idx.shape[0], tables[0].shape[1], dtype=torch.float32, device=dev)
        a = _embed_args(idx, tables)
        a.out, a.ld_out = _lib.dev_ptr(out, torch.float32, "out"), out.stride(0)
        _lib.check(_lib.lib().pna_embed_sum_fwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_embed_sum_fwd_f32")
        ctx.save_for_backward(idx, *tables)
        return out

    @staticmethod
    def backward(ctx, go):
        idx, *tables = ctx.saved_tensors
        dev = go.device
        go = _rows(go)
        a = _embed_args(idx, tables)
        F = tables[0].shape[1]
        rows = [w.shape[0] for w in tables]
        flat = torch.empty(sum(rows) * F, dtype=torch.float32, device=dev)     # every table's gradient, one allocation
        grads, at = [], 0
        for j, r in enumerate(rows):
            grads.append(flat[at:at + r * F].view(r, F))
            a.grad_table[j] = flat.data_ptr() + 4 * at
            at += r * F
        nbytes = _lib.lib().pna_embed_sum_workspace_bytes(a.V, a.n_table, a.rows, a.F)
        a.workspace, a.workspace_bytes = _device_workspace(_embed_ws, dev, nbytes)[1], nbytes
        a.grad_out, a.ld_go = _lib.dev_ptr(go, torch.float32, "grad_out"), go.stride(0)
        _lib.check(_lib.lib().pna_embed_sum_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_embed_sum_bwd_f32")
        return (None, *[g if ctx.needs_input_grad[1 + j] else None for j, g in enumerate(grads)])


def embed_sum(idx, tables):
    """sum_j tables[j][idx[:, j]] through EmbedSumFn."""
    return EmbedSumFn.apply(idx, *tables)


def _readout_args(offsets, G, V, F, op):
    a = _lib.PnaReadoutArgs()
    a.offsets = _lib.dev_ptr(offsets, torch.int32, "offsets")
    a.G, a.V, a.F, a.op = G, V, F, _lib.AGG_CODES[op]
    return a


class ReadoutFn(torch.autograd.Function):
    """(G, F) sum / mean / max of the node rows of every graph of a batch (dgl.sum_nodes / mean_nodes / max_nodes) as ONE C call
    (pna_readout_fwd_f32) and its backward as one (pna_readout_bwd_f32).  offsets: int32 [G + 1], the contiguous node range of every
    graph, none empty.  No workspace; max keeps its (G, F) arg rows for the backward."""

    @staticmethod
    def forward(ctx, h, offsets, op):
        h = _rows(h)
        V, F = h.shape
        G = offsets.numel() - 1
        dev = h.device
        out = torch.empty(G, F, dtype=torch.float32, device=dev)
        arg = torch.empty(G, F, dtype=torch.int32, device=dev) if op == "max" else None
        a = _readout_args(offsets, G, V, F, op)
        a.h, a.ldh = _lib.dev_ptr(h, torch.float32, "h"), h.stride(0)
        a.out, a.ld_out = _lib.dev_ptr(out, torch.float32, "out"), out.stride(0)
        a.argmax = _lib.dev_ptr(arg, torch.int32, "argmax")
        _lib.check(_lib.lib().pna_readout_fwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_readout_fwd_f32")
        ctx.offsets, ctx.op, ctx.shape, ctx.arg = offsets, op, (G, V, F), arg
        return out

    @staticmethod
    def backward(ctx, go):
        G, V, F = ctx.shape
        dev = go.device
        go = _rows(go)
        gh = torch.empty(V, F, dtype=torch.float32, device=dev)
        a = _readout_args(ctx.offsets, G, V, F, ctx.op)
        a.argmax = _lib.dev_ptr(ctx.arg, torch.int32, "argmax")
        a.grad_out, a.ld_go = _lib.dev_ptr(go, torch.float32, "grad_out"), go.stride(0)
        a.grad_h, a.ld_gh = _lib.dev_ptr(gh, torch.float32, "grad_h"), gh.stride(0)
        _lib.check(_lib.lib().pna_readout_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_readout_bwd_f32")
        return gh, None, None


def readout(h, offsets, op):
    """Per-graph sum / mean / max of h's rows through ReadoutFn."""
    return ReadoutFn.apply(h, offsets, op)


# ---- the GRU update between two message-passing steps: nn.GRU over a length-1 sequence as a cell over rows (pna_gru.hip) -------------
_gru_ws = {}        # device -> the backward's reusable workspace; nothing is keyed per module: a shared GRU has several calls alive


def _gru_saved(V, H, dev):
    """The saved state of ONE call, (4, V, H): r | z | n | gh_n.  Allocated per call -- a shared GRU keeps one per application alive."""
    return torch.empty(4, V, H, dtype=torch.float32, device=dev)


def _gru_args(x, h, w_ih, w_hh):
    a = _lib.PnaGruCellArgs()
    a.V, a.I, a.Hc, a.input_size, a.hidden_size, a.dtype = x.shape[0], x.shape[1], h.shape[1], w_ih.shape[1], w_hh.shape[1], _lib.PNA_GRU_F32
    a.x, a.ldx = _lib.dev_ptr(x, torch.float32, "x"), x.stride(0)
    a.h, a.ldh = _lib.dev_ptr(h, torch.float32, "h"), h.stride(0)
    a.w_ih, a.ld_wih = _lib.dev_ptr(w_ih, torch.float32, "weight_ih"), w_ih.stride(0)
    a.w_hh, a.ld_whh = _lib.dev_ptr(w_hh, torch.float32, "weight_hh"), w_hh.stride(0)
    return a


class GruCellFn(torch.autograd.Function):
    """torch.nn.GRU (one layer, one direction, bias) over a length-1 sequence as ONE C call (pna_gru_cell_fwd_f32) and its backward as
    one (pna_gru_cell_bwd_f32: at most three launches, no atomics, bitwise repeatable).  x: (V, I <= input_size), h: (V, Hc <=
    hidden_size), fp32 with unit column stride and any row pitch; missing columns are zero padding, never materialised.  Once
    differentiable.  The saved state is allocated per call (`keep`; not at all under no_grad or when nothing requires a gradient); the
    workspace is one cached buffer per device, grown on demand."""

    @staticmethod
    def forward(ctx, x, h, w_ih, w_hh, b_ih, b_hh, keep):
        x, h, w_ih, w_hh = _rows(x), _rows(h), _rows(w_ih), _rows(w_hh)
        b_ih, b_hh = b_ih.contiguous(), b_hh.contiguous()
        dev, V, H = x.device, x.shape[0], w_hh.shape[1]
        out = torch.empty(V, H, dtype=torch.float32, device=dev)
        saved = _gru_saved(V, H, dev) if keep else None
        a = _gru_args(x, h, w_ih, w_hh)
        a.b_ih, a.b_hh = _lib.dev_ptr(b_ih, torch.float32, "bias_ih"), _lib.dev_ptr(b_hh, torch.float32, "bias_hh")
        a.out, a.ld_out = _lib.dev_ptr(out, torch.float32, "out"), out.stride(0)
        a.saved = _lib.dev_ptr(saved, torch.float32, "saved")
        _lib.check(_lib.lib().pna_gru_cell_fwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_gru_cell_fwd_f32")
        if saved is not None:
            ctx.save_for_backward(x, h, w_ih, w_hh, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        x, h, w_ih, w_hh, saved = ctx.saved_tensors
        dev, V, H = go.device, x.shape[0], w_hh.shape[1]
        I, Hc, IN = x.shape[1], h.shape[1], w_ih.shape[1]
        go = _rows(go)                                     # (the cotangent of out.sum(0) is an expand: strides (0, 1))
        need = ctx.needs_input_grad
        a = _gru_args(x, h, w_ih, w_hh)
        a.saved = _lib.dev_ptr(saved, torch.float32, "saved")
        a.grad_out, a.ld_go = _lib.dev_ptr(go, torch.float32, "grad_out"), go.stride(0)
        gx = torch.empty(V, I, dtype=torch.float32, device=dev) if need[0] else None
        gh = torch.empty(V, Hc, dtype=torch.float32, device=dev) if need[1] else None
        gwi = torch.empty(3 * H, IN, dtype=torch.float32, device=dev) if need[2] else None
        gwh = torch.empty(3 * H, H, dtype=torch.float32, device=dev) if need[3] else None
        gbi = torch.empty(3 * H, dtype=torch.float32, device=dev) if need[4] else None
        gbh = torch.empty(3 * H, dtype=torch.float32, device=dev) if need[5] else None
        if gx is not None:
            a.grad_x, a.ld_gx = _lib.dev_ptr(gx, torch.float32, "grad_x"), gx.stride(0)
        if gh is not None:
            a.grad_h, a.ld_gh = _lib.dev_ptr(gh, torch.float32, "grad_h"), gh.stride(0)
        a.grad_w_ih, a.grad_w_hh = _lib.dev_ptr(gwi, torch.float32, "grad_w_ih"), _lib.dev_ptr(gwh, torch.float32, "grad_w_hh")
        a.grad_b_ih, a.grad_b_hh = _lib.dev_ptr(gbi, torch.float32, "grad_b_ih"), _lib.dev_ptr(gbh, torch.float32, "grad_b_hh")
        a.need_x, a.need_h, a.need_w_ih, a.need_w_hh, a.need_b_ih, a.need_b_hh = [int(bool(n)) for n in need[:6]]
        nbytes = _lib.lib().pna_gru_cell_workspace_bytes(V, I, Hc, H)
        a.workspace, a.workspace_bytes = _device_workspace(_gru_ws, dev, nbytes)[1], nbytes
        _lib.check(_lib.lib().pna_gru_cell_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_gru_cell_bwd_f32")
        return gx, gh, gwi, gwh, gbi, gbh, None


def gru_cell(x, h, gru):
    """One step of `gru` (an nn.GRU: one layer, one direction, bias) from hidden rows h on input rows x through GruCellFn.  The state the
    backward needs is kept only when one will come: grad mode on and an input or parameter that requires a gradient."""
    ts = (x, h, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)
    return GruCellFn.apply(*ts, torch.is_grad_enabled() and any(t.requires_grad for t in ts))


# ---- the dense heads: 1 to 4 Linear layers with none / ReLU / LeakyReLU over rows as one C call each way (pna_mlp_head.hip) --------------
_mlp_ws = {}        # device -> the backward's reusable workspace; nothing is keyed per module


def _mlp_head_args(x, acts, ws, bs):
    a = _lib.PnaMlpHeadArgs()
    a.V, a.n_layers = x.shape[0], len(ws)
    a.widths[0] = x.shape[1]
    a.x, a.ldx = _lib.dev_ptr(x, torch.float32, "x"), x.stride(0)
    for l, (w, b, (code, slope)) in enumerate(zip(ws, bs, acts)):
        a.widths[l + 1], a.act[l], a.slope[l] = w.shape[0], code, slope
        a.w[l], a.ldw[l] = _lib.dev_ptr(w, torch.float32, "weight"), w.stride(0)
        a.b[l] = _lib.dev_ptr(b, torch.float32, "bias")
    return a


class MlpHeadFn(torch.autograd.Function):
    """y = f_L(... f_1(x)), f_l(h) = act_l(h W_l^T + b_l), as ONE C call (pna_mlp_head_fwd_f32: one launch) and its backward as one
    (pna_mlp_head_bwd_f32: at most three launches, no atomics, bitwise repeatable).  x: (V, widths[0]) fp32 with unit column stride and
    any row pitch; acts: one (PNA_MLP_ACT_* code, slope) per layer; params: W_1, b_1, .., W_L, b_L as nn.Linear keeps them (a bias may be
    None).  Once differentiable.  Only the inputs are saved: the backward rebuilds the hidden rows.  The workspace is one cached buffer
    per device, grown on demand."""

    @staticmethod
    def forward(ctx, x, acts, *params):
        x = _rows(x)
        ws = [_rows(w) for w in params[0::2]]
        bs = [None if b is None else b.contiguous() for b in params[1::2]]
        dev, V = x.device, x.shape[0]
        y = torch.empty(V, ws[-1].shape[0], dtype=torch.float32, device=dev)
        a = _mlp_head_args(x, acts, ws, bs)
        a.y, a.ldy = _lib.dev_ptr(y, torch.float32, "y"), y.stride(0)
        _lib.check(_lib.lib().pna_mlp_head_fwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_mlp_head_fwd_f32")
        ctx.acts, ctx.has_bias = acts, [b is not None for b in bs]
        ctx.save_for_backward(x, *ws, *[b for b in bs if b is not None])
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        x, *rest = ctx.saved_tensors
        L = len(ctx.acts)
        ws, kept = rest[:L], list(rest[L:])
        bs = [kept.pop(0) if has else None for has in ctx.has_bias]
        dev, V = go.device, x.shape[0]
        go = _rows(go)                                     # (the cotangent of y.sum() is an expand: strides (0, 0))
        need = ctx.needs_input_grad
        a = _mlp_head_args(x, ctx.acts, ws, bs)
        a.grad_out, a.ld_go = _lib.dev_ptr(go, torch.float32, "grad_out"), go.stride(0)
        gx = torch.empty(V, x.shape[1], dtype=torch.float32, device=dev) if need[0] else None
        if gx is not None:
            a.grad_x, a.ld_gx, a.need_x = _lib.dev_ptr(gx, torch.float32, "grad_x"), gx.stride(0), 1
        grads = []
        for l in range(L):
            gw = torch.empty(ws[l].shape, dtype=torch.float32, device=dev) if need[2 + 2 * l] else None
            gb = torch.empty(ws[l].shape[0], dtype=torch.float32, device=dev) if bs[l] is not None and need[3 + 2 * l] else None
            a.grad_w[l], a.grad_b[l] = _lib.dev_ptr(gw, torch.float32, "grad_w"), _lib.dev_ptr(gb, torch.float32, "grad_b")
            a.need_w[l], a.need_b[l] = int(gw is not None), int(gb is not None)
            grads += [gw, gb]
        if any(g is not None for g in grads):
            nbytes = _lib.lib().pna_mlp_head_workspace_bytes(V, L, a.widths)
            a.workspace, a.workspace_bytes = _device_workspace(_mlp_ws, dev, nbytes)[1], nbytes
        _lib.check(_lib.lib().pna_mlp_head_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_mlp_head_bwd_f32")
        return (gx, None, *grads)


def mlp_head(x, linears, acts):
    """The head `linears` (nn.Linear modules, in order) with `acts` (one (PNA_MLP_ACT_* code, slope) per layer: functional.mlp_head_act)
    on the rows x (V, in_features) through MlpHeadFn."""
    params = []
    for lin in linears:
        params += [lin.weight, lin.bias]
    return MlpHeadFn.apply(x, tuple(acts), *params)


# ---- the dense-adjacency PNALayer (the multitask GNN's convolution) as one C call each way (pna_dense_layer.hip) -------------------------
_dense_ws = {}      # device -> the backward's reusable workspace (the slabs' gradient images)


def _dense_args(cfg, x, adj, avg_log, avg_lin, params):
    T, Fi, Fo, divide, self_loop, aggr, scalers, slope = cfg
    a = _lib.PnaDenseLayerArgs()
    a.B, a.N, a.in_dim, a.n_tower, a.Fi, a.Fo = x.shape[0], x.shape[1], x.shape[2], T, Fi, Fo
    a.divide_input, a.self_loop, a.slope = int(divide), int(self_loop), slope
    a.n_aggr, a.n_scaler = len(aggr), len(scalers)
    for k, name in enumerate(aggr):
        a.aggr[k] = _lib.AGG_CODES[name]
    for k, name in enumerate(scalers):
        a.scaler[k] = _lib.DENSE_SCALER_CODES[name]
    a.x, a.adj = _lib.dev_ptr(x, torch.float32, "input"), _lib.dev_ptr(adj, torch.float32, "adj")
    a.avg_log, a.avg_lin = _lib.dev_ptr(avg_log, torch.float32, "avg_d['log']"), _lib.dev_ptr(avg_lin, torch.float32, "avg_d['lin']")
    for t in range(T):
        for k, f in enumerate(("w_pre", "b_pre", "w_post", "b_post")):
            getattr(a, f)[t] = _lib.dev_ptr(params[4 * t + k], torch.float32, f).value
    a.w_mix, a.b_mix = _lib.dev_ptr(params[4 * T], torch.float32, "w_mix"), _lib.dev_ptr(params[4 * T + 1], torch.float32, "b_mix")
    return a


class DenseLayerFn(torch.autograd.Function):
    """pna_amd.pytorch.pna.layer.PNALayer (1-layer pretrans and posttrans, aggregators out of mean / max / min / std, Linear + LeakyReLU
    mixing) as ONE C call (pna_dense_layer_fwd_f32: one launch) and its backward as one (pna_dense_layer_bwd_f32: at most two launches, no
    atomics, bitwise repeatable).  Nothing is saved but the inputs: the backward rebuilds the forward in LDS.  `cfg` = (towers, Fi, Fo,
    divide_input, self_loop, aggregator names, scaler names, slope); `params` = per tower the pretrans weight and bias and the posttrans
    weight and bias, then the mixing weight and bias, contiguous fp32.  avg_log / avg_lin: one device float each, or None where no scaler
    reads it.  adj gets no gradient.  Once differentiable."""

    @staticmethod
    def forward(ctx, x, adj, avg_log, avg_lin, cfg, *params):
        T, Fo = cfg[0], cfg[2]
        dev, (B, N, _) = x.device, x.shape
        out = torch.empty(B, N, T * Fo, dtype=torch.float32, device=dev)
        a = _dense_args(cfg, x, adj, avg_log, avg_lin, params)
        a.out = _lib.dev_ptr(out, torch.float32, "out")
        _lib.check(_lib.lib().pna_dense_layer_fwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_dense_layer_fwd_f32")
        ctx.cfg, ctx.has_log, ctx.has_lin = cfg, avg_log is not None, avg_lin is not None
        ctx.save_for_backward(x, adj, *[t for t in (avg_log, avg_lin) if t is not None], *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        cfg = ctx.cfg
        T, Fi, Fo, aggr, scalers = cfg[0], cfg[1], cfg[2], cfg[5], cfg[6]
        saved = list(ctx.saved_tensors)
        x, adj = saved[:2]
        k = 2
        avg_log = avg_lin = None
        if ctx.has_log:
            avg_log, k = saved[k], k + 1
        if ctx.has_lin:
            avg_lin, k = saved[k], k + 1
        params = saved[k:]
        dev, (B, N, _) = x.device, x.shape
        go = go.contiguous()
        need = ctx.needs_input_grad
        a = _dense_args(cfg, x, adj, avg_log, avg_lin, params)
        a.grad_out = _lib.dev_ptr(go, torch.float32, "grad_out")
        gx = torch.empty_like(x) if need[0] else None
        a.grad_x = _lib.dev_ptr(gx, torch.float32, "grad_x")
        grads = [torch.empty_like(p) if need[5 + i] else None for i, p in enumerate(params)]
        for t in range(T):
            for j, f in enumerate(("grad_w_pre", "grad_b_pre", "grad_w_post", "grad_b_post")):
                gt = grads[4 * t + j]
                getattr(a, f)[t] = None if gt is None else gt.data_ptr()
        a.grad_w_mix, a.grad_b_mix = _lib.dev_ptr(grads[4 * T], torch.float32, "grad_w_mix"), _lib.dev_ptr(grads[4 * T + 1], torch.float32, "grad_b_mix")
        from .functional import dense_layer_workspace_bytes
        nbytes = dense_layer_workspace_bytes(B, N, T, Fi, Fo, len(aggr), len(scalers))
        a.workspace, a.workspace_bytes = _device_workspace(_dense_ws, dev, nbytes)[1], nbytes
        _lib.check(_lib.lib().pna_dense_layer_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_dense_layer_bwd_f32")
        return (gx, None, None, None, None, *grads)


def _dense_avg(v, dev):
    """avg_d[key] as one fp32 float on `dev`: a 0-dim or 1-element fp32 tensor already there is passed as it is; a Python number or a
    tensor on the host becomes a fresh device scalar per call -- one small fill launch, stream-ordered, nothing read from the device and
    nothing kept, so there is no cached operand to go stale (DESIGN.md 4.13's census has no row for this route)."""
    if torch.is_tensor(v):
        if v.device == dev and v.dtype == torch.float32 and v.numel() == 1:
            return v.detach()
        if v.is_cuda:
            return v.detach().to(device=dev, dtype=torch.float32).reshape(1)      # (device to device: stream-ordered)
    return torch.full((1,), float(v), dtype=torch.float32, device=dev)


def dense_layer(layer, x, adj):
    """`layer` (a pna_amd.pytorch.pna.layer.PNALayer inside the scope of its `_one_call_path`) on x (B, N, in) and adj (B, N, N) through
    DenseLayerFn.  Reads no float on the host and waits for nothing: capturable."""
    t0 = layer.towers[0]
    scalers = tuple(t0.scalers)
    avg_log = _dense_avg(t0.avg_d["log"], x.device) if ("amplification" in scalers or "attenuation" in scalers) else None
    avg_lin = _dense_avg(t0.avg_d["lin"], x.device) if ("linear" in scalers or "inverse_linear" in scalers) else None
    params = []
    for t in layer.towers:
        pre, post = t.pretrans.fully_connected[0].linear, t.posttrans.fully_connected[0].linear
        params += [pre.weight, pre.bias, post.weight, post.bias]
    mix = layer.mixing_network
    params += [mix.linear.weight, mix.linear.bias]
    cfg = (len(layer.towers), t0.in_features, t0.out_features, bool(layer.divide_input), bool(t0.self_loop), tuple(t0.aggregators), scalers,
           float(mix.activation.negative_slope))
    return DenseLayerFn.apply(x, adj, avg_log, avg_lin, cfg, *params)


# ---- the Set2Set graph readout (layers.Set2Set: the multitask GNN's graph head) as one C call each way (pna_set2set.hip) ----------------
_s2s_ws = {}        # device -> the backward's reusable workspace (the slabs' records and gradient images)


def _s2s_args(x, w_ih, w_hh, b_ih, b_hh, steps):
    a = _lib.PnaSet2setArgs()
    a.B, a.N, a.D, a.steps, a.dtype = x.shape[0], x.shape[1], x.shape[2], steps, _lib.PNA_S2S_F32
    a.x = _lib.dev_ptr(x, torch.float32, "x")
    a.w_ih, a.w_hh = _lib.dev_ptr(w_ih, torch.float32, "weight_ih"), _lib.dev_ptr(w_hh, torch.float32, "weight_hh")
    a.b_ih, a.b_hh = _lib.dev_ptr(b_ih, torch.float32, "bias_ih"), _lib.dev_ptr(b_hh, torch.float32, "bias_hh")
    return a


class Set2SetFn(torch.autograd.Function):
    """models/layers.py:81-98 (`steps` rounds of a one-step nn.LSTM(2D, D), the scores, a softmax over the nodes and the weighted sum) as
    ONE C call (pna_set2set_fwd_f32: one launch) and its backward as one (pna_set2set_bwd_f32: at most two launches, no atomics, bitwise
    repeatable).  x: (B, N, D) contiguous fp32; the four nn.LSTM parameters as they are.  Nothing is saved but the inputs: the backward
    rebuilds the forward.  The workspace is one cached buffer per device, grown on demand.  Once differentiable."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, steps):
        w_ih, w_hh, b_ih, b_hh = w_ih.contiguous(), w_hh.contiguous(), b_ih.contiguous(), b_hh.contiguous()
        dev, (B, _, D) = x.device, x.shape
        out = torch.empty(B, 2 * D, dtype=torch.float32, device=dev)
        a = _s2s_args(x, w_ih, w_hh, b_ih, b_hh, steps)
        a.out = _lib.dev_ptr(out, torch.float32, "out")
        _lib.check(_lib.lib().pna_set2set_fwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_set2set_fwd_f32")
        ctx.steps = steps
        ctx.save_for_backward(x, w_ih, w_hh, b_ih, b_hh)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        x, w_ih, w_hh, b_ih, b_hh = ctx.saved_tensors
        dev, (B, N, D) = x.device, x.shape
        go = go.contiguous()
        need = ctx.needs_input_grad
        a = _s2s_args(x, w_ih, w_hh, b_ih, b_hh, ctx.steps)
        a.grad_out = _lib.dev_ptr(go, torch.float32, "grad_out")
        grads = [torch.empty_like(t) if need[i] else None for i, t in enumerate((x, w_ih, w_hh, b_ih, b_hh))]
        for f, t in zip(("grad_x", "grad_w_ih", "grad_w_hh", "grad_b_ih", "grad_b_hh"), grads):
            setattr(a, f, _lib.dev_ptr(t, torch.float32, f))
        from .functional import set2set_workspace_bytes
        nbytes = set2set_workspace_bytes(B, N, D, ctx.steps)
        a.workspace, a.workspace_bytes = _device_workspace(_s2s_ws, dev, nbytes)[1], nbytes
        _lib.check(_lib.lib().pna_set2set_bwd_f32(ctypes.byref(a), _lib.stream_ptr(dev)), "pna_set2set_bwd_f32")
        return (*grads, None)


def set2set(x, lstm, steps):
    """`steps` rounds of Set2Set on x (B, N, D) with `lstm` (an nn.LSTM(2D, D): one layer, one direction, bias) through Set2SetFn.  Reads
    nothing on the host and waits for nothing: capturable."""
    return Set2SetFn.apply(x, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, int(steps))


def tower_layer_aggr_small_train(layer, graph, h, e, snorm_n, scales):
    """The three wrappers above for a layer with another list of aggregators, through TowerLayerAggrSmallTrainFn; with tower dropout the
    mask's key is drawn as tower_layer_drop_small_train draws it."""
    from . import functional as PF
    snorm, *params = _tower_train_inputs(layer, snorm_n)
    p, key = float(layer.towers[0].dropout), None
    if p > 0:
        seed, offset = PF.tower_dropout_key(h.device, h.shape[0] * layer.out_dim)
        key = (p, seed, offset)
    aggr = tuple(_lib.AGG_CODES[n] for n in layer.towers[0].aggregators)
    return TowerLayerAggrSmallTrainFn.apply(h, e if layer.edge_features else None, layer, graph, tuple(scales), snorm, key, aggr, *params)


def _pyg_conv_args(plan, r, pre, enc, saved, grads=None):
    """The pna_pyg_conv_train_args around the list block `r`: the layer's own pretrans tensors `pre` = [(w_pre, b_pre)] per tower and
    `enc` = (w_enc, b_enc) or None; grads = ([(grad_w_pre, grad_b_pre)], (grad_w_enc, grad_b_enc) or None) in a backward."""
    y = _lib.PnaPygConvTrainArgs()
    y.aggr = ctypes.cast(ctypes.pointer(r), ctypes.c_void_p)
    for t, (w, b) in enumerate(pre):
        y.w_pre[t], y.b_pre[t] = w.data_ptr(), b.data_ptr()
    if enc is not None:
        y.w_enc, y.b_enc = _lib.dev_ptr(enc[0], torch.float32, "w_enc"), _lib.dev_ptr(enc[1], torch.float32, "b_enc")
    y.packed = plan.packed(saved).data_ptr()
    if grads is not None:
        for t, (gw, gb) in enumerate(grads[0]):
            y.grad_w_pre[t], y.grad_b_pre[t] = gw.data_ptr(), gb.data_ptr()
        if grads[1] is not None:
            y.grad_w_enc, y.grad_b_enc = grads[1][0].data_ptr(), grads[1][1].data_ptr()
    y._keep = r
    return y


def _pyg_conv_call(which, y, dev):
    """pna_pyg_conv_train_fwd_f32 or pna_pyg_conv_train_bwd_f32 (`which` = "fwd" or "bwd") on the block `y`."""
    name = f"pna_pyg_conv_train_{which}_f32"
    _lib.check(getattr(_lib.lib(), name)(ctypes.byref(y), _lib.stream_ptr(dev)), name)


def _pyg_towers(params, T):
    """Per tower (w_pre, b_pre, w_post, b_post, no BatchNorm: gamma, beta, running_mean, running_var None, eps 0, momentum < 0) for
    _TowerTrainPlan.args out of PygConvFn's params."""
    return [(*params[4 * t:4 * t + 4], None, None, None, None, 0.0, -1.0) for t in range(T)]


class PygConvFn(torch.autograd.Function):
    """pytorch_geometric.PNAConv with pre_layers == post_layers == 1 (models/pytorch_geometric/pna.py:120-159) on a molecule-sized batch
    as ONE C call (pna_pyg_conv_train_fwd_f32) and its backward as one (pna_pyg_conv_train_bwd_f32): the kernels of the tower training
    routes without BatchNorm and with the PyG statistics, behind a pack launch that turns the layer's [W_i | W_j | W_e] and its edge
    encoder into the tower call's image.  `e` (E, edge_dim) in edge_index order, None for a layer without edge_dim;
    `aggr` the aggregator codes in the layer's order; `params`: per tower w_pre, b_pre, w_post, b_post, then lin's weight and bias, then
    with edge features the encoder's weight and bias.  A call under no_grad is the forward alone."""

    @staticmethod
    def forward(ctx, x, e, layer, graph, scales, aggr, *params):
        T, Fi, Fo, S = layer.towers, layer.F_in, layer.F_out, len(scales)
        dev = x.device
        x = _rows(x)
        ed = int(layer.edge_dim) if e is not None else 0
        ef = _rows(e) if ed else None
        params = _row_major(params)
        plan = _TowerTrainPlan(graph, T, Fi, Fo, S, layer.divide_input, dev, edge_dim=ed, aggr=aggr, pyg=True)
        out = torch.empty(plan.V, T * Fo, dtype=torch.float32, device=dev)
        saved = plan.new_saved()
        a = plan.args(graph, x, None, scales, _pyg_towers(params, T), params[4 * T], params[4 * T + 1], 1.0, False, saved)
        a.out, a.ld_out = _lib.dev_ptr(out, torch.float32, "out"), out.stride(0)
        q = plan.edge_args(a, ef, saved) if ed else None
        r = plan.aggr_args(a, q, None, saved)
        y = _pyg_conv_args(plan, r, [params[4 * t:4 * t + 2] for t in range(T)], params[4 * T + 2:4 * T + 4] if ed else None, saved)
        _pyg_conv_call("fwd", y, dev)
        ctx.plan, ctx.graph, ctx.scales, ctx.state = plan, graph, scales, saved
        ctx.save_for_backward(x, *([ef] if ed else []), *params)
        return out

    @staticmethod
    def backward(ctx, go):
        x, *params = ctx.saved_tensors
        plan = ctx.plan
        T, Fi, Fo, S, ed = plan.T, plan.Fi, plan.Fo, plan.S, plan.edge_dim
        ef = params.pop(0) if ed else None
        C = T * Fo
        dev = x.device
        go = _rows(go)
        need = ctx.needs_input_grad
        g_x = torch.empty(plan.V, x.shape[1], dtype=torch.float32, device=dev)
        g_e = torch.empty(plan.E, ed, dtype=torch.float32, device=dev) if (ed and need[1]) else None
        g_wpre = torch.empty(T, Fi, (3 if ed else 2) * Fi, dtype=torch.float32, device=dev)
        g_wpost = torch.empty(T, Fo, (1 + plan.A * S) * Fi, dtype=torch.float32, device=dev)
        g_bpre = torch.empty(T, Fi, dtype=torch.float32, device=dev)
        g_bpost = torch.empty(T, Fo, dtype=torch.float32, device=dev)
        g_mix = torch.empty(C + 1, C, dtype=torch.float32, device=dev)       # grad of lin's weight | bias
        g_enc = torch.empty(Fi, ed + 1, dtype=torch.float32, device=dev).view(-1) if ed else None
        enc_grads = (g_enc[:Fi * ed].view(Fi, ed), g_enc[Fi * ed:]) if ed else None
        mix_w, mix_b = params[4 * T], params[4 * T + 1]
        a = plan.args(ctx.graph, x, None, ctx.scales, _pyg_towers(params, T), mix_w, mix_b, 1.0, False, ctx.state)
        plan.set_backward(a, go, g_x, [(g_wpre[t], g_bpre[t], g_wpost[t], g_bpost[t], None, None) for t in range(T)], g_mix[:C], g_mix[C])
        q = plan.edge_args(a, ef, ctx.state, grad_e=g_e, backward=True) if ed else None
        r = plan.aggr_args(a, q, None, ctx.state, backward=True)
        y = _pyg_conv_args(plan, r, [params[4 * t:4 * t + 2] for t in range(T)], params[4 * T + 2:4 * T + 4] if ed else None, ctx.state,
                           grads=([(g_wpre[t], g_bpre[t]) for t in range(T)], enc_grads))
        _pyg_conv_call("bwd", y, dev)
        res = [g_x, g_e, None, None, None, None]
        for t in range(T):
            res += [g_wpre[t], g_bpre[t], g_wpost[t], g_bpost[t]]
        res += [g_mix[:C], g_mix[C]]
        if ed:
            res += list(enc_grads)
        return tuple(r_ if (r_ is None or need[i]) else None for i, r_ in enumerate(res))


def pyg_conv_one_call(layer, graph, x, edge_attr, scales):
    """lin(cat_t post_nn_t([x_t | scalers(aggregators(pre_nn_t([x_i | x_j | enc(e)])))])) of a PNAConv through PygConvFn."""
    params = []
    for pre, post in zip(layer.pre_nns, layer.post_nns):
        params += [pre[0].weight, pre[0].bias, post[0].weight, post[0].bias]
    params += [layer.lin.weight, layer.lin.bias]
    if layer.edge_dim is not None:
        params += [layer.edge_encoder.weight, layer.edge_encoder.bias]
    aggr = tuple(_lib.AGG_CODES[n] for n in layer.aggregator_names)
    return PygConvFn.apply(x, edge_attr if layer.edge_dim is not None else None, layer, graph, tuple(scales), aggr, *params)
