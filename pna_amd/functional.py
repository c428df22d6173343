"""Graph-level functional API used by the layers: `aggregate` (gather + segment-reduce kernel) and
`posttrans` (MFMA contraction), both differentiable through custom autograd Functions.
"""
import ctypes
import os
from typing import NamedTuple, Optional

import torch

from . import _lib, degree_groups as DG, ops
from .shard import HaloGraph
from ._cache import DropsCachesOnConversion, drop_weight_caches, memo, tensor_key  # noqa: F401  (PF.drop_weight_caches, PF.DropsCachesOnConversion)


def _unit_stride(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError(f"pna_amd computes in fp32 like the reference; got {t.dtype}")
    if t.stride(-1) == 1 and not (t.dim() == 2 and t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        return t
    return t.contiguous()      # (also a broadcast row, strides (0, 1): the kernels take a row pitch of at least the width)


def aggregate(graph, x, F, aggregators, *, n_tower=1, dst_term=None, edge_term=None, row_scales=(None,),
              edge_resident=False, edge_weight=None, col_override=None, edge_type=None):
    """(V, n_tower * S * A * F) aggregate of the messages flowing into every node of `graph`.

    message(u->v) = x[u] (+ dst_term[v]) (+ edge_term[k]);  with edge_resident=True, x already holds
    one message per edge in CSR order.  Tower t reads columns [t*F, (t+1)*F).  Column layout of the
    result: tower-major, then scaler-major, then aggregator-major (the reference's cat order).
    edge_weight: fp32 [E] in CSR order (dense-variant adjacency weights).  col_override: int32 [E] row of
    `x` to gather for each CSR edge instead of the edge's source node (x then holds per-edge messages in
    some other edge order).  edge_type: int32 [E] in CSR order -- edge_term then has one row per edge TYPE (inference only).
    """
    x, dst_term, edge_term = _unit_stride(x), _unit_stride(dst_term), _unit_stride(edge_term)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, dst_term, edge_term)):
        graph.finish_exchange()
        from .autograd import AggregateFn
        return AggregateFn.apply(graph, x, dst_term, edge_term, F, tuple(aggregators), n_tower, tuple(row_scales),
                                 edge_resident, edge_weight, col_override)
    csr = graph.csr
    col = None if edge_resident else (csr.col if col_override is None else col_override)
    if getattr(graph, "_pending", None) is not None:
        # a sharded graph whose halo exchange is still in flight (HaloGraph.source_features(defer=True)): the rows that only
        # read local sources go first, on the hand-scheduled kernel (the only one that honours a partial work list)
        done = None
        if (col is csr.col and edge_term is None and edge_weight is None and tuple(aggregators) == ("mean", "max", "min", "std")
                and all(r is None for r in row_scales)):
            _, items_in, items_bd = graph.split_work_lists()
            A = len(aggregators)
            out = torch.empty(csr.rowptr.numel() - 1, n_tower * A * F, dtype=torch.float32, device=x.device)
            try:
                if items_in.shape[0]:
                    ops.segreduce(csr.rowptr, col, x, F, aggregators, row_scales, n_tower=n_tower, tower_stride_in=F,
                                  dst_term=dst_term, out=out, items=items_in, tune=dict(generic=2))
                graph.finish_exchange()
                if items_bd.shape[0]:
                    ops.segreduce(csr.rowptr, col, x, F, aggregators, row_scales, n_tower=n_tower, tower_stride_in=F,
                                  dst_term=dst_term, out=out, heavy=graph.heavy_schedule(), workspace=graph.workspace,
                                  items=items_bd, tune=dict(generic=2))
                done = out
            except RuntimeError as ex:                       # the call does not qualify for that kernel: one ordinary launch
                if "hand-scheduled kernel was required" not in str(ex):
                    raise
        graph.finish_exchange()
        if done is not None:
            return done
    return ops.segreduce(csr.rowptr, col, x, F, aggregators, row_scales,
                         n_tower=n_tower, tower_stride_in=F, dst_term=dst_term, edge_term=edge_term,
                         edge_weight=edge_weight, heavy=graph.heavy_schedule(), workspace=graph.workspace,
                         items=graph.work_items(), edge_type=edge_type)


def _bn_tensors(bn):
    """weight, bias, running mean and running variance of a BatchNorm1d, None where it has none -- through the module's own dictionaries
    (nn.Module.__getattr__ costs about 1 us per name, on every call of a 0.1 ms layer)."""
    p, b = bn._parameters, bn._buffers
    return [p["weight"], p["bias"], b["running_mean"], b["running_var"]]


def _first_linear(mlp):
    """mlp.fully_connected[0].linear through the modules' own dictionaries (nn.Module.__getattr__ and ModuleList indexing cost 4 us
    per chain, and the cache lookups walk up to 2 T chains on every call of a 0.1 ms layer)."""
    return mlp._modules["fully_connected"]._modules["0"]._modules["linear"]


def _tower_tensors(towers, pre=False, post=False, bn=False, mix=None):
    """The keyed tensor list of a builder over "every tower's first pretrans / posttrans Linear (weight, bias), BatchNorm tensors and
    the mixing Linear": the groups the builder READS, None where a module has no such tensor."""
    ts = []
    for t in towers:
        m = t._modules
        if pre:
            ts += _first_linear(m["pretrans"])._parameters.values()
        if post:
            ts += _first_linear(m["posttrans"])._parameters.values()
        if bn:
            ts += _bn_tensors(m["batchnorm_h"])
    if mix is not None:
        ts += mix._modules["linear"]._parameters.values()
    return ts


def _as_is(t):
    return t


def _fold(bn, tag, up):
    w, b, mean, var = ts = _bn_tensors(bn)

    def build():
        cs = (up(w) if w is not None else 1.0) * torch.rsqrt(up(var) + bn.eps)
        ct = (up(b) if b is not None else 0.0) - up(mean) * cs
        return cs.contiguous(), ct.contiguous()
    return memo(bn, tag, ts, bn.eps, build)


def _fold_batchnorm(bn):
    """Eval-mode BatchNorm1d as y = x * col_scale + col_shift; cached ON the module per state of its parameters and buffers so
    that an inference loop does not relaunch the five little fold kernels every forward."""
    return _fold(bn, "_pna_amd_fold", _as_is)                 # (in the module's own dtype)


def _fold_batchnorm_f32(bn):
    """_fold_batchnorm of a bf16 BatchNorm1d, folded in fp32 from the bf16 parameters and running statistics (the bf16 epilogue
    of pna_posttrans_bf16 takes fp32 column constants): the same body over the tensors' .float(), under a tag of its own."""
    return _fold(bn, "_pna_amd_fold_f32", torch.Tensor.float)


def posttrans(agg, K, weight, bias, row_scales, h_self=None, *, row_post=None, bn=None, relu=False, residual=None,
              out=None, degree_graph=None):
    """y = W [h_self | s_0*agg | s_1*agg | ...] + b with `weight` in the reference's nn.Linear layout
    (N, Kh + S*K) -- models/dgl/pna_layer.py:65-68 / :206 -- computed without materialising the
    scaled copies of `agg` (row_scales[s] is a per-row vector or None for the identity scaler).

    Optional fused tail (inference): row_post = snorm_n (V,1)/(V,), bn = an nn.BatchNorm1d in eval mode (folded
    to a per-column affine map), relu, residual -- applied in the reference's order
    (pna_layer.py:71-75 / :209-213)."""
    agg, h_self = _unit_stride(agg), _unit_stride(h_self)
    Kh = 0 if h_self is None else h_self.shape[1]
    if weight.shape[1] != Kh + len(row_scales) * K:
        raise ValueError(f"posttrans weight has {weight.shape[1]} input columns, expected {Kh + len(row_scales) * K}")
    if K < 4 or 0 < Kh < 4:
        # the MFMA kernel reads its operands in 16-byte pieces: widen tiny operands (multitask layers: 2 features
        # per tower) to 4 columns with zeros, and give the weight matching zero columns
        S, N = len(row_scales), weight.shape[0]
        Kp, Khp = max(K, 4), (max(Kh, 4) if Kh else 0)
        wb = [weight[:, :Kh]] + [weight[:, Kh + s * K:Kh + (s + 1) * K] for s in range(S)]
        wb = [torch.nn.functional.pad(w, (0, (Khp if i == 0 else Kp) - w.shape[1])) for i, w in enumerate(wb)]
        weight = torch.cat(wb if Kh else wb[1:], dim=1)
        agg = torch.nn.functional.pad(agg[:, :K], (0, Kp - K))
        if Kh:
            h_self = torch.nn.functional.pad(h_self, (0, Khp - Kh))
        K, Kh = Kp, Khp
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (agg, weight, bias, h_self)):
        from .autograd import PosttransFn
        if row_post is not None or bn is not None or relu or residual is not None:
            raise RuntimeError("the fused posttrans tail is inference-only")
        # degree_graph: the (unsharded) Graph whose degree scalers `row_scales` are -- lets the weight gradient walk the rows in the
        # graph's degree-plan order (autograd.PosttransFn.backward)
        return PosttransFn.apply(agg, K, weight, bias, tuple(row_scales), h_self, degree_graph)
    col_scale = col_shift = None
    if bn is not None:
        if bn.training:
            raise RuntimeError("only an eval-mode BatchNorm (running statistics) can be folded into the epilogue")
        col_scale, col_shift = _fold_batchnorm(bn)
    if row_post is not None:
        row_post = row_post.reshape(-1).contiguous()
    w = weight if weight.stride(-1) == 1 else weight.contiguous()
    return ops.posttrans(agg, K, w, row_scales, bias, h_self, out=out, row_post=row_post, col_scale=col_scale,
                         col_shift=col_shift, relu=relu, residual=_unit_stride(residual))


def _stack_cached(owner, tag, tensors):
    """torch.stack(tensors) cached on `owner` per state of every tensor: the per-tower biases and folded BatchNorm constants of a
    layer, which would otherwise cost a concatenation launch per forward."""
    return memo(owner, tag, tensors, None, lambda: torch.stack([t.detach() for t in tensors]).contiguous())


def posttrans_towers(agg, K, towers_lin, row_scales, hs, h_shared, out, row_post=None, bns=None, relu=False):
    """Inference-only: the first posttrans Linear of every tower (+ graph-norm / folded eval BatchNorm) in ONE call.
    towers_lin: the nn.Linear of each tower; hs: the (V, Kh) shared input or the (V, T*Kh) divided one; bns: per-tower
    BatchNorm1d modules (eval) or None."""
    weights = [lin.weight for lin in towers_lin]
    owner = towers_lin[0]
    biases = _stack_cached(owner, "_pna_amd_bias_stack", [lin.bias for lin in towers_lin]) if towers_lin[0].bias is not None else None
    cs = ct = None
    if bns is not None:
        folds = [_fold_batchnorm(bn) for bn in bns]
        cs = _stack_cached(owner, "_pna_amd_cs_stack", [f[0] for f in folds])
        ct = _stack_cached(owner, "_pna_amd_ct_stack", [f[1] for f in folds])
    if row_post is not None:
        row_post = row_post.reshape(-1).contiguous()
    return ops.posttrans_towers(_unit_stride(agg), K, weights, row_scales, biases, _unit_stride(hs), h_shared, out, row_post=row_post,
                                col_scale=cs, col_shift=ct, relu=relu)


def linear_act(x, weight, bias, leaky_slope=None, relu=False, residual=None, out=None):
    """act(x @ weight^T + bias) (+ residual) on the contraction kernels (inference): the tower layers' mixing network
    (FCLayer(out, out, 'LeakyReLU') + residual, models/dgl/pna_layer.py:128,:141-144) as one launch."""
    w = weight if weight.stride(-1) == 1 else weight.contiguous()
    return ops.posttrans(_unit_stride(x), x.shape[1], w, [None], bias, out=out, relu=relu, leaky_slope=leaky_slope,
                         residual=_unit_stride(residual))


# ---- molecule-sized batches: the whole tower layer as one C call (pna_tower_layer_f32) --------------------------------------
SMALL_TOWER_ROWS = int(os.environ.get("PNA_AMD_SMALL_TOWER_ROWS", "32768"))   # batches up to this many nodes take that path


def small_tower_fits(T, Fi, Fo, divided, No=None):
    """pna_tower_layer_f32's own LDS check (pna_tower_layer_lds_bytes): its tile at a single tower per pass, the smallest it can run
    with, within the budget.  No: the mixing network's output width, None without one.  The last shape's answer is kept (one memo
    entry on this function): a layer whose whole call is some 30 us asks on every call."""
    shape = (T, Fi, Fo, No or 0, bool(divided))
    return 0 < memo(small_tower_fits, "_pna_amd_answer", (), shape, lambda: _lib.lib().pna_tower_layer_lds_bytes(*shape)) <= ops.LDS_BUDGET


# bf16 batches up to this many nodes take pna_tower_layer_bf16 (one C call); 0 turns the path off.  The default follows
# tools/bench_bf16_small.py (profiles/bf16_small.json): the largest measured batch on which the one-call kernel is
# not slower than the multi-launch path.
BF16_SMALL_ROWS = int(os.environ.get("PNA_AMD_BF16_SMALL_ROWS", "4096"))


def bf16_small_applies(graph, V, *, T, Fi, Fo, A, divide_input, posttrans_affine, edge_features=False, etab=None, No=None,
                       no_self_panel=False):
    """Whether a bf16 inference call is served by pna_tower_layer_bf16: a molecule-sized batch (0 < V <= BF16_SMALL_ROWS) without
    heavy rows (hub rows keep the segment path of the multi-launch kernels), a posttrans that is one Linear, edge features that are
    absent or an edge-type table `etab` (Graph.edge_type_table: <= 4 distinct rows), and a 16-row tile that fits the LDS."""
    if not 0 < V <= BF16_SMALL_ROWS or not posttrans_affine:
        return False
    if edge_features and etab is None:
        return False
    if not 0 < ops.tower_layer_bf16_lds_bytes(T, Fi, Fo, A, divide_input, No=No, no_self_panel=no_self_panel) <= ops.LDS_BUDGET:
        return False
    return graph.heavy_schedule().n_heavy == 0


def _no_plan():
    """What a copied / unpickled layer holds in place of its one-call plan (_SmallTowerPlan.__reduce__): nothing."""
    return None


class _SmallTowerPlan:
    """Everything pna_tower_layer_f32 reads besides the graph and h -- the packed projection / posttrans / mixing images, the
    concatenated biases and folded BatchNorm constants -- and a pre-filled argument block, built once per weight state.  The
    host side of this path is on the critical path (the two launches take ~50 us for a 128-molecule batch), so a call only
    compares the parameters' version counters and fills in the per-call pointers."""

    edge_dim = 0                                               # (plans without edge features: _SmallSimplePlan)
    _etab = None

    def __init__(self, towers, mix, divide_input):
        t0 = towers[0]
        self.edge_dim = t0.edge_dim if t0.edge_features else 0
        self._etab = None                                      # (edge_table's entry: the graph's type rows projected, W_e . ef_t)
        pre = [t.pretrans.fully_connected[0].linear for t in towers]
        post = [t.posttrans.fully_connected[0].linear for t in towers]
        if t0.batch_norm and any(t.batchnorm_h.training for t in towers):
            raise RuntimeError("only an eval-mode BatchNorm (running statistics) can be folded into the epilogue")
        self.ts = _tower_tensors(towers, pre=True, post=True, bn=t0.batch_norm, mix=mix)
        self.versions = tensor_key(self.ts)
        T, Fi, Fo, S = len(towers), t0.in_dim, t0.out_dim, len(t0.scalers)
        self.T, self.Fi, self.Fo, self.S, self.divide_input = T, Fi, Fo, S, divide_input
        with torch.no_grad():
            Wa = [l.weight[:, :Fi] for l in pre]
            Wb = [l.weight[:, Fi:2 * Fi] for l in pre]
            if divide_input:
                Wcat = torch.cat([torch.block_diag(*Wa), torch.block_diag(*Wb)], dim=0)
            else:
                Wcat = torch.cat(Wa + Wb, dim=0)
            b = torch.cat([l.bias if l.bias is not None else torch.zeros(Fi, device=Wcat.device) for l in pre])
            # W_e of every tower stacked (T*Fi, edge_dim): the <= 4 edge-type rows are projected through it once per (graph batch, e)
            self.We = torch.cat([l.weight[:, 2 * Fi:2 * Fi + self.edge_dim] for l in pre], dim=0).contiguous() if self.edge_dim else None
            keep = dict(proj_img=ops.pack_small(Wcat.contiguous()), proj_bias=torch.cat([torch.zeros_like(b), b]).contiguous(),
                        post_img=ops.pack_tower_post([l.weight for l in post], Fi, Fo, S),
                        post_bias=torch.cat([l.bias for l in post]).contiguous() if post[0].bias is not None else None)
            if t0.batch_norm:
                folds = [_fold_batchnorm(t.batchnorm_h) for t in towers]
                keep["col_scale"] = torch.cat([f[0] for f in folds]).contiguous()
                keep["col_shift"] = torch.cat([f[1] for f in folds]).contiguous()
            if mix is not None:
                keep["mix_img"] = ops.pack_small(mix.linear.weight)
                keep["mix_bias"] = mix.linear.bias.detach().contiguous() if mix.linear.bias is not None else None
        self.keep = keep                                       # the device buffers the argument block points into
        self.device = Wcat.device
        self.width = mix.linear.weight.shape[0] if mix is not None else T * Fo
        self.xw = 2 * T * Fi
        self.graph_norm = bool(t0.graph_norm)
        a = _lib.PnaTowerLayerArgs()
        a.n_tower, a.Fi, a.Fo, a.divide_input, a.n_scaler = T, Fi, Fo, 1 if divide_input else 0, S
        for k, v in keep.items():
            if v is not None:
                setattr(a, k, _lib.dev_ptr(v, torch.float32, k))
        if mix is not None:
            a.No = self.width
            if isinstance(mix.activation, torch.nn.LeakyReLU):
                a.mix_act, a.mix_slope = 2, float(mix.activation.negative_slope)
            elif mix.activation is not None:
                a.mix_act = 1
        self.args, self.ref = a, ctypes.byref(a)
        self.fn = _lib.lib().pna_tower_layer_f32
        self.check, self.stream_ptr = _lib.check, _lib.stream_ptr

    def __reduce__(self):
        # copy.deepcopy / pickle / torch.save of a warm layer: the plan holds a ctypes argument block (not copyable) that points into
        # THIS layer's device buffers -- a copy carries no plan and builds its own on its first call
        return (_no_plan, ())

    def stale(self):
        return tensor_key(self.ts) != self.versions

    def edge_table(self, etab):
        """(n_types, T*Fi) = type rows @ W_e^T, kept per state of the graph's type rows (graph.edge_type_table: cached per feature
        tensor) -- the weights' own staleness replaces the whole plan."""
        return memo(self, "_etab", [etab[1]], None, lambda: (etab[1].to(torch.float32) @ self.We.t()).contiguous())

    def run(self, graph, h, snorm_n, row_scales, residual, etab=None):
        if h.stride(-1) != 1:
            h = h.contiguous()
        dev = h.device
        if dev != self.device:
            raise RuntimeError(f"layer parameters live on {self.device}, features on {dev}")
        V = h.shape[0]
        csr = graph.csr
        out = torch.empty((V, self.width), dtype=torch.float32, device=dev)
        xc = torch.empty((V, self.xw), dtype=torch.float32, device=dev)
        a = type(self.args)()                                # per-call copy of the pre-filled block: concurrent calls of one layer from
        ctypes.memmove(ctypes.byref(a), self.ref, ctypes.sizeof(a))      # two host threads / streams do not race on it
        a.rowptr, a.col, a.V = csr.rowptr.data_ptr(), csr.col.data_ptr(), V
        a.h, a.ldh = h.data_ptr(), h.stride(0)
        a.x_cat, a.ldx = xc.data_ptr(), self.xw
        for i in range(self.S):
            rs = row_scales[i]
            a.row_scale[i] = None if rs is None else rs.data_ptr()
        if self.graph_norm and snorm_n is not None:
            if snorm_n.dtype != torch.float32 or snorm_n.numel() != V or snorm_n.device != dev or not snorm_n.is_contiguous():
                snorm_n = snorm_n.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
                if snorm_n.numel() != V:
                    raise ValueError("snorm_n must hold one factor per node")
            a.row_post = snorm_n.data_ptr()
        else:
            a.row_post = None
        if residual:
            a.residual, a.ld_res = a.h, a.ldh
        else:
            a.residual = None
        a.y, a.ldy = out.data_ptr(), self.width
        if self.edge_dim:
            if etab is None:
                raise RuntimeError("tower_layer_small: an edge-feature layer needs the graph's edge-type table")
            tab = self.edge_table(etab)
            a.edge_type, a.edge_table, a.ld_edge_table, a.n_edge_types = etab[0].data_ptr(), tab.data_ptr(), tab.stride(0), tab.shape[0]
        rc = self.fn(ctypes.byref(a), self.stream_ptr(dev))
        if rc != 0:
            self.check(rc, "pna_tower_layer_f32")
        del snorm_n, xc                                      # (stream-ordered allocator: safe to release after the launch)
        return out


def degree_grouped_aggregate(layer, graph, h, plan, out=None, x=None):
    """The (plan.rows, 4F) aggregate in the plan's row order (degree groups padded to whole tiles, then the rest): the gather's
    work list carries the output row of every whole-row record, heavy_out the output rows of the hub rows.  On a sharded
    graph the halo exchange is started first and the rows that read only local sources are aggregated while it is in flight
    (two launches, like functional.aggregate); `x`: the source table with the halo already in place (no exchange here)."""
    F = layer.in_dim
    K = len(layer.aggregators) * F
    if x is None:
        x = graph.source_features(h, defer=True)
    x = _unit_stride(x)
    csr = graph.csr
    if out is None:
        out = torch.empty(plan.rows, DG.agg_pitch(K), dtype=torch.float32, device=h.device)[:, :K]     # line-aligned rows
    if getattr(graph, "_pending", None) is not None:
        items_in, items_bd = plan.split_items(graph)
        try:
            if items_in.shape[0]:
                ops.segreduce(csr.rowptr, csr.col, x, F, layer.aggregators, (None,), tower_stride_in=F, out=out, items=items_in,
                              tune=dict(generic=2))
        finally:
            graph.finish_exchange()
        if items_bd.shape[0]:
            ops.segreduce(csr.rowptr, csr.col, x, F, layer.aggregators, (None,), tower_stride_in=F, out=out,
                          heavy=graph.heavy_schedule(), workspace=graph.workspace, items=items_bd, heavy_out=plan.heavy_out,
                          tune=dict(generic=2))
        return out
    ops.segreduce(csr.rowptr, csr.col, x, F, layer.aggregators, (None,), tower_stride_in=F, out=out,
                  heavy=graph.heavy_schedule(), workspace=graph.workspace, items=plan.items, heavy_out=plan.heavy_out, tune=dict(generic=2))
    return out


def _simple_layer_state(layer):
    """The state (tensor_key) of every tensor a cached FusedDegreeCall of `layer` snapshots: the posttrans Linear and the BatchNorm.
    Part of a dictionary key of SimpleLayerRows._calls; the cached call holds `layer`, which holds these tensors: the ids stay taken."""
    lin = layer.posttrans.fully_connected[0].linear
    ts = [lin.weight, lin.bias]
    if layer.batch_norm:
        bn = layer.batchnorm_h
        ts += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    return tensor_key(ts)


def _layer_tail_operands(layer, h):
    """(column scale, column shift, residual) of the simple layer's epilogue: eval BatchNorm folded, the input as residual."""
    cs = ct = None
    if layer.batch_norm:
        cs, ct = _fold_batchnorm(layer.batchnorm_h)
    return cs, ct, (_unit_stride(h) if layer.residual else None)


def _rest_posttrans(layer, graph, agg_rest, plan, scales, y, cs, ct, res):
    """The rows no degree group holds (rare degrees, hub rows): the ordinary three-block contraction over their compact list
    `agg_rest` ((plan.NRp, 4F): the four STANDARD statistics, virtual order; (plan.NRp, 5F) with room for a fifth block when the layer
    aggregates `sum`), rows scattered to node order.  A layer with another aggregator list (round 6) contracts against its weight
    re-expressed over those statistics (degree_groups.virtual_layer_weight); the sum block = in-degree x mean is formed here."""
    F, N = layer.in_dim, layer.out_dim
    K = 4 * F
    lin = layer.posttrans.fully_connected[0].linear
    from .dgl.pna_layer import _avg_log_value
    rest_scales = plan.rest_scales(tuple(layer.scalers) + (_avg_log_value(layer.avg_d),), scales)
    weight = lin.weight
    if tuple(layer.aggregators) != DG.STANDARD_AGGREGATORS:
        weight, K = DG.virtual_layer_weight(lin.weight, F, layer.aggregators, len(scales))
        if K == 5 * F:
            deg = plan.__dict__.get("_rest_deg")
            if deg is None:
                deg = torch.zeros(max(plan.NRp, 1), 1, dtype=torch.float32, device=y.device)
                deg[:plan.NR, 0] = plan._deg[plan.rest_rows].to(torch.float32)
                deg = plan.__dict__["_rest_deg"] = deg[:plan.NRp]
            torch.mul(agg_rest[:, :F], deg, out=agg_rest[:, 4 * F:5 * F])
    _contract_rest_rows(plan, agg_rest, K, weight, rest_scales, lin.bias, y, N, col_scale=cs, col_shift=ct, relu=True, residual=res)


def _contract_rest_rows(plan, agg, K, weight, rest_scales, bias, y, N, **tail):
    """The three-block contraction over the rest rows' compact list `agg` (plan.NRp rows, virtual order), rows scattered to node order in
    `y`; `tail`: the epilogue operands of ops.posttrans (row_post in virtual order, residual in node order)."""
    if N <= 80 and len(rest_scales) == 3:
        ops.posttrans(agg, K, weight, rest_scales, bias, out=y, row_perm=plan.perm_rest, n_out=N, **tail)
        return
    # 128-column block (three blocks x three weight buffers do not fit the LDS) or another scaler count (no grouped instantiation): the few
    # rest rows take the ordinary kernel over their compact list and are scattered by index (three small torch kernels)
    rr, post, res = plan.rest_rows, tail.pop("row_post", None), tail.pop("residual", None)
    y_r = ops.posttrans(agg[:plan.NR], K, weight, [None if r is None else r[:plan.NR] for r in rest_scales], bias,
                        row_post=None if post is None else post[:plan.NR], residual=None if res is None else res.index_select(0, rr),
                        arith="bf16x3", **tail)
    y.index_copy_(0, rr, y_r)


def degree_grouped_posttrans(layer, graph, h, agg, plan, out=None):
    """The two contractions over `agg` (degree_grouped_aggregate): one combined block per degree tile, three blocks for the rest;
    both scatter their rows to node order with BatchNorm / ReLU / residual in the epilogue."""
    from .dgl.pna_layer import _row_scales
    F, N = layer.in_dim, layer.out_dim
    K = len(layer.aggregators) * F
    lin = layer.posttrans.fully_connected[0].linear
    scales = _row_scales(graph, layer.scalers, layer.avg_d, h.device)
    y = torch.empty(h.shape[0], N, dtype=torch.float32, device=h.device) if out is None else out
    cs, ct, res = _layer_tail_operands(layer, h)
    if plan.G:
        img, stride = DG.combined_images(lin.weight, K, scales, plan)
        ops.posttrans(agg[:plan.NV], K, lin.weight, [None], lin.bias, out=y, col_scale=cs, col_shift=ct, relu=True, residual=res,
                      row_perm=plan.perm, tile_image=plan.tile_image, w_img=img, image_stride=stride, n_out=N)
    if plan.NR:                 # (on a side stream beside the grouped launch: measured, no gain -- one after the other)
        _rest_posttrans(layer, graph, agg[plan.NV:], plan, scales, y, cs, ct, res)
    return y


def _tower_collapsed_weights(owner, towers, mix, divide_input):
    """The tower layers' posttrans Linear, graph norm, eval BatchNorm and the mixing Linear have NO non-linearity between them
    (models/dgl/pna_layer.py:65-75, :141): for all towers t with z_t = [h_t | S a_t],
        W_m concat_t BN_t(snorm (W_t z_t + b_t)) + b_m  =  snorm (sum_t C_t z_t + d) + c,
        C_t = W_m[:, t] P_t W_t,   d = sum_t W_m[:, t] P_t b_t,   c = sum_t W_m[:, t] q_t + b_m        (BN_t(u) = P_t u + q_t)
    -- one contraction of [a_1 .. a_T | h] against the collapsed weight instead of T posttrans contractions, a (V, T Fo)
    intermediate and a mixing GEMM.  Returned as a virtual nn.Linear weight (out, S * K) in scaler blocks of
    K = T * 4 Fi + in_dim columns [C_1,s | .. | C_T,s | h panel (block 0 only)], so that the degree-grouped machinery of the simple
    layer (combined images W_D, three-block rest) applies unchanged; formed in float64, rounded once.  Cached on `owner`."""
    t0 = towers[0]
    T, Fi, Fo, S = len(towers), t0.in_dim, t0.out_dim, len(t0.scalers)
    ts = _tower_tensors(towers, post=True, bn=t0.batch_norm, mix=mix)

    def build():
        lins = [t.posttrans.fully_connected[0].linear for t in towers]
        Wm = mix.linear.weight.double()
        out = Wm.shape[0]
        in_dim = T * Fi if divide_input else Fi
        K = T * 4 * Fi + in_dim
        Wv = torch.zeros(out, S * K, dtype=torch.float64, device=Wm.device)
        d = torch.zeros(out, dtype=torch.float64, device=Wm.device)
        c = mix.linear.bias.double().clone() if mix.linear.bias is not None else torch.zeros(out, dtype=torch.float64, device=Wm.device)
        for t, (tower, lin) in enumerate(zip(towers, lins)):
            if tower.batch_norm:
                bn = tower.batchnorm_h
                p = (bn.weight.double() if bn.weight is not None else 1.0) / torch.sqrt(bn.running_var.double() + bn.eps)
                q = (bn.bias.double() if bn.bias is not None else 0.0) - bn.running_mean.double() * p
            else:
                p, q = torch.ones(Fo, dtype=torch.float64, device=Wm.device), torch.zeros(Fo, dtype=torch.float64, device=Wm.device)
            WmP = Wm[:, t * Fo:(t + 1) * Fo] * p[None, :]
            C = WmP @ lin.weight.double()                                        # (out, Fi + S * 4 Fi): [h | scaler blocks]
            if lin.bias is not None:
                d += WmP @ lin.bias.double()
            c += Wm[:, t * Fo:(t + 1) * Fo] @ q
            for s_ in range(S):
                Wv[:, s_ * K + t * 4 * Fi:s_ * K + (t + 1) * 4 * Fi] = C[:, Fi + s_ * 4 * Fi:Fi + (s_ + 1) * 4 * Fi]
            hcol = T * 4 * Fi + (t * Fi if divide_input else 0)
            Wv[:, hcol:hcol + Fi] += C[:, :Fi]                                   # block 0 (the identity scaler's) carries the h panel
        return (Wv.float().contiguous(), d.float().contiguous(), c.float().contiguous(), torch.ones(out, dtype=torch.float32, device=Wm.device), K)
    return memo(owner, "_pna_amd_collapsed", ts, divide_input, build)


def tower_layer_degree_grouped_applies(layer, graph, h):
    """Whether PNALayer.forward (eval) takes the degree-grouped path below: a large whole graph, 1-layer pretrans / posttrans, no
    edge features, the four standard aggregators, 3 scalers led by `identity`, a LeakyReLU mixing network without batch norm."""
    from .graph import Graph
    towers = list(layer.towers)
    t0, mix = towers[0], layer.mixing_network
    if layer.training or not h.is_cuda or h.dtype != torch.float32 or type(graph) is not Graph or layer.edge_features:
        return False
    if not (DG.ENABLED and DG.TOWERS and h.shape[0] >= DG.MIN_ROWS and DG.MIN_OUT <= layer.out_dim <= 128 and t0.in_dim >= 4 and ops.POSTTRANS_ARITH != "f32"):
        return False
    if not (tuple(t0.aggregators) == ("mean", "max", "min", "std") and len(t0.scalers) == 3 and t0.scalers[0] == "identity"
            and isinstance(mix.activation, torch.nn.LeakyReLU) and mix.b_norm is None and mix.linear.bias is not None
            and all(t.pretrans.is_affine and t.posttrans.is_affine and t.scalers == t0.scalers and t.aggregators == t0.aggregators
                    and t.graph_norm == t0.graph_norm and t.batch_norm == t0.batch_norm and not t.training for t in towers)):
        return False
    if torch.is_grad_enabled() and (h.requires_grad or any(p.requires_grad for p in layer.parameters())):
        return False
    n_edges = graph.csr.col.numel()
    if not (0 < n_edges < (1 << 30)) or h.shape[0] >= (1 << 24):
        return False
    plan = DG.plan_of(graph)
    K = len(towers) * 4 * t0.in_dim + layer.in_dim
    return plan.G > 0 and plan.NR <= DG.MAX_REST_FRACTION * h.shape[0] and plan.rows * DG.agg_pitch(K) * 4 < (1 << 34)


def tower_layer_degree_grouped(layer, graph, h, snorm_n, x_src, x_dst):
    """PNALayer.forward (eval; models/dgl/pna_layer.py:130-145 over :55-76) after the node-level projections: the gather writes
    every tower's aggregate in DEGREE order (pna_segreduce_args.out_row_of), the rows' own features are copied behind it, and ONE
    degree-grouped contraction per row class (combined block W_D over the degree tiles, three scaler blocks over the rest) applies
    the collapsed posttrans . graph norm . BatchNorm . mixing weight (see _tower_collapsed_weights) with LeakyReLU and the
    residual in its epilogue."""
    from .dgl.pna_layer import _row_scales
    towers, mix = list(layer.towers), layer.mixing_network
    t0 = towers[0]
    T, Fi = len(towers), t0.in_dim
    V, dev = h.shape[0], h.device
    plan = DG.plan_of(graph)
    Wv, d, c, ones, K = _tower_collapsed_weights(layer, towers, mix, layer.divide_input)
    N = Wv.shape[0]
    Ka = T * 4 * Fi
    buf = torch.empty(plan.rows, DG.agg_pitch(K), dtype=torch.float32, device=dev)
    csr = graph.csr
    ops.segreduce(csr.rowptr, csr.col, _unit_stride(x_src), Fi, t0.aggregators, (None,), n_tower=T, tower_stride_in=Fi, dst_term=_unit_stride(x_dst),
                  out=buf, tower_stride_out=4 * Fi, heavy=graph.heavy_schedule(), workspace=graph.workspace, items=graph.work_items(),
                  out_row_of=plan.vmap32(), heavy_out=plan.heavy_out, tune=dict(generic=2))
    hc = _unit_stride(h)
    ops.pack_rows(hc, plan.perm_all(), out=buf[:, Ka:Ka + hc.shape[1]])
    scales = _row_scales(graph, t0.scalers, t0.avg_d, dev)
    y = torch.empty(V, N, dtype=torch.float32, device=dev)
    res = hc if layer.residual else None
    slope = float(mix.activation.negative_slope)
    post_g, post_r = _graph_norm_rows(plan, snorm_n, t0.graph_norm)
    if plan.G:
        img, stride = DG.combined_images(Wv, K, scales, plan)
        ops.posttrans(buf[:plan.NV, :K], K, Wv, [None], d, out=y, row_post=post_g, col_scale=ones, col_shift=c, leaky_slope=slope, residual=res,
                      row_perm=plan.perm, tile_image=plan.tile_image, w_img=img, image_stride=stride, n_out=N)
    if plan.NR:
        from .dgl.pna_layer import _avg_log_value
        rest_scales = plan.rest_scales(tuple(t0.scalers) + (_avg_log_value(t0.avg_d),), scales)
        _contract_rest_rows(plan, buf[plan.NV:, :K], K, Wv, rest_scales, d, y, N, row_post=post_r, col_scale=ones, col_shift=c, leaky_slope=slope,
                            residual=res)
    return y


def tower_projection_pitch(Fi):
    """Column pitch of one half of the [x_src | x_dst] table the one-kernel tower layer gathers from: rows 16-byte aligned, the
    last strip inside the half."""
    return (Fi + 7) // 8 * 8


def tower_layer_degree_fused_applies(layer, graph, h):
    """Whether the grouped tower path runs its group rows through pna_fused_degree_f32's tower mode: gathers of 49..80 message
    features, at most 80 outputs, features the kernel can read in 16-byte pieces.  That is a layer with one tower; T towers with
    divide_input=True (round 5; models/dgl/pna_layer.py:133-136: tower t sees the input slice [t Fi, (t+1) Fi), so all towers' messages
    together are in_dim = T Fi wide: ONE gather over the block-diagonal projection, and the collapsed posttrans . BatchNorm . mixing
    weight is dense anyway); and -- round 6 -- T towers with divide_input=False (:137-139: T DIFFERENT projections of the whole input,
    T x in_dim message features per edge): one launch per tower over its own 49..80 projected features, the partial sums carried from
    launch to launch (FusedMultiTowerCall)."""
    towers = list(layer.towers)
    T, Fi = len(towers), towers[0].in_dim
    if not DG.FUSED or not 4 <= layer.out_dim <= 80:
        return False
    if T == 1 or layer.divide_input:
        Fe = T * Fi                                        # message features per edge, all towers
        if not (49 <= Fe <= 80 and layer.in_dim == Fe and DG.fused_applies(graph, h, Fe, layer.out_dim)):
            return False
        return h.shape[0] * 2 * tower_projection_pitch(Fe) * 4 < (1 << 32)
    if not (49 <= Fi <= 80 and layer.in_dim == Fi and T <= FUSED_MAX_TOWER_PASSES and DG.fused_applies(graph, h, Fi, layer.out_dim)):
        return False
    return h.shape[0] * 2 * T * tower_projection_pitch(Fi) * 4 < (1 << 32)


FUSED_MAX_TOWER_PASSES = 8     # towers of a divide_input=False layer the one-kernel path takes (one launch -- one gather -- per tower)


def _tower_flat_weights(layer, towers, mix):
    """_tower_collapsed_weights for the one-kernel tower layer: the same collapsed weight with the columns of every scaler block
    re-ordered from tower-major [t: mean | max | min | std] (Fi each) to aggregator-major over ALL towers' features
    [mean (T Fi) | max | min | std | h panel] -- the layout of ONE tower of Fe = T Fi features, which is what the gather over the
    block-diagonal projection produces (divide_input=True; one tower: the identity)."""
    Wv, d, c, ones, K = _tower_collapsed_weights(layer, towers, mix, layer.divide_input)
    T, Fi = len(towers), towers[0].in_dim
    if T == 1:
        return Wv, d, c, ones, K

    def build():
        S = Wv.shape[1] // K
        Fe = T * Fi
        a_ = torch.arange(4, device=Wv.device).view(4, 1, 1)
        t_ = torch.arange(T, device=Wv.device).view(1, T, 1)
        f_ = torch.arange(Fi, device=Wv.device).view(1, 1, Fi)
        cols = torch.cat([(t_ * 4 * Fi + a_ * Fi + f_).reshape(-1), torch.arange(4 * Fe, K, device=Wv.device)])      # new column -> old column
        idx = torch.cat([s_ * K + cols for s_ in range(S)])
        return Wv.index_select(1, idx).contiguous()
    return memo(layer, "_pna_amd_flat", [Wv], None, build), d, c, ones, K


_SIDE_STREAMS = {}
# How a one-kernel layer's two halves are recorded while a hipGraph is being CAPTURED (round 6): "beside" = as in eager
# mode (fork / join events become two branches of the graph), "behind" = one after the other on the capturing stream, whole device each,
# "rest_first" = the same with the small launches in front.  tools/graph_replay_ab.py measures the three against the eager step.
CAPTURE_OVERLAP = os.environ.get("PNA_AMD_CAPTURE_OVERLAP", "beside")


def _side_stream(device):
    """The second stream beside the CALLER's current stream: where the rest-row launches of the one-kernel layers run.  One side
    stream per (device, caller stream), so callers on different streams do not serialise on one another's chains.  What stays
    shared per GRAPH is its reallocating `graph.workspace` and the plan's lazily filled caches: layers over ONE Graph object must be
    run from one stream / thread at a time; different Graph objects are independent."""
    idx = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    key = (idx, torch.cuda.current_stream(idx).cuda_stream)
    hit = _SIDE_STREAMS.get(key)
    if hit is None:
        if len(_SIDE_STREAMS) > 64:
            _SIDE_STREAMS.clear()
        hit = _SIDE_STREAMS[key] = torch.cuda.Stream(device=idx)
    return hit


def run_fused_call(call):
    """The two halves of a one-kernel layer (a _FusedCall): the persistent kernel over the group rows and the
    chain of small launches over the rest rows (hub rows, rare degrees).  On a large graph the chain runs BESIDE the kernel: the
    kernel books every register of every CU it sits on, so it leaves `degree_groups.FUSED_SPARE_WGS` of its workgroups out and
    the chain goes to a second stream, forked and joined with events around the call (benchmark graph: 0.852 -> 0.807 ms; the two
    halves write disjoint rows of y).  The caller's stream sees one call: everything it issued before is visible to both halves,
    everything it issues afterwards waits for both."""
    plan = call.plan
    call.stream = _lib.stream_ptr(call.y.device)             # (the kernel goes to the stream that is current NOW, like every other launch)
    call.prologue()                                          # (what BOTH halves read: in front of the fork)
    overlap = plan.rest_overlap_applies(call.layer_F())
    if overlap and CAPTURE_OVERLAP != "beside" and torch.cuda.is_current_stream_capturing():
        overlap = False                                      # (see CAPTURE_OVERLAP)
        if CAPTURE_OVERLAP == "rest_first":
            call.set_spare(False)
            call.rest_rows()
            call.group_rows()
            return call.y
    if not overlap:
        call.set_spare(False)
        call.group_rows()
        return call.rest_rows()
    dev = call.y.device
    main = torch.cuda.current_stream(dev)
    side, fork, join = _side_stream(dev), torch.cuda.Event(), torch.cuda.Event()   # (events per call; one Graph object: one caller at a time)
    call.set_spare(True)
    fork.record(main)
    call.group_rows()
    side.wait_event(fork)
    with torch.cuda.stream(side):
        call.rest_rows()
        join.record(side)
    main.wait_event(join)
    return call.y


out_pitch = DG.out_pitch


def own_buffer_cols(pitch, c0, c1, N):
    """pna_fused_degree_args.y_cols_writable for the column panel [c0, c1) of a row of N columns in a buffer THIS module allocated at `pitch`
    floats (out_pitch): the last panel may write zeros into the row's padding up to the next multiple of 16 columns -- whole 32-byte
    sectors and one 16-byte store for the row's last window (WRITE_PADDING = False: off, for A/B runs)."""
    if not WRITE_PADDING or c1 != N:
        return 0
    return max(c1 - c0, min(pitch - c0, (c1 - c0 + 15) // 16 * 16))


WRITE_PADDING = os.environ.get("PNA_AMD_WRITE_PADDING", "1") != "0"


def _fused_grid(device, spare, n_tiles64):
    """Workgroups pna_fused_degree_f32 launches for the 4-wavefront shapes (pna_fused_degree.hip: two per CU, less the spare ones, never
    below one per CU, never more than tiles)."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    wgs = 2 * cus
    if spare > 0:
        wgs = wgs - spare if wgs - spare > cus else cus
    return max(1, min(wgs, n_tiles64))


DEBUG_COUNTERS = os.environ.get("PNA_AMD_DEBUG_COUNTERS", "0") == "1"   # host-side check (one sync per launch) that the tile counter pair and the
# guard's working words are zero in front of a launch of the one-kernel layer: a launch that left them non-zero would make every later launch
# on the plan skip tiles silently


class _TileOrder(NamedTuple):
    """What one (spare, balance knobs, stream) binds into the argument blocks: device pointers, and `keep` = the tensors behind them
    (tile_desc, row_perm, row_post, tile counter, guard workspace)."""
    tile_desc: int
    row_perm: int
    tile_counter: Optional[int]
    row_post: Optional[int]
    guard_ws: Optional[int]
    keep: tuple


class _FusedCall:
    """What the three drivers of pna_fused_degree_f32 share: the argument blocks of the layer's launches, the helpers that fill them and
    the binding of the tile order.  A subclass builds its blocks in launch order (`_block`, then `_final` or `_partial`), names the PRIMARY
    one -- the block whose row_post follows the tile order -- in `_bind`, and brings `rest_rows()`: the rows no degree group holds, on the
    two-kernel path over their compact list."""

    def __init__(self, layer, graph, plan, h, scales, y, keep):
        self.layer, self.graph, self.plan, self.h, self.scales, self.y = layer, graph, plan, h, scales, y
        self.keep = list(plan.fused_tables()[:2]) + keep    # every tensor the blocks point into
        self.blocks, self.primary = [], 0                    # [(args, byref)] in launch order
        self.args = self.ref = self.arith = None             # the primary block; the arithmetic of the launches (_lib.FD_ARITH_*)
        self.post_g = None                                   # per-row factor of the group rows in plan order (graph norm, or ones), if any
        self._orders, self._post_b, self._bound = {}, {}, None     # _TileOrder per grid; post_g per balanced order; the order bound last
        self.fn, self.check, self.stream = _lib.lib().pna_fused_degree_f32, _lib.check, _lib.stream_ptr(y.device)

    launch_order = panel_args = property(lambda self: self.blocks)

    def _block(self, weight, F, x, N, tower=False, pre_add=None, **panel):
        """A new block with what every launch has: the plan's tables, the source slice `x` (its width = the features gathered), the rows,
        the images of `weight` over F features for the arithmetic (degree_groups.bind_fused_arith; `panel`: the part of it this launch
        takes) and the partial sums the launch adds to, if any."""
        plan = self.plan
        desc, ids, n_rec = plan.fused_tables()
        a = _lib.PnaFusedDegreeArgs()
        self.arith = DG.bind_fused_arith(a, self.keep, weight, F, self.scales, plan, tower, **panel)
        a.tile_desc, a.tile_ids, a.n_records = _lib.dev_ptr(desc, torch.int32, "tile_desc"), _lib.dev_ptr(ids, torch.int32, "tile_ids"), n_rec
        a.x, a.ldx, a.x_rows, a.F, a.N = _lib.dev_ptr(x, torch.float32, "x"), x.stride(0), x.shape[0], x.shape[1], N
        a.row_perm, a.M, a.n_nodes = _lib.dev_ptr(plan.perm, torch.int32, "row_perm"), plan.NV, self.h.shape[0]
        if pre_add is not None:
            a.pre_add, a.ld_pre_add = _lib.dev_ptr(pre_add, torch.float32, "pre_add"), pre_add.stride(0)
        self.blocks.append((a, ctypes.byref(a)))
        return a

    @staticmethod
    def _final(a, y, bias, col_scale, col_shift, residual, relu, act_slope=0.0, cols_writable=0):
        """The epilogue of a launch that finishes its columns of the layer (row_post: see _bind_tile_order)."""
        a.bias = _lib.dev_ptr(bias, torch.float32, "bias")
        a.col_scale, a.col_shift = _lib.dev_ptr(col_scale, torch.float32, "col_scale"), _lib.dev_ptr(col_shift, torch.float32, "col_shift")
        if residual is not None:
            a.residual, a.ld_res = _lib.dev_ptr(residual, torch.float32, "residual"), residual.stride(0)
        a.y, a.ldy, a.relu, a.act_slope = _lib.dev_ptr(y, torch.float32, "y"), y.stride(0), relu, act_slope
        a.y_cols_writable = cols_writable

    @staticmethod
    def _partial(a, buf, c0, c1):
        """A launch that leaves partial sums in the columns [c0, c1) of `buf`: no bias, no factor, no activation, no residual."""
        a.y, a.ldy, a.relu = _lib.dev_ptr(buf[:, c0:c1], torch.float32, "y"), buf.stride(0), 0
        a.y_cols_writable = own_buffer_cols(buf.stride(0), c0, c1, buf.shape[1])

    def _bind(self, primary):
        self.primary = primary
        self.args, self.ref = self.blocks[primary]
        self._bind_tile_order(0)

    def layer_F(self):
        return self.layer.in_dim

    def set_spare(self, on):
        self._bind_tile_order(DG.FUSED_SPARE_WGS if on else 0)

    def prologue(self):
        """What both halves read (run_fused_call launches it in front of the fork): nothing, unless a subclass says so."""

    def group_rows(self):
        for _, ref in self.blocks:
            self.check(self.fn(ref, self.stream), "pna_fused_degree_f32")
        return self.y

    def _bind_tile_order(self, spare):
        """Point every block at the plan's tile list for the grid `spare` gives, on the current stream (_tile_order).  Per (grid, balance
        knobs, stream) the pointers only: this runs in front of every launch."""
        if DEBUG_COUNTERS and self._bound is not None:
            self._check_working_words()
        spare = int(spare)
        stream = int(torch.cuda.current_stream(self.y.device).cuda_stream)      # (the counter pair and the guard's workspace belong to the stream)
        key = (spare, DG.balance_key(), stream)
        o = self._orders.get(key)
        if o is None:
            o = self._orders[key] = self._tile_order(spare, stream)
        self._bound = o
        for a, _ in self.blocks:
            a.spare_workgroups, a.tile_desc, a.row_perm, a.tile_counter = spare, o.tile_desc, o.row_perm, o.tile_counter
            if o.guard_ws is not None:
                a.guard_ws = o.guard_ws
        if o.row_post is not None:
            self.args.row_post = o.row_post

    def _tile_order(self, spare, stream):
        """The _TileOrder of a grid: the load-balanced order (DegreePlan.fused_balance) for the production instantiations of the 64-row-tile
        shapes, the plan's own order otherwise (the verification instantiation writes agg_out in plan order; the 8-wavefront build of the
        wide shapes has 128-row tiles); post_g permuted with its rows; the stream's tile counter pair and guard workspace."""
        plan, a, dev = self.plan, self.args, self.y.device
        bal = None
        if not a.agg_out and plan.NV and _lib.lib().pna_fused_degree_tile_rows(a.F, a.N) == 64:
            bal = plan.fused_balance(_fused_grid(dev, spare, plan.NV // 64))
        post = self.post_g
        if bal is None:
            desc, perm = plan.fused_tables()[0], plan.perm
        else:
            desc, perm, src = bal
            if post is not None and post is not plan.ones_rows():
                moved = self._post_b.get(src.data_ptr())
                if moved is None:
                    moved = self._post_b[src.data_ptr()] = post.view(plan.NV // 64, 64)[src].reshape(-1).contiguous()
                post = moved
        counter = None
        if bal is not None and DG.FUSED_BALANCE == "dynamic":
            # ONE counter pair per (plan, stream) (zero between launches: the kernel's last workgroup resets it; launches on one stream are
            # ordered, launches on different streams get different pairs): a per-call tensor would put an allocation and a fill kernel in
            # front of every forward
            counters = plan.__dict__.setdefault("_tile_counters", {})
            counter = counters.get((str(dev), stream))
            if counter is None:                                  # (claims | finished: the kernel leaves them zero)
                if len(counters) > 16:
                    counters.clear()
                counter = counters[(str(dev), stream)] = torch.zeros(2, dtype=torch.int32, device=dev)
        gws = None
        if a.arith == _lib.FD_ARITH_GUARDED:                     # the guard's hand-over workspace: one per (plan, stream) too
            gws = DG.guard_workspace(plan, dev)
            for b, _ in self.blocks:
                b.guard_ws_bytes = gws.numel() * 4

        def ptr(t, dtype, name):
            return None if t is None else _lib.dev_ptr(t, dtype, name).value
        return _TileOrder(ptr(desc, torch.int32, "tile_desc"), ptr(perm, torch.int32, "row_perm"), ptr(counter, torch.int32, "tile_counter"),
                          ptr(post, torch.float32, "row_post"), ptr(gws, torch.int32, "guard_ws"), (desc, perm, post, counter, gws))

    def _check_working_words(self):
        """DEBUG_COUNTERS: the tile counter pair and the guard's working words of the order bound last are zero."""
        *_, counter, gws = self._bound.keep
        torch.cuda.current_stream(self.y.device).synchronize()
        for name, t in (("tile_counter", counter), ("guard workspace", gws)):
            if t is not None and t[:2].tolist() != [0, 0]:
                raise RuntimeError(f"pna_amd: the {name} of this plan / stream is {t[:2].tolist()} in front of a launch (expected [0, 0]): an earlier launch "
                                   "was aborted or ran on another stream than it was bound on")


def _graph_norm_rows(plan, snorm_n, graph_norm, ones=False):
    """(post_g, post_r): the graph norm's per-row factor in the plan's order, group rows | rest rows.  Without graph norm: (None, None), or
    -- `ones`, the one-kernel tower calls, whose kernel always multiplies -- (plan.ones_rows(), None)."""
    if graph_norm and snorm_n is not None:
        post = snorm_n.reshape(-1).to(torch.float32)[plan.perm_all().long()]
        return post[:plan.NV].contiguous(), post[plan.NV:].contiguous()
    return (plan.ones_rows() if ones else None), None


class _FusedTowerRows(_FusedCall):
    """What the two tower drivers share: the collapsed epilogue (bias d, graph norm, constants c, LeakyReLU, residual) and the rest rows
    -- gather over the projected sources, the rows' own term copied behind the statistics, three-block contraction; a subclass gives the
    gather's arguments (`_rest_operands`)."""

    def __init__(self, layer, graph, h, snorm_n, keep):
        from .dgl.pna_layer import _row_scales
        plan, t0 = DG.plan_of(graph), layer.towers[0]
        N = layer.out_dim
        y = torch.empty(h.shape[0], out_pitch(N), dtype=torch.float32, device=h.device)[:, :N]
        super().__init__(layer, graph, plan, h, _row_scales(graph, t0.scalers, t0.avg_d, h.device), y, keep)
        self.t0, self.res, self.slope = t0, (h if layer.residual else None), float(layer.mixing_network.activation.negative_slope)
        self.post_g, self.post_r = _graph_norm_rows(plan, snorm_n, t0.graph_norm, ones=True)

    def _tower_final(self, a):
        N = self.y.shape[1]
        self._final(a, self.y, self.d, self.ones, self.c, self.res, 2, self.slope, own_buffer_cols(self.y.stride(0), 0, N, N))

    def rest_rows(self):
        plan, graph, t0 = self.plan, self.graph, self.t0
        if plan.NR:
            from .dgl.pna_layer import _avg_log_value
            F, n_tower, gather, own, weight = self._rest_operands()
            Ka = n_tower * 4 * F
            K = Ka + own.shape[1]
            agg = torch.empty(plan.NRp, DG.agg_pitch(K), dtype=torch.float32, device=self.y.device)
            csr = graph.csr
            ops.segreduce(csr.rowptr, csr.col, self.x_src, F, t0.aggregators, (None,), n_tower=n_tower, out=agg, tower_stride_out=4 * F,
                          workspace=graph.workspace, tune=dict(generic=2, rows_per_group=DG.REST_ROWS_PER_GROUP), **gather)
            ops.pack_rows(own, plan.perm_all()[plan.NV:], out=agg[:, Ka:K])
            rest_scales = plan.rest_scales(tuple(t0.scalers) + (_avg_log_value(t0.avg_d),), self.scales)
            _contract_rest_rows(plan, agg[:, :K], K, weight, rest_scales, self.d, self.y, self.y.shape[1], row_post=self.post_r,
                                col_scale=self.ones, col_shift=self.c, leaky_slope=self.slope, residual=self.res)
        return self.y


class FusedTowerCall(_FusedTowerRows):
    """One PNALayer forward (one tower, or T towers with divide_input=True; eval) on the one-kernel path after the node-level projection, cut into its launches like
    FusedDegreeCall: `group_rows()` = pna_fused_degree_f32 in tower mode, `rest_rows()` = gather with the destination term + the
    rows' own features + three-block contraction over the compact list of the rows no degree group holds."""

    def __init__(self, layer, graph, h, snorm_n, x_cat):
        towers = list(layer.towers)
        Fi = len(towers) * towers[0].in_dim                  # (message features per edge, ALL towers -- see _tower_flat_weights)
        P = x_cat.shape[1] // 2
        super().__init__(layer, graph, h, snorm_n, [x_cat])
        self.Wv, self.d, self.c, self.ones, self.K = _tower_flat_weights(layer, towers, layer.mixing_network)
        self.Fe, self.x_src, self.x_dst = Fi, x_cat[:, :Fi], x_cat[:, P:P + Fi]
        a = self._block(self.Wv, Fi, self.x_src, self.Wv.shape[0], tower=True)
        a.x_dst, a.ld_xdst = _lib.dev_ptr(self.x_dst, torch.float32, "x_dst"), x_cat.stride(0)
        a.h_self, a.ld_h = _lib.dev_ptr(h, torch.float32, "h"), h.stride(0)
        self._tower_final(a)
        self._bind(0)

    def _rest_operands(self):
        items, orow, hout, hs = self.plan.rest_items_by_node(self.graph)
        gather = dict(tower_stride_in=self.Fe, dst_term=self.x_dst, heavy=hs, items=items, out_row_of=orow, heavy_out=hout)
        return self.Fe, 1, gather, _unit_stride(self.h), self.Wv


def _tower_pass_weights(layer, towers, mix):
    """The collapsed weight of a divide_input=False layer (_tower_collapsed_weights: scaler blocks [C_1,s | .. | C_T,s | h panel (block 0)])
    cut for FusedMultiTowerCall: per tower the weight of its statistics, (N, S * 4 Fi) in scaler blocks [mean | max | min | std] -- the
    layer-proper format --, and ONE dense weight for everything that is linear in the row's own features h_v:
        mean / max / min of (a_u + b_v) = those of a_u, + b_v;  b_v = W_b,t h_v + beta_t   (models/dgl/pna_layer.py:35-40: the pretrans Linear)
        =>  dst term = sum_s scale_s(D_v) [deg_v > 0] (M_s h_v + beta_s),   M_s = sum_t (C_t,s^mean + C_t,s^max + C_t,s^min) W_b,t,
                                                                            beta_s = sum_t (C_t,s^mean + C_t,s^max + C_t,s^min) beta_t
    and the self panel W_self h_v: (N, in_dim + S in_dim) = [W_self | M_0 | .. | M_S-1], the layout of functional.posttrans with h_self = agg = h.
    Formed in float64, rounded once.  Cached on the layer."""
    Wv, d, c, ones, K = _tower_collapsed_weights(layer, towers, mix, False)
    # Wd and beta read every tower's PRETRANS weight and bias, which the collapsed weight's key does not cover: keyed here beside Wv

    def build():
        T, Fi = len(towers), towers[0].in_dim
        S = Wv.shape[1] // K
        N = Wv.shape[0]
        Ws = []
        for t in range(T):
            W = torch.empty(N, S * 4 * Fi, dtype=torch.float32, device=Wv.device)
            for s_ in range(S):
                W[:, s_ * 4 * Fi:(s_ + 1) * 4 * Fi] = Wv[:, s_ * K + t * 4 * Fi:s_ * K + (t + 1) * 4 * Fi]
            Ws.append(W.contiguous())
        Wd = torch.zeros(N, (1 + S) * Fi, dtype=torch.float64, device=Wv.device)
        Wd[:, :Fi] = Wv[:, T * 4 * Fi:T * 4 * Fi + Fi].double()
        beta = torch.zeros(S, N, dtype=torch.float64, device=Wv.device)
        for t, tw in enumerate(towers):
            lin = tw.pretrans.fully_connected[0].linear
            Wb, bt = lin.weight[:, Fi:2 * Fi].double(), (lin.bias.double() if lin.bias is not None else torch.zeros(Fi, dtype=torch.float64, device=Wv.device))
            for s_ in range(S):
                Ct = Wv[:, s_ * K + t * 4 * Fi:s_ * K + (t + 1) * 4 * Fi].double()
                Wsum = Ct[:, :Fi] + Ct[:, Fi:2 * Fi] + Ct[:, 2 * Fi:3 * Fi]
                Wd[:, (1 + s_) * Fi:(2 + s_) * Fi] += Wsum @ Wb
                beta[s_] += Wsum @ bt
        # the rest rows (two-kernel path over their compact list): scaler blocks [the towers' aggregator columns | an N-column panel], the
        # panel the identity in block 0 (the identity scaler's) and zero elsewhere -- it carries the row's dense term, copied behind the
        # statistics of a_u in the aggregate buffer
        Ka = T * 4 * Fi
        Wr = torch.zeros(N, S * (Ka + N), dtype=torch.float32, device=Wv.device)
        for s_ in range(S):
            Wr[:, s_ * (Ka + N):s_ * (Ka + N) + Ka] = Wv[:, s_ * K:s_ * K + Ka]
        Wr[:, Ka:Ka + N] = torch.eye(N, dtype=torch.float32, device=Wv.device)
        return (Ws, Wd.float().contiguous(), beta.float().contiguous(), Wr.contiguous(), d, c, ones)
    return memo(layer, "_pna_amd_pass_w", [Wv] + _tower_tensors(towers, pre=True), None, build)


DENSE_TERM_RESIDENT = True          # FusedMultiTowerCall.dense_term through pna_project_scaled_f32 where it applies (False: contraction + rank-S update)


class FusedMultiTowerCall(_FusedTowerRows):
    """One PNALayer forward with T towers over the WHOLE input (divide_input=False; models/dgl/pna_layer.py:137-139; eval) on the one-kernel
    path (round 6).  Every tower has its own projection of the input -- T x Fi message features per edge -- and a wavefront
    cannot hold T x 80 running statistics: the layer is one dense launch over the rows' own features (everything linear in h_v: the
    destination terms of all towers and the self panel, _tower_pass_weights) and T launches of pna_fused_degree_f32 -- the LAYER-PROPER
    instantiation, no node panels --, launch t gathering tower t's Fi features out of the (V, T P) source projection and adding
    W_t a_t to the partial sums of the launches before it (pna_fused_degree_args.pre_add); the last one applies bias, graph norm, the
    collapsed BatchNorm / mixing constants, LeakyReLU and the residual.  The aggregates never reach HBM; what does is T x 2 x 4 N bytes per
    row of partial sums.  `rest_rows()`: the rows no degree group holds, all towers at once on the two-kernel path."""

    def __init__(self, layer, graph, h, snorm_n, x_src):
        towers = list(layer.towers)
        T, Fi, V, dev = len(towers), towers[0].in_dim, h.shape[0], h.device
        Ws, self.Wd, self.beta, self.Wr, self.d, self.c, self.ones = _tower_pass_weights(layer, towers, layer.mixing_network)
        super().__init__(layer, graph, h, snorm_n, [x_src, Ws])
        self.T, self.Fi, self.P, self.x_src = T, Fi, x_src.shape[1] // T, x_src
        N, P = Ws[0].shape[0], self.P
        # partial sums ping-pong between two buffers: a launch never writes the rows it reads -- the guard's second launch computes a
        # handed-over tile AGAIN from the same pre_add rows (in place it would add the tile's share twice: found by tools/fuzz_fused.py)
        self._part_full = torch.empty(V, out_pitch(N), dtype=torch.float32, device=dev)
        self.part = self._part_full[:, :N]
        self.part2 = torch.empty(V, out_pitch(N), dtype=torch.float32, device=dev)[:, :N] if T > 1 else None
        # beta padded to the buffer's pitch: the rank-S update runs in place on the whole buffer
        self.beta_pad = memo(layer, "_pna_amd_beta_pad", [self.beta], out_pitch(N),
                             lambda: torch.nn.functional.pad(self.beta, (0, out_pitch(N) - N)))
        # the scalers of the dense term: zero for rows without in-edges (DGL leaves their aggregate -- the destination term with it -- at zero)
        self.mscales, self.mscale_mat = self.plan.masked_scales(self.scales)
        for t in range(T):
            src_buf, dst_buf = (self.part, self.part2) if t % 2 == 0 else (self.part2, self.part)
            a = self._block(Ws[t], Fi, x_src[:, t * P:t * P + Fi], N, pre_add=src_buf)
            if t == T - 1:
                self._tower_final(a)
            else:
                self._partial(a, dst_buf, 0, N)
        self._bind(T - 1)

    def dense_term(self):
        """part = W_self h + sum_s scale_s [deg > 0] (M_s h + beta_s): one contraction launch over the rows' own features + a rank-S update."""
        h, Fi = _unit_stride(self.h), self.Fi
        if DENSE_TERM_RESIDENT and ops.project_scaled_applies(h, Fi, self.Wd.shape[0], 1 + len(self.mscales)):
            # every block of the weight resident in LDS, h read once, beta inside (0.66 -> 0.3 ms at 1 M rows: tools/multi_tower_time.py)
            return ops.project_scaled(h, Fi, self.Wd, self.mscale_mat, self.beta, True, out=self.part)
        ops.posttrans(h, Fi, self.Wd, self.mscales, None, h, out=self.part)
        torch.addmm(self._part_full, self.mscale_mat, self.beta_pad, out=self._part_full)   # (+= [deg > 0] scale_s beta_s; the padding columns stay unread)
        return self.part

    prologue = dense_term                                    # (what both halves read: run_fused_call launches it in front of the fork)

    def _rest_operands(self):
        # statistics of a_u alone, all towers (the destination term is in the dense term, like the group rows'); the dense term rides behind them
        items, hout, hs = self.plan.rest_items(self.graph)
        return self.Fi, self.T, dict(tower_stride_in=self.P, heavy=hs, items=items, heavy_out=hout), self.part, self.Wr


def tower_layer_degree_fused_multi(layer, graph, h, snorm_n, x_src):
    """PNALayer.forward (eval, T towers, divide_input=False) after the node-level SOURCE projection x_src = [W_a,0 h | .. | W_a,T-1 h]
    (blocks of tower_projection_pitch columns): FusedMultiTowerCall."""
    return run_fused_call(FusedMultiTowerCall(layer, graph, h, snorm_n, x_src))


def tower_layer_degree_fused(layer, graph, h, snorm_n, x_cat):
    """PNALayer.forward (eval, ONE tower; models/dgl/pna_layer.py:130-145 over :33-76) after the node-level projection
    x_cat = [x_src | x_dst] (halves of tower_projection_pitch columns): gather over x_src, the destination term, the row's own
    features, the collapsed posttrans . graph norm . BatchNorm . mixing weight, LeakyReLU and the residual in ONE kernel for the
    rows of the degree groups; the aggregate never reaches HBM."""
    return run_fused_call(FusedTowerCall(layer, graph, h, snorm_n, x_cat))


class FusedDegreeCall(_FusedCall):
    """One PNASimpleLayer forward on the one-kernel path, cut into its two halves so that bench.py can time them apart:
    `group_rows()` = pna_fused_degree_f32 (99.6 % of the benchmark graph's rows) -- one launch per output-column panel
    (degree_groups.fused_panels: one, unless the layer is wider than an instantiation) --, `rest_rows()` = gather + three-block
    contraction over the compact list of the rows no degree group holds.  Holds the argument blocks and every tensor they point into."""

    def __init__(self, layer, graph, h, x=None, out=None, agg_out=None, plan=None):
        from .dgl.pna_layer import _row_scales
        F, N, V = layer.in_dim, layer.out_dim, h.shape[0]
        self.x = x = graph.source_features(h) if x is None else x
        lin = layer.posttrans.fully_connected[0].linear
        # (rows at a 16-byte aligned pitch: the next layer of a stack can read them in 16-byte strips, i.e. stay on this path)
        y = torch.empty(V, out_pitch(N), dtype=torch.float32, device=h.device)[:, :N] if out is None else out
        super().__init__(layer, graph, DG.plan_of(graph) if plan is None else plan, h,      # (plan: a row block's)
                         _row_scales(graph, layer.scalers, layer.avg_d, h.device), y, [lin, agg_out, h])
        self.cs, self.ct, self.res = cs, ct, res = _layer_tail_operands(layer, h)
        aggs = tuple(layer.aggregators)
        panels = DG.fused_panels(F, N)
        if panels is None or not DG.aggregators_fusable(aggs):
            raise RuntimeError(f"pna_fused_degree: no instantiation for F={F}, N={N}, aggregators={aggs}")
        if agg_out is not None and (len(panels) != 1 or aggs != DG.STANDARD_AGGREGATORS):
            raise RuntimeError("pna_fused_degree: agg_out (verification) takes the four standard aggregators and a one-launch layer")
        whole = len(panels) == 1
        last_f0 = panels[-1][0]                               # (the feature panel whose launches apply the epilogue)
        self.part = None
        if any(f0 != last_f0 for f0, _, _, _ in panels):      # feature panels: partial sums between the launches
            self.part = torch.empty(V, out_pitch(N), dtype=torch.float32, device=h.device)[:, :N]
        for f0, f1, c0, c1 in panels:
            a = self._block(lin.weight, F, x[:, f0:f1], c1 - c0, pre_add=self.part[:, c0:c1] if f0 else None, verification=agg_out is not None,
                            rows=None if whole else (c0, c1), aggregators=aggs, feats=None if (f0, f1) == (0, F) else (f0, f1))
            sl = lambda t: None if t is None else t[c0:c1]      # noqa: E731  (a panel's slice of a per-column vector: still unit stride)
            if f0 == last_f0:
                self._final(a, y[:, c0:c1], sl(lin.bias), sl(cs), sl(ct), None if res is None else res[:, c0:c1], 1,
                            cols_writable=own_buffer_cols(y.stride(0), c0, c1, N) if out is None else 0)
            else:
                self._partial(a, self.part, c0, c1)
            if agg_out is not None:
                a.agg_out, a.ld_agg = _lib.dev_ptr(agg_out, torch.float32, "agg_out"), agg_out.stride(0)
        self._bind(0)

    def rest_rows(self):
        plan, layer, graph = self.plan, self.layer, self.graph
        if plan.NR:
            F = layer.in_dim
            K = 4 * F                                        # (the four standard statistics whatever the layer's list: _rest_posttrans)
            Kb = 5 * F if "sum" in layer.aggregators else K  # (+ room for the sum block)
            items, hout, hs = plan.rest_items(graph)
            agg = torch.empty(plan.NRp, DG.agg_pitch(Kb), dtype=torch.float32, device=self.y.device)[:, :Kb]
            csr = graph.csr
            ops.segreduce(csr.rowptr, csr.col, _unit_stride(self.x), F, DG.STANDARD_AGGREGATORS, (None,), tower_stride_in=F, out=agg[:, :K],
                          heavy=hs, workspace=graph.workspace, items=items, heavy_out=hout,
                          tune=dict(generic=2, rows_per_group=DG.REST_ROWS_PER_GROUP))
            _rest_posttrans(layer, graph, agg, plan, self.scales, self.y, self.cs, self.ct, self.res)
        return self.y


def simple_layer_degree_fused(layer, graph, h, x=None, out=None, agg_out=None):
    """PNASimpleLayer.forward (eval) with the group rows in ONE kernel (pna_fused_degree_f32): gather, the four
    aggregators, the combined scaler block W_D and the posttrans contraction with its BatchNorm / ReLU / residual epilogue; the
    4F aggregate of those rows never reaches HBM.  The rows no degree group holds (rare degrees, hub rows: 0.4 % of the benchmark
    graph's rows, 5 % of its edges) take the two-kernel path over their compact list.  `x`: the source table (halo in place on
    a sharded graph); `agg_out` (verification): (plan.NV, >= 4F) receives the statistics the contraction consumed."""
    src = graph.source_features(h) if x is None else x
    return run_fused_call(FusedDegreeCall(layer, graph, h, x=src, out=out, agg_out=agg_out))


def simple_layer_degree_grouped(layer, graph, h):
    """PNASimpleLayer.forward (eval) with the rows grouped by in-degree (pna_amd/degree_groups.py): the gather writes the
    aggregate in degree order, the contraction multiplies every tile by its degree's combined weight W_D = sum_s s_s(D) W_s
    (one scaler block instead of three), the rows of rare degrees and the hub rows take the ordinary three-block contraction
    over a compacted list."""
    plan = DG.plan_of(graph)
    from .graph import Graph
    aggs = tuple(layer.aggregators)
    if type(graph) is Graph and DG.fused_applies(graph, h, layer.in_dim, layer.out_dim, aggs):
        return simple_layer_degree_fused(layer, graph, h, x=h)
    # A shard (HaloGraph).  The two-kernel path cuts its gather into the rows that read only local sources -- aggregated while
    # the halo exchange is in flight -- and the rest; the one-kernel path needs the whole [local | halo] table first.  Which one
    # pays depends on how many rows the overlap covers: on a graph without locality (the benchmark graph: 1 % interior rows) the
    # overlap hides next to nothing and the one-kernel layer saves a third of the compute, so: exchange, then ONE kernel over the
    # extended table (features in the shard's resident table at a 16-byte aligned pitch); with many interior rows, the overlap.
    two = DG.two_kernel_applies(layer.out_dim, len(layer.scalers), aggs)
    if (isinstance(graph, HaloGraph) and DG.FUSED and graph._resident(h) and graph._pending is None
            and (graph.interior_fraction() < DG.FUSED_HALO_MAX_INTERIOR or not two)):
        x_ext = graph._ext[:, : h.shape[1]]
        if DG.fused_applies(graph, x_ext, layer.in_dim, layer.out_dim, aggs):
            return simple_layer_degree_fused(layer, graph, h, x=graph.source_features(h))
    if not two:
        # (an operator set / width only the one-kernel layer serves, and it does not apply to this call: PNASimpleLayer.forward
        # catches this and takes the ordinary path)
        raise RuntimeError("pna_amd: the hand-scheduled kernel was required (one-kernel layer) but does not apply to this call")
    return degree_grouped_posttrans(layer, graph, h, degree_grouped_aggregate(layer, graph, h, plan), plan)


class _SmallSimplePlan(_SmallTowerPlan):
    """PNASimpleLayer (models/dgl/pna_layer.py:197-216, eval mode) on the same one-call kernel: a tower layer with ONE tower,
    the identity as pretrans (messages are the raw source features: x_cat = [I ; 0] h), no self panel in the posttrans
    (W_h = 0), and the identity as mixing network with the layer's ReLU and residual in its epilogue.  Products with 1 and sums
    with 0 are exact: the result is the three-kernel path's up to the summation order of the contraction.  One difference for
    NON-FINITE inputs: since round 4 the kernel multiplies ZEROS (not h) with the zero self block (`no_self_panel`), so a
    node whose own feature is Inf / NaN keeps the finite output the reference and the three-kernel path give it."""

    def __init__(self, layer):
        lin = layer.posttrans.fully_connected[0].linear
        bn = layer.batchnorm_h if layer.batch_norm else None
        if bn is not None and bn.training:
            raise RuntimeError("only an eval-mode BatchNorm (running statistics) can be folded into the epilogue")
        self.ts = [lin.weight, lin.bias] + (_bn_tensors(bn) if bn is not None else [])
        self.versions = tensor_key(self.ts)
        Fi, Fo, S = layer.in_dim, layer.out_dim, len(layer.scalers)
        self.T, self.Fi, self.Fo, self.S, self.divide_input = 1, Fi, Fo, S, False
        dev = lin.weight.device
        with torch.no_grad():
            eye = torch.eye(Fi, device=dev)
            w_ext = torch.cat([torch.zeros(Fo, Fi, device=dev), lin.weight], dim=1).contiguous()      # [h panel = 0 | scaler blocks]
            keep = dict(proj_img=ops.pack_small(torch.cat([eye, torch.zeros_like(eye)], dim=0).contiguous()),
                        proj_bias=torch.zeros(2 * Fi, device=dev),
                        post_img=ops.pack_tower_post([w_ext], Fi, Fo, S),
                        post_bias=lin.bias.detach().contiguous() if lin.bias is not None else None,
                        mix_img=ops.pack_small(torch.eye(Fo, device=dev)), mix_bias=None)
            if bn is not None:
                keep["col_scale"], keep["col_shift"] = (x.contiguous() for x in _fold_batchnorm(bn))
        self.keep, self.device, self.width, self.xw, self.graph_norm = keep, dev, Fo, 2 * Fi, False
        a = _lib.PnaTowerLayerArgs()
        a.n_tower, a.Fi, a.Fo, a.divide_input, a.n_scaler = 1, Fi, Fo, 0, S
        for k, v in keep.items():
            if v is not None:
                setattr(a, k, _lib.dev_ptr(v, torch.float32, k))
        a.No, a.mix_act = Fo, 1                                # ReLU (pna_layer.py:211)
        a.no_self_panel = 1                                    # (zeros, not h, against the zero self block: Inf / NaN own features stay out)
        self.args, self.ref = a, ctypes.byref(a)
        self.fn = _lib.lib().pna_tower_layer_f32
        self.check, self.stream_ptr = _lib.check, _lib.stream_ptr


SMALL_SIMPLE_ROWS = int(os.environ.get("PNA_AMD_SMALL_SIMPLE_ROWS", "4096"))   # PNASimpleLayer batches up to this many nodes (measured
# crossover with the three-kernel path at hidden 80: 0.026 vs 0.048 ms at 1.6-3 k nodes, equal at 6.4 k, 0.087 vs 0.056 at 13 k:
# profiles/r02_small_simple_layer.json)


# PNASimpleLayer TRAINING batches up to this many nodes take the one-call route (autograd.SimpleLayerSmallTrainFn:
# pna_simple_train_fwd_f32 / _bwd_f32).  0 = off (the default: the crossover with the generic route is in DESIGN.md 4.16)
SMALL_TRAIN_ROWS = int(os.environ.get("PNA_AMD_SMALL_TRAIN_ROWS", "0"))


def small_train_fits(F, N):
    """Whether the widths are inside pna_simple_train_*_f32's scope, by the library's own check."""
    # (the workspace query takes the whole shape: asked at the smallest batch of the scope, two rows without edges and one scaler)
    return _lib.lib().pna_simple_train_workspace_bytes(2, 0, F, N, 1) >= 0


# PNALayer TRAINING batches up to this many nodes take the one-call route (autograd.TowerLayerSmallTrainFn:
# pna_tower_train_fwd_f32 / _bwd_f32).  0 = off, the default
SMALL_TOWER_TRAIN_ROWS = int(os.environ.get("PNA_AMD_SMALL_TOWER_TRAIN_ROWS", "0"))


def small_tower_train_fits(T, Fi, Fo, S=3):
    """Whether towers, widths and scalers are inside pna_tower_train_*_f32's scope, by the library's own check."""
    # (the workspace query takes the whole shape: asked at the smallest batch of the scope, two rows without edges)
    return _lib.lib().pna_tower_train_workspace_bytes(2, 0, T, Fi, Fo, S, 0) >= 0


# PNALayer TRAINING batches WITH EDGE FEATURES up to this many nodes take the one-call route (autograd.TowerLayerEdgeSmallTrainFn:
# pna_tower_edge_train_fwd_f32 / _bwd_f32).  A knob of its own: SMALL_TOWER_TRAIN_ROWS keeps its meaning.  0 = off, the default
# 
SMALL_TOWER_TRAIN_EDGE_ROWS = int(os.environ.get("PNA_AMD_SMALL_TOWER_TRAIN_EDGE_ROWS", "0"))


def small_tower_train_edge_fits(T, Fi, Fo, S=3, edge_dim=0):
    """Whether towers, widths, scalers and edge_dim are inside pna_tower_edge_train_*_f32's scope, by the library's own check."""
    # (the workspace query takes the whole shape: asked at the smallest batch of the scope, two rows without edges)
    return _lib.lib().pna_tower_edge_train_workspace_bytes(2, 0, T, Fi, Fo, S, 0, edge_dim) >= 0


# PNALayer TRAINING batches whose towers have DROPOUT (0 < p < 1), with or without edge features, up to this many nodes take the
# one-call route (autograd.TowerLayerDropSmallTrainFn: pna_tower_drop_train_fwd_f32 / _bwd_f32).  A knob of its own: the two above keep
# their meaning and never serve such a layer.  0 = off, the default
SMALL_TOWER_TRAIN_DROPOUT_ROWS = int(os.environ.get("PNA_AMD_SMALL_TOWER_TRAIN_DROPOUT_ROWS", "0"))


# PNALayer TRAINING batches whose towers aggregate with ANY 1-4 distinct aggregators out of mean sum max min std var -- except the list
# mean max min std in that order, which the three knobs above serve -- up to this many nodes take the one-call route
# (autograd.TowerLayerAggrSmallTrainFn: pna_tower_aggr_train_fwd_f32 / _bwd_f32), with or without edge features and tower dropout.  A knob
# of its own: the three above keep their meaning and their scope.  0 = off, the default
SMALL_TOWER_TRAIN_AGGR_ROWS = int(os.environ.get("PNA_AMD_SMALL_TOWER_TRAIN_AGGR_ROWS", "0"))

TOWER_TRAIN_AGGREGATORS = ("mean", "sum", "max", "min", "std", "var")

# pytorch_geometric.PNAConv calls (fp32, training or not) on batches up to this many nodes take the one-call route (autograd.PygConvFn:
# pna_pyg_conv_train_fwd_f32 / _bwd_f32 -- the tower training kernels without BatchNorm and with the PyG statistics).  0 = off, the
# default
PYG_TRAIN_ROWS = int(os.environ.get("PNA_AMD_PYG_TRAIN_ROWS", "0"))


def pyg_conv_train_fits(T, Fi, Fo, S, edge_dim, codes):
    """Whether towers, widths, scalers, edge_dim (0 = no edge features) and the list of aggregator codes are inside
    pna_pyg_conv_train_*_f32's scope, by the library's own check."""
    # (the workspace query takes the whole shape: asked at the smallest batch of the scope, two rows without edges)
    arr = (ctypes.c_int32 * max(len(codes), 1))(*[int(c) for c in codes])
    return _lib.lib().pna_pyg_conv_train_workspace_bytes(2, 0, T, Fi, Fo, S, 0, edge_dim, len(codes), arr) >= 0


def small_tower_aggr_train_fits(T, Fi, Fo, S, edge_dim, codes):
    """Whether towers, widths, scalers, edge_dim (0 = no edge features) and the list of aggregator codes are inside
    pna_tower_aggr_train_*_f32's scope, by the library's own check."""
    # (the workspace query takes the whole shape: asked at the smallest batch of the scope, two rows without edges)
    codes = [int(c) for c in codes]
    if not all(-2 ** 31 <= c < 2 ** 31 for c in codes):
        return False
    arr = (ctypes.c_int32 * max(len(codes), 1))(*codes)
    return _lib.lib().pna_tower_aggr_train_workspace_bytes(2, 0, T, Fi, Fo, S, 0, edge_dim, len(codes), arr) >= 0


def tower_dropout_key(device, n):
    """(seed, offset) of one dropout mask over n elements, taken from the device's default torch generator, which then moves past the
    4 ceil(n / 4) words the mask may use: torch.manual_seed makes a run reproducible and torch's own random ops behind the call draw
    from fresh counters.  Host state only: no synchronisation."""
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[index]
    seed, offset = int(gen.initial_seed()), int(gen.get_offset())
    gen.set_offset(offset + 4 * ((int(n) + 3) // 4))
    return seed, offset


def dropout_mask(V, C, p, seed, offset, device):
    """The (V, C) fp32 factors of the mask rule of include/pna_amd.h (pna_dropout_mask_f32): 0 for a dropped element, 1 / (1 - p) for a
    kept one -- what pna_tower_drop_train_*_f32 apply to the towers' concatenated BatchNorm output under the key (seed, offset)."""
    out = torch.empty(int(V), int(C), dtype=torch.float32, device=device)
    _lib.check(_lib.lib().pna_dropout_mask_f32(out.data_ptr(), out.stride(0) if V else int(C), int(V), int(C), float(p), int(seed) & (2 ** 64 - 1),
                                               int(offset) & (2 ** 64 - 1), _lib.stream_ptr(out.device)), "pna_dropout_mask_f32")
    return out


# The two ENDS of the molecule nets -- the sum of embedding tables (AtomEncoderStandIn, nets.embed) and the per-graph readout
# (nets.readout_nodes) -- take the one-call route (autograd.EmbedSumFn / ReadoutFn: pna_embed_sum_*_f32, pna_readout_*_f32) on calls of up
# to this many rows.  0 = off, the default
NET_ENDS_ROWS = int(os.environ.get("PNA_AMD_NET_ENDS_ROWS", "0"))


def embed_sum_workspace_bytes(V, rows, F):
    """pna_embed_sum_workspace_bytes: the backward's bytes for V index rows over tables of `rows` rows each; -1 outside the scope."""
    return _lib.lib().pna_embed_sum_workspace_bytes(V, len(rows), (ctypes.c_int32 * len(rows))(*rows), F)


def embed_sum_fits(rows, F):
    """Whether the tables and the width are inside pna_embed_sum_*_f32's scope, by the library's own check."""
    # (the workspace query takes the whole shape: asked at the smallest call of the scope, one index row; the last shape's answer is
    # kept, one memo entry on this function: the encoder's whole step can be 120 us and asks on every call)
    shape = (tuple(rows), F)
    return memo(embed_sum_fits, "_pna_amd_answer", (), shape, lambda: embed_sum_workspace_bytes(1, rows, F)) >= 0


# The GRU update between two message-passing steps (nets.GRU, layers.GRU: nn.GRU over a length-1 sequence) takes the one-call route
# (autograd.GruCellFn: pna_gru_cell_fwd_f32 / _bwd_f32) on calls of 2 .. this many rows.  0 = off, the default
GRU_ROWS = int(os.environ.get("PNA_AMD_GRU_ROWS", "0"))


def gru_cell_fits(I, Hc, input_size, hidden_size):
    """Whether the widths are inside pna_gru_cell_*_f32's scope, by the entry points' own check (pna_gru_cell_in_scope)."""
    # (the check takes the whole shape: asked at the smallest call of the scope, two rows)
    return bool(_lib.lib().pna_gru_cell_in_scope(2, I, Hc, input_size, hidden_size))


def gru_cell_workspace_bytes(V, I, Hc, hidden_size):
    """pna_gru_cell_workspace_bytes: the backward's bytes (dgi / dgh and one image of the parameter gradients per slab); -1 outside the
    scope."""
    return _lib.lib().pna_gru_cell_workspace_bytes(V, I, Hc, hidden_size)


# The dense heads (nets.MLPReadout, layers.MLP without dropout and batch-norm, the superpixel net's Linear embeddings) take the one-call
# route (autograd.MlpHeadFn: pna_mlp_head_fwd_f32 / _bwd_f32) on calls of up to this many rows.  0 = off, the default
MLP_HEAD_ROWS = int(os.environ.get("PNA_AMD_MLP_HEAD_ROWS", "0"))


def _mlp_head_ints(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def mlp_head_act(act):
    """(PNA_MLP_ACT_* code, slope) of a layer's activation -- None, nn.ReLU or nn.LeakyReLU (exact types) -- else None."""
    if act is None:
        return _lib.PNA_MLP_ACT_NONE, 0.0
    if type(act) is torch.nn.ReLU:
        return _lib.PNA_MLP_ACT_RELU, 0.0
    if type(act) is torch.nn.LeakyReLU:
        return _lib.PNA_MLP_ACT_LEAKY, float(act.negative_slope)
    return None


def mlp_head_path(x, linears, acts):
    """Whether the head `linears` with the activation modules `acts` on x is served by pna_mlp_head_fwd_f32 / _bwd_f32 (autograd.MlpHeadFn:
    one C call each way, train and eval, with and without grad): the knob PNA_AMD_MLP_HEAD_ROWS is on and covers the rows; x is fp32 on a
    GPU, 2-D with unit column stride and a row pitch of at least the width, or 3-D contiguous (taken as its (B N, D) view); every layer
    is a plain nn.Linear whose parameters are fp32 on that GPU and whose input is the layer before's output; every activation is None,
    nn.ReLU or nn.LeakyReLU; the shape fits the call (mlp_head_fits).  No float is read."""
    if not MLP_HEAD_ROWS > 0:
        return False
    if not (x.is_cuda and x.dtype == torch.float32):
        return False
    if x.dim() == 3:
        if not x.is_contiguous():
            return False
        V, D = x.shape[0] * x.shape[1], x.shape[2]
    elif x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1]:
        V, D = x.shape
    else:
        return False
    if not (1 <= V <= MLP_HEAD_ROWS and 1 <= len(linears) == len(acts)):
        return False
    widths, codes = [D], []
    for lin, act in zip(linears, acts):
        if type(lin) is not torch.nn.Linear or lin.in_features != widths[-1]:
            return False
        for p in (lin.weight, lin.bias):
            if p is not None and not (p.is_cuda and p.dtype == torch.float32 and p.device == x.device):
                return False
        code = mlp_head_act(act)
        if code is None:
            return False
        widths.append(lin.out_features)
        codes.append(code[0])
    return mlp_head_fits(widths, codes)


def mlp_head_fits(widths, acts):
    """Whether a head of len(acts) layers with these widths (the input's first) and activation codes (_lib.PNA_MLP_ACT_*) is inside
    pna_mlp_head_*_f32's scope, by the entry points' own check (pna_mlp_head_in_scope)."""
    # (the check takes the whole shape: asked at the smallest call of the scope, one row)
    if len(widths) != len(acts) + 1:
        return False
    return bool(_lib.lib().pna_mlp_head_in_scope(1, len(acts), _mlp_head_ints(widths), _mlp_head_ints(acts)))


def mlp_head_workspace_bytes(V, widths):
    """pna_mlp_head_workspace_bytes: the backward's bytes (the hidden rows, the layers' cotangents and one image of the parameter
    gradients per slab); -1 outside the scope."""
    return _lib.lib().pna_mlp_head_workspace_bytes(V, len(widths) - 1, _mlp_head_ints(widths))


# The dense-adjacency PNALayer (pna_amd.pytorch.pna.layer.PNALayer: the multitask GNN's convolution) takes the one-call route
# (autograd.DenseLayerFn: pna_dense_layer_fwd_f32 / _bwd_f32) on calls of up to this many rows B N.  0 = off, the default
DENSE_LAYER_ROWS = int(os.environ.get("PNA_AMD_DENSE_LAYER_ROWS", "0"))
DENSE_LAYER_AGGREGATORS = ("mean", "max", "min", "std")


def dense_layer_lds_bytes(N, T, Fi, Fo, A, S):
    """pna_dense_layer_lds_bytes: the LDS bytes of one graph's workgroup; -1 where the widths are outside the scope."""
    return _lib.lib().pna_dense_layer_lds_bytes(N, T, Fi, Fo, A, S)


def dense_layer_workspace_bytes(B, N, T, Fi, Fo, A, S):
    """pna_dense_layer_workspace_bytes: the backward's bytes (images of every parameter gradient); -1 outside the scope."""
    return _lib.lib().pna_dense_layer_workspace_bytes(B, N, T, Fi, Fo, A, S)


def dense_layer_fits(N, T, Fi, Fo, A, S):
    """Whether one graph's shapes are inside pna_dense_layer_*_f32's scope (the widths, and the graph inside a workgroup's LDS), by the
    library's own check."""
    # (the workspace query takes the whole shape: asked at the smallest batch of the scope, one graph)
    return dense_layer_workspace_bytes(1, N, T, Fi, Fo, A, S) > 0


# The Set2Set graph readout (layers.Set2Set: the multitask GNN's graph head) takes the one-call route (autograd.Set2SetFn:
# pna_set2set_fwd_f32 / _bwd_f32) on calls of up to this many rows B N.  0 = off, the default
S2S_ROWS = int(os.environ.get("PNA_AMD_S2S_ROWS", "0"))


def set2set_lds_bytes(N, D):
    """pna_set2set_lds_bytes: the LDS bytes of the backward's workgroup; -1 where N or D is outside the scope."""
    return _lib.lib().pna_set2set_lds_bytes(N, D)


def set2set_workspace_bytes(B, N, D, steps):
    """pna_set2set_workspace_bytes: the backward's bytes (images of the parameter gradients and the steps' records); -1 outside the
    scope."""
    return _lib.lib().pna_set2set_workspace_bytes(B, N, D, steps)


def set2set_fits(N, D, steps):
    """Whether one graph's shapes and the step count are inside pna_set2set_*_f32's scope, by the library's own check."""
    # (the workspace query takes the whole shape: asked at the smallest batch of the scope, one graph)
    return set2set_workspace_bytes(1, N, D, steps) > 0


def simple_layer_small(layer, graph, h, row_scales):
    """PNASimpleLayer.forward (eval) through pna_tower_layer_f32; the plan is cached on the layer."""
    plan = layer.__dict__.get("_pna_amd_small")
    if plan is None or plan.stale():
        plan = _SmallSimplePlan(layer)
        layer.__dict__["_pna_amd_small"] = plan
    return plan.run(graph, h, None, row_scales, layer.residual)


def tower_layer_small(owner, towers, mix, graph, h, snorm_n, row_scales, divide_input, residual, etab=None):
    """models/dgl/pna_layer.py:133-148 in eval mode through pna_tower_layer_f32.  `mix`: the mixing FCLayer (Linear + LeakyReLU /
    ReLU / none, no batch-norm) or None.  The plan is cached on `owner` (dropped by PNALayer._apply on device / dtype moves)."""
    plan = owner.__dict__.get("_pna_amd_small")
    if plan is None or plan.divide_input != divide_input or plan.stale():
        plan = _SmallTowerPlan(towers, mix, divide_input)
        owner.__dict__["_pna_amd_small"] = plan
    return plan.run(graph, h, snorm_n, row_scales, residual, etab)


class SimpleLayerRows:
    """layer_rows callback of shard.BlockPipeline for a stack of PNASimpleLayer (eval): rows [r0, r1) of layer l from the complete
    [local | halo] table into the next table -- the gather over the block's work list (hub rows ride with block 0: their
    finalize writes wherever they live) and the three-block contraction over the block's slice of the aggregate.  Every row is
    computed by the same kernels in the same order as on one GPU: bit-identical to the unsharded ordinary path."""

    wants_full_out = True          # BlockPipeline hands __call__ the whole next table (the one-kernel layer scatters rows by node id)

    def __init__(self, layers, graph, n_blocks, fused=None):
        self.layers, self.g = list(layers), graph
        l0 = self.layers[0]
        self.F = l0.in_dim
        self.fused = DG.FUSED if fused is None else bool(fused)
        self.n_blocks, self._plans, self._calls = int(n_blocks), {}, {}
        if any(l.in_dim != self.F or l.out_dim != self.F or tuple(l.aggregators) != ("mean", "max", "min", "std") or l.training for l in self.layers):
            raise ValueError("SimpleLayerRows: a stack of eval-mode PNASimpleLayer(F -> F) with the four standard aggregators")
        V = graph.num_nodes
        self.agg = torch.empty(V, DG.agg_pitch(4 * self.F), dtype=torch.float32, device=graph.device)
        hs = graph.heavy_schedule()
        deg = graph.csr.rowptr[1:] - graph.csr.rowptr[:-1]
        light = (deg <= hs.threshold) if hs.threshold > 0 else torch.ones_like(deg, dtype=torch.bool)
        rows = torch.arange(V, device=graph.device)
        self.items = []
        for b in range(n_blocks):
            r0, r1 = (V * b) // n_blocks, (V * (b + 1)) // n_blocks
            self.items.append(graph.work_items_subset(light & (rows >= r0) & (rows < r1), include_heavy=(b == 0)))
        self.hs = hs

    def block_plan(self, b, r0, r1):
        """The degree plan of row block b, or None when the blocks do not qualify for the one-kernel layer (a block without a
        degree value that fills a tile, mostly leftover rows).  Blocks 1.. hold only the rows of their range whose degree fills
        tiles INSIDE the block (one launch each); block 0 takes, besides its own rows, the hub rows and every block's leftovers
        (its chain of small rest-row launches runs once per layer, first: a row may be ready earlier than its block, never later)."""
        if not self._plans:
            V, B = self.g.num_nodes, self.n_blocks
            bounds = [(V * i) // B for i in range(B + 1)]
            plans, left = {}, []
            for i in range(1, B):
                plans[i] = DG.DegreePlan(self.g, row_range=(bounds[i], bounds[i + 1]), with_heavy=False, drop_rest=True)
                left.append(plans[i].dropped_rest)
            plans[0] = DG.DegreePlan(self.g, row_range=(bounds[0], bounds[1]), with_heavy=True, extra_rows=torch.cat(left) if left else None)
            ok = (all(p.G > 0 and p.fused_tables() is not False for p in plans.values())
                  and plans[0].NR <= DG.MAX_REST_FRACTION * max(1, V // B))
            self._plans = plans if ok else {i: None for i in range(B)}
        return self._plans[b]

    def __call__(self, l, table, r0, r1, out, b):
        from .dgl.pna_layer import _row_scales
        layer, g, F = self.layers[l], self.g, self.F
        csr = g.csr
        K = 4 * F
        x = table[:, :F]
        n_local = g.num_nodes
        full = out.shape[0] == table.shape[0]                 # (BlockPipeline: the whole next table; older callers: its rows [r0, r1))
        if self.fused and full and r1 > r0 and table.is_cuda and len(layer.scalers) == 3 and DG.fused_shape_ok(x, F, layer.out_dim):
            plan = self.block_plan(b, r0, r1)
            if plan is not None:
                # the block through the one-kernel layer: its own degree groups (pna_fused_degree_f32) + its rest rows; rows are
                # scattered to their node ids in the next table (1.47 -> ~0.85 ms / layer of compute at C3 shape)
                # the cached call snapshots the packed weight images and the folded BatchNorm scale / shift: the parameters' (version,
                # address) belong in the key, or an optimizer step / load_state_dict between two runs leaves the group rows on stale
                # weights while the rest rows read the live ones
                key = (l, b, table.data_ptr(), out.data_ptr()) + _simple_layer_state(layer)
                call = self._calls.get(key)
                if call is None:
                    if len(self._calls) > 4 * len(self.layers) * self.n_blocks:
                        self._calls.clear()
                    call = self._calls[key] = FusedDegreeCall(layer, g, table[:n_local, :F], x=x, out=out[:n_local, :layer.out_dim], plan=plan)
                run_fused_call(call)
                return
        if full:
            out = out[r0:r1]
        items = self.items[b]
        if items.shape[0]:
            ops.segreduce(csr.rowptr, csr.col, x, F, layer.aggregators, (None,), tower_stride_in=F, out=self.agg,
                          heavy=self.hs if b == 0 else None, workspace=g.workspace, items=items, tune=dict(generic=2))
        if r1 > r0:
            lin = layer.posttrans.fully_connected[0].linear
            scales = _row_scales(g, layer.scalers, layer.avg_d, table.device)
            cs, ct, _ = _layer_tail_operands(layer, x)
            ops.posttrans(self.agg[r0:r1, :K], K, lin.weight, [None if r is None else r[r0:r1] for r in scales], lin.bias, out=out[:, :layer.out_dim],
                          col_scale=cs, col_shift=ct, relu=True, residual=x[r0:r1] if layer.residual else None)


def _shard_gather_bf16(graph, x, F, aggregators, bs, **terms):
    """The bf16 aggregate of a shard's local rows from the local source rows x (n_local, >= F; any pitch) and the halo rows of the
    peers: HaloGraph.start_halo posts the exchange of x's rows, pna_gather_rows_bf16 reduces the interior rows (local sources only,
    no hub) while it is in flight and, after finish_exchange(), the boundary rows and the hub segments into the same aggregate,
    reading the halo rows from the receive buffer (no concatenated table).  `terms`: dst_term / edge_rows / edge_type of
    ops.gather_rows_bf16.  Every row is reduced by one lane group (or the heavy schedule) in its edge order: the bits of the
    unsharded ops.segreduce_bf16 / ops.gather_bf16."""
    csr, n = graph.csr, graph.num_nodes
    A = len(aggregators)
    width = A * bs if bs % 8 == 0 else (A - 1) * bs + F
    agg = torch.empty(n, (width + 7) // 8 * 8, dtype=torch.bfloat16, device=x.device)[:, :width]
    interior, boundary = graph.split_rows()
    halo = graph.start_halo(x, F)
    if not graph.any_exchange or graph.n_halo == 0:
        halo = None                               # no rank exchanges, or this rank reads local rows only
    common = dict(block_stride=bs, out=agg, **terms)
    if interior.numel():
        ops.gather_rows_bf16(csr.rowptr, csr.col, x, F, aggregators, rows=interior, **common)
    graph.finish_exchange()
    # (run also with an empty boundary list: the hub rows belong to this call)
    ops.gather_rows_bf16(csr.rowptr, csr.col, x, F, aggregators, rows=boundary, x_halo=halo, n_local=n,
                         heavy=graph.heavy_schedule(), workspace=graph.workspace, **common)
    return agg


def simple_layer_bf16(layer, graph, h):
    """PNASimpleLayer.forward (models/dgl/pna_layer.py:197-216) in inference on bf16 features and parameters: the bf16 aggregate of
    pna_segreduce_fwd_bf16 (blocks round8(F) columns apart, fp32 statistics), then pna_posttrans_bf16 with the degree scalers,
    bias, folded BatchNorm, ReLU and residual in its epilogue.  A deeper posttrans MLP runs its first Linear on the kernel (no
    epilogue) and the rest -- its later layers, BatchNorm, ReLU, residual -- as the module's own bf16 torch ops."""
    from .dgl.pna_layer import _row_scales
    F = layer.in_dim
    if h.dim() != 2 or h.shape[1] != F:
        raise ValueError(f"expected features of shape (V, {F}), got {tuple(h.shape)}")
    if h.stride(-1) != 1:
        h = h.contiguous()
    A = len(layer.aggregators)
    Fb = (F + 7) // 8 * 8
    csr = graph.csr
    sharded = isinstance(graph, HaloGraph)
    if not sharded and (not layer.residual or F == layer.out_dim) and bf16_small_applies(
            graph, h.shape[0], T=1, Fi=F, Fo=layer.out_dim, A=A, divide_input=False, posttrans_affine=layer.posttrans.is_affine,
            no_self_panel=True):
        im = _small_simple_images_bf16(layer)
        return ops.tower_layer_bf16(csr.rowptr, csr.col, h, n_tower=1, Fi=F, Fo=layer.out_dim, divide_input=False,
                                    aggregators=layer.aggregators, row_scales=_row_scales(graph, layer.scalers, layer.avg_d, h.device),
                                    post_img=im["post"], post_bias=im["post_bias"], col_scale=im["cs"], col_shift=im["ct"], slope=0.0,
                                    residual=h if layer.residual else None, no_self_panel=True)
    if sharded:
        agg = _shard_gather_bf16(graph, h, F, layer.aggregators, Fb)
    else:
        agg = ops.segreduce_bf16(csr.rowptr, csr.col, h, F, layer.aggregators, block_stride=Fb, heavy=graph.heavy_schedule(),
                                 workspace=graph.workspace)
    scales = _row_scales(graph, layer.scalers, layer.avg_d, h.device)
    lin = layer.posttrans.fully_connected[0].linear
    w_img = ops.pack_posttrans_weight_bf16(lin.weight, len(scales), A, F, Fb)
    if layer.posttrans.is_affine:
        if layer.residual and h.shape[1] != layer.out_dim:
            raise RuntimeError(f"The size of tensor a ({h.shape[1]}) must match the size of tensor b "
                               f"({layer.out_dim}) at non-singleton dimension 1")   # same failure as the reference (:213)
        cs = ct = None
        if layer.batch_norm:
            cs, ct = _fold_batchnorm_f32(layer.batchnorm_h)
        return ops.posttrans_bf16(agg, A * Fb, w_img, lin.out_features, scales, lin.bias, epilogue=True, relu=True,
                                  col_scale=cs, col_shift=ct, residual=h if layer.residual else None)
    y = ops.posttrans_bf16(agg, A * Fb, w_img, lin.out_features, scales, lin.bias)
    y = layer.posttrans.tail(y)
    if layer.batch_norm:
        y = layer.batchnorm_h(y)
    y = torch.relu(y)
    if layer.residual:
        y = h + y
    return y


def _build_tower_images_bf16(pre, post, Fi, ed, scalers, A, divide_input, bns, dst_first=False, tower_pitch=None):
    """The images of _tower_images_bf16 from the towers' first pretrans (`pre`) and posttrans (`post`) Linear modules.  ed: columns
    of the edge part of a pretrans weight (0: none).  dst_first: the pretrans weight's columns are [destination | source | edge]
    (the PyG order of PNAConv.pre_nns) rather than [source | destination | edge] (the DGL order).  tower_pitch: columns between the
    towers' blocks in x_src / x_dst / the edge rows / every aggregator block (default Fi: packed; round8(Fi): the per-tower padded
    layout pna_edge_mlp_bf16 reads and writes), P = round8(T tower_pitch)."""
    T, No, S = len(pre), post[0].out_features, len(scalers)
    Fs = Fi if tower_pitch is None else tower_pitch
    P = (T * Fs + 7) // 8 * 8
    Kin = T * Fi if divide_input else Fi
    dev, bf = pre[0].weight.device, torch.bfloat16
    cs, cd = (slice(Fi, 2 * Fi), slice(0, Fi)) if dst_first else (slice(0, Fi), slice(Fi, 2 * Fi))
    perm = sorted(range(S), key=lambda s: scalers[s] != "identity")           # stable: an identity scaler first
    proj = torch.zeros(1, 2 * P, Kin, dtype=bf, device=dev)
    pbias = torch.zeros(2 * P, dtype=bf, device=dev)
    edge = torch.zeros(1, P, max(ed, 1), dtype=bf, device=dev)
    wpost = torch.zeros(S, T * No, A * P, dtype=bf, device=dev)
    wself = torch.zeros(1, T * No, Kin, dtype=bf, device=dev)
    for t in range(T):
        r = slice(t * Fs, t * Fs + Fi)
        c = slice(t * Fi, (t + 1) * Fi) if divide_input else slice(0, Fi)
        W = pre[t].weight
        proj[0, r, c] = W[:, cs]
        proj[0, P + t * Fs:P + t * Fs + Fi, c] = W[:, cd]
        pbias[P + t * Fs:P + t * Fs + Fi] = pre[t].bias
        if ed:
            edge[0, r, :ed] = W[:, 2 * Fi:]
        Wp = post[t].weight                                                    # (No, (S A + 1) Fi): [h | scaler-major aggregates]
        o = slice(t * No, (t + 1) * No)
        wself[0, o, c] = Wp[:, :Fi]
        blocks = Wp[:, Fi:].reshape(No, S, A, Fi)
        for j, s in enumerate(perm):
            wpost[j, o].view(No, A, P)[:, :, r] = blocks[:, s]
    res = {
        "P": P, "perm": perm,
        "proj": ops.contract_image_bf16(proj), "proj_bias": pbias,
        "edge": ops.contract_image_bf16(edge) if ed else None,
        "post": ops.contract_image_bf16(wpost), "self": ops.contract_image_bf16(wself),
        "post_bias": torch.cat([l.bias for l in post]).contiguous(),
        "cs": None, "ct": None,
    }
    if bns:
        folds = [_fold_batchnorm_f32(bn) for bn in bns]
        res["cs"] = torch.cat([f[0] for f in folds]).contiguous()
        res["ct"] = torch.cat([f[1] for f in folds]).contiguous()
    return res


def _tower_images_bf16(towers, divide_input):
    """The weight images of the bf16 tower layer (ops.contract_image_bf16), built once per version of EVERY tensor they are made
    from -- the pretrans and first posttrans Linear and the BatchNorm tensors of every tower -- and cached on the first tower.
    With T towers of input width Fi, output width No, P = round8(T * Fi), A aggregators and S scalers:
      proj  (1, 2P, Kin)   rows [t Fi, (t+1) Fi): W_a of tower t, rows P + the same: W_b; bias [0 | b]   (x_src | x_dst, 16-byte halves)
      edge  (1, P, ed)     rows [t Fi, (t+1) Fi): W_e of tower t
      post  (S, T No, A P) row t No + n, column a P + t Fi + f of block s: the posttrans weight of tower t on aggregator a, scaler s;
                           zero where a tower does not read a column.  Blocks are ordered identity scaler first (`perm`)
      self  (1, T No, Kin) the posttrans weight on the tower's own features
    Kin = T Fi with divide_input (tower t reads the input slice [t Fi, (t+1) Fi): block-diagonal), else Fi."""
    t0 = towers[0]
    bns = [t.batchnorm_h for t in towers] if t0.batch_norm and t0.posttrans.is_affine else []
    ts = _tower_tensors(towers, pre=True, post=True, bn=bool(bns))

    def build():
        pre = [t.pretrans.fully_connected[0].linear for t in towers]
        post = [t.posttrans.fully_connected[0].linear for t in towers]
        return _build_tower_images_bf16(pre, post, t0.in_dim, t0.edge_dim, t0.scalers, len(t0.aggregators), divide_input, bns)
    return memo(t0, "_pna_amd_bf16_images", ts, (divide_input, tuple(t0.scalers), tuple(t0.aggregators), tuple(bn.eps for bn in bns)), build)


def _build_small_simple_images_bf16(lin, bn, A, S, F):
    """The images of _small_simple_images_bf16 from the posttrans Linear `lin` (N, S A F) and the BatchNorm `bn` (None: none)."""
    N = lin.out_features
    Fp, Kp = (F + 7) // 8 * 8, (A * ((F + 7) // 8 * 8) + 31) // 32 * 32
    blk = torch.zeros(S, N, A, Fp, dtype=torch.bfloat16, device=lin.weight.device)
    blk[..., :F] = lin.weight.reshape(N, S, A, F).permute(1, 0, 2, 3)
    post = torch.zeros(1, S, (N + 15) // 16 * 16, Kp, dtype=torch.bfloat16, device=lin.weight.device)
    post[0, :, :N, :A * Fp] = blk.reshape(S, N, A * Fp)
    cs, ct = _fold_batchnorm_f32(bn) if bn else (None, None)
    return {"post": post, "post_bias": lin.bias, "cs": cs, "ct": ct}


def _small_simple_images_bf16(layer):
    """The images of pna_tower_layer_bf16 in its PNASimpleLayer form: post (1, S, round16(N), round32(A round8(F))) from the
    reference-layout posttrans weight (N, S A F), the bias and the fp32-folded BatchNorm; cached per version of every source tensor."""
    lin, bn = layer.posttrans.fully_connected[0].linear, layer.batchnorm_h if layer.batch_norm else None
    ts = [lin.weight, lin.bias] + (_bn_tensors(bn) if bn else [])
    A, S, F = len(layer.aggregators), len(layer.scalers), layer.in_dim
    return memo(layer, "_pna_amd_bf16_small", ts, (A, S, bn.eps if bn else None),
                lambda: _build_small_simple_images_bf16(lin, bn, A, S, F))


def _build_small_images_bf16(pre, post, Fi, ed, S, A, divide_input, bns, mix_lin, dst_first=False):
    """The images of _small_images_bf16 from the towers' first pretrans / posttrans Linear modules and the mixing Linear (None: none);
    ed and dst_first as in _build_tower_images_bf16."""
    T, Fo = len(pre), post[0].out_features
    r = lambda x, m: (x + m - 1) // m * m   # noqa: E731
    Fp, Fop, Kp, Khp = r(Fi, 8), r(Fo, 16), r(A * r(Fi, 8), 32), r(Fi, 32)
    Kin = T * Fi if divide_input else Fi
    dev, bf = pre[0].weight.device, torch.bfloat16
    cs, cd = (slice(Fi, 2 * Fi), slice(0, Fi)) if dst_first else (slice(0, Fi), slice(Fi, 2 * Fi))
    proj = torch.zeros(1, 2 * T * Fp, Kin, dtype=bf, device=dev)
    pbias = torch.zeros(2 * T * Fp, dtype=bf, device=dev)
    edge = torch.zeros(1, T * Fp, max(ed, 1), dtype=bf, device=dev)
    wpost = torch.zeros(T, S, Fop, Kp, dtype=bf, device=dev)
    wself = torch.zeros(T, Fop, Khp, dtype=bf, device=dev)
    for t in range(T):
        c = slice(t * Fi, (t + 1) * Fi) if divide_input else slice(0, Fi)
        W = pre[t].weight
        proj[0, t * Fp:t * Fp + Fi, c] = W[:, cs]
        proj[0, (T + t) * Fp:(T + t) * Fp + Fi, c] = W[:, cd]
        pbias[(T + t) * Fp:(T + t) * Fp + Fi] = pre[t].bias
        if ed:
            edge[0, t * Fp:t * Fp + Fi, :ed] = W[:, 2 * Fi:]
        Wp = post[t].weight                                                    # (Fo, (S A + 1) Fi): [h | scaler-major aggregates]
        wself[t, :Fo, :Fi] = Wp[:, :Fi]
        blk = torch.zeros(S, Fo, A, Fp, dtype=bf, device=dev)
        blk[..., :Fi] = Wp[:, Fi:].reshape(Fo, S, A, Fi).permute(1, 0, 2, 3)
        wpost[t, :, :Fo, :A * Fp] = blk.reshape(S, Fo, A * Fp)
    res = {
        "proj": ops.contract_image_bf16(proj), "proj_bias": pbias,
        "edge": ops.contract_image_bf16(edge) if ed else None,
        "post": torch.cat([wpost.reshape(-1), wself.reshape(-1)]),
        "post_bias": torch.cat([l.bias for l in post]).contiguous(),
        "cs": None, "ct": None, "mix": None, "mix_bias": None, "etab": None,
    }
    if bns:
        folds = [_fold_batchnorm_f32(bn) for bn in bns]
        res["cs"] = torch.cat([f[0] for f in folds]).contiguous()
        res["ct"] = torch.cat([f[1] for f in folds]).contiguous()
    if mix_lin is not None:
        No = mix_lin.weight.shape[0]
        res["mix"] = torch.zeros(r(No, 16), r(T * Fo, 32), dtype=bf, device=dev)
        res["mix"][:No, :T * Fo] = mix_lin.weight
        res["mix_bias"] = mix_lin.bias
    return res


def _small_images_bf16(towers, mix, divide_input):
    """The images of pna_tower_layer_bf16 (include/pna_amd.h) for T towers and, with `mix`, the mixing network, built once per version
    of EVERY tensor they are made from -- the key of _tower_images_bf16 plus the mixing tensors -- and cached on the first tower.
    With Fp = round8(Fi), Fop = round16(Fo), Kp = round32(A Fp), Khp = round32(Fi):
      proj  the contraction image of the (2 T Fp, Kin) projection rows: W_a of tower t at rows t Fp, W_b at T Fp + t Fp; proj_bias
      edge  the contraction image of the (T Fp, ed) edge rows: W_e of tower t at rows t Fp
      post  [T][S][Fop][Kp] (each tower's OWN blocks, scalers in the layer's order) followed by the self blocks [T][Fop][Khp], flat
      mix   (round16(No), round32(T Fo))"""
    t0 = towers[0]
    bns = [t._modules["batchnorm_h"] for t in towers] if t0.batch_norm else []
    ts = _tower_tensors(towers, pre=True, post=True, bn=t0.batch_norm, mix=mix)

    def build():
        pre = [t.pretrans.fully_connected[0].linear for t in towers]
        post = [t.posttrans.fully_connected[0].linear for t in towers]
        return _build_small_images_bf16(pre, post, t0.in_dim, t0.edge_dim, len(t0.scalers), len(t0.aggregators), divide_input, bns,
                                        mix.linear if mix is not None else None)
    return memo(t0, "_pna_amd_bf16_small", ts,
                (divide_input, tuple(t0.scalers), tuple(t0.aggregators), tuple(bn.eps for bn in bns), mix is not None), build)


def _small_edge_table_bf16(im, rows, ed, width):
    """bf16 (n_types, width) = R(rows W_e^T) for the <= 4 type rows of Graph.edge_type_table, kept with the images while the rows are
    the same storage at the same version (PNANet's rows are its embedding weight: one launch per weight state, not per call).  A key
    of its own, WITHOUT the object: PNANet registers its rows on the graph in every forward and the graph keeps `rows.detach()` -- a new
    tensor object per forward over the same storage and version counter, which _cache.tensor_key would take for a new state."""
    key = (rows.data_ptr(), rows._version, rows.shape, rows.dtype, rows.device)
    hit = im["etab"]
    if hit is None or hit[0] != key:
        with torch.no_grad():
            hit = im["etab"] = (key, ops.contract_bf16(rows.contiguous(), ed, im["edge"], width), rows)   # (rows: the address stays taken)
    return hit[1]


def _towers_small_bf16(towers, mix, graph, h, e, snorm_n, divide_input, residual):
    """PNATower / PNALayer through pna_tower_layer_bf16 when bf16_small_applies says so, else None (the multi-launch path follows)."""
    from .dgl.pna_layer import _row_scales
    t0 = towers[0]
    T, Fi, ed, Fo = len(towers), t0.in_dim, t0.edge_dim, t0.out_dim
    V = h.shape[0]
    if not 0 < V <= BF16_SMALL_ROWS:
        return None
    etab = None
    if t0.edge_features:
        if e is None:
            raise ValueError("edge_features=True but no edge features were given")
        # while a stream is capturing the table is taken only from register_edge_types (device-side results): a table hashed from the
        # VALUES of e would freeze the captured example's types into the replay, the per-edge route is captured instead
        if not torch.cuda.is_current_stream_capturing() or graph.edge_types_registered(e):
            etab = graph.edge_type_table(e)
    No = mix.linear.weight.shape[0] if mix is not None else None
    if not bf16_small_applies(graph, V, T=T, Fi=Fi, Fo=Fo, A=len(t0.aggregators), divide_input=divide_input,
                              posttrans_affine=t0.posttrans.is_affine, edge_features=t0.edge_features, etab=etab, No=No):
        return None
    if t0.edge_features and not graph.edge_types_registered(e):
        # a capture that follows these warm-up calls takes the per-edge multi-launch route for the first time: its images exist by then
        _tower_images_bf16(towers, divide_input)
        if mix is not None:
            _mix_image_bf16(mix)
    im = _small_images_bf16(towers, mix, divide_input)
    csr = graph.csr
    edge_type = edge_table = None
    if etab is not None:
        edge_type, edge_table = etab[0], _small_edge_table_bf16(im, etab[1], ed, T * ((Fi + 7) // 8 * 8))
    slope = 1.0
    if mix is not None:
        slope = 1.0 if mix.activation is None else 0.0 if isinstance(mix.activation, torch.nn.ReLU) else mix.activation.negative_slope
    return ops.tower_layer_bf16(csr.rowptr, csr.col, h, n_tower=T, Fi=Fi, Fo=Fo, divide_input=divide_input, aggregators=t0.aggregators,
                                row_scales=_row_scales(graph, t0.scalers, t0.avg_d, h.device), post_img=im["post"],
                                post_bias=im["post_bias"], proj_img=im["proj"], proj_bias=im["proj_bias"],
                                row_post=snorm_n.reshape(-1).float() if t0.graph_norm else None, col_scale=im["cs"], col_shift=im["ct"],
                                mix_img=im["mix"], mix_bias=im["mix_bias"], No=No or 0, slope=slope,
                                residual=h if residual else None, edge_type=edge_type, edge_table=edge_table)


def _mix_image_bf16(mix):
    """The pna_contract_bf16 image of the mixing weight, cached on the module per weight state."""
    w = mix.linear.weight
    return memo(mix, "_pna_amd_bf16_mix", [w], None, lambda: ops.contract_image_bf16(w.unsqueeze(0)))


def towers_bf16(towers, graph, h, e, snorm_n, divide_input):
    """The concatenated tower outputs h_cat (V, T * out_dim per tower) of PNATower.forward, models/dgl/pna_layer.py:55-76, in inference
    on bf16 features and parameters with a 1-layer pretrans.  Four launches: the node-level projections x_src = W_a h,
    x_dst = W_b h + b of all towers (pna_contract_bf16, rounded to bf16), [the edge term W_e ef per edge type or per edge,] the
    gather of x_src[u] + x_dst[v] + x_edge in fp32 with fp32 statistics (pna_gather_bf16, one row of width T * Fi for all towers)
    and the posttrans of all towers against one block-structured weight image with the degree scalers, bias, graph norm and the
    folded BatchNorm in its epilogue.  A deeper posttrans MLP runs its first Linear on the kernel and the rest -- later layers, graph
    norm, BatchNorm -- as each tower's own bf16 torch ops.  The result's pitch is a multiple of 8 elements."""
    from .dgl.pna_layer import _row_scales
    t0 = towers[0]
    T, Fi, ed, No = len(towers), t0.in_dim, t0.edge_dim, t0.out_dim
    Kin = T * Fi if divide_input else Fi
    if h.dim() != 2 or h.shape[1] != Kin:
        raise ValueError(f"expected features of shape (V, {Kin}), got {tuple(h.shape)}")
    if h.stride(-1) != 1:
        h = h.contiguous()
    sharded = isinstance(graph, HaloGraph)
    out = None if sharded else _towers_small_bf16(towers, None, graph, h, e, snorm_n, divide_input, False)
    if out is not None:
        return out
    im = _tower_images_bf16(towers, divide_input)
    P, csr = im["P"], graph.csr
    x_cat = ops.contract_bf16(h, Kin, im["proj"], 2 * P, (None,), im["proj_bias"])
    edge_rows = edge_type = None
    if t0.edge_features:
        if e is None:
            raise ValueError("edge_features=True but no edge features were given")
        etab = None                                      # an embedding of <= 4 edge types: W_e ef once per type (not from the VALUES of
        if not torch.cuda.is_current_stream_capturing() or graph.edge_types_registered(e):     # e while a hipGraph is being captured)
            etab = graph.edge_type_table(e)
        if etab is not None:
            edge_type, ef = etab
        else:
            ef = e[csr.eid.long()]                       # per-edge features in CSR (dst-sorted) order
        edge_rows = ops.contract_bf16(ef.contiguous(), ed, im["edge"], P)
    if sharded:                                          # the halo exchanges PROJECTED rows, as the fp32 route does
        agg = _shard_gather_bf16(graph, x_cat[:, :P], T * Fi, t0.aggregators, P, dst_term=x_cat[:, P:P + T * Fi],
                                 edge_rows=edge_rows, edge_type=edge_type)
    else:
        agg = ops.gather_bf16(csr.rowptr, csr.col, x_cat[:, :T * Fi], T * Fi, t0.aggregators, dst_term=x_cat[:, P:P + T * Fi],
                              edge_rows=edge_rows, edge_type=edge_type, block_stride=P, heavy=graph.heavy_schedule(),
                              workspace=graph.workspace)
    scales = _row_scales(graph, t0.scalers, t0.avg_d, h.device)
    scales = [scales[s] for s in im["perm"]]
    A = len(t0.aggregators)
    if t0.posttrans.is_affine:
        post = snorm_n.reshape(-1).float() if t0.graph_norm else None
        return ops.contract_bf16(agg, A * P, im["post"], T * No, scales, im["post_bias"], h_self=h, w_self=im["self"],
                                 row_post=post, col_scale=im["cs"], col_shift=im["ct"])
    y = ops.contract_bf16(agg, A * P, im["post"], T * No, scales, im["post_bias"], h_self=h, w_self=im["self"])
    sn = snorm_n.to(torch.bfloat16)
    outs = [tower.tail(y[:, t * No:(t + 1) * No], sn) for t, tower in enumerate(towers)]
    return torch.cat(outs, dim=1) if T > 1 else outs[0]


def tower_layer_bf16(layer, graph, h, e, snorm_n):
    """PNALayer.forward (models/dgl/pna_layer.py:130-145) in inference on bf16 features and parameters: towers_bf16, then the mixing
    network -- Linear, LeakyReLU and the residual -- as one more pna_contract_bf16 launch."""
    mix = layer.mixing_network
    towers = list(layer.towers)
    Kin = len(towers) * towers[0].in_dim if layer.divide_input else towers[0].in_dim
    if h.dim() == 2 and h.shape[1] == Kin:
        hs = h if h.stride(-1) == 1 else h.contiguous()
        out = None if isinstance(graph, HaloGraph) else _towers_small_bf16(towers, mix, graph, hs, e, snorm_n, layer.divide_input, layer.residual)
        if out is not None:
            return out
    h_cat = towers_bf16(towers, graph, h, e, snorm_n, layer.divide_input)
    img = _mix_image_bf16(mix)
    N = layer.out_dim
    out = torch.empty(h.shape[0], N, dtype=torch.bfloat16, device=h.device)
    slope = 1.0 if mix.activation is None else 0.0 if isinstance(mix.activation, torch.nn.ReLU) else mix.activation.negative_slope
    return ops.contract_bf16(h_cat, N, img, N, (None,), mix.linear.bias, slope=slope,
                             residual=(h if h.stride(-1) == 1 else h.contiguous()) if layer.residual else None, out=out)


# ---- bf16 inference of the PyG front end (pytorch_geometric/pna.py: PNAConv, PNAConvSimple) ---------------------------------------
# kernel names of the PyG aggregators in bf16: `var` is not clamped, `std` of a row without in-edges is sqrt(1e-5) (both in the device code)
_PYG_BF16_AGG = {"sum": "sum", "mean": "mean", "min": "min", "max": "max", "var": "var_raw", "std": "std_pyg"}


def pyg_row_factors(graph, scalers, avg_deg):
    """fp32 [V] row factors of the PyG scalers (None = identity), computed by pytorch_geometric.scalers.row_factor once per graph,
    scaler name and avg_deg value and kept on the graph: no device-to-host step on a later call."""
    cache = graph.__dict__.setdefault("_pyg_row_factors", {})
    out, deg = [], None
    for s in scalers:
        if s == "identity":
            out.append(None)
            continue
        key = (s, avg_deg["lin"], avg_deg["log"])
        f = cache.get(key)
        if f is None:
            from .pytorch_geometric.scalers import row_factor
            if deg is None:
                deg = graph.in_degrees().to(torch.float32)
            f = cache[key] = row_factor(s, deg, avg_deg).contiguous()
        out.append(f)
    return out


def _edge_ids(graph):
    """int32 arange(E) on the graph's device, cached on the graph: the identity `col` under which the gather kernels aggregate
    messages that are stored one row per CSR edge."""
    ids = graph.__dict__.get("_edge_ids")
    if ids is None:
        ids = graph.__dict__["_edge_ids"] = torch.arange(graph.csr.col.numel(), dtype=torch.int32, device=graph.csr.col.device)
    return ids


def pyg_simple_bf16(conv, graph, x):
    """PNAConvSimple.forward (models/pytorch_geometric/pna.py:232-253) in inference on bf16 features and parameters: the structure of
    simple_layer_bf16 without BatchNorm, ReLU and residual -- pna_tower_layer_bf16 (slope 1) for molecule batches, else
    pna_segreduce_fwd_bf16 and pna_posttrans_bf16 without epilogue -- under the PyG statistics rules.  A deeper post_nn runs its first
    Linear on the kernel and the rest as the module's own bf16 ops."""
    F, N = conv.F_in, conv.F_out
    if x.dim() != 2 or x.shape[1] != F:
        raise ValueError(f"expected features of shape (V, {F}), got {tuple(x.shape)}")
    if x.stride(-1) != 1:
        x = x.contiguous()
    names = [_PYG_BF16_AGG[a] for a in conv.aggregator_names]
    A, S = len(names), len(conv.scaler_names)
    post = list(conv.post_nn)
    lin = post[0]
    scales = pyg_row_factors(graph, conv.scaler_names, conv.avg_deg)
    csr = graph.csr
    if bf16_small_applies(graph, x.shape[0], T=1, Fi=F, Fo=N, A=A, divide_input=False, posttrans_affine=len(post) == 1, no_self_panel=True):
        im = memo(conv, "_pna_amd_bf16_small", [lin.weight, lin.bias], (A, S), lambda: _build_small_simple_images_bf16(lin, None, A, S, F))
        return ops.tower_layer_bf16(csr.rowptr, csr.col, x, n_tower=1, Fi=F, Fo=N, divide_input=False, aggregators=names, row_scales=scales,
                                    post_img=im["post"], post_bias=im["post_bias"], slope=1.0, no_self_panel=True)
    Fb = (F + 7) // 8 * 8
    agg = ops.segreduce_bf16(csr.rowptr, csr.col, x, F, names, block_stride=Fb, heavy=graph.heavy_schedule(), workspace=graph.workspace)
    w_img = ops.pack_posttrans_weight_bf16(lin.weight, S, A, F, Fb)
    y = ops.posttrans_bf16(agg, A * Fb, w_img, N, scales, lin.bias)
    for m in post[1:]:
        y = m(y)
    return y


def _pyg_conv_linears(conv):
    """(first pre_nn Linear, hidden pre_nn Linears, first post_nn Linear) of every tower of a PNAConv."""
    pre = [list(nn) for nn in conv.pre_nns]
    return [p[0] for p in pre], [p[2::2] for p in pre], [nn[0] for nn in conv.post_nns]


def _pyg_conv_tensors(conv, hidden):
    """The keyed tensor list of the PNAConv image builders: every Linear they read -- edge_encoder, the first (and, `hidden`, every
    later) pre_nn Linear and the first post_nn Linear of every tower, lin."""
    pre, hid, post = _pyg_conv_linears(conv)
    lins = pre + post + [conv.lin] + ([conv.edge_encoder] if conv.edge_dim is not None else [])
    if hidden:
        lins += [l for h in hid for l in h]
    return [p for l in lins for p in (l.weight, l.bias)]


def _pyg_conv_images_bf16(conv):
    """The images of the multi-launch bf16 PNAConv, cached on the module per version of every source tensor: _build_tower_images_bf16
    over the PyG column order [x_i (destination) | x_j (source) | enc] of pre_nns[t][0].weight -- packed towers with pre_layers = 1,
    the per-tower padded layout with the image of pna_edge_mlp_bf16 (`mlp`, `mlp_bias`) for a deeper pre_nn -- plus the contraction
    images of edge_encoder (`enc`, `enc_bias`) and of lin (`mix`)."""
    deep = len(conv.pre_nns[0]) > 1
    ts = _pyg_conv_tensors(conv, deep)

    def build():
        pre, hid, post = _pyg_conv_linears(conv)
        Fi, use_edge = conv.F_in, conv.edge_dim is not None
        im = _build_tower_images_bf16(pre, post, Fi, Fi if use_edge else 0, conv.scaler_names, len(conv.aggregator_names),
                                      conv.divide_input, [], dst_first=True, tower_pitch=(Fi + 7) // 8 * 8 if deep else None)
        im["mix"] = ops.contract_image_bf16(conv.lin.weight.unsqueeze(0))
        im["enc"] = ops.contract_image_bf16(conv.edge_encoder.weight.unsqueeze(0)) if use_edge else None
        im["enc_bias"] = conv.edge_encoder.bias if use_edge else None
        if deep:
            im["mlp"], im["mlp_bias"] = ops.edge_mlp_image_bf16([[l.weight for l in h] for h in hid], [[l.bias for l in h] for h in hid])
        return im
    return memo(conv, "_pna_amd_bf16_images", ts, (conv.divide_input, tuple(conv.scaler_names), tuple(conv.aggregator_names)), build)


def _pyg_conv_small_images_bf16(conv):
    """The images of pna_tower_layer_bf16 for a PNAConv with 1-layer pre_nns and post_nns (lin is the mixing network, slope 1), plus the
    contraction image of edge_encoder; cached on the module per version of every source tensor."""
    ts = _pyg_conv_tensors(conv, False)

    def build():
        pre, _, post = _pyg_conv_linears(conv)
        Fi, use_edge = conv.F_in, conv.edge_dim is not None
        im = _build_small_images_bf16(pre, post, Fi, Fi if use_edge else 0, len(conv.scaler_names), len(conv.aggregator_names),
                                      conv.divide_input, [], conv.lin, dst_first=True)
        im["enc"] = ops.contract_image_bf16(conv.edge_encoder.weight.unsqueeze(0)) if use_edge else None
        im["enc_bias"] = conv.edge_encoder.bias if use_edge else None
        return im
    return memo(conv, "_pna_amd_bf16_small", ts, (conv.divide_input, tuple(conv.scaler_names), tuple(conv.aggregator_names)), build)


def _pyg_edge_rows_bf16(im, ef, edge_dim, Fi, width):
    """x_edge = R(W_e R(W_enc ef + b_enc)) for the rows of ef (CSR edges, or the rows of an edge-type table): two pna_contract_bf16
    launches, no matmul per edge in torch."""
    enc = ops.contract_bf16(ef.contiguous(), edge_dim, im["enc"], Fi, (None,), im["enc_bias"])
    return ops.contract_bf16(enc, Fi, im["edge"], width)


def _pyg_small_edge_table_bf16(im, rows, edge_dim, Fi, width):
    """_pyg_edge_rows_bf16 of the <= 4 rows of Graph.edge_type_table, kept with the images while the rows are the same storage at the
    same version (the key of _small_edge_table_bf16)."""
    key = (rows.data_ptr(), rows._version, rows.shape, rows.dtype, rows.device)
    hit = im["etab"]
    if hit is None or hit[0] != key:
        with torch.no_grad():
            hit = im["etab"] = (key, _pyg_edge_rows_bf16(im, rows, edge_dim, Fi, width), rows)
    return hit[1]


def pyg_conv_bf16(conv, graph, x, edge_attr):
    """PNAConv.forward (models/pytorch_geometric/pna.py:121-165) in inference on bf16 features and parameters: the structure of
    tower_layer_bf16 without graph norm, BatchNorm and residual, with `lin` as the mixing network, under the PyG statistics rules.
      pre_layers = 1   the node-level projections x_src = W_j x, x_dst = W_i x + b (pna_contract_bf16), the edge term
                       W_e R(W_enc e + b_enc) per edge-type row or per edge (two more launches), pna_gather_bf16, the post_nns of all
                       towers in one contraction, lin -- or ONE call, pna_tower_layer_bf16, when bf16_small_applies
      pre_layers >= 2  the same projections in the per-tower padded layout, pna_edge_mlp_bf16 for the hidden layers (messages
                       materialised in bf16, one row per CSR edge), pna_segreduce_fwd_bf16 over them under an identity `col`
    A deeper post_nn runs its first Linear on the kernel and the rest as the module's own bf16 ops."""
    T, Fi, Fo, N = conv.towers, conv.F_in, conv.F_out, conv.out_channels
    Kin = T * Fi if conv.divide_input else Fi
    if x.dim() != 2 or x.shape[1] != Kin:
        raise ValueError(f"expected features of shape (V, {Kin}), got {tuple(x.shape)}")
    if x.stride(-1) != 1:
        x = x.contiguous()
    names = [_PYG_BF16_AGG[a] for a in conv.aggregator_names]
    A = len(names)
    deep, post_affine = len(conv.pre_nns[0]) > 1, len(conv.post_nns[0]) == 1
    use_edge = conv.edge_dim is not None
    csr = graph.csr
    etab = None
    if use_edge:
        # while a stream is capturing the table is taken only from register_edge_types: a table hashed from the VALUES of edge_attr
        # would freeze the captured example's types into the replay (towers_bf16)
        if not torch.cuda.is_current_stream_capturing() or graph.edge_types_registered(edge_attr):
            etab = graph.edge_type_table(edge_attr)
    scales = pyg_row_factors(graph, conv.scaler_names, conv.avg_deg)
    if not deep and bf16_small_applies(graph, x.shape[0], T=T, Fi=Fi, Fo=Fo, A=A, divide_input=conv.divide_input, posttrans_affine=post_affine,
                                       edge_features=use_edge, etab=etab, No=N):
        im = _pyg_conv_small_images_bf16(conv)
        if use_edge and not graph.edge_types_registered(edge_attr):
            # a capture that follows these warm-up calls takes the per-edge multi-launch route for the first time: its images exist by
            # then.  Both image sets are keyed on the same tensors, so the key just computed tells whether they are current.
            d = conv.__dict__
            hit = d.get("_pna_amd_bf16_images")
            if hit is None or hit[0] != d["_pna_amd_bf16_small"][0]:
                _pyg_conv_images_bf16(conv)
        edge_type = edge_table = None
        if etab is not None:
            edge_type, edge_table = etab[0], _pyg_small_edge_table_bf16(im, etab[1], conv.edge_dim, Fi, T * ((Fi + 7) // 8 * 8))
        return ops.tower_layer_bf16(csr.rowptr, csr.col, x, n_tower=T, Fi=Fi, Fo=Fo, divide_input=conv.divide_input, aggregators=names,
                                    row_scales=scales, post_img=im["post"], post_bias=im["post_bias"], proj_img=im["proj"],
                                    proj_bias=im["proj_bias"], mix_img=im["mix"], mix_bias=im["mix_bias"], No=N, slope=1.0,
                                    edge_type=edge_type, edge_table=edge_table)
    im = _pyg_conv_images_bf16(conv)
    P = im["P"]
    x_cat = ops.contract_bf16(x, Kin, im["proj"], 2 * P, (None,), im["proj_bias"])
    edge_rows = edge_type = None
    if use_edge:
        if etab is not None:
            edge_type, ef = etab
        else:
            ef = edge_attr[csr.eid]                       # per-edge features in CSR (destination-sorted) order
        edge_rows = _pyg_edge_rows_bf16(im, ef, conv.edge_dim, Fi, P)
    if deep:
        msgs = ops.edge_mlp_bf16(csr.col, csr.row, x_cat[:, :P], x_cat[:, P:], n_tower=T, F=Fi, w_img=im["mlp"], bias=im["mlp_bias"],
                                 edge_rows=edge_rows, edge_type=edge_type)
        agg = ops.segreduce_bf16(csr.rowptr, _edge_ids(graph), msgs, P, names, block_stride=P, heavy=graph.heavy_schedule(),
                                 workspace=graph.workspace)
    else:
        agg = ops.gather_bf16(csr.rowptr, csr.col, x_cat[:, :T * Fi], T * Fi, names, dst_term=x_cat[:, P:P + T * Fi], edge_rows=edge_rows,
                              edge_type=edge_type, block_stride=P, heavy=graph.heavy_schedule(), workspace=graph.workspace)
    y = ops.contract_bf16(agg, A * P, im["post"], T * Fo, [scales[s] for s in im["perm"]], im["post_bias"], h_self=x, w_self=im["self"])
    if not post_affine:
        outs = []
        for t, nn in enumerate(conv.post_nns):
            z = y[:, t * Fo:(t + 1) * Fo]
            for m in list(nn)[1:]:
                z = m(z)
            outs.append(z)
        y = torch.cat(outs, dim=1) if T > 1 else outs[0]
    return ops.contract_bf16(y, N, im["mix"], N, (None,), conv.lin.bias, slope=1.0)
