/*
 * pna_amd.h -- C ABI of libpna_amd.so, the MI355X (gfx950) implementation of the PNA
 * message-passing hot path of lukecavabarrett/pna.
 *
 * The reference has no FFI of its own (it is pure Python/PyTorch); the boundary it exposes is the
 * `reduce_func` / aggregator / scaler operator set that DGL's `update_all` schedules, plus the
 * dense `nn.Linear` that follows it.  Each entry point below names the reference code it
 * replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C, no ownership transfer: every pointer is a DEVICE pointer owned by the caller
 *     (except where marked host), valid until the stream reaches the end of the call's work;
 *   - stream-ordered and asynchronous: nothing here synchronises the device;
 *   - re-entrant: no global mutable state except the per-thread last-error string;
 *   - return value 0 = success, negative = error (see PNA_E_*); pna_last_error() gives the text;
 *   - all data is fp32 and all arithmetic is fp32, except the bf16 entry points of ABI 22 / 23 (bf16 data, fp32 accumulation) (pna_posttrans_x3_f32 evaluates each fp32 product as six exact
 *     bf16 partial products accumulated in fp32 -- fp32-level accuracy, see there); indices are int32; row strides
 *     (ld*) are in floats.
 */
#ifndef PNA_AMD_H
#define PNA_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNA_ABI_VERSION 23 /* 23, additive: + pna_pyg_conv_train_fwd_f32 / pna_pyg_conv_train_bwd_f32 / pna_pyg_conv_train_workspace_bytes /
                                  pna_pyg_conv_train_args (PNAConv's training forward and backward, one call each, on the kernels of the
                                  tower training routes without BatchNorm and with the PyG statistics); no existing struct or entry point changed.
                                  23, additive: + pna_tower_aggr_train_fwd_f32 / pna_tower_aggr_train_bwd_f32 / pna_tower_aggr_train_workspace_bytes /
                                  pna_tower_aggr_train_args (the one-call tower training routes for any 1-4 distinct aggregators out of mean,
                                  sum, max, min, std, var, with or without edge features and dropout); no existing struct or entry point changed.
                                  23, additive: + pna_batch_plan_i32 / pna_batch_plan_limits / pna_batch_plan_workspace_bytes / pna_batch_plan_args (every
                                  index array of a fresh batch of small graphs -- CSR, transposed CSR, work lists, per-batch tables -- from
                                  one call, no library sort); no existing struct or entry point changed.
                                  23, additive: + pna_mlp_head_fwd_f32 / pna_mlp_head_bwd_f32 / pna_mlp_head_workspace_bytes / pna_mlp_head_in_scope /
                                  pna_mlp_head_args, PNA_MAX_MLP_LAYERS, PNA_MLP_MAX_WIDTH, PNA_MLP_ACT_*, PNA_MLP_SLAB_ROWS, PNA_MLP_MAX_SLABS (the dense
                                  heads of the nets: 1 to 4 Linear layers with none / ReLU / LeakyReLU over rows, one call each way); no
                                  existing struct or entry point changed.
                                  23, additive: + pna_gru_cell_in_scope, pna_tower_layer_lds_bytes, pna_tower_layer_bf16_lds_bytes (host-only queries: the
                                  scope and tile checks of pna_gru_cell_*_f32, pna_tower_layer_f32 and pna_tower_layer_bf16, so that a binding asks
                                  the library where it would otherwise copy a bound); no existing struct or entry point changed.
                                  23, additive: + pna_tower_drop_train_fwd_f32 / pna_tower_drop_train_bwd_f32 / pna_tower_drop_args, pna_dropout_mask_f32
                                  (the one-call tower training routes, with and without edge features, with the towers' dropout between
                                  their BatchNorm and the mixing Linear: a Philox4x32-10 mask regenerated in the backward from a 128-bit
                                  key); no existing struct or entry point changed.
                                  23, additive: + pna_set2set_fwd_f32 / pna_set2set_bwd_f32 / pna_set2set_workspace_bytes / pna_set2set_lds_bytes /
                                  pna_set2set_args, PNA_S2S_F32, PNA_S2S_MAX_WIDTH, PNA_S2S_MAX_NODES, PNA_S2S_MAX_STEPS, PNA_S2S_MAX_SLABS (the Set2Set
                                  graph readout of the multitask GNN, one call each way); no existing struct or entry point changed.
                                  23, additive: + pna_dense_layer_fwd_f32 / pna_dense_layer_bwd_f32 / pna_dense_layer_workspace_bytes /
                                  pna_dense_layer_lds_bytes / pna_dense_layer_args, PNA_DENSE_MAX_NODES, PNA_DENSE_MAX_SLABS, PNA_DENSE_SCALER_* (the
                                  dense-adjacency PNALayer of the multitask GNN, one call each way); no existing struct or entry point changed.
                                  23, additive: + pna_gru_cell_fwd_f32 / pna_gru_cell_bwd_f32 / pna_gru_cell_workspace_bytes / pna_gru_cell_args,
                                  PNA_GRU_F32, PNA_GRU_SLAB_ROWS, PNA_GRU_MAX_SLABS (the GRU update between two message-passing steps: nn.GRU over
                                  a length-1 sequence as a cell over rows, one call each way); no existing struct or entry point changed.
                                  23, additive: + pna_embed_sum_fwd_f32 / pna_embed_sum_bwd_f32 / pna_embed_sum_workspace_bytes / pna_embed_sum_args,
                                  pna_readout_fwd_f32 / pna_readout_bwd_f32 / pna_readout_args, PNA_MAX_EMBED_TABLE (the two ends of the molecule
                                  nets: the sum of embedding tables and the per-graph readout, one call each way); no existing struct or entry
                                  point changed.
                                  23, additive: + pna_tower_train_fwd_f32 / pna_tower_train_bwd_f32 / pna_tower_train_workspace_bytes /
                                  pna_tower_train_args, PNA_MAX_TOWER (PNALayer's TRAINING forward and backward on molecule batches, one call
                                  each); no existing struct or entry point changed.
                                  23, additive: + pna_tower_edge_train_fwd_f32 / pna_tower_edge_train_bwd_f32 / pna_tower_edge_train_workspace_bytes /
                                  pna_tower_edge_train_args (the same with per-edge features, edge_features=True: grad_e returned); no existing
                                  struct or entry point changed.
                                  23, additive: + pna_simple_train_fwd_f32 / pna_simple_train_bwd_f32 / pna_simple_train_workspace_bytes /
                                  pna_simple_train_args (PNASimpleLayer's TRAINING forward and backward on molecule batches, one call each);
                                  no existing struct or entry point changed.
                                  23: + pna_gather_bf16 / pna_contract_bf16 / pna_contract_bf16_tiles (bf16 inference of PNALayer / PNATower and the nets;
                                  pna_gather_bf16_args, pna_contract_bf16_args).
                                  23, additive: + pna_tower_layer_bf16 / pna_tower_layer_bf16_args (the bf16 tower layer of molecule batches
                                  as one call); no existing struct or entry point changed.
                                  23, additive: + pna_edge_mlp_bf16 / pna_edge_mlp_bf16_args (the hidden layers of a deep pre_nn per edge: bf16
                                  inference of the PyG front end) and PNA_AGG_STD_PYG, which the three bf16 statistics entry points accept
                                  beside PNA_AGG_VAR_RAW; no existing struct changed.
                                  23, additive: + pna_pack_rows_bf16, pna_gather_rows_bf16 / pna_gather_rows_bf16_args (bf16 inference on the
                                  shards of a destination-sharded graph: the halo pack on bf16 rows and the row-list, split-table member of
                                  the bf16 gather family); no existing struct or entry point changed.
                              22: + pna_segreduce_fwd_bf16 / pna_segreduce_bf16_partials_bytes, pna_posttrans_bf16 / pna_posttrans_bf16_tiles
                                  (bf16 inference of PNASimpleLayer; pna_segreduce_bf16_args, pna_posttrans_bf16_args).
                              21: the GUARDED fp16 x 2 contraction of the one-kernel layer (round 6): + pna_fused_degree_args.{w_img_x3,
                                  image_stride_x3, guard_ws, guard_ws_bytes, arith}, PNA_FD_ARITH_*, pna_fused_image_bytes, pna_fused_pack_f32,
                                  pna_fused_degree_guard_bytes; the fp16 x 2 images carry a 1024-byte tail (column scales + the guard's column
                                  thresholds); image_stride must EQUAL pna_fused_image_bytes; row scale bound in [2^14, 2^15).
                              20: - pna_fused_roles_{supported,image_bytes,grid,f32} (ABI 19's one-kernel layer with gather / multiply wavefront
                                  roles: parity-green, 2.1-2.7x slower than pna_fused_degree_f32, never on a product path -- removed from the
                                  library in round 5; the source lives on as tools/ubench/fused_roles.hip, the result in DESIGN.md 4.9).
                                  + pna_fused_degree_args.tile_counter (dynamic tile schedule), pna_fused_degree_tile_rows.
                                  pna_fused_degree_{image_bytes,pack_f32,f32}: images of two fp16 terms + a 512-byte tail of column scales
                                  (an opaque format between the pack function and the kernel of ONE library; the byte count changed).
                                  The trailing fields added "inside 19" are part of 20's structs: a binding that knows them no longer
                                  passes the version check of a library that does not.  Every args struct carries struct_size first.
                              19: struct_size first in every args struct; + pna_posttrans_dw_f32 / pna_posttrans_dw_grouped_f32
                                  (+ _workspace_bytes), pna_tower_layer_args.{edge_type, edge_table, ld_edge_table, n_edge_types, no_self_panel},
                                  pna_segreduce_bwd_args.{stat_row_of, stat_node_of, stat_rows}, the packed / in-place rows of
                                  pna_segreduce_bwd_pull_f32, 64-bit source-row addressing (x_rows < 2^32, any pitch >= F).
                              18: + pna_bn_tail_{workspace_bytes,fwd_f32,bwd_f32}: batch-statistics BatchNorm + ReLU + residual of the training path.
                              17: + pna_fused_degree_args.spare_workgroups (the rest-row launches beside the persistent kernel).
                              16: + pna_segreduce_bwd_pull_f32 (the backward's max / min terms inside the pull: no scatter atomics).
                              15: pna_fused_degree_*: wide shapes (F in 113..128 and / or N in 81..128).
                              14: pna_segreduce_args.edge_type / n_edge_types (edge terms from a table of edge types); the hand-scheduled gather takes
                                  edge terms (per edge or per type).
                              13: pna_fused_degree_args.x_dst / h_self / row_post + pna_fused_tower_{image_bytes,pack_f32}: the one-kernel layer
                                  for PNALayer with one tower.
                              12: pna_segreduce_args.out_row_of (the tower layers' aggregate written in degree order).
                              11: - pna_posttrans_x3w_* (ABI 8's contraction on 32x32 tiles: parity-green, 5 % slower than the 16x16 kernel on every
                                  shape measured, never selected -- removed, round 3).
                              10: + pna_fused_degree_{image_bytes,pack_f32,f32} (gather + degree-grouped contraction in one kernel).
                              9: pna_posttrans_args.row_perm / tile_image / image_stride (degree-grouped contraction),
                                pna_segreduce_args.heavy_out_rows.
                             8: + pna_posttrans_x3w_* (the bf16x3 contraction on 32x32 matrix-core tiles).
                             7: + pna_small_*, pna_tower_post_*, pna_tower_layer_f32 (the molecule-batch tower layer).
                             6: pna_posttrans_args: act_slope (LeakyReLU), n_tower + tower strides.
                             5: pna_posttrans_args.pipeline; the hand-scheduled gather takes dst_term; + pna_pack_rows_f32.
                             4: + pna_posttrans_x3_*, pna_fused_simple_f32, pna_collate_*, PNA_AGG_VAR_RAW */

#define PNA_OK 0
#define PNA_E_INVALID (-1)   /* bad argument (null pointer, unsupported size, unknown code) */
#define PNA_E_LAUNCH (-2)    /* the HIP runtime refused a launch / copy */
#define PNA_E_NODEVICE (-3)  /* no gfx950 device visible */

typedef void* pna_stream_t; /* a hipStream_t (0 = the null stream) */

/* Every *_args struct starts with `struct_size` = sizeof of the struct in the header the CALLER was compiled against (ABI 19, round 4:
 * fields had been appended through 18 ABI versions with only pna_abi_version() between a stale binding and a wild pointer).  An entry
 * point refuses a struct shorter than its own (PNA_E_INVALID, pna_last_error names the two sizes); fields appended in later ABI
 * versions therefore never read past a caller's struct.  PNA_ARGS_INIT zero-fills and stamps a struct in C. */
#define PNA_ARGS_INIT(type) ((type){ .struct_size = (uint32_t)sizeof(type) })

/* Aggregator codes -- models/dgl/aggregators.py:54-56 (AGGREGATORS dict) and
 * models/pytorch/pna/aggregators.py:149-152.  The order of codes in `aggr[]` is the order of the
 * F-wide blocks in the output, exactly like the order of names on the reference's command line. */
enum {
  PNA_AGG_MEAN = 0, /* dgl/aggregators.py:6-7    sum / D                                  */
  PNA_AGG_SUM = 1,  /* dgl/aggregators.py:50-51                                            */
  PNA_AGG_MAX = 2,  /* dgl/aggregators.py:10-11  NaN-propagating, like torch.max           */
  PNA_AGG_MIN = 3,  /* dgl/aggregators.py:14-15                                            */
  PNA_AGG_STD = 4,  /* dgl/aggregators.py:18-19  sqrt(relu(E[x^2]-E[x]^2) + 1e-5)          */
  PNA_AGG_VAR = 5,  /* dgl/aggregators.py:22-26  relu(E[x^2]-E[x]^2)                       */
  PNA_AGG_VAR_RAW = 6, /* pytorch_geometric/aggregators.py:25-28  E[x^2]-E[x]^2, NOT clamped (forward only) */
  PNA_AGG_STD_PYG = 7  /* pytorch_geometric/aggregators.py:31-32  std whose row without in-edges is sqrtf(1e-5f), not 0 (bf16 entry points only) */
};
#define PNA_MAX_AGGR 8
#define PNA_MAX_SCALER 8
#define PNA_MAX_TOWER 8   /* towers of one pna_tower_train_args */
#define PNA_MAX_EMBED_TABLE 16   /* tables of one pna_embed_sum_args */

/* Optional launch tuning; all-zero = library defaults. */
typedef struct pna_tuning {
  int32_t lanes_per_row;   /* lanes of a 64-wide wavefront that share one destination row (each lane owns
                              `vec` consecutive features); 0 = auto = min(64, ceil(F/vec))             */
  int32_t unroll;          /* in-edges of one row gathered per loop trip (2,4,8); 0 = auto            */
  int32_t rows_per_group;  /* destination rows processed back to back by one lane group; 0 = auto    */
  int32_t vec;             /* features per lane: 4 (dwordx4 gathers) or 1; 0 = auto                   */
  int32_t nt_store;        /* 1 = non-temporal output stores; 0 = auto(1); -1 = plain stores          */
  int32_t prefetch;        /* 1 = fetch the next row's source ids one row ahead; 0 = auto(1); -1 = off */
  int32_t reserved[2];     /* [0]: ignored by the shipped library (bench-experiment knobs that exist only in the
                                   separate -DPNA_AMD_EXPERIMENTS build of tools/build_experiments.sh);
                              [1]: 1 = force the compiler-scheduled kernel instead of the hand-scheduled one;
                                   2 = REQUIRE the hand-scheduled kernel (PNA_E_INVALID if the call does not qualify):
                                   a work list that covers only part of the rows is only honoured by that kernel */
} pna_tuning;

/*
 * Fused gather + multi-aggregator segment-reduce + degree scalers over a destination-sorted CSR.
 *
 * Replaces, in one launch: DGL `update_all(message, reduce_func)` with
 *   reduce_func            models/dgl/pna_layer.py:45-50 (PNATower) and :189-194 (PNASimpleLayer)
 *   the aggregators        models/dgl/aggregators.py:6-26,50-51
 *   the scalers            models/dgl/scalers.py:7-19
 * and, for the dense variant, models/pytorch/pna/layer.py:43-44 with aggregators.py:17-84 and
 * scalers.py:7-38 (edge_weight = adjacency weight).
 *
 * Message of CSR edge k (k in [rowptr[v], rowptr[v+1]) for destination v):
 *     m_k = x[col[k]]  (+ dst_term[v])  (+ edge_term[k])             each an F-vector
 *   col == NULL  -> x is edge-resident, m_k = x[k] (already-materialised per-edge messages, e.g. the
 *                   output of a multi-layer pretrans MLP, models/dgl/pna_layer.py:35-40);
 *   dst_term/edge_term are the h_dst / edge-feature halves of a 1-layer (affine) pretrans that has
 *   been factorised to node level: W[h_src|h_dst|ef]+b = (W_a h_src) + (W_b h_dst + b) + (W_e ef).
 * Output row v, block (s * n_aggr + a), feature f:
 *     out[v*ldo + (s*n_aggr + a)*block_stride + f] = aggr[a](m_k : k in row v)[f] * row_scale[s][v]
 *   (row_scale[s] == NULL means the identity scaler).  Scaler-major / aggregator-minor is the
 *   reference's concatenation order (pna_layer.py:48-49).
 * Rows with no in-edges get 0 in every block (DGL's zero initialiser; undefined in the reference).
 * Arithmetic: fp32, no FMA contraction, sums in CSR edge order (hub rows: per 128-edge segment, then over segments).
 * mean = s / D and E[x^2] = q / D are the reference's divisions bit for bit (one IEEE division per row for 1 / D, then
 * Markstein's fma correction per feature; round 1 used s * (1/D), 1 ulp off, which the cancellation in
 * std = sqrt(E[x^2] - E[x]^2 + 1e-5) amplifies to percents when all neighbours are equal); max, min and the degree
 * scalers are bit-exact; mean / std differ from the reference only through the summation ORDER of s and q.
 * edge_weight (nullable, [E]): mean/sum/std/var use sum_k w_k m_k and D = sum_k w_k; max/min use
 *   only edges with w_k > 0.
 * argmax/argmin (nullable, (V, ld_arg) int32): CSR edge position k of the first max / min, -1 for
 *   empty rows -- what the backward pass needs.
 *
 * Heavy rows: destinations with more than `heavy_threshold` in-edges are not walked by one lane
 * group; they are listed in `heavy_rows` and cut into segments of `seg_len` edges that are reduced
 * in parallel into `partials` and combined in segment order by a second small kernel, so results do
 * not depend on the launch geometry.  heavy_threshold <= 0 disables the split.
 */
typedef struct pna_segreduce_args {
  uint32_t struct_size;    /* sizeof(pna_segreduce_args) of the CALLER's header (ABI 19): a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* rowptr; /* [V+1] */
  const int32_t* col;    /* [E] or NULL */
  int32_t V;
  int32_t F;
  const float* x;
  int64_t ldx;
  int64_t x_rows;        /* rows of x (source nodes, or E when col == NULL); 0 = unknown (64-bit addressing) */
  const float* dst_term; /* nullable (V, ld_dst) */
  int64_t ld_dst;
  const float* edge_term; /* nullable (E, ld_edge) */
  int64_t ld_edge;
  const float* edge_weight; /* nullable [E] */

  /* Towers: the same graph reduced over n_tower independent feature slices of width F in one launch
   * (the reference loops over towers in Python, models/dgl/pna_layer.py:133-139).  Tower t reads
   * columns [t*tower_stride_in, +F) of x / dst_term / edge_term (and argmax/argmin) and writes its
   * n_scaler*n_aggr blocks starting at column t*tower_stride_out of out.  n_tower <= 1: one slice,
   * strides ignored. */
  int32_t n_tower;
  int32_t _pad_t;
  int64_t tower_stride_in;
  int64_t tower_stride_out;

  int32_t n_aggr;
  int32_t aggr[PNA_MAX_AGGR];
  int32_t n_scaler;
  int32_t _pad0;
  const float* row_scale[PNA_MAX_SCALER]; /* each nullable, [V] */

  float* out;
  int64_t ldo;
  int32_t block_stride;
  int32_t _pad1;
  int32_t* argmax; /* nullable */
  int32_t* argmin; /* nullable */
  int64_t ld_arg;

  /* heavy-row schedule (all optional; produced once per graph by the host, see pna_amd/graph.py) */
  int32_t heavy_threshold;   /* rows with degree > threshold are skipped by the main walk          */
  int32_t seg_len;           /* edges per heavy segment                                            */
  int32_t n_heavy;           /* number of heavy rows                                               */
  int32_t n_seg;             /* total number of segments                                           */
  const int32_t* heavy_rows; /* [n_heavy] row ids, ascending                                       */
  const int32_t* heavy_segptr; /* [n_heavy+1] first segment of each heavy row                      */
  const int32_t* seg_heavy;  /* [n_seg] index into heavy_rows of the row each segment belongs to   */
  float* partials;           /* workspace, pna_segreduce_partials_bytes(n_seg, F, n_tower) bytes   */

  /* Optional work list for the hand-scheduled kernel (used when the call is the 4-aggregator gather
   * mean|max|min|std with the identity scaler, messages x[col[k]] or x[col[k]] + dst_term[v] -- i.e. what
   * PNASimpleLayer and the PNATower layers issue; ABI 14: also with edge_term, per edge or per edge type): n_work_items records {row, beg, end, slot} (int32 x 4).  slot < 0:
   * the record is a whole row [beg,end) = [rowptr[row], rowptr[row+1]) whose result is finalised and stored;
   * slot >= 0: the record is heavy segment number `slot` (its partials go to partials[slot]; the segments of a
   * heavy row must be the ones heavy_segptr describes).  Every row must be covered exactly once, either by one
   * whole-row record or by its segments.  The host orders the records by length (pna_amd/graph.py) so that the
   * lane groups of a wavefront walk equally long records; results do not depend on the order.  NULL = the
   * compiler-scheduled kernel in natural row order. */
  const int32_t* work_items;
  int32_t n_work_items;
  int32_t _pad2;
  int64_t n_edges; /* = rowptr[V] (length of col); required with work_items */
  pna_tuning tune;
  /* ABI 9: where the aggregate of heavy row i (heavy_rows[i]) is written, as a row index of `out` (nullable: the row itself).
   * Together with work_items whose `row` field holds the OUTPUT row of a whole-row record (the hand-scheduled kernel uses that
   * field for nothing else when there is no dst_term) this lets a caller have the aggregate written in any row order -- e.g.
   * grouped by in-degree for pna_posttrans_args.row_perm.  `out` must then have as many rows as the largest index + 1. */
  const int32_t* heavy_out_rows;
  /* ABI 12: with dst_term (where the work list's `row` must stay the node), the row of `out` that receives node v's aggregate:
   * out_row_of[v] for whole-row records (heavy rows: heavy_out_rows).  Nullable; hand-scheduled kernel with work_items only. */
  const int32_t* out_row_of;
  /* ABI 14: edge terms from a table.  When the edge features are an embedding of an edge TYPE (the molecule nets: bond type,
   * realworld_benchmark/nets/molecules_graph_regression/pna_net.py with --edge_feat True), W_e . ef has one distinct row per type:
   * edge_term is then (n_edge_types, ld_edge) and the term of CSR edge k is row edge_type[k] (int32 [E], CSR order).  NULL: edge_term
   * has one row per edge.  n_edge_types <= 4 keeps the table in registers of the hand-scheduled kernel. */
  const int32_t* edge_type;
  int32_t n_edge_types;
  int32_t _pad3;
} pna_segreduce_args;

/* Launches the kernels described above on `stream`. */
int pna_segreduce_fwd_f32(const pna_segreduce_args* args, pna_stream_t stream);

/* Bytes of `partials` workspace needed for n_seg heavy segments of n_tower slices of width F. */
int64_t pna_segreduce_partials_bytes(int32_t n_seg, int32_t F, int32_t n_tower);

/*
 * Backward of pna_segreduce_fwd_f32 (what autograd derives through the reference's per-bucket torch ops,
 * models/dgl/aggregators.py:6-26).  `gagg` is the gradient w.r.t. the UNSCALED aggregates in the forward's
 * identity-scaler layout: row v, tower t, aggregator i (aggr[i]) at column t*tower_stride_g + i*F of an
 * (V, ld_g) matrix (the caller folds the degree scalers in: G_i = sum_s row_scale[s] * dOut[s, i]).
 * The kernel rebuilds every message m_k = x[col[k]] (+ dst_term[v]) (+ edge_term[k]) and scatters
 *     dL/dm_k = G_mean/D + G_sum + [k = argmax] G_max + [k = argmin] G_min
 *             + (G_var + G_std/(2 std)) [var > 0] (2/D) (m_k - mean)
 * into grad_x[col[k]] (fp32 hardware atomics: zero-fill grad_x first; plain stores when col == NULL),
 * grad_dst[v] (sum over the row's edges; zero-fill first) and grad_edge[k].  Any of the three may be NULL.
 * mean / stdv / var are the forward results (identity-scaled), (V, ld_stat) with tower stride
 * tower_stride_stat -- needed only when std or var is among aggr[] (stdv or var, one is enough);
 * argmax / argmin are the forward's (V, ld_arg) outputs, tower stride tower_stride_in.
 * x / dst_term / edge_term are only read when std or var is among aggr[].
 */
typedef struct pna_segreduce_bwd_args {
  uint32_t struct_size;    /* sizeof(pna_segreduce_bwd_args) of the CALLER's header (ABI 19): a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* rowptr;
  const int32_t* col; /* nullable: x edge-resident */
  int32_t V;
  int32_t F;
  const float* x;
  int64_t ldx;
  const float* dst_term;
  int64_t ld_dst;
  const float* edge_term;
  int64_t ld_edge;
  int32_t n_tower;
  int32_t n_aggr;
  int64_t tower_stride_in;
  int32_t aggr[PNA_MAX_AGGR];
  const float* gagg;
  int64_t ld_g;
  int64_t tower_stride_g;
  const float* mean;
  const float* stdv;
  const float* var;
  int64_t ld_stat;
  int64_t tower_stride_stat;
  const int32_t* argmax;
  const int32_t* argmin;
  int64_t ld_arg;
  float* grad_x;
  int64_t ld_gx;
  float* grad_dst;
  int64_t ld_gd;
  float* grad_edge;
  int64_t ld_ge;
  int32_t heavy_threshold;
  int32_t seg_len;
  int32_t n_heavy;
  int32_t n_seg;
  const int32_t* heavy_rows;
  const int32_t* heavy_segptr;
  const int32_t* seg_heavy;
  const int32_t* stat_row_of;  /* nullable [V] (pna_segreduce_bwd_rowprep_f32 / _pull_f32 only): mean / stdv / var / argmax / argmin hold node
                                * v's values in row stat_row_of[v] -- a forward that wrote them in a degree plan's row order */
  const int32_t* stat_node_of; /* nullable [stat_rows], the inverse map (takes precedence): the rowprep pass then WALKS the statistics' rows in
                                * their own order -- row r belongs to node stat_node_of[r], < 0 = a padding row -- and touches the per-node
                                * tensors (gagg, the table) at node rows: sequential reads of the big tensors, every node exactly once */
  int64_t stat_rows;
} pna_segreduce_bwd_args;

int pna_segreduce_bwd_f32(const pna_segreduce_bwd_args* args, pna_stream_t stream);

/*
 * Pull formulation of the same backward for messages WITHOUT a per-edge term (m_k = x[col_k] + dst_term[v]):
 *     dL/dm_k = R1[v] + R2[v] * x[col_k] + [k = argmax] G_max[v] + [k = argmin] G_min[v]
 *     R2 = (G_var + G_std / (2 std)) [var > 0] (2/D),   R1 = G_mean/D + G_sum + R2 * (dst_term[v] - mean[v])
 * so grad_x[u] = sum_{out-edges (u,v)} R1[v] + x[u] * sum_{out-edges} R2[v] + the max/min terms: the two sums are
 * pna_segreduce_fwd_f32 ("sum", 2 * n_tower towers) over the TRANSPOSED graph on the table written by
 * pna_segreduce_bwd_rowprep_f32 -- table[v] = [R1 (n_tower*F) | R2 (n_tower*F, only if std/var is among aggr[])] --
 * and pna_segreduce_bwd_argscatter_f32 adds the max/min terms with V*n_tower*F atomics each (instead of one atomic
 * per edge and feature).  rowprep also writes grad_dst[v] = D*(G_mean/D + G_sum) + G_max + G_min when grad_dst != NULL
 * (the variance term sums to zero over a row).  Same args struct; fields the formulation does not need are ignored.
 */
int pna_segreduce_bwd_rowprep_f32(const pna_segreduce_bwd_args* args, float* table, int64_t ld_table, pna_stream_t stream);
int pna_segreduce_bwd_argscatter_f32(const pna_segreduce_bwd_args* args, pna_stream_t stream);

/* ABI 16: the same gradient with the max / min terms INSIDE the pull -- no atomics except for the segments of hub SOURCE rows.
 * After pna_segreduce_bwd_rowprep_f32 (table = [R1 | R2]) -- or with run_rowprep set, instead of it:
 *   grad_x[u] = sum over out-edges (u -> v), the k-th in-edge of v, of  R1[v] + [k = argmax[v] - rowptr[v]] G_max[v] + [k = argmin[v] - rowptr[v]] G_min[v]
 *               + x[u] * sum R2[v]
 * base: rowptr (forward CSR), argmax / argmin, gagg / aggr[] (max, min and std or var among them), n_tower, F, V, x (the source
 * table) and grad_x (n_src rows; rows of hub sources -- work-list records with slot >= 0 -- must be ZERO on entry, every other row is
 * overwritten).  col_t / rank_t: destination v and in-list rank k of every edge of the TRANSPOSED CSR (edges sorted by source);
 * items_t: its work list {source row, beg, end, slot} (slot < 0: whole row; slot >= 0: a segment, added atomically).  ranks:
 * workspace (V, ld_rank >= 2 T F) of uint16 -- in-degrees up to 65534.  4 <= F <= 256.  * PACKED rows (round 4): with run_rowprep != 0, ld_table >= 5 T F and ranks == (uint16_t*)(table + 4 T F), the rowprep pass also
 * copies G_max | G_min to table[v][2 T F .. 4 T F) and the pull reads ONE contiguous row [R1 | R2 | G_max | G_min | ranks] per
 * out-edge (12 cache lines at F = 75 with a 1536-byte pitch instead of ~14.7 for three separate pieces); ld_rank then = 2 ld_table.
 * IN PLACE: packed rows with base->gagg == table, one tower and base->aggr[] = {mean, std, max, min} (ld_g == ld_table): the caller's
 * d agg contraction has written [G_mean | G_std | G_max | G_min] straight into the rows; rowprep overwrites the first two blocks
 * with R1 | R2 and copies nothing.
 */
typedef struct pna_segreduce_bwd_pull_args {
  uint32_t struct_size;    /* sizeof(pna_segreduce_bwd_pull_args) of the CALLER's header (ABI 19): a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const pna_segreduce_bwd_args* base;
  const float* table;
  int64_t ld_table;
  const int32_t* col_t;
  const int32_t* rank_t;
  const int32_t* items_t;
  int32_t n_items_t;
  int32_t run_rowprep;   /* != 0: `table` is a WORKSPACE; the call runs the rowprep pass itself (table, base->grad_dst and the ranks in one sweep) */
  uint16_t* ranks;
  int64_t ld_rank;
  /* round 6 (ABI 21), optional: the pull over PER-EDGE rows.  edge_rows != NULL: a (n_edges, ld_edge >= F) workspace; the call first walks the
   * FORWARD work list `items` (n_items records {row, beg, end, slot}, pna_segreduce_args.work_items) and writes, in CSR order,
   *     P[e] = R1[v] + [e = argmax[v]] G_max[v] + [e = argmin[v]] G_min[v]        and R2[v] into table (V, ld_table >= F),
   * then pulls per out-edge P[pos_t[j]] and R2[col_t[j]] (pos_t: position of every transposed edge in the forward CSR): 2 x 4F bytes per
   * edge instead of 20F + ranks; the same additions in the same order: bit-identical gradients.  One tower, no dst_term, aggr[] = mean, std,
   * max, min (any order); rank_t / ranks / run_rowprep are not used. */
  float* edge_rows;
  int64_t ld_edge;
  const int32_t* pos_t;
  const int32_t* items;
  int32_t n_items;
  int32_t _pad_e;
} pna_segreduce_bwd_pull_args;
int pna_segreduce_bwd_pull_f32(const pna_segreduce_bwd_pull_args* args, pna_stream_t stream);

/*
 * Per-row degree scalers of the DGL variant -- models/dgl/scalers.py:12-19 evaluated with the
 * reference's exact fp32 rounding sequence (np.log in float64, rounded to fp32, then
 * Tensor.__rtruediv__ = reciprocal()*scalar for amplification and a true division for attenuation):
 *     amp[v] = fl32( fl32(1/avg_log) * fl32(log(D_v + 1)) ),   att[v] = fl32( avg_log / fl32(log(D_v + 1)) )
 * with D_v = rowptr[v+1]-rowptr[v].  Rows with D_v = 0 get amp = 0, att = 0 (their aggregates are 0).
 * amp / att nullable.
 */
int pna_degree_scalers_f32(const int32_t* rowptr, int32_t V, float avg_log, float* amp, float* att,
                           pna_stream_t stream);

/*
 * Post-aggregation tower contraction on the fp32 matrix cores -- replaces the `posttrans` nn.Linear
 * applied to the concatenated [self | scaler-major aggregate] row (models/dgl/pna_layer.py:65-68,
 * :206; models/pytorch/pna/layer.py:47-48) WITHOUT materialising the (V, A*S*F) operand, and -- in
 * eval mode -- the elementwise tail that follows it (graph-norm :71-72, BatchNorm with running stats
 * :73-74 / :209-210, ReLU :211, residual :212-213):
 *     z[v]  = bias + W_self . h[v] + sum_s row_scale[s][v] * ( W_s . a[v] )
 *     y[v]  = residual[v] + act( (z[v] * row_post[v]) * col_scale + col_shift )
 * where `a` is the (M, K = n_aggr*F)-wide identity-scaler output of pna_segreduce_fwd_f32 and W_s the
 * column block of the reference weight that multiplies scaler s; row_post / col_scale+col_shift /
 * relu / residual are each optional (NULL / 0 = skipped).  Uses v_mfma_f32_16x16x4_f32 (exact fp32
 * products, fp32 accumulate).  K >= 4 and (when h is given) Kh >= 4: narrower operands are padded with zero
 * columns by the caller (pna_amd/functional.py does).
 *
 * The weight is consumed in a packed, zero-padded tile image produced once per weight update by
 * pna_posttrans_pack_f32 from the reference layout: w_ref is the nn.Linear weight, (N, ldw_ref)
 * row-major, input columns ordered [h (Kh) | scaler 0 (K) | scaler 1 (K) | ...] exactly as the
 * reference concatenates them (pna_layer.py:48-49,:65).  pna_posttrans_packed_floats returns the
 * number of floats of w_img (and of wh_img through *wh_floats).
 */
int64_t pna_posttrans_packed_floats(int32_t K, int32_t N, int32_t n_scaler, int32_t Kh, int64_t* wh_floats);
int pna_posttrans_pack_f32(const float* w_ref, int64_t ldw_ref, int32_t N, int32_t K, int32_t n_scaler, int32_t Kh,
                           float* w_img, float* wh_img /* nullable when Kh == 0 */, pna_stream_t stream);

typedef struct pna_posttrans_args {
  uint32_t struct_size;    /* sizeof(pna_posttrans_args) of the CALLER's header (ABI 19): a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const float* a;   /* (M, lda), K columns used */
  int64_t lda;
  int32_t M;
  int32_t K;
  int32_t N;
  int32_t n_scaler; /* 1..5 */
  const float* row_scale[PNA_MAX_SCALER]; /* each [M] or NULL = identity */
  const float* w_img;  /* packed aggregate weight */
  const float* h;      /* nullable (M, ldh): the node's own features (tower variant) */
  int64_t ldh;
  int32_t Kh;
  int32_t relu;        /* activation after the affine column map: 0 = none, 1 = ReLU, 2 = LeakyReLU (act_slope) */
  const float* wh_img; /* packed self weight (when h != NULL) */
  const float* bias;   /* nullable [N] */
  const float* row_post;  /* nullable [M]: graph-norm factor snorm_n */
  const float* col_scale; /* nullable [N]: gamma / sqrt(running_var + eps)            (eval BatchNorm) */
  const float* col_shift; /* nullable [N]: beta - running_mean * col_scale            (with col_scale) */
  const float* residual;  /* nullable (M, ld_res): added after the activation */
  int64_t ld_res;
  float* y;            /* (M, ldy), N columns */
  int64_t ldy;
  int32_t pipeline;    /* pna_posttrans_x3_f32 only: 0 = library default; 2 = two weight buffers in LDS, one barrier at every
                          chunk boundary; 3 = three weight buffers, one barrier in the middle of every chunk (wavefronts
                          cross chunk boundaries unsynchronised).  Same arithmetic, bit-identical results. */
  float act_slope;     /* relu == 2: LeakyReLU, act(v) = v < 0 ? act_slope * v : v (the FCLayer 'LeakyReLU' of the tower layers'
                          mixing network, models/layers.py:157, slope 0.01); ignored for relu == 0 / 1 */
  /* Towers (models/dgl/pna_layer.py:133-139 runs the towers' posttrans one after the other): n_tower > 1 evaluates n_tower
   * independent contractions of the same shape in ONE call.  Tower t reads a + t*tower_stride_a and h + t*tower_stride_h
   * (0 = all towers share h), the images w_img + t*tower_stride_w / wh_img + t*tower_stride_wh (floats for pna_posttrans_f32,
   * BYTES for pna_posttrans_x3_f32: t-th image of a buffer of n_tower images packed one after the other), bias / col_scale /
   * col_shift + t*N, and writes y + t*tower_stride_y (column slices of one row-major matrix).  row_scale / row_post are shared;
   * residual must be NULL.  n_tower <= 1: one contraction, strides ignored. */
  int32_t n_tower;
  int32_t _pad_t;
  int64_t tower_stride_a;
  int64_t tower_stride_h;
  int64_t tower_stride_w;
  int64_t tower_stride_wh;
  int64_t tower_stride_y;
  /* Degree-grouped rows (ABI 9, pna_posttrans_x3_f32 only; NULL = off).  Every PNA scaler is a function of the in-degree
   * alone (models/dgl/scalers.py:7-19), so for the rows of ONE degree D the three scaler blocks of the posttrans weight
   * collapse into one:  sum_s scale_s(D) (W_s a) = (sum_s scale_s(D) W_s) a  -- a third of the multiply-adds.  The caller
   * orders the rows by degree: `a`, `row_scale[]`, `row_post` are indexed by a VIRTUAL row v in [0, M) (M a multiple of the
   * workgroup tile R = 128 rows for n_scaler = 1, 192 for n_scaler = 3: every degree group padded to whole tiles), row_perm[v] is
   * the row of `y` / `residual` that virtual row v is (or -1: padding, nothing is stored), and tile t (virtual rows [R t, R t + R)) multiplies by the weight image number
   * tile_image[t] of a buffer of images packed one after the other, image_stride BYTES apart (pna_posttrans_x3_pack_f32 of a
   * (G * 80, K) matrix whose rows [80 g, 80 g + N) are group g's combined weight: G column blocks = G images).  tile_image
   * NULL: every tile uses w_img as it is (the rows no group holds, with their per-row scalers: n_scaler = 3).
   * Needs N <= 80 (one 80-column block whatever N: the grouped kernel is bound by its A stream, not by the matrix pipe), no h
   * panel, n_tower <= 1, n_scaler 1 or 3 -- or 80 < N <= 128 with n_scaler = 1 (one 128-column
   * block; its images are packed one by one, pna_posttrans_x3_pack_f32 of a (128, K) matrix each, image_stride =
   * pna_posttrans_x3_packed_bytes(K, 128, 1, 0); the caller sends the rows no group holds through an ordinary call).
   * pna_segreduce_args.work_items (row = output row) and heavy_out_rows write the aggregate in that virtual order in the
   * first place. */
  const int32_t* row_perm;
  const int32_t* tile_image;
  int64_t image_stride;
} pna_posttrans_args;

int pna_posttrans_f32(const pna_posttrans_args* args, pna_stream_t stream);

/* ---- the same contraction on the bf16 matrix pipe at fp32 accuracy ("bf16x3") ---------------------
 *
 * Same operation, arguments and epilogue as pna_posttrans_f32 (n_scaler <= 3).  Every fp32 operand is
 * cut exactly into three bf16 terms (8+8+8 mantissa bits, by truncation) and each product is evaluated
 * as its six partial products of weight >= 2^-16, accumulated in fp32 by v_mfma_f32_16x16x32_bf16; the
 * dropped partial products are below 2^-23 of the product (the size of one fp32 rounding).  Inputs and
 * outputs stay fp32; results agree with pna_posttrans_f32 to fp32 summation-order noise.
 * Non-finite operands: NaN propagates; a +-Inf in `a` / `h` / the weight keeps its row's results +-Inf / NaN exactly as
 * in pna_posttrans_f32 when the other operand's three bf16 terms are all non-zero (any generic fp32 value), and gives
 * NaN instead of +-Inf where the other operand is exactly bf16-representable (its residual terms are 0: Inf * 0) --
 * non-finite wherever the fp32 contraction is non-finite, never finite garbage (before the ReLU of the epilogue,
 * which maps -Inf to 0 but keeps NaN).  Subnormal bf16 terms (operands below 2^-126, residual terms of operands below
 * ~2^-110) may be flushed by the matrix pipe: an absolute error of at most 2^-126 * |other operand| per product.
 * tests/test_gpu_posttrans_x3.py pins all of this (mixed 1e-20..1e20 magnitudes, cancellation between scaler blocks,
 * K = 900 equal-sign sums, subnormals, single infinities).  w_img / wh_img of the args are the images made by pna_posttrans_x3_pack_f32 (a
 * different format from pna_posttrans_pack_f32's; sizes in BYTES from pna_posttrans_x3_packed_bytes).
 */
int64_t pna_posttrans_x3_packed_bytes(int32_t K, int32_t N, int32_t n_scaler, int32_t Kh, int64_t* wh_bytes);
int pna_posttrans_x3_pack_f32(const float* w_ref, int64_t ldw_ref, int32_t N, int32_t K, int32_t n_scaler, int32_t Kh,
                              void* w_img, void* wh_img /* nullable when Kh == 0 */, pna_stream_t stream);
int pna_posttrans_x3_f32(const pna_posttrans_args* args, pna_stream_t stream);

/* ---- fused PNASimpleLayer forward (inference) -----------------------------------------------------
 *
 * One launch for the whole of models/dgl/pna_layer.py:197-216 with aggregators "mean max min std":
 *   a[v]  = [mean | max | min | std] over in-edges of x[col[e]]          (:168-187, :189-194)
 *   y[v]  = residual[v] + relu((bias + sum_s row_scale[s][v] * (W_s . a[v])) * col_scale + col_shift)
 * The (V, 4F) aggregate never reaches HBM: it is built per 32-row tile in LDS and contracted from there.
 * w_img is the pna_posttrans_pack_f32 image of the Linear weight re-laid with each aggregator block
 * zero-padded from F to B4 = round_up(F, 4) input columns (K = 4*B4 per scaler, Kh = 0).
 * Rows with degree > heavy_threshold (0 = never) are reduced by the whole workgroup.
 * Supported: 4 <= F <= 80, N <= 80, n_scaler <= 3.  Same numerics as the two-kernel path except for the
 * summation order over hub rows' edges and over k (tolerance-level, not bit-level, agreement).
 */
typedef struct pna_fused_simple_args {
  uint32_t struct_size;    /* sizeof(pna_fused_simple_args) of the CALLER's header (ABI 19): a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* rowptr; /* [V+1] CSR by destination */
  const int32_t* col;    /* [E] source row of x per edge */
  const float* x;        /* (x_rows, ldx) source features */
  int64_t ldx;
  int32_t V;
  int32_t F;
  int32_t N;
  int32_t n_scaler;
  const float* row_scale[PNA_MAX_SCALER]; /* each [V] or NULL = identity */
  const float* w_img;
  const float* bias;      /* nullable [N] */
  const float* col_scale; /* nullable [N] */
  const float* col_shift; /* nullable [N] (with col_scale) */
  const float* residual;  /* nullable (V, ld_res) */
  int64_t ld_res;
  float* y;               /* (V, ldy) */
  int64_t ldy;
  int32_t relu;
  int32_t heavy_threshold;
} pna_fused_simple_args;

int pna_fused_simple_f32(const pna_fused_simple_args* args, pna_stream_t stream);

/* ---- PNASimpleLayer forward on degree-ordered rows: gather + scalers + posttrans in ONE kernel (ABI 10) ------------------
 *
 * Replaces, for inference on large graphs, the whole of models/dgl/pna_layer.py:197-216 with aggregators "mean max min std"
 * (reduce_func :189-194, posttrans :206, BatchNorm :209-210, ReLU :211, residual :212-213).  The (V, 4F) aggregate -- the
 * reference materialises (V, 12F) -- never reaches HBM.  Every PNA scaler is a function of the destination's in-degree alone
 * (models/dgl/scalers.py:7-19), so all rows of one in-degree D share ONE combined weight  W_D = sum_s scale_s(D) W_s :
 *
 *   a[v]        = [mean | max | min | std] over the in-edges of x[src]                     (bit-identical to pna_segreduce_fwd_f32
 *                                                                                             for rows one lane group walks alone)
 *   y[perm[v]]  = residual[perm[v]] + act((bias + W_D(v) . a[v]) * col_scale + col_shift)   (fp32 in and out, fp32 accumulation; see ARITHMETIC)
 *
 * ARITHMETIC (`arith`, ABI 21).  PNA_FD_ARITH_X3: every statistic and every weight as three bf16 terms, six partial products (the bf16x3
 * arithmetic of pna_posttrans_x3_f32, rounds 3-4): componentwise fp32-accurate for operands of any dynamic range.  PNA_FD_ARITH_H2 (round 5):
 * TWO fp16 terms, x = h0 + h1 + r with h0 = fp16(x), h1 = fp16(x - h0) (round to nearest), and three partial products (h1 w0, h0 w1, h0 w0;
 * v_mfma_f32_16x16x32_f16, fp32 accumulation): half the matrix instructions and two thirds of the weight stream.  fp16's range is narrow, so
 * the operands are first multiplied by powers of two (exact): row v's statistics by 2^s(v), chosen in the kernel so that twice the row's
 * largest message magnitude lies in [2^14, 2^15), and column n of the weights by 2^t(n), chosen by the pack function from the largest
 * |W_D[n][k]| over k and over all images into [2^13, 2^14) (2^-t(n) rides in each image's tail); the accumulator is multiplied by 2^-(s + t)
 * in the bias' fma.  In these units |r| <= max(2^-22 |x|, 2^-25): an operand below 2^-3 -- more than 2^17 below its row's (2^16 below its
 * column's) bound -- sits on fp16's subnormal grid with its second term and carries an ABSOLUTE error of up to 2^-25, a relative one of
 * 2^-25 / |x|: the form is normwise-, not componentwise-accurate (a statistic 1e7 x the rest of its row with a zero weight on it: 5.6e-5
 * relative on the outputs; at 1e13 the small statistics vanish).  PNA_FD_ARITH_GUARDED (the default) = the same fp16 x 2 launch with that
 * FLOOR error bounded per output: the kernel adds up the exact floor errors fs(v) of a row's statistics (the part of |r| above 2^-22 |x|;
 * zero for almost every row), the pack function those of a column's weights fw(n), and an output is certified when
 *     |acc| >= 2^34 fs(v) + 2^35 fw(n)          (floor error <= 2^-20 |acc|: everything else of the split's error is relative term by term);
 * a 64-row (wide shapes: 64-row) workgroup tile with an uncertified output is appended to a device-side list and a second launch computes
 * exactly those tiles again in bf16 x 3 (no host round trip; on Gaussian features and weights nothing is handed over, the launch finds an
 * empty list and costs ~6 us; rows without in-edges outside tower mode have exact zeros for operands and certify themselves).  In tower mode the row's scale also covers its own x_dst / h_self strips: it is lowered when they arrive,
 * mid-row, and the accumulator with it (exact).  Measured against float64 on BASELINE configs[2] / [4] shapes: 1.25 x the error of bf16x3, a
 * fifth of an fp32 GEMM's.
 * Non-finite operands: NaN propagates; a row that holds an infinite statistic (column: an infinite weight) is non-finite in every output
 * it reaches, as in fp32 -- but its FINITE elements are scaled against FLT_MAX and may underflow, so where fp32 gives +-Inf the result
 * may be +-Inf or NaN, never finite garbage (such rows are not the guard's: a non-finite accumulator certifies itself).
 *
 * The caller (pna_amd/degree_groups.py) orders the rows by in-degree into VIRTUAL rows v in [0, M):
 *   row_perm[v]   node of virtual row v, or -1 = padding (nothing is stored); M a multiple of pna_fused_degree_tile_rows(F, N) (64 or 128); every aligned block of 16
 *                 virtual rows holds rows of ONE in-degree (padding aside), every aligned block of 64 rows uses ONE weight image;
 *   tile_desc     [M / 16][4] = {first record, in-degree D, weight image, 0} of every 16-row block;
 *   tile_ids      n_records records of 16 int32: record (first + e)[i] = source row (row of x) of the e-th in-edge of the block's
 *                 i-th row, e in [0, D), in the row's edge order; a padding row repeats the block's first row; a block owns
 *                 max(4, round_up(D, 4)) records, the ones past D being copies of record D - 1 (D = 0: any valid row) -- they
 *                 feed the id prefetch and never the sums; for D > 4 their rows are not requested (the block's first row aside);
 *                 D is ANY in-degree >= 0 -- the degrees of a tile's four (eight) blocks may all differ, and nothing ties D to the
 *                 caller's hub threshold: the only limit is n_records < 2^26 (tests/test_gpu_fused_degree_plans.py pins D = 0 .. 9,
 *                 12, 13, 16, 17, 31 .. 33, 127 .. 129 and 300, one degree per tile and four per tile);
 *   w_img         n_img images, image_stride == pna_fused_image_bytes(F, N, tower, 0) bytes apart (the pack function's layout), from pna_fused_pack_f32
 *                 (w_img_x3 / image_stride_x3: the bf16 x 3 images, x3 = 1):
 *                 w_ref is the Linear weight (N, n_scaler * 4F) in the reference's column order [scaler][aggregator][feature]
 *                 (pna_layer.py:192-193), scale (n_img, n_scaler) the scalers' values for image i (NULL with n_scaler = 1:
 *                 the weight itself); W_D is formed in fp32 in scaler order, like the reference's blocks.
 * x: (x_rows, ldx) rows, 4-byte aligned, any ldx >= F (a contiguous (x_rows, F) table included: no read leaves a row's F floats),
 * x_rows < 2^32, ldx < 2^29; y and residual: n_nodes rows, each table < 4 GiB.
 * F in 17..80, or (ABI 15; 97..112 since ABI 21) 97..128 -- the features in two gather passes (BASELINE configs[4]: 128 -> 128);
 * N in 4..80, or (ABI 15) 81..128 -- the output columns in two panels of 64 (needs F in 49..64 or 97..128).  pna_fused_degree_image_bytes(F, N) > 0
 * is the authoritative test.
 * relu: 0 none / 1 ReLU / 2 LeakyReLU(act_slope).  agg_out (nullable): (M, ld_agg) receives the
 * statistics the contraction consumed, [mean | max | min | std] x F per virtual row (verification; a slower instantiation).
 * Rows of degrees too rare to fill a tile, and hub rows, are the caller's: pna_segreduce_fwd_f32 + pna_posttrans_x3_f32 over
 * their compact list.
 *
 * TOWER MODE (ABI 13; x_dst, h_self and row_post non-null together): PNALayer.forward with ONE tower, 1-layer pretrans / posttrans,
 * no edge features (models/dgl/pna_layer.py:33-76, :130-145), inference.  The pretrans Linear of [h_u | h_v] is x_src[u] + x_dst[v]
 * (two node-level projections, the caller's): x = x_src, and with a[v] the statistics of x_src over the in-edges as above
 *
 *   y[perm[v]] = residual + act(((bias + W_D . a[v] + [deg > 0] (W_D,mean + W_D,max + W_D,min) . x_dst[perm[v]] + W_self . h_self[perm[v]])
 *                                 * row_post[v]) * col_scale + col_shift)
 *
 * -- mean / max / min of (a_u + b) are those of a_u plus b (max / min: the same bits, rounding is monotone), the std does not see
 * the shift.  x_dst, h_self: (n_nodes, ld) tables in node order under x's alignment rules; row_post: [M] in VIRTUAL row order
 * (graph norm; ones without); residual additionally 16-byte aligned with ld_res % 4 == 0.  49 <= F <= 80.  The images come from
 * pna_fused_tower_pack_f32: w_ref (N, n_scaler * 5F) in scaler blocks [4F aggregators | F self panel (block 0 only)] -- the
 * posttrans Linear with its h columns moved behind the first block, or posttrans . BatchNorm . mixing Linear collapsed into one
 * weight (pna_amd/functional.py::_tower_collapsed_weights).  No agg_out in this mode.
 */
typedef struct pna_fused_degree_args {
  uint32_t struct_size;    /* sizeof(pna_fused_degree_args) of the CALLER's header (ABI 19): a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* tile_desc;
  const int32_t* tile_ids;
  int64_t n_records;
  const float* x;
  int64_t ldx;
  int64_t x_rows;
  int32_t F;
  int32_t N;
  const int32_t* row_perm;
  int64_t M;
  int64_t n_nodes;        /* rows of y / residual */
  const void* w_img;
  int64_t image_stride;
  const float* bias;      /* nullable [N] */
  const float* col_scale; /* nullable [N] */
  const float* col_shift; /* nullable [N] (with col_scale) */
  const float* residual;  /* nullable (n_nodes, ld_res), node order */
  int64_t ld_res;
  float* y;               /* (n_nodes, ldy), node order */
  int64_t ldy;
  int32_t relu;
  float act_slope;
  float* agg_out;         /* nullable (M, ld_agg) */
  int64_t ld_agg;
  const float* x_dst;     /* tower mode (ABI 13): (n_nodes, ld_xdst) */
  int64_t ld_xdst;
  const float* h_self;    /* (n_nodes, ld_h) */
  int64_t ld_h;
  const float* row_post;  /* [M], virtual row order */
  int32_t spare_workgroups; /* ABI 17: workgroups to leave OUT of the launch (0: two per CU, the whole device).  The kernel is
                             * persistent and books every register of a CU, so launches on another stream wait until it retires;
                             * with a few workgroups left out they run beside it (the caller's rest-row launches: DESIGN.md 4.8.9). */
  int32_t _pad4;
  int32_t* tile_counter;  /* ABI 20, nullable: TWO device int32 the call owns while it runs, ZERO before the first launch (the kernel
                           * leaves them zero: the last workgroup to finish resets them, so back-to-back launches on one stream need
                           * nothing in between).  Non-null: DYNAMIC tile schedule -- a workgroup's first four tiles are b, b + G,
                           * b + 2 G, b + 3 G (G = the launch's grid), every later tile index is 4 G + a claim from the first word,
                           * so a workgroup that falls behind simply takes fewer tiles; tiles are started in tile_desc order
                           * device-wide.  Null: the static schedule b, b + G, b + 2 G, ...  The results do not depend on it
                           * (bit-identical). */
  /* ABI 21 (round 6): the arithmetic of the contraction, see ARITHMETIC above */
  const void* w_img_x3;     /* bf16 x 3 images (pna_fused_pack_f32(.., x3 = 1)), image_stride_x3 == pna_fused_image_bytes(F, N, tower, 1) apart:
                             * PNA_FD_ARITH_GUARDED and PNA_FD_ARITH_X3; w_img / image_stride: the fp16 x 2 images (GUARDED and H2) */
  int64_t image_stride_x3;
  void* guard_ws;           /* PNA_FD_ARITH_GUARDED: pna_fused_degree_guard_bytes(M) bytes, 16-byte aligned, owned by the call while it runs, its first 16
                             * bytes ZERO before the first launch (the library leaves words 0..1 zero behind every call).  int32 words: [0] tiles
                             * handed over by the running call, [1] internal, [2] tiles handed over since the caller last zeroed it, [3] calls */
  int64_t guard_ws_bytes;
  int32_t arith;            /* PNA_FD_ARITH_GUARDED (0, the default) | PNA_FD_ARITH_X3 | PNA_FD_ARITH_H2 */
  int32_t _pad5;
  const float* pre_add;     /* tower mode, nullable: (n_nodes, ld_pre_add) rows, node order, added to the biased accumulator IN FRONT of the row factor:
                             *   y = residual + act(((bias + W_D . a + .. + pre_add[perm[v]]) * row_post[v]) * col_scale + col_shift)
                             * -- a PNALayer of T towers over the whole input (divide_input=False, models/dgl/pna_layer.py:137-139) is T launches, one per
                             * tower's 75 message features, the partial sums carried from launch to launch; only the last one applies bias / row factor /
                             * BatchNorm / activation / residual.  pre_add must NOT alias y under PNA_FD_ARITH_GUARDED: the second launch computes
                             * a handed-over tile again from the same pre_add rows.  Also taken by the layer proper (with row_post as its
                             * optional row factor): a layer in feature panels, FusedMultiTowerCall's launches */
  int64_t ld_pre_add;
  int32_t y_cols_writable;  /* 0 (= N), or N <= y_cols_writable <= min(ldy, 16 ceil(N / 16)): the columns of a row of y the kernel may WRITE; the ones
                             * behind N receive zeros.  With the padding of its own output buffer writable, a row of N = 75 floats is ten whole
                             * 32-byte sectors (no partially written sector for the memory side to complete by reading it first) and the row's last
                             * window one 16-byte store instead of three scalar ones.  Never set it for a y that is a view of wider rows. */
  int32_t _pad6;
} pna_fused_degree_args;

#define PNA_FD_ARITH_GUARDED 0 /* fp16 x 2 with the floor-error guard: tiles it cannot certify are computed again in bf16 x 3 (a second launch) */
#define PNA_FD_ARITH_X3 1      /* bf16 x 3 everywhere: componentwise fp32-accurate for operands of any dynamic range (rounds 3-4) */
#define PNA_FD_ARITH_H2 2      /* fp16 x 2 without the guard (round 5): operands of moderate dynamic range only; the verification instantiation */
int64_t pna_fused_image_bytes(int32_t F, int32_t N, int32_t tower, int32_t x3);   /* bytes of one image = the stride between images; 0 = unsupported shape */
int pna_fused_pack_f32(const float* w_ref, int64_t ldw_ref, int32_t N, int32_t F, int32_t n_scaler, const float* scale, int32_t n_img, void* img,
                       int32_t tower, int32_t x3, pna_stream_t stream);          /* the images of either arithmetic, layer or tower mode */
int64_t pna_fused_degree_guard_bytes(int64_t M);               /* size of pna_fused_degree_args.guard_ws for M virtual rows */
int64_t pna_fused_degree_image_bytes(int32_t F, int32_t N);   /* = pna_fused_image_bytes(F, N, 0, 0); 0 = unsupported shape */
int32_t pna_fused_degree_tile_rows(int32_t F, int32_t N);     /* rows of a workgroup tile for the shape (M must be a multiple; all of
                                                                  one degree and one weight image): 64, or 128 for the wide shapes when the
                                                                  library runs them as 8-wavefront workgroups; 0 = unsupported shape */
int pna_fused_degree_pack_f32(const float* w_ref, int64_t ldw_ref, int32_t N, int32_t F, int32_t n_scaler, const float* scale,
                              int32_t n_img, void* img, pna_stream_t stream);
int pna_fused_degree_f32(const pna_fused_degree_args* args, pna_stream_t stream);
int64_t pna_fused_tower_image_bytes(int32_t F, int32_t N);    /* 0 = unsupported shape */
int pna_fused_tower_pack_f32(const float* w_ref, int64_t ldw_ref, int32_t N, int32_t F, int32_t n_scaler, const float* scale,
                             int32_t n_img, void* img, pna_stream_t stream);

/* ---- the tower layer of molecule-sized batches: one call, two launches (BASELINE.json configs[1]) -------------------
 *
 * At ~3 k nodes / ~6 k edges per batch the layer is bound by launch and load LATENCY, so the work is cut by destination rows
 * instead of by operator (pna_tower_fused.hip).  pna_tower_layer_f32 evaluates, in eval mode, all of
 * models/dgl/pna_layer.py:133-148 (PNALayer.forward) with 1-layer pretrans / posttrans and no edge features:
 *   launch 1   x_cat[v] = [ W_a,t h_t[v] | W_b,t h_t[v] + b_t ]_t          the pretrans Linear(2 Fi -> Fi) of every tower,
 *                                                                          factorised to node level (:35-40)
 *   launch 2   per 16 destination rows, never leaving the CU:
 *              a_t[v]   = [mean | max | min | std] over in-edges (u -> v) of x_src,t[u] + x_dst,t[v]      (:42-56)
 *              z_t[v]   = ((b_t + W_h,t h_t[v] + sum_s row_scale[s][v] (W_s,t a_t[v])) * row_post[v]) * col_scale + col_shift   (:65-74)
 *              y[v]     = residual[v] + act(W_mix [z_0 .. z_T-1][v] + b_mix)                               (:141-147)
 *   (mix_img == NULL: y = [z_0 .. z_T-1], the plain concatenation; PNATower on its own.)
 * h_t = h[:, t*Fi .. (t+1)*Fi) when divide_input, else all of h (then Fin = Fi).  Exact fp32 products on
 * v_mfma_f32_16x16x4_f32; the aggregation is the light-row arithmetic of pna_segreduce_fwd_f32 (edge order, s / D correctly
 * rounded), for every row whatever its degree; results agree with the large-graph path to fp32 summation-order noise.
 * Aggregators are fixed to mean|max|min|std, n_scaler <= 3.  Returns PNA_E_INVALID when one tower's 16-row tile does not fit
 * the LDS (Fi > ~570): callers use the large-graph kernels then.
 *
 * Weight images (made once per weight update):
 *   pna_small_pack_f32       a Linear weight (N, K) for pna_small_linear_f32: proj_img = pack of [W_a ; W_b] (2*T*Fi, Fin)
 *                            (block-diagonal in Fin when divide_input), mix_img = pack of the mixing weight (No, T*Fo)
 *   pna_tower_post_pack_f32  ONE tower's posttrans weight (Fo, Fi + n_scaler*4*Fi) in the reference's column order
 *                            [h | scaler 0: mean max min std | scaler 1 ...] (:65); post_img = the T images one after the other,
 *                            each pna_tower_post_packed_floats(Fi, Fo, n_scaler) floats
 * pna_small_linear_f32 is launch 1 on its own: y = residual + act(x W^T + bias) for row counts where a library GEMM is
 * launch-bound; any M, K <= 2500.
 */
int64_t pna_small_packed_floats(int32_t N, int32_t K);
int pna_small_pack_f32(const float* w_ref, int64_t ldw_ref, int32_t N, int32_t K, float* img, pna_stream_t stream);

typedef struct pna_small_linear_args {
  uint32_t struct_size;    /* sizeof(pna_small_linear_args) of the CALLER's header (ABI 19): a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const float* x;        /* (M, ldx), K columns used */
  int64_t ldx;
  int32_t M;
  int32_t K;
  int32_t N;
  int32_t act;           /* 0 = none, 1 = ReLU, 2 = LeakyReLU(act_slope) */
  const float* img;      /* pna_small_pack_f32 image of the (N, K) weight */
  const float* bias;     /* nullable [N] */
  float act_slope;
  int32_t _pad;
  const float* residual; /* nullable (M, ld_res): added after the activation */
  int64_t ld_res;
  float* y;              /* (M, ldy) */
  int64_t ldy;
} pna_small_linear_args;

int pna_small_linear_f32(const pna_small_linear_args* args, pna_stream_t stream);

int64_t pna_tower_post_packed_floats(int32_t Fi, int32_t Fo, int32_t n_scaler);
int pna_tower_post_pack_f32(const float* w_ref, int64_t ldw_ref, int32_t Fi, int32_t Fo, int32_t n_scaler, float* img,
                            pna_stream_t stream);

typedef struct pna_tower_layer_args {
  uint32_t struct_size;    /* sizeof(pna_tower_layer_args) of the CALLER's header (ABI 19): a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* rowptr;  /* [V+1] CSR by destination */
  const int32_t* col;     /* [E] source node per CSR edge */
  int32_t V;
  int32_t n_tower;        /* T */
  int32_t Fi;             /* per-tower input width (= pretrans output width) */
  int32_t Fo;             /* per-tower output width */
  int32_t divide_input;   /* 0: every tower reads all of h (ldh >= Fi); 1: tower t reads columns [t*Fi, (t+1)*Fi) (ldh >= T*Fi) */
  int32_t n_scaler;       /* 1..3 */
  const float* h;         /* (V, ldh) node features */
  int64_t ldh;
  float* x_cat;           /* (V, ldx) workspace, 2*T*Fi columns: written by launch 1, read by launch 2 */
  int64_t ldx;
  const float* proj_img;  /* pna_small_pack_f32 image of [W_a ; W_b] (2*T*Fi, Fin) */
  const float* proj_bias; /* [2*T*Fi] = [0 ; b], nullable */
  const float* row_scale[PNA_MAX_SCALER]; /* each [V] or NULL = identity */
  const float* post_img;  /* T pna_tower_post_pack_f32 images */
  const float* post_bias; /* nullable [T*Fo] */
  const float* row_post;  /* nullable [V]: graph-norm factor */
  const float* col_scale; /* nullable [T*Fo]: eval BatchNorm scale of every tower, concatenated */
  const float* col_shift; /* nullable [T*Fo] (with col_scale) */
  const float* mix_img;   /* nullable: pna_small_pack_f32 image of the mixing weight (No, T*Fo) */
  const float* mix_bias;  /* nullable [No] */
  int32_t No;             /* mixing output width (ignored without mix_img: the output is T*Fo wide) */
  int32_t mix_act;        /* 0 = none, 1 = ReLU, 2 = LeakyReLU(mix_slope) */
  float mix_slope;
  int32_t _pad;
  const float* residual;  /* nullable (V, ld_res): added after the mixing activation */
  int64_t ld_res;
  float* y;               /* (V, ldy) */
  int64_t ldy;
  /* edge features that are an embedding of <= 4 edge types (the molecule nets: pna_net.py `e = self.embedding_e(e)`; the W_e . ef
   * part of the factorised pretrans, models/dgl/pna_layer.py:35-40): message = (W_a h_u + (W_b h_v + b)) + edge_table[edge_type[k]].
   * All NULL / 0: a layer without edge features. */
  const int32_t* edge_type;  /* nullable [E]: type of every CSR edge, 0 <= type < n_edge_types (not checked on the device) */
  const float* edge_table;   /* (n_edge_types, ld_edge_table): row t = W_e . ef_t of every tower, concatenated (n_tower * Fi columns) */
  int64_t ld_edge_table;
  int32_t n_edge_types;      /* 1..4 with edge_type */
  int32_t no_self_panel;     /* != 0: the PNASimpleLayer form (models/dgl/pna_layer.py:197-206: messages are the raw source features, the
                              * posttrans never reads the node's own h): no destination term (the second half of x_cat is not read) and zeros
                              * instead of h against the image's (zero) self block -- so a node whose own feature is Inf / NaN keeps the
                              * finite output the reference gives it instead of 0 * Inf = NaN */
} pna_tower_layer_args;

int pna_tower_layer_f32(const pna_tower_layer_args* args, pna_stream_t stream);
/* Host only.  LDS bytes of pna_tower_layer_f32's tile with ONE tower per pass, the smallest it can run with, by the entry point's own
 * code (it refuses a layer whose smallest tile exceeds 160 KiB); No = the mixing network's output width, 0 without one.  -1 when n_tower,
 * Fi or Fo is below 1 or No is negative. */
int64_t pna_tower_layer_lds_bytes(int32_t n_tower, int32_t Fi, int32_t Fo, int32_t No, int32_t divide_input);

/* ---- weight / bias gradient of the posttrans contraction (round 4) ------------------------------------------
 * replaces: the autograd node of `self.posttrans(torch.cat([h, scaled aggregate], dim=1))` (models/dgl/pna_layer.py:206; the
 * training loop's loss.backward(), realworld_benchmark/train/train_molecules_graph_regression.py:29-32) for the Linear's
 * weight and bias -- rounds 2-3 used the vendor GEMM library here:
 *
 *   grad_w[n, Kh + s K + k] = sum_m row_scale[s][m] gy[m, n] a[m, k]        (row_scale[s] == NULL: 1)
 *   grad_w[n, j]            = sum_m gy[m, n] h[m, j]                        j < Kh
 *   grad_b[n]               = sum_m gy[m, n]                                (grad_b nullable)
 *
 * bf16x3 arithmetic (each fp32 operand cut exactly into three bf16 terms, six partial products, fp32 accumulation per slab of
 * rows, float64 across the slabs in a fixed order: deterministic).  Shapes: 1 <= n_scaler <= 3, N <= 128, n_scaler * N <= 240,
 * K + Kh + 1 <= 384 (pna_posttrans_dw_workspace_bytes returns -1 otherwise: the caller keeps its library route); rows 4-byte
 * aligned; with an h panel or grad_b, row_scale[0] must be NULL (they are formed from the first copy of gy -- the identity scaler
 * comes first in every reference configuration).  Non-finite inputs give NaN in the columns / rows they touch.  workspace: no
 * initialisation needed.
 */
typedef struct pna_posttrans_dw_args {
  uint32_t struct_size;    /* sizeof(pna_posttrans_dw_args) of the CALLER's header (ABI 19): a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const float* gy;         /* (M, ldg): gradient of the contraction's output, N columns */
  int64_t ldg;
  int64_t M;
  int32_t N;
  int32_t n_scaler;
  const float* a;          /* (M, lda): the aggregate the forward multiplied, K columns (identity-scaled) */
  int64_t lda;
  int32_t K;
  int32_t Kh;              /* columns of h (0: no self panel) */
  const float* h;          /* nullable (M, ldh) */
  int64_t ldh;
  const float* row_scale[PNA_MAX_SCALER];  /* each [M] or NULL = identity */
  float* grad_w;           /* (N, ldw): [h panel | scaler block 0 | 1 | 2], the Linear's weight layout */
  int64_t ldw;
  float* grad_b;           /* nullable [N] */
  void* workspace;
  int64_t workspace_bytes; /* >= pna_posttrans_dw_workspace_bytes(M, N, n_scaler, K, Kh) */
} pna_posttrans_dw_args;

int64_t pna_posttrans_dw_workspace_bytes(int64_t M, int32_t N, int32_t n_scaler, int32_t K, int32_t Kh);
int pna_posttrans_dw_f32(const pna_posttrans_dw_args* args, pna_stream_t stream);

/* The same gradient for the rows of a DEGREE PLAN (pna_amd/degree_groups.py: virtual rows in 128-row tiles of one in-degree).  The
 * degree scalers are functions of the in-degree alone (models/dgl/scalers.py:7-19), so with the rows walked in plan order
 *   grad_w block s = sum over degree runs  group_scale[group][s] * sum_{m in run} gy[m]^T a[m]
 * needs one unscaled copy of gy and a third of the multiply-adds; the rows are loaded through row_perm (no packing pass).
 * Covers the plan's group rows only: the caller adds the (few) rest rows' part.  Workgroup w walks tiles [wg_range[2w],
 * wg_range[2w+1]) and writes one partial product per degree run it meets into workspace entries wg_entry[w], wg_entry[w] + 1, ...;
 * entry_group[e] = the degree group of entry e.  N <= 80, K + Kh + 1 <= 384, n_scaler in 1..3. */
typedef struct pna_posttrans_dw_grouped_args {
  uint32_t struct_size;    /* sizeof(pna_posttrans_dw_grouped_args) of the CALLER's header (ABI 19): a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const float* gy;         /* (n_nodes, ldg) */
  int64_t ldg;
  int32_t N;
  int32_t n_scaler;
  const float* a;          /* (n_nodes, lda): aggregate in NODE order, K columns */
  int64_t lda;
  int32_t K;
  int32_t Kh;
  const float* h;          /* nullable (n_nodes, ldh) */
  int64_t ldh;
  const int32_t* row_perm;    /* [128 * n_tiles]: node of every virtual row, -1 = padding */
  const int32_t* tile_group;  /* [n_tiles]: degree group of every 128-row tile, runs of equal values */
  const int32_t* wg_range;    /* [n_workgroups][2] */
  const int32_t* wg_entry;    /* [n_workgroups] */
  int32_t n_workgroups;
  int32_t n_entries;
  const int32_t* entry_group; /* [n_entries] */
  const float* group_scale;   /* [n_groups][n_scaler] */
  float* grad_w;           /* (N, ldw) */
  int64_t ldw;
  float* grad_b;           /* nullable [N] */
  void* workspace;
  int64_t workspace_bytes; /* >= pna_posttrans_dw_grouped_workspace_bytes(N, K, Kh, n_entries) */
  int32_t a_plan_order;    /* != 0: `a` is already in the plan's row order (row r of `a` = virtual row r): read in sequence, not through row_perm */
  int32_t _pad;
} pna_posttrans_dw_grouped_args;

int64_t pna_posttrans_dw_grouped_workspace_bytes(int32_t N, int32_t K, int32_t Kh, int32_t n_entries);
int pna_posttrans_dw_grouped_f32(const pna_posttrans_dw_grouped_args* args, pna_stream_t stream);

/* ---- batching + destination-sorted CSR on the device ----------------------------------
 *
 * Replaces dgl.batch (realworld_benchmark/data/molecules.py:153-164: offset + concatenate the member graphs' edge
 * lists) and the in-edge CSR DGL builds inside update_all (models/dgl/pna_layer.py:64,:202).
 *   global ids:  dst[k] + node_offset[edge_graph[k]]  (same for src; both NULL = ids are already global)
 *   rowptr[V+1], col[E] (source per CSR edge), eid[E] (original edge per CSR edge), row[E] (destination per CSR edge)
 * grouped by destination and STABLE inside a group (the original edge order: DGL's mailbox order).  One radix sort
 * over the bits the node count needs; workspace from pna_collate_workspace_bytes (-1 if a size leaves int32).
 */
int64_t pna_collate_workspace_bytes(int64_t n_edges, int32_t n_nodes);
int pna_collate_csr_i32(const int32_t* src, const int32_t* dst, int64_t n_edges, int32_t n_nodes,
                        const int32_t* edge_graph /* nullable [E] */, const int32_t* node_offset /* nullable [n_graphs] */,
                        int32_t* rowptr, int32_t* col, int32_t* eid, int32_t* row,
                        void* workspace, int64_t workspace_bytes, pna_stream_t stream);

/* ---- halo packing for the destination-sharded multi-GPU path (the reference has no distributed code) ------
 *
 *   out[i, 0:F] = x[idx[i], 0:F]      i in [0, n)
 * One launch packs the feature rows every peer asked for (idx = the peers' request lists, concatenated in peer order) into
 * the contiguous send buffer of the per-layer all-to-all; pna_amd/shard.py is the caller.  Rows need 4-byte alignment only.
 */
int pna_pack_rows_f32(const float* x, int64_t ldx, const int32_t* idx, int64_t n, int32_t F, float* out, int64_t ldo,
                      pna_stream_t stream);

/* ---- node-level projection with a wide output (ABI 21) ------------------------------------------------------------------
 * replaces: the source half of `self.pretrans` of every tower of a PNALayer whose towers all read the whole input
 * (models/dgl/pna_layer.py:137-139 divide_input=False; models/dgl/pna_layer.py:36-44 pretrans_edges), factorised to node level:
 *
 *   y[m, 0:N] = sum_k x[m, k] w[n, k]            x (M, K) fp32, 4 <= K <= 128;  w (N, K) row-major (nn.Linear's layout), N <= 512
 *
 * fp32 operands, exact fp32 products (v_mfma_f32_16x16x4_f32), fp32 accumulation: an fp32 GEMM up to the order of the sum.  The whole
 * weight stays in LDS (16 ceil(K / 16) x (80 ceil(N / 80) + 4) floats <= 160 KB, else PNA_E_INVALID), x is read once and every row
 * of y is written once, whatever N -- the product is bound by its output stream.  Columns [N, ldy) of y are left alone.
 */
int pna_project_f32(const float* x, int64_t ldx, int64_t M, int32_t K, const float* w, int64_t ldw, int32_t N, float* y, int64_t ldy,
                    pna_stream_t stream);

/* The scaled form (ABI 21): the part of a multi-tower PNALayer that is linear in the row's OWN features -- the destination half of every
 * tower's pretrans (models/dgl/pna_layer.py:36-44: mean / max / min of (a_u + b_v) = those of a_u, + b_v), through the scalers
 * (models/dgl/scalers.py:11-26) and the collapsed posttrans . mixing weight, plus the self panel of posttrans (pna_layer.py:69-72):
 *
 *   y[m, n] = [self_block] sum_k x[m, k] w[n, k]  +  sum_{s < n_scaled} scales[m, s] (sum_k x[m, k] w[n, (self_block + s) K + k] + beta[s, n])
 *
 * w (N <= 80, blocks x K) row-major, blocks = self_block + n_scaled in 1..4 (four: K <= 80) side by side along a row; scales (M, n_scaled) (zero for a row
 * without in-edges); beta (n_scaled, N) nullable.  Same arithmetic and residency as pna_project_f32; one pass, every block's accumulators
 * in registers, the combination lane-local.  pna_amd/functional.py::FusedMultiTowerCall.dense_term is the caller.
 */
int pna_project_scaled_f32(const float* x, int64_t ldx, int64_t M, int32_t K, const float* w, int64_t ldw, int32_t N, int32_t n_scaled,
                           int32_t self_block, const float* scales, int64_t ld_scales, const float* beta /* nullable */, int64_t ld_beta,
                           float* y, int64_t ldy, pna_stream_t stream);

/* The grouped form (ABI 21): one weight per DEGREE GROUP of a degree plan, rows through the plan's permutation --
 *
 *   y[node, 0:N] = sum_k x[node, k] w_groups[g][n, k]        node = row_perm[v] (-1: padding, skipped), g = tile_group[v / 128], v in [0, M)
 *
 * the backward's d agg = gy W_D^T of a PNASimpleLayer in training (autograd of models/dgl/pna_layer.py:197-206): every scaler is a function
 * of the in-degree alone (models/dgl/scalers.py:7-19), so for the rows of one degree the three scaler blocks collapse into one 4F x N
 * matrix.  w_groups: n_groups dense (N, K) matrices group_stride FLOATS apart; M a multiple of 128.  A workgroup walks a contiguous piece of
 * the tiles and refills its LDS image when the group changes: list the tiles sorted by group (they are independent -- any order of
 * (128 entries of row_perm, one entry of tile_group) pairs is the same product).
 * Same arithmetic and limits as pna_project_f32.  Rows of y that no virtual row names are left alone.
 */
int pna_project_grouped_f32(const float* x, int64_t ldx, int64_t x_rows, int32_t K, const float* w_groups, int64_t group_stride, int32_t n_groups,
                            int32_t N, const int32_t* row_perm, int64_t M, const int32_t* tile_group, float* y, int64_t ldy, pna_stream_t stream);

/* ---- the tail of PNASimpleLayer's TRAINING forward, and its backward (ABI 18) ----------------------------------------
 * replaces: models/dgl/pna_layer.py:207-213 in training mode -- `h = self.batchnorm_h(h)` (nn.BatchNorm1d, batch statistics),
 * `h = F.relu(h)`, `h = h_in + h` -- and their autograd nodes:
 *
 *   mean_c, var_c = batch statistics of y[:, c] (biased variance);  save_mean = mean, save_invstd = 1 / sqrt(var + eps)
 *   out = residual + act((y - mean) * (gamma * save_invstd) + beta)                   act = ReLU when relu != 0
 *   running_mean = (1 - momentum) running_mean + momentum mean;  running_var likewise with var * M / (M - 1)
 *                                                                 (both skipped when running_mean is NULL or momentum < 0)
 *   backward (g' = grad_out where the activation passed, xhat = (y - mean) save_invstd):
 *   grad_beta = sum_r g',  grad_gamma = sum_r g' xhat,  grad_y = gamma save_invstd (g' - mean_r g' - xhat mean_r(g' xhat))
 *   (the residual's gradient is grad_out itself: the caller's)
 *
 * Two streaming passes each way (column sums, then the element-wise pass) instead of the ~10 library passes; the forward's column
 * sums are taken of y - k in fp32 over the at most 64 rows of one thread, k the median of the first three of those rows (one unusual
 * row, or a run of them at the front, does not become the shift), and are re-based on one shift and added in float64 across the
 * threads of a workgroup and across the workgroups, in a fixed order.  M >= 2 rows (nn.BatchNorm1d raises below that: the
 * caller's), 1 <= N <= 128, rows 4-byte aligned, ld >= N.  workspace: pna_bn_tail_workspace_bytes(M, N) bytes, no
 * initialisation needed, not kept between the two calls.
 */
typedef struct pna_bn_tail_args {
  uint32_t struct_size;    /* sizeof(pna_bn_tail_args) of the CALLER's header (ABI 19): a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const float* y;          /* (M, ldy): the posttrans output */
  int64_t ldy;
  int64_t M;
  int32_t N;
  int32_t relu;
  const float* gamma;      /* nullable [N] (affine=False: 1) */
  const float* beta;       /* nullable [N] */
  float eps;
  float momentum;          /* < 0: leave the running statistics alone */
  float* running_mean;     /* nullable [N]; with running_var */
  float* running_var;
  const float* residual;   /* fwd, nullable (M, ld_res) */
  int64_t ld_res;
  float* out;              /* fwd (M, ld_out) */
  int64_t ld_out;
  float* save_mean;        /* [N]: written by fwd, read by bwd */
  float* save_invstd;      /* [N] */
  void* workspace;
  int64_t workspace_bytes;
  const float* grad_out;   /* bwd (M, ld_go) */
  int64_t ld_go;
  float* grad_y;           /* bwd (M, ld_gy) */
  int64_t ld_gy;
  float* grad_gamma;       /* bwd, nullable [N] */
  float* grad_beta;        /* bwd, nullable [N] */
} pna_bn_tail_args;

int64_t pna_bn_tail_workspace_bytes(int64_t M, int32_t N);
int pna_bn_tail_fwd_f32(const pna_bn_tail_args* args, pna_stream_t stream);
int pna_bn_tail_bwd_f32(const pna_bn_tail_args* args, pna_stream_t stream);

/* ---- bf16 inference of PNASimpleLayer (ABI 22) ------------------------------------------------------------------------------
 *
 * Two entry points for a layer whose features and parameters are bf16 (pna_amd.functional.simple_layer_bf16); together they
 * replace PNASimpleLayer.reduce_func + forward, models/dgl/pna_layer.py:189-216, with the aggregators of models/dgl/aggregators.py.  Data pointers typed
 * `void*` below hold bf16 values (the upper 16 bits of an IEEE fp32); row strides (ld*) are in ELEMENTS of the pointed-to type.
 *
 * pna_segreduce_fwd_bf16 -- replaces reduce_func of PNASimpleLayer, models/dgl/pna_layer.py:189-194 (copy_u message + update_all,
 * :202), with the aggregators of models/dgl/aggregators.py:6-26,50-51 (mean, sum, max, min, std, var; identity scaler only):
 *     out[v * ldo + a * block_stride + f] = bf16( aggr[a]( x[col[k]][f] : k in [rowptr[v], rowptr[v+1]) ) )
 * Every statistic is accumulated in fp32 in CSR edge order (hub rows: per heavy segment, then over segments in segment order) with
 * the formulas of pna_segreduce_fwd_f32 (mean = s / D correctly rounded; var = relu(E[x^2] - E[x]^2); std = sqrt(var + 1e-5)),
 * then rounded to bf16 ONCE.  Rows with no in-edges give 0.  No atomics: repeated calls give identical bits.
 * With block_stride a multiple of 8, columns [F, round8(F)) of every block are written as 0 and the stores are 16 bytes wide;
 * otherwise only the F columns of each block are written.  x: any pitch ldx >= F; with ldx a multiple of 8 and a 16-byte aligned
 * x, rows are gathered in 16-byte pieces when F is a multiple of 8 or x_tail_readable = 1 (columns [F, round8(F)) of every row of
 * x may be read; their values are ignored).  Hub rows: the Graph's heavy-row schedule (pna_segreduce_args "Heavy rows"), with
 * `partials` = pna_segreduce_bf16_partials_bytes(n_seg, F) bytes of fp32 workspace.  F <= 512. */
typedef struct pna_segreduce_bf16_args {
  uint32_t struct_size;    /* sizeof(pna_segreduce_bf16_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* rowptr;   /* [V+1] */
  const int32_t* col;      /* [E] source row of each CSR edge */
  int32_t V;
  int32_t F;
  const void* x;           /* bf16 (x_rows, ldx) */
  int64_t ldx;
  int32_t x_tail_readable; /* 1 = columns [F, round8(F)) of every row of x may be read */
  int32_t n_aggr;
  int32_t aggr[PNA_MAX_AGGR]; /* PNA_AGG_MEAN .. PNA_AGG_STD_PYG */
  void* out;               /* bf16 (V, ldo), 16-byte aligned, ldo a multiple of 8 and >= (n_aggr - 1) * block_stride + F */
  int64_t ldo;
  int32_t block_stride;    /* columns between aggregator blocks (>= F); 0 = F */
  int32_t heavy_threshold; /* rows with more in-edges are reduced through the heavy schedule (when n_heavy > 0) */
  int32_t seg_len;
  int32_t n_heavy;
  int32_t n_seg;
  int32_t _pad0;
  const int32_t* heavy_rows;   /* [n_heavy] */
  const int32_t* heavy_segptr; /* [n_heavy+1] */
  const int32_t* seg_heavy;    /* [n_seg] */
  float* partials;             /* workspace */
} pna_segreduce_bf16_args;

int pna_segreduce_fwd_bf16(const pna_segreduce_bf16_args* args, pna_stream_t stream);
int64_t pna_segreduce_bf16_partials_bytes(int32_t n_seg, int32_t F);

/* pna_posttrans_bf16 -- replaces the posttrans nn.Linear and, with `epilogue`, the eval-mode tail of PNASimpleLayer,
 * models/dgl/pna_layer.py:206-213 (BatchNorm with running statistics :209-210, ReLU :211, residual :212-213):
 *     z[v] = sum_s row_scale[s][v] * (W_s . a[v]) + bias
 *     y[v] = bf16( epilogue ? residual[v] + relu(z[v] * col_scale + col_shift) : z[v] )
 * `a` is the (M, K) bf16 aggregate of pna_segreduce_fwd_bf16 (K a multiple of 8; every one of its K columns must be finite where
 * the weight is zero), W_s the column block of the reference weight that multiplies scaler s (models/dgl/pna_layer.py:48-49).
 * The products are single bf16 x bf16 products on v_mfma_f32_16x16x32_bf16, accumulated in fp32 per scaler block; the row scalers
 * (fp32, models/dgl/scalers.py:7-19 -- Graph.degree_scalers) multiply those fp32 sums, so the (M, S K) scaled operand is never
 * formed.  y is rounded to bf16 once.  w_img: bf16 (n_scaler, 16 T, round32(K)) row-major, T = pna_posttrans_bf16_tiles(N),
 * element [s][n][k] = W_s[n][k], zero outside n < N, k < K.  bias (bf16 [N]), row_scale[s] (fp32 [M]; NULL = identity),
 * col_scale / col_shift (fp32 [N], the folded BatchNorm; NULL = none) and residual (bf16 (M, ld_res)) are optional; relu and the
 * three after the bias apply only with epilogue = 1.  1 <= N <= 128, n_scaler <= 3. */
typedef struct pna_posttrans_bf16_args {
  uint32_t struct_size;    /* sizeof(pna_posttrans_bf16_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const void* a;           /* bf16 (M, lda), 16-byte aligned, lda a multiple of 8 */
  int64_t lda;
  int32_t M;
  int32_t K;
  int32_t N;
  int32_t n_scaler;
  const float* row_scale[PNA_MAX_SCALER];
  const void* w_img;       /* bf16 image, 16-byte aligned */
  const void* bias;        /* bf16 [N], nullable */
  int32_t epilogue;        /* 1 = BatchNorm fold / ReLU / residual after the bias; 0 = y = z */
  int32_t relu;
  const float* col_scale;  /* nullable [N]: gamma / sqrt(running_var + eps) */
  const float* col_shift;  /* nullable [N]: beta - running_mean * col_scale */
  const void* residual;    /* bf16 (M, ld_res), nullable */
  int64_t ld_res;
  void* y;                 /* bf16 (M, ldy) */
  int64_t ldy;
} pna_posttrans_bf16_args;

int pna_posttrans_bf16(const pna_posttrans_bf16_args* args, pna_stream_t stream);
/* Column tiles of 16 the weight image of an N-column contraction has (2, 4, 5 or 8); -1 when N is outside 1..128. */
int pna_posttrans_bf16_tiles(int32_t N);

/* ---- bf16 inference of PNALayer / PNATower (ABI 23) ------------------------------------------------------------------------------
 *
 * Two entry points for the tower layer on bf16 features and parameters (pna_amd.functional.tower_layer_bf16); with the node-level
 * projections of the factorised 1-layer pretrans they replace PNATower.forward and PNALayer.forward, models/dgl/pna_layer.py:35-76,
 * :130-145.  `void*` data pointers hold bf16 values; row strides (ld*) are in ELEMENTS of the pointed-to type.
 *
 * pna_gather_bf16 -- replaces pretrans_edges + reduce_func of PNATower, models/dgl/pna_layer.py:35-50 (update_all, :64), for a
 * pretrans that is one Linear, with the aggregators of models/dgl/aggregators.py:6-26,50-51:
 *     m(k)  = x[col[k]][f] + dst_term[v][f] + edge_term(k)[f]                 fp32, in registers, never rounded or stored
 *     out[v * ldo + a * block_stride + f] = bf16( aggr[a]( m(k) : k in [rowptr[v], rowptr[v+1]) ) )
 * x = W_a h, dst_term = W_b h + b (one row per destination, added once per edge; NULL = no term), edge_term(k) = row
 * edge_type[k] of edge_rows (W_e ef of every edge type) or, with edge_type NULL, row k of edge_rows (W_e ef of CSR edge k);
 * edge_rows NULL = no term.  All towers of a layer go through one call as rows of width F = towers * in_dim (the aggregators
 * are per feature).  Statistics, hub rows, rounding, empty rows (0) and the layout of `out`: exactly pna_segreduce_fwd_bf16.
 * Rows are read in 16-byte pieces when x, dst_term and edge_rows are all 16-byte aligned with pitches that are multiples of 8
 * and F is a multiple of 8 or tails_readable = 1 (columns [F, round8(F)) of every row of the three may be read; their values
 * are ignored); in 2-byte pieces otherwise.  F <= 512. */
typedef struct pna_gather_bf16_args {
  uint32_t struct_size;    /* sizeof(pna_gather_bf16_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* rowptr;   /* [V+1] */
  const int32_t* col;      /* [E] source row of each CSR edge */
  int32_t V;
  int32_t F;
  const void* x;           /* bf16 (x_rows, ldx): the source-side term */
  int64_t ldx;
  const void* dst_term;    /* bf16 (V, ld_dst), nullable */
  int64_t ld_dst;
  const void* edge_rows;   /* bf16 (n_types or E, ld_edge), nullable */
  int64_t ld_edge;
  const int32_t* edge_type; /* [E] in CSR order, values in [0, n_edge_rows); NULL = edge_rows has one row per CSR edge */
  int32_t n_edge_rows;     /* rows of edge_rows */
  int32_t tails_readable;  /* 1 = columns [F, round8(F)) of every row of x, dst_term and edge_rows may be read */
  int32_t n_aggr;
  int32_t block_stride;    /* columns between aggregator blocks (>= F); 0 = F */
  int32_t aggr[PNA_MAX_AGGR]; /* PNA_AGG_MEAN .. PNA_AGG_STD_PYG */
  void* out;               /* bf16 (V, ldo), 16-byte aligned, ldo a multiple of 8 and >= (n_aggr - 1) * block_stride + F */
  int64_t ldo;
  int32_t heavy_threshold; /* the heavy-row schedule of pna_segreduce_bf16_args */
  int32_t seg_len;
  int32_t n_heavy;
  int32_t n_seg;
  const int32_t* heavy_rows;   /* [n_heavy] */
  const int32_t* heavy_segptr; /* [n_heavy+1] */
  const int32_t* seg_heavy;    /* [n_seg] */
  float* partials;             /* pna_segreduce_bf16_partials_bytes(n_seg, F) bytes */
} pna_gather_bf16_args;

int pna_gather_bf16(const pna_gather_bf16_args* args, pna_stream_t stream);

/* pna_contract_bf16 -- one contraction for the three dense stages of the bf16 tower layer: the node-level projections of the
 * pretrans (models/dgl/pna_layer.py:35-40 -- no scaler, no epilogue), the posttrans Linear of all towers with graph norm and
 * eval-mode BatchNorm (:65-74) and the mixing network (:128, :141-144):
 *     z[v] = sum_s row_scale[s][v] * (W_s . a[v]) + W_h . h_self[v] + bias
 *     y[v] = bf16( residual[v] + act( (z[v] * row_post[v]) * col_scale + col_shift ) ),   act(t) = t < 0 ? slope * t : t
 * Single bf16 x bf16 products on v_mfma_f32_16x16x32_bf16, fp32 accumulators per scaler block; the fp32 row scalers multiply the fp32
 * sums; y is rounded once.  h_self (bf16 (M, Kh), nullable) is the unscaled operand: when row_scale[0] is NULL (an identity
 * scaler first) it shares that block's accumulators, else it gets a set of its own.  a: (M, K); the 16-byte loads need a 16-byte
 * aligned base, lda a multiple of 8 and K a multiple of 8 (likewise h_self / ld_self / Kh), other operands are read in 2-byte pieces
 * with columns >= K taken as 0.  w_img: bf16 (n_scaler, R, round32(K)) row-major with R = 16 T ceil(N / (16 T)) rows,
 * T = pna_contract_bf16_tiles(N); element [s][n][k] = W_s[n][k], zero elsewhere.  w_self: bf16 (R, round32(Kh)) likewise.
 * bias (bf16 [N]), row_scale[s] (fp32 [M]; NULL = 1), row_post (fp32 [M]), col_scale / col_shift (fp32 [N], both or neither) and
 * residual (bf16 (M, ld_res)) are optional; slope 1 = no activation, 0 = ReLU, 0.01 = LeakyReLU.  n_scaler <= 3; N <= 128 with more
 * than one scaler block or with h_self, N <= 4096 otherwise (column slabs of 128). */
typedef struct pna_contract_bf16_args {
  uint32_t struct_size;    /* sizeof(pna_contract_bf16_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const void* a;           /* bf16 (M, lda) */
  int64_t lda;
  int32_t M;
  int32_t K;
  int32_t N;
  int32_t n_scaler;
  const float* row_scale[PNA_MAX_SCALER];
  const void* w_img;       /* bf16 image, 16-byte aligned */
  const void* h_self;      /* bf16 (M, ld_self), nullable */
  int64_t ld_self;
  int32_t Kh;
  int32_t _pad0;
  const void* w_self;      /* bf16 image, 16-byte aligned; required with h_self */
  const void* bias;        /* bf16 [N], nullable */
  const float* row_post;   /* nullable [M] */
  const float* col_scale;  /* nullable [N] */
  const float* col_shift;  /* nullable [N] */
  float slope;             /* 1 = none, 0 = ReLU, 0.01 = LeakyReLU */
  int32_t _pad1;
  const void* residual;    /* bf16 (M, ld_res), nullable */
  int64_t ld_res;
  void* y;                 /* bf16 (M, ldy) */
  int64_t ldy;
} pna_contract_bf16_args;

int pna_contract_bf16(const pna_contract_bf16_args* args, pna_stream_t stream);
/* Column tiles of 16 per workgroup the weight images of an N-column contraction are laid out for (2, 4, 5 or 8; 8 for N > 128);
 * -1 when N is outside 1..4096. */
int pna_contract_bf16_tiles(int32_t N);

/* ---- the bf16 tower layer of molecule-sized batches: one call, at most two launches (ABI 23, additive) ----------------------------
 *
 * pna_tower_layer_bf16 is the bf16 counterpart of pna_tower_layer_f32: in eval mode, all of PNALayer.forward
 * (models/dgl/pna_layer.py:130-148) with 1-layer pretrans / posttrans, PNATower.forward (:55-76, mix_img == NULL) or
 * PNASimpleLayer.forward (:197-216, no_self_panel) for batches whose rows all have few in-edges.  `void*` data pointers hold bf16
 * values; row strides (ld*) are in ELEMENTS.  With Fp = round8(Fi), R = round to bf16 once, everything in between fp32:
 *   launch 1   x_cat[v] = R([ W_a,t h_t[v] ]_t | [ W_b,t h_t[v] + b_t ]_t)      tower t's block at columns t Fp (+ T Fp for the second
 *              half); pna_contract_bf16 on proj_img.  Skipped with no_self_panel.
 *   launch 2   per 16 destination rows, never leaving the CU:
 *              a_t[v]   = R(aggr[i]( x_src,t[u] + x_dst,t[v] + edge_table[edge_type[k]] : in-edges k = (u -> v) ))   fp32 statistics
 *                         of pna_gather_bf16 (max / min are selections; rows without in-edges give 0)
 *              z_t[v]   = R(((b_t + W_h,t h_t[v] + sum_s row_scale[s][v] (W_s,t a_t[v])) * row_post[v]) * col_scale + col_shift)
 *              y[v]     = R(residual[v] + act(W_mix [z_0 .. z_T-1][v] + b_mix)),   act(t) = t < 0 ? mix_slope * t : t
 *   mix_img == NULL: y[v] = R(residual[v] + act(((...)) * col_scale + col_shift)) of the concatenation, ONE rounding (PNATower on
 *   its own: mix_slope = 1, residual NULL).  no_self_panel: the messages are the raw rows h[u] (x = h, no destination term, no
 *   self block, n_tower = 1, no mixing network): two roundings, the aggregate and y = R(h + relu(BN(...))) with mix_slope = 0.
 * Each tower is contracted against its own weight blocks only (v_mfma_f32_16x16x32_bf16).  No atomics: identical bits on every run.
 * Rows of any in-degree are served, one lane per 8 features walking the whole row: callers keep hub rows on pna_gather_bf16.
 *
 * Weight images (bf16, 16-byte aligned, zero where nothing is named), Fop = round16(Fo), Kp = round32(n_aggr Fp), Khp = round32(Fi):
 *   proj_img   the pna_contract_bf16 image (1, R, round32(Kin)) of the 2 T Fp projection rows (Kin = T Fi block-diagonal with
 *              divide_input, else Fi); proj_bias bf16 [2 T Fp] = [0 | b_t at T Fp + t Fp]
 *   post_img   [T][n_scaler][Fop][Kp]: element [t][s][n][a Fp + f] = posttrans weight of tower t, output n, scaler s, aggregator a,
 *              feature f; followed (unless no_self_panel) by [T][Fop][Khp]: element [t][n][f] = the weight on the tower's own h_t
 *   mix_img    [round16(No)][round32(T Fo)]
 * Returns PNA_E_INVALID when the 16-row tile -- 32 (T Kp + [T or 1] Khp + round32(T Fo) + 24) bytes -- exceeds 160 KiB of LDS. */
typedef struct pna_tower_layer_bf16_args {
  uint32_t struct_size;    /* sizeof(pna_tower_layer_bf16_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* rowptr;   /* [V+1] CSR by destination */
  const int32_t* col;      /* [E] source node per CSR edge */
  int32_t V;
  int32_t n_tower;         /* T */
  int32_t Fi;              /* per-tower input width (= pretrans output width) */
  int32_t Fo;              /* per-tower output width */
  int32_t divide_input;    /* 0: every tower reads all of h (ldh >= Fi); 1: tower t reads columns [t Fi, (t+1) Fi) */
  int32_t n_scaler;        /* 1..3 */
  int32_t n_aggr;          /* 1..PNA_MAX_AGGR */
  int32_t no_self_panel;   /* != 0: the PNASimpleLayer form */
  int32_t aggr[PNA_MAX_AGGR]; /* PNA_AGG_MEAN .. PNA_AGG_STD_PYG */
  const void* h;           /* bf16 (V, ldh) node features */
  int64_t ldh;
  void* x_cat;             /* bf16 (V, ldx) workspace, 2 T Fp columns, 16-byte aligned, ldx a multiple of 8 */
  int64_t ldx;
  const void* proj_img;
  const void* proj_bias;   /* bf16 [2 T Fp], nullable */
  const float* row_scale[PNA_MAX_SCALER]; /* each fp32 [V] or NULL = identity */
  const void* post_img;
  const void* post_bias;   /* bf16 [T Fo], nullable */
  const float* row_post;   /* nullable fp32 [V]: graph-norm factor */
  const float* col_scale;  /* nullable fp32 [T Fo]: eval BatchNorm scale of every tower, concatenated */
  const float* col_shift;  /* nullable fp32 [T Fo] (with col_scale) */
  const void* mix_img;     /* nullable */
  const void* mix_bias;    /* bf16 [No], nullable */
  int32_t No;              /* mixing output width (ignored without mix_img: the output is T Fo wide) */
  float mix_slope;         /* 1 = no activation, 0 = ReLU, 0.01 = LeakyReLU */
  const void* residual;    /* bf16 (V, ld_res), nullable: added after the activation */
  int64_t ld_res;
  void* y;                 /* bf16 (V, ldy) */
  int64_t ldy;
  const int32_t* edge_type;  /* nullable [E]: type of every CSR edge; values outside [0, n_edge_types) read the nearest table row */
  const void* edge_table;    /* bf16 (n_edge_types, ld_edge_table), 16-byte aligned rows: R(W_e ef) of tower t at columns t Fp */
  int64_t ld_edge_table;
  int32_t n_edge_types;      /* 1..4 with edge_type */
  int32_t h_tail_readable;   /* no_self_panel: 1 = columns [Fi, round8(Fi)) of every row of h may be read (16-byte gathers) */
} pna_tower_layer_bf16_args;

int pna_tower_layer_bf16(const pna_tower_layer_bf16_args* args, pna_stream_t stream);
/* Host only.  LDS bytes of pna_tower_layer_bf16's 16-row tile, by the entry point's own code (it refuses more than 160 KiB); No = 0: no
 * mixing image.  -1 when n_tower, Fi, Fo or n_aggr is below 1 or No is negative. */
int64_t pna_tower_layer_bf16_lds_bytes(int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_aggr, int32_t divide_input, int32_t No,
                                       int32_t no_self_panel);

/* ---- the per-edge MLP of a deep pre_nn on bf16 messages (ABI 23, additive) --------------------------------------------------------
 *
 * pna_edge_mlp_bf16 -- the layers 2..L of PNAConv.pre_nns[t] = Linear, (ReLU, Linear) x (L - 1), models/pytorch_geometric/pna.py:
 * 135-149, for every CSR edge and tower, from the node-level terms of the FIRST Linear (pna_contract_bf16) and without the
 * (E, 2-3 F) concatenation.  With R = round to bf16 once, everything in between fp32, k = (j -> i) a CSR edge, j = col[k], i = row[k]:
 *     z_1(k)  = R(relu((x_src[j] + x_dst[i]) + edge term(k)))              the three rows are added in this order
 *     z_l(k)  = R(relu(W_l z_(l-1)(k) + b_l))        1 < l < L
 *     out[k]  = R(W_L z_(L-1)(k) + b_L)                                    n_hidden = L - 1 >= 1 matrix layers in all
 * Tower t lives at columns [t Fp, t Fp + F) of x_src, x_dst, edge_rows and out, Fp = round8(F): every 8-feature piece is one aligned
 * 16-byte access; the columns [F, Fp) of the inputs are ignored and those of out are written as zeros.  edge term(k) = row
 * edge_type[k] of edge_rows (values outside [0, n_edge_rows) read the nearest row) or, with edge_type NULL, row k; edge_rows NULL
 * = no term.  Tiles of 16 consecutive CSR edges per wavefront on v_mfma_f32_16x16x32_bf16; the hidden weights of one tower stay in
 * LDS.  No atomics, a fixed order of every sum: identical bits on every run.
 *     w_img   bf16 [T][n_hidden][round16(F)][round32(Fp)], 16-byte aligned: element [t][l][n][k] = W_(l+2),t[n][k], zero elsewhere
 *     bias    bf16 [T][n_hidden][F], required
 * Returns PNA_E_INVALID for F outside 1..128 and when one tower's weights and the four 16-edge tiles of a workgroup --
 * 2 (n_hidden round16(F) (round32(Fp) + 16) + 64 (round32(Fp) + 8)) bytes -- exceed 160 KiB of LDS. */
typedef struct pna_edge_mlp_bf16_args {
  uint32_t struct_size;    /* sizeof(pna_edge_mlp_bf16_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  int32_t E;               /* CSR edges */
  int32_t T;               /* towers, 1..64 */
  int32_t F;               /* width of every hidden layer per tower, 1..128 */
  int32_t n_hidden;        /* L - 1 >= 1 */
  const int32_t* col;      /* [E] source node of each CSR edge */
  const int32_t* row;      /* [E] destination node of each CSR edge */
  const void* x_src;       /* bf16 (nodes, ld_src), 16-byte aligned, ld_src a multiple of 8 and >= T Fp */
  int64_t ld_src;
  const void* x_dst;       /* bf16 (nodes, ld_dst), likewise */
  int64_t ld_dst;
  const void* edge_rows;   /* bf16 (n_edge_rows or E, ld_edge), likewise; nullable */
  int64_t ld_edge;
  const int32_t* edge_type; /* nullable [E] in CSR order */
  int32_t n_edge_rows;     /* rows of edge_rows (>= 1 with edge_type) */
  int32_t _pad0;
  const void* w_img;
  const void* bias;
  void* out;               /* bf16 (E, ld_out), 16-byte aligned, ld_out a multiple of 8 and >= T Fp */
  int64_t ld_out;
} pna_edge_mlp_bf16_args;

int pna_edge_mlp_bf16(const pna_edge_mlp_bf16_args* args, pna_stream_t stream);
/* LDS bytes of one workgroup of pna_edge_mlp_bf16 (the formula above); -1 when F or n_hidden is out of range. */
int64_t pna_edge_mlp_bf16_lds_bytes(int32_t F, int32_t n_hidden);

/* ---- bf16 inference on sharded graphs (ABI 23, additive) -------------------------------------------------------------------------
 *
 * pna_pack_rows_bf16 -- replaces the send-side pack of pna_amd/shard.py (pna_pack_rows_f32 on the GPU, Tensor.index_select on the
 * host) for bf16 rows:   out[i * ldo + f] = x[idx[i] * ldx + f] for f < F,   0 for F <= f < ldo,   i < n.
 * The send buffer leaves as whole rows of ldo elements with a defined tail (HaloGraph.start_halo sends rows of round8(F) elements:
 * the receiver gathers them in 16-byte pieces).  16-byte moves when x and out are 16-byte aligned and ldx, ldo are multiples of 8
 * (nothing beyond the F columns of a source row is read), 2-byte moves otherwise; non-temporal stores.  Strides in ELEMENTS. */
int pna_pack_rows_bf16(const void* x, int64_t ldx, const int32_t* idx, int64_t n, int32_t F, void* out, int64_t ldo,
                       pna_stream_t stream);

/* pna_gather_rows_bf16 -- the row-list, split-table member of the bf16 gather family: on a shard it replaces the two-launch split
 * of pna_amd.functional.aggregate (interior work list while the halo exchange is in flight, boundary rows and hub segments after
 * it: pna_segreduce_fwd_f32 over HaloGraph.split_work_lists) and the concatenated [local | halo] table that split reads.  Every
 * operand of pna_gather_bf16_args means what it means there; three additions:
 *   rows, n_rows   lane group i reduces destination row rows[i] and writes out[rows[i]]; a row that is not listed is not touched
 *                  (ids outside [0, V) are skipped).  rows NULL = every row of [0, V), n_rows is ignored.
 *   x_halo, ld_halo, n_local   a source id c < n_local reads x + c * ldx, an id >= n_local reads x_halo + (c - n_local) * ld_halo.
 *                  x_halo NULL = one table.  16-byte pieces need BOTH tables (and the term operands) 16-byte aligned with
 *                  pitches that are multiples of 8, and F a multiple of 8 or tails_readable = 1, which covers x_halo too.
 *   heavy rows     the segment and finalize kernels of the heavy-row schedule run in this call exactly when n_heavy > 0, whatever
 *                  `rows` lists; listed rows above heavy_threshold are then left to them.  CONTRACT: a call with n_heavy = 0 is
 *                  given light rows only (a listed hub row would be reduced by one lane group: correct sums in another order
 *                  than the schedule's).  pna_amd.functional guarantees it: HaloGraph.split_rows() lists no hub row.
 * For every listed row the bits of out equal those of the whole-V entry points on the concatenated table: pna_gather_bf16 when
 * dst_term or edge_rows is given, pna_segreduce_fwd_bf16 when neither is (no zero term is added to the gathered rows). */
typedef struct pna_gather_rows_bf16_args {
  uint32_t struct_size;    /* sizeof(pna_gather_rows_bf16_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* rowptr;   /* [V+1] */
  const int32_t* col;      /* [E] source id of each CSR edge, in [0, n_local + halo rows) */
  int32_t V;
  int32_t F;
  const void* x;           /* bf16 (n_local, ldx): the source-side term of the local rows */
  int64_t ldx;
  const void* x_halo;      /* bf16 (halo rows, ld_halo), nullable */
  int64_t ld_halo;
  const int32_t* rows;     /* [n_rows] destination rows of this call, nullable */
  int32_t n_rows;
  int32_t n_local;         /* rows of x (>= 1 with x_halo) */
  const void* dst_term;    /* bf16 (V, ld_dst), nullable */
  int64_t ld_dst;
  const void* edge_rows;   /* bf16 (n_types or E, ld_edge), nullable */
  int64_t ld_edge;
  const int32_t* edge_type; /* [E] in CSR order, values in [0, n_edge_rows); NULL = edge_rows has one row per CSR edge */
  int32_t n_edge_rows;     /* rows of edge_rows */
  int32_t tails_readable;  /* 1 = columns [F, round8(F)) of every row of x, x_halo, dst_term and edge_rows may be read */
  int32_t n_aggr;
  int32_t block_stride;    /* columns between aggregator blocks (>= F); 0 = F */
  int32_t aggr[PNA_MAX_AGGR]; /* PNA_AGG_MEAN .. PNA_AGG_STD_PYG */
  void* out;               /* bf16 (V, ldo), 16-byte aligned, ldo a multiple of 8 and >= (n_aggr - 1) * block_stride + F */
  int64_t ldo;
  int32_t heavy_threshold; /* the heavy-row schedule of pna_segreduce_bf16_args */
  int32_t seg_len;
  int32_t n_heavy;
  int32_t n_seg;
  const int32_t* heavy_rows;   /* [n_heavy] */
  const int32_t* heavy_segptr; /* [n_heavy+1] */
  const int32_t* seg_heavy;    /* [n_seg] */
  float* partials;             /* pna_segreduce_bf16_partials_bytes(n_seg, F) bytes */
} pna_gather_rows_bf16_args;

int pna_gather_rows_bf16(const pna_gather_rows_bf16_args* args, pna_stream_t stream);

/* ---- PNASimpleLayer TRAINING on molecule batches: the layer's forward and its backward as ONE call each -------------------------
 * replaces: models/dgl/pna_layer.py:197-213 in train mode -- update_all(message, reduce) with mean | max | min | std and the degree
 * scalers, the 1-layer posttrans Linear, BatchNorm1d with BATCH statistics, ReLU and the residual -- and what autograd derives from
 * it in loss.backward() (realworld_benchmark/train/train_HIV_graph_classification.py:4-26).
 *
 * Scope (PNA_E_INVALID outside it, pna_simple_train_workspace_bytes returns -1): aggregators mean, max, min, std in that order;
 * 1 <= n_scaler <= 3; 4 <= F <= 128; 1 <= N <= 128; V >= 2; a residual needs F == N; any in-degree (a row is reduced serially in CSR
 * order: for in-degrees <= 128 the saved aggregate and arg indices carry pna_segreduce_fwd_f32's bits and tie rule); in-degrees
 * < 65535 in the backward (16-bit ranks of the pull).  fp32 throughout; the contractions are exact-product fp32 MFMAs
 * (v_mfma_f32_16x16x4_f32) except the weight gradient, which is pna_posttrans_dw_f32's kernel (bf16x3) where that kernel's shape
 * limits hold (N <= 128 -- this scope's own cap --, n_scaler * N <= 240, 4 F + 1 <= 384) and a plain fp32 kernel otherwise.  NO float atomics: every sum has a fixed order, repeated
 * calls give identical bits.
 *
 * pna_simple_train_fwd_f32 (three launches):
 *   1. per 16 destination rows: gather h[col], a = [mean | max | min | std] (V, 4F) and argmax / argmin (V, F) are stored (the saved
 *      state), z = b + sum_s row_scale[s][v] (W_s a[v]) from the tile in LDS (the (V, n_scaler 4F) scaled aggregate never exists), z
 *      stored, the tile's BatchNorm column sums of d = z - z[first row of the tile] and d^2 (fp32) to a workspace slot of its own;
 *   2. per column: the tiles' sums re-based on z[0, c] and added in tile order in float64 (pna_bn_tail's shifted sums); save_mean,
 *      save_invstd; running_mean / running_var updated as pna_bn_tail_fwd_f32 documents (unbiased variance, momentum; NULL: not kept);
 *   3. out = residual + relu((z - mean) (gamma invstd) + beta).
 * pna_simple_train_bwd_f32 (six launches): column sums of g' = grad_out [pre-activation > 0] and g' xhat per 128 rows (fp32), added in
 *   float64 in slab order by every workgroup of the rows kernel; per 16 rows gz = gamma invstd (g' - mean g' - xhat mean(g' xhat))
 *   stored to the workspace, G[v] = sum_s row_scale[s][v] (gz[v] W_s) written as [G_mean | G_std | G_max | G_min] into the packed
 *   rows of pna_segreduce_bwd_pull_f32 (IN PLACE form); that call's rowprep and pull over the transposed graph (grad_h; the residual's
 *   grad_out is added in the pull's store); the weight gradient (grad_w (N, n_scaler 4F), grad_b).  grad_gamma = sum g' xhat,
 *   grad_beta = sum g'.
 * w is the Linear's weight (N, ldw >= n_scaler 4F), scaler block s at columns [s 4F, (s+1) 4F), read directly (no packed image: an
 * optimiser changes it every step); w 16-byte aligned, ldw a multiple of 4.  The transposed graph (backward only): col_t / rank_t as in
 * pna_segreduce_bwd_pull_args, items_t = ONE whole-row record {u, beg, end, -1} per source row (n_items_t == V: no hub segments, so
 * no atomics).  workspace: pna_simple_train_workspace_bytes(V, E, F, N, n_scaler) bytes, 256-byte aligned, no initialisation; the
 * backward reads nothing the forward left in it. */
typedef struct pna_simple_train_args {
  uint32_t struct_size;    /* sizeof(pna_simple_train_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* rowptr;   /* [V+1] */
  const int32_t* col;      /* [E] (may be NULL when E == 0) */
  int32_t V;
  int32_t E;
  int32_t F;
  int32_t N;
  int32_t n_scaler;
  int32_t residual;        /* != 0: out = h + ..., grad_h += grad_out (needs F == N) */
  const float* h;          /* (V, ldh >= F) */
  int64_t ldh;
  const float* row_scale[PNA_MAX_SCALER];  /* first n_scaler: [V] or NULL = identity */
  const float* w;
  int64_t ldw;
  const float* bias;       /* [N] or NULL */
  const float* gamma;      /* [N] or NULL (both) */
  const float* beta;
  float eps;
  float momentum;          /* forward: < 0 or running_mean NULL = running statistics not updated */
  float* running_mean;     /* [N], nullable (both) */
  float* running_var;
  float* a;                /* saved (V, 4F) contiguous: [mean | max | min | std]; forward writes, backward reads */
  int32_t* argmax;         /* saved (V, F) contiguous */
  int32_t* argmin;
  float* z;                /* saved (V, N) contiguous: the Linear's output */
  float* save_mean;        /* saved [N] */
  float* save_invstd;      /* saved [N] */
  float* out;              /* forward (V, ld_out >= N) */
  int64_t ld_out;
  const float* grad_out;   /* backward (V, ld_go >= N) */
  int64_t ld_go;
  const int32_t* col_t;    /* backward: the transposed graph */
  const int32_t* rank_t;
  const int32_t* items_t;
  int32_t n_items_t;
  int32_t _pad0;
  float* grad_h;           /* backward (V, F) contiguous */
  float* grad_w;           /* backward (N, n_scaler 4F) contiguous */
  float* grad_b;           /* [N] */
  float* grad_gamma;       /* [N] */
  float* grad_beta;        /* [N] */
  void* workspace;
  int64_t workspace_bytes;
} pna_simple_train_args;

int64_t pna_simple_train_workspace_bytes(int64_t V, int64_t E, int32_t F, int32_t N, int32_t n_scaler);
int pna_simple_train_fwd_f32(const pna_simple_train_args* args, pna_stream_t stream);
int pna_simple_train_bwd_f32(const pna_simple_train_args* args, pna_stream_t stream);

/* ---- PNALayer TRAINING on molecule batches: the layer's forward and its backward as ONE call each --------------------------------
 * replaces: models/dgl/pna_layer.py:55-76, 130-145 in train mode -- per tower the 1-layer pretrans on [h_u | h_v], update_all with
 * mean | max | min | std and the degree scalers, the 1-layer posttrans on [h | aggregate], graph norm, BatchNorm1d with BATCH
 * statistics (dropout 0); then the mixing Linear + LeakyReLU and the residual -- and what autograd derives from it in
 * loss.backward() (realworld_benchmark/train/train_molecules_graph_regression.py:29-32; the ZINC configuration of
 * realworld_benchmark/README.md:61 without edge features).
 *
 * Scope (PNA_E_INVALID outside it, pna_tower_train_workspace_bytes returns -1): 1 <= n_tower <= PNA_MAX_TOWER; aggregators mean, max,
 * min, std in that order; 1 <= n_scaler <= 3; per-tower widths 4 <= Fi <= 128, n_tower Fi <= 512, 1 <= Fo, n_tower Fo <= 128;
 * in_dim = n_tower Fi when divide_input, else Fi; V >= 2; a residual needs in_dim == n_tower Fo; no edge features; in-degrees < 65535
 * in the backward (16-bit ranks of the pull).  Tower t's pretrans weight is (Fi, 2 Fi) = [W_a | W_b], its posttrans weight
 * (Fo, (1 + 4 n_scaler) Fi) = [W_h | W_s0 | W_s1 | W_s2], w_mix (C, C) with C = n_tower Fo: all CONTIGUOUS, read directly through the
 * per-tower pointers (no packed image, no alignment beyond 4 bytes: an optimiser changes them every step).  fp32 throughout; the
 * contractions are exact-product fp32 MFMAs (v_mfma_f32_16x16x4_f32) except the weight gradients, which are pna_posttrans_dw_f32's
 * kernel (bf16x3) where that kernel's shape limits hold (5 Fi + 1 <= 384, n_scaler Fo <= 240, row_scale[0] == NULL) and a plain
 * fixed-order fp32 kernel otherwise.  NO float atomics: every sum has a fixed order, repeated calls give identical bits.
 *
 * pna_tower_train_fwd_f32 (four launches):
 *   1. x_cat (V, 2 T Fi) = [x_src | x_dst], x_src,t = W_a,t h_t, x_dst,t = W_b,t h_t + b_t (saved: the backward's pull reads it);
 *   2. per 16 destination rows, one tower at a time: the messages x_src,t[u] + x_dst,t[v] folded in CSR order (for in-degrees <= 128
 *      pna_segreduce_fwd_f32's bits and tie rule with dst_term = x_dst) give mean | max | min and argmax / argmin; the std is that of
 *      x_src,t[u] ALONE (that call's bits without dst_term: a shift does not change a std, and the shifted form loses the variance's
 *      low digits when x_dst dwarfs the neighbours' spread); a (V, T 4 Fi) = per tower [mean | max | min | std] and argmax / argmin
 *      (V, T Fi) stored; z_t = (c_t + W_h,t h_t + sum_s row_scale[s][v] (W_s,t a_t[v])) snorm_n[v] from the tile in LDS
 *      (the scaled (V, 12 Fi) operand never exists); z (V, C) stored; the tile's shifted BatchNorm column sums to a workspace slot;
 *   3. per column: the tiles' sums re-based on z[0, c] and added in tile order in float64; save_mean, save_invstd; every tower's
 *      running_mean / running_var updated as pna_bn_tail_fwd_f32 documents (unbiased variance, momentum; NULL or momentum < 0: not kept);
 *   4. per 16 rows: hcat = (z - mean) (gamma invstd) + beta, p = W_mix hcat + b_mix (saved: the backward's LeakyReLU mask is the
 *      forward's by construction), out = [h +] leaky(p).
 * pna_tower_train_bwd_f32 (6 launches + 2 per weight gradient, 3 n_tower + 1 of them): g_p = grad_out leaky'(p), g_hcat = g_p W_mix and
 *   its column sums per 16-row tile; a finalize launch adds them in float64 (grad_gamma, grad_beta, the two column means); per 16 rows
 *   gz = snorm_n gamma invstd (g_hcat - mean - xhat mean(g_hcat xhat)) and per tower G = sum_s row_scale[s] (gz_t W_s,t); rowprep and the
 *   ranked pull of pna_segreduce_bwd_pull_f32 over the transposed graph with n_tower towers and dst_term = x_dst (gx_src; rowprep's
 *   grad_dst is gx_dst); grad_h = [grad_out +] sum_t (gz_t W_h,t + gx_src,t W_a,t + gx_dst,t W_b,t), tower t's slice when divide_input,
 *   summed in tower order otherwise; grad_w_post,t = gz_t^T [h_t | row_scale[s] a_t], grad_b_post,t = colsum gz_t, grad_w_pre,t =
 *   [gx_src,t^T h_t | gx_dst,t^T h_t], grad_b_pre,t = colsum gx_dst,t, grad_w_mix = g_p^T hcat, grad_b_mix = colsum g_p.
 * The transposed graph (backward only): col_t / rank_t as in pna_segreduce_bwd_pull_args, items_t = ONE whole-row record {u, beg, end, -1}
 * per source row (n_items_t == V: no hub segments, so no atomics).  workspace: pna_tower_train_workspace_bytes(...) bytes, 256-byte
 * aligned, no initialisation; the backward reads nothing the forward left in it. */
typedef struct pna_tower_train_args {
  uint32_t struct_size;    /* sizeof(pna_tower_train_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* rowptr;   /* [V+1] */
  const int32_t* col;      /* [E] (may be NULL when E == 0) */
  int32_t V;
  int32_t E;
  int32_t n_tower;
  int32_t Fi;              /* a tower's input width */
  int32_t Fo;              /* a tower's output width */
  int32_t n_scaler;
  int32_t divide_input;    /* 1: tower t reads columns [t Fi, (t+1) Fi) of h; 0: every tower reads all Fi columns */
  int32_t residual;        /* != 0: out = h + ..., grad_h += grad_out (needs in_dim == n_tower Fo) */
  const float* h;          /* (V, ldh >= in_dim) */
  int64_t ldh;
  const float* snorm_n;    /* [V] graph-norm factor or NULL = graph norm off */
  const float* row_scale[PNA_MAX_SCALER];  /* first n_scaler: [V] or NULL = identity */
  const float* w_pre[PNA_MAX_TOWER];       /* first n_tower of each: (Fi, 2 Fi) */
  const float* b_pre[PNA_MAX_TOWER];       /* [Fi] */
  const float* w_post[PNA_MAX_TOWER];      /* (Fo, (1 + 4 n_scaler) Fi) */
  const float* b_post[PNA_MAX_TOWER];      /* [Fo] */
  const float* gamma[PNA_MAX_TOWER];       /* [Fo] or NULL (with beta; all towers or none) */
  const float* beta[PNA_MAX_TOWER];
  float* running_mean[PNA_MAX_TOWER];      /* [Fo], nullable (with running_var) */
  float* running_var[PNA_MAX_TOWER];
  const float* w_mix;      /* (C, C), C = n_tower Fo */
  const float* b_mix;      /* [C] or NULL */
  float slope;             /* the LeakyReLU's negative slope */
  float eps;
  float momentum;          /* forward: < 0 = running statistics not updated */
  int32_t _pad0;
  float* x_cat;            /* saved (V, 2 T Fi) contiguous: [x_src | x_dst]; forward writes, backward reads */
  float* a;                /* saved (V, T 4 Fi) contiguous: per tower [mean | max | min | std] */
  int32_t* argmax;         /* saved (V, T Fi) contiguous */
  int32_t* argmin;
  float* z;                /* saved (V, C) contiguous: the BatchNorms' input */
  float* p;                /* saved (V, C) contiguous: the mixing Linear's output */
  float* save_mean;        /* saved [C] */
  float* save_invstd;      /* saved [C] */
  float* out;              /* forward (V, ld_out >= C) */
  int64_t ld_out;
  const float* grad_out;   /* backward (V, ld_go >= C) */
  int64_t ld_go;
  const int32_t* col_t;    /* backward: the transposed graph */
  const int32_t* rank_t;
  const int32_t* items_t;
  int32_t n_items_t;
  int32_t _pad1;
  float* grad_h;           /* backward (V, in_dim) contiguous */
  float* grad_w_pre[PNA_MAX_TOWER];        /* backward, first n_tower of each: the parameter's shape, contiguous */
  float* grad_b_pre[PNA_MAX_TOWER];
  float* grad_w_post[PNA_MAX_TOWER];
  float* grad_b_post[PNA_MAX_TOWER];
  float* grad_gamma[PNA_MAX_TOWER];        /* [Fo] (NULL where gamma is) */
  float* grad_beta[PNA_MAX_TOWER];
  float* grad_w_mix;       /* (C, C) */
  float* grad_b_mix;       /* [C] */
  void* workspace;
  int64_t workspace_bytes;
} pna_tower_train_args;

int64_t pna_tower_train_workspace_bytes(int64_t V, int64_t E, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_scaler, int32_t divide_input);
int pna_tower_train_fwd_f32(const pna_tower_train_args* args, pna_stream_t stream);
int pna_tower_train_bwd_f32(const pna_tower_train_args* args, pna_stream_t stream);

/* ---- PNALayer TRAINING with EDGE FEATURES on molecule batches: forward and backward as ONE call each ----------------------------
 * replaces: models/dgl/pna_layer.py:35-40 (pretrans_edges with edge_features: the pretrans on [h_u | h_v | ef]), :55-76 and :130-145 in
 * train mode, and what autograd derives from them in loss.backward() (realworld_benchmark/train/train_molecules_graph_regression.py:
 * 29-32), the gradient of the edge features included (nets/molecules_graph_regression/pna_net.py:72-73: e = embedding_e(bond type));
 * the ZINC configuration of realworld_benchmark/README.md:62 (--edge_feat=True --edge_dim=50, 5 towers, hidden 70, out 60).
 *
 * The message of CSR edge k = (u -> v) is (W_a h_u + (W_b h_v + b)) + W_e e[eid[k]] -- pna_segreduce_fwd_f32's order with dst_term and
 * edge_term.  Scope: that of pna_tower_train_*_f32 (`base`), and 1 <= edge_dim <= 64.  Differences to the base call: w_pre[t] and
 * grad_w_pre[t] are (Fi, 2 Fi + edge_dim) = [W_a | W_b | W_e], contiguous; the workspace has
 * pna_tower_edge_train_workspace_bytes(...) bytes; col_t / rank_t are not read (the pull reads pos_t).  NO float atomics, fixed
 * summation orders: repeated calls give identical bits, grad_e included.  E == 0: both calls succeed, launch no zero-sized grid, the
 * W_e block of grad_w_pre is zero.
 *
 * pna_tower_edge_train_fwd_f32 (five launches): the base forward with, after its projection, x_edge (E, T Fi) = W_e,t e[eid[k]] per 16
 *   CSR edges on exact fp32 MFMAs (saved); the rows launch takes mean | max | min and the arg indices (absolute CSR positions, the first
 *   extremal edge wins) of the message above -- for in-degrees <= 128 pna_segreduce_fwd_f32's bits with x = x_src, dst_term = x_dst,
 *   edge_term = x_edge -- and the std of x_src[u] + x_edge[k] WITHOUT x_dst (that call's bits without dst_term).
 * pna_tower_edge_train_bwd_f32: the base backward with rowprep + the ranked pull replaced by
 *   dm[k] = G_mean[v] / D + [std^2 - 1e-5 > 0] G_std[v] / (std[v] D) ((x_src[u] + x_edge[k]) - (mean[v] - x_dst[v]))
 *           + [k = argmax[v]] G_max[v] + [k = argmin[v]] G_min[v]                  per edge, in CSR order, to the workspace,
 *   gx_dst[v] = G_mean + G_max + G_min (0 for a row without in-edges), gx_src[u] = sum of dm[pos_t[j]] over the whole-row record of u in
 *   items_t in list order, grad_e[eid[k]] = sum_t dm_t[k] W_e,t (when grad_e != NULL; every row written exactly once) and one more
 *   weight gradient per tower, grad_W_e,t = dm_t^T e[eid] over the E edges, into columns [2 Fi, 2 Fi + edge_dim) of grad_w_pre[t]. */
typedef struct pna_tower_edge_train_args {
  uint32_t struct_size;    /* sizeof(pna_tower_edge_train_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const pna_tower_train_args* base;  /* everything pna_tower_train_*_f32 takes, with the differences above */
  int32_t edge_dim;        /* 1 <= edge_dim <= 64 */
  int32_t _pad0;
  const float* e;          /* (E, ld_e >= edge_dim), ORIGINAL edge order (may be NULL when E == 0) */
  int64_t ld_e;
  const int32_t* eid;      /* [E] original edge id of CSR edge k (a permutation) */
  float* x_edge;           /* saved (E, T Fi) contiguous, CSR order: x_edge,t[k] = W_e,t e[eid[k]]; forward writes, backward reads */
  const int32_t* pos_t;    /* backward: [E] position in the forward CSR of transposed edge j */
  float* grad_e;           /* backward (E, ld_ge >= edge_dim), original edge order; NULL = not wanted */
  int64_t ld_ge;
} pna_tower_edge_train_args;

int64_t pna_tower_edge_train_workspace_bytes(int64_t V, int64_t E, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_scaler, int32_t divide_input,
                                             int32_t edge_dim);   /* -1 outside the scope */
int pna_tower_edge_train_fwd_f32(const pna_tower_edge_train_args* args, pna_stream_t stream);
int pna_tower_edge_train_bwd_f32(const pna_tower_edge_train_args* args, pna_stream_t stream);

/* ---- The two calls above WITH THE TOWERS' DROPOUT: forward and backward as ONE call each ---------------------------------------
 * replaces: models/dgl/pna_layer.py:71-75 (graph norm, BatchNorm, then F.dropout(h, self.dropout, training=self.training) inside every
 * tower) in front of :134-141 (cat, the mixing network) in train mode, and what autograd derives from them; every superpixel
 * configuration of realworld_benchmark/README.md:65-100 trains with --dropout 0.1, 0.2 or 0.3.
 *
 * The mask rule.  Element (v, c) of hcat (V, C = n_tower Fo) has index e = v C + c (64 bits).  Its word is word e & 3 of
 * Philox4x32-10(counter = (lo32(e >> 2), hi32(e >> 2), lo32(offset), hi32(offset)), key = (lo32(seed), hi32(seed))); multipliers
 * 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85.  The element is KEPT iff word >= thr, thr = (uint32) min(floor((double) p
 * 2^32), 2^32 - 1); a kept element is multiplied by 1.0f / (1.0f - p) (formed once in fp32), a dropped one is exactly 0.0f.
 *
 * pna_tower_drop_train_fwd_f32: the base forward (edge == NULL: pna_tower_train_fwd_f32 on `base`; else pna_tower_edge_train_fwd_f32 on
 *   `edge`, edge->base == base) whose last launch multiplies mask * hcat into the mixing Linear.  z, the batch statistics and the
 *   running statistics are those of the undropped rows.
 * pna_tower_drop_train_bwd_f32: the base backward whose first launch regenerates the mask: the hcat of the mixing weight's gradient is
 *   the masked one and g_hcat = mask * (g_p W_mix) before it is stored and summed.  Nothing but (p, seed, offset) goes from the forward
 *   to the backward.  Workspace and saved tensors: the base route's.  No float atomics; one key gives identical bits; p == 0 gives
 *   the bits of the base calls.  PNA_E_INVALID: p outside [0, 1) or NaN, a short struct, base == NULL, edge->base != base, and
 *   whatever the base call refuses.
 * pna_dropout_mask_f32 (one launch): out[v, c] (V, ld >= C) = 0.0f or 1.0f / (1.0f - p) by the rule above; V C <= 2^40. */
typedef struct pna_tower_drop_args {
  uint32_t struct_size;    /* sizeof(pna_tower_drop_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const pna_tower_train_args* base;        /* everything the route without dropout takes */
  const pna_tower_edge_train_args* edge;   /* NULL: no edge features; else edge->base == base */
  float p;                 /* 0 <= p < 1 */
  int32_t _pad0;
  uint64_t seed;           /* the mask's key ... */
  uint64_t offset;         /* ... and the high half of its counters */
} pna_tower_drop_args;

int pna_tower_drop_train_fwd_f32(const pna_tower_drop_args* args, pna_stream_t stream);
int pna_tower_drop_train_bwd_f32(const pna_tower_drop_args* args, pna_stream_t stream);
int pna_dropout_mask_f32(float* out, int64_t ld, int64_t V, int32_t C, float p, uint64_t seed, uint64_t offset, pna_stream_t stream);

/* ---- The three calls above for ANY LIST OF AGGREGATORS: forward and backward as ONE call each ------------------------------------
 * replaces: models/dgl/aggregators.py:6-26, 50-51 (mean, max, min, std, var, sum) under models/dgl/pna_layer.py:55-76, 130-145 in train
 * mode, and what autograd derives from them, for a layer whose towers aggregate with 1 to 4 DISTINCT aggregators out of those six in any
 * order: the MPNN rows of realworld_benchmark/README.md:54 and :91-100 (--aggregators="sum" or "max", --scalers="identity") and every
 * aggregator ablation.  Write A for n_aggr.  The scope is the base call's in everything else (4 <= Fi <= 128, n_tower Fi <= 512,
 * n_tower Fo <= 128, 1-3 scalers, V >= 2, edge_dim 1..64, 0 <= p < 1); since A <= 4 no tile or saved tensor is larger than the base's.
 *
 * Differences to the base call: a is (V, T A Fi), per tower the listed blocks in list order; w_post[t] and grad_w_post[t] are
 * (Fo, (1 + A n_scaler) Fi); argmax is required only when max is listed, argmin only when min is (each may be NULL otherwise); col_t /
 * rank_t are not read; the workspace has pna_tower_aggr_train_workspace_bytes(...) bytes.
 *
 * Statistics of row v with in-degree D > 0 (every listed block of a row without in-edges is 0).  The messages are formed and folded as in
 * the base call, m = (x_src[u] + x_dst[v]) [+ x_edge[k]] in CSR order; mean, max, min, std and the arg indices are the base call's bits;
 * sum is the fold's own sum of m; var = relu(E[m0^2] - E[m0]^2) of m0 = x_src[u] [+ x_edge[k]], the message without the destination term
 * (the std's radicand before + 1e-5; a shift does not change a variance); row_mean = E[m0], written when it is required.
 * Backward, one tower column, CSR edge k, only listed terms:
 *   mean0 = row_mean[v] when it was saved, else mean[v] - x_dst[v]
 *   dm[k] = (G_mean / D + G_sum) + ([std^2 - 1e-5 > 0] G_std / (std D) + [var > 0] 2 G_var / D) (m0[k] - mean0)
 *           + [k = argmax[v]] G_max + [k = argmin[v]] G_min
 *   gx_dst[v] = G_mean + D G_sum + G_max + G_min (0 when D == 0), gx_src[u] = sum of dm[pos_t[j]] over u's whole-row record of items_t in
 *   list order -- the per-edge formulation of pna_tower_edge_train_bwd_f32, with or without edge features (without them no copy of e, no
 *   grad_e, no W_e gradient).  Everything else is the base backward with K = A Fi.  No float atomics; repeated calls give identical bits.
 * With {mean, max, min, std} the forward's out and saved tensors, and with edge features every gradient, are the bits of the three
 * calls above.  PNA_E_INVALID: n_aggr outside 1..4, a repeated code, a code above PNA_AGG_VAR, a missing row_mean / argmax / argmin /
 * pos_t (pos_t: backward with E > 0 and edge == NULL), inconsistent blocks, a short struct or workspace, and whatever the base refuses. */
typedef struct pna_tower_aggr_train_args {
  uint32_t struct_size;    /* sizeof(pna_tower_aggr_train_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const pna_tower_train_args* base;        /* with the differences above */
  const pna_tower_edge_train_args* edge;   /* NULL, or edge->base == base */
  const pna_tower_drop_args* drop;         /* NULL, or drop->base == base and drop->edge == edge */
  int32_t n_aggr;                          /* 1..4 */
  int32_t aggr[PNA_MAX_AGGR];              /* distinct codes PNA_AGG_MEAN .. PNA_AGG_VAR, the layer's order */
  int32_t _pad0;
  float* row_mean;                         /* saved (V, T Fi): the mean of the variance's message; required iff std or var is listed and mean
                                              is not, else may be NULL */
  const int32_t* pos_t;                    /* backward, when edge == NULL: [E] CSR position of transposed edge j */
} pna_tower_aggr_train_args;

int64_t pna_tower_aggr_train_workspace_bytes(int64_t V, int64_t E, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_scaler, int32_t divide_input,
                                             int32_t edge_dim /* 0 = none */, int32_t n_aggr, const int32_t* aggr);   /* -1 outside the scope */
int pna_tower_aggr_train_fwd_f32(const pna_tower_aggr_train_args* args, pna_stream_t stream);
int pna_tower_aggr_train_bwd_f32(const pna_tower_aggr_train_args* args, pna_stream_t stream);

/* ---- PNAConv (the PyG formulation) TRAINING on molecule batches: forward and backward as ONE call each ----------------------------
 * replaces: models/pytorch_geometric/pna.py:120-159 (forward, message, aggregate and update of PNAConv with pre_layers == post_layers
 * == 1: per tower pre_nn on [x_i | x_j | edge_encoder(edge_attr)], the aggregators of aggregators.py:6-32 and the scalers of
 * scalers.py:7-29 on the result, post_nn on [x | aggregate], cat, lin) and what autograd derives from it in loss.backward().
 *
 * The kernels are those of pna_tower_aggr_train_*_f32 in two modes that only these entries switch on:
 *   no BatchNorm    hcat = z (the forward launches no column-sum and no finalise kernel), gz = g_hcat; base->gamma / beta / running_* /
 *                   save_mean / save_invstd / eps / momentum / grad_gamma / grad_beta are NOT read and may be NULL / 0;
 *   PyG statistics  var = E[m0^2] - E[m0]^2 NOT clamped, its gradient 2 G_var / D (m0 - mean0) without the [var > 0] gate
 *                   (aggregators.py:25-28); std = sqrt(relu(var) + 1e-5) (:31-32); a row without in-edges has std = sqrtf(1e-5f) with a
 *                   zero gradient and 0 in every other block (the rules of PNA_AGG_STD_PYG and PNA_AGG_VAR_RAW; the list itself is
 *                   written with PNA_AGG_MEAN .. PNA_AGG_VAR).
 * lin is a plain Linear: the entries run the mixing launch with slope 1.0f (leaky(p) = p and go * slope = go exactly), whatever
 * base->slope holds.  base->snorm_n must be NULL and base->residual 0 (the layer has neither).  drop must be NULL.
 *
 * The layer's tensors, read as the optimiser leaves them: w_pre[t] (Fi, (2 | 3) Fi) = [W_i | W_j | W_e] with x_i the DESTINATION
 * (pna.py:145), b_pre[t] [Fi], and with edge features w_enc (Fi, edge_dim), b_enc [Fi] of edge_encoder.  base->w_pre / b_pre /
 * grad_w_pre / grad_b_pre are NOT read: the forward's first launch PACKS, per tower, the tower call's image
 *   [W_j,t | W_i,t | M_t] (Fi, 2 Fi + edge_dim), M_t = W_e,t W_enc, and the bias b_t + W_e,t b_enc
 * into `packed` (saved: n_tower Fi (2 Fi + edge_dim + 1) floats, the T images first, then the T biases; the backward reads the
 * forward's image), and the tower call runs as the edge route on e = edge_attr itself: no (E, Fi) encoded tensor exists, and the bound
 * is edge_dim <= 64.  The backward's last launch UNPACKS the tower call's gW'_t = [gA | gB | gM_t], gb'_t (in the workspace):
 *   grad_w_pre[t] = [gB | gA | gM_t W_enc^T + gb'_t b_enc^T], grad_b_pre[t] = gb'_t,
 *   grad_w_enc = sum_t W_e,t^T gM_t, grad_b_enc = sum_t W_e,t^T gb'_t (both in tower order),
 * and grad_e is the edge route's under M_t.  Every product of the pack and the unpack is a float64 FMA chain in index order (k, then
 * for the sums over towers t outermost), rounded to fp32 once.  No float atomics: two calls give identical bits.
 * Launches: forward 1 (pack) + 3 (4 with edge features); backward 5 (6 with edge features when grad_e is wanted) + 2 per weight gradient
 * (3 n_tower + 1 of them, 4 n_tower + 1 with edge features) + 1 (unpack).
 * Scope (PNA_E_INVALID outside it, the workspace query returns -1): that of pna_tower_aggr_train_*_f32 -- 1 <= n_tower <= 8,
 * 4 <= Fi <= 128, n_tower Fi <= 512, n_tower Fo <= 128, 1-4 distinct aggregators, 1-3 scalers (base->row_scale, already with the
 * deg == 0 rules of scalers.py:16-19, 26-29), edge_dim 0 (aggr->edge == NULL, w_enc == b_enc == NULL) or 1..64, V >= 2. */
typedef struct pna_pyg_conv_train_args {
  uint32_t struct_size;    /* sizeof(pna_pyg_conv_train_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const pna_tower_aggr_train_args* aggr;   /* its base and edge members as above; the workspace has pna_pyg_conv_train_workspace_bytes(...) bytes */
  const float* w_pre[PNA_MAX_TOWER];       /* first n_tower of each: (Fi, 2 Fi) or (Fi, 3 Fi), contiguous */
  const float* b_pre[PNA_MAX_TOWER];       /* [Fi] */
  const float* w_enc;                      /* (Fi, edge_dim) contiguous, or NULL without edge features */
  const float* b_enc;                      /* [Fi], with w_enc */
  float* packed;                           /* saved, n_tower Fi (2 Fi + edge_dim + 1) floats: forward writes, backward reads */
  float* grad_w_pre[PNA_MAX_TOWER];        /* backward: the parameters' shapes, contiguous */
  float* grad_b_pre[PNA_MAX_TOWER];
  float* grad_w_enc;                       /* backward, with w_enc */
  float* grad_b_enc;
} pna_pyg_conv_train_args;

int64_t pna_pyg_conv_train_workspace_bytes(int64_t V, int64_t E, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_scaler, int32_t divide_input,
                                           int32_t edge_dim /* 0 = none */, int32_t n_aggr, const int32_t* aggr);   /* -1 outside the scope */
int pna_pyg_conv_train_fwd_f32(const pna_pyg_conv_train_args* args, pna_stream_t stream);
int pna_pyg_conv_train_bwd_f32(const pna_pyg_conv_train_args* args, pna_stream_t stream);

/* ---- The two ENDS of the molecule nets: the sum of embedding tables and the per-graph readout, one call each way ----------------
 * replaces: ogb's AtomEncoder as nets/HIV_graph_classification/pna_net.py:42 calls it (a sum of nine nn.Embedding lookups), the single
 * nn.Embedding of nets/molecules_graph_regression/pna_net.py:68-73, what autograd derives from them, and dgl.sum_nodes / mean_nodes /
 * max_nodes of pna_net.py:83-90 with their backward.
 *
 * pna_embed_sum_fwd_f32 (one launch): out[v, :] = ((0 + table_0[idx[v, 0], :]) + table_1[idx[v, 1], :]) + ... in table order, fp32.
 * pna_embed_sum_bwd_f32 (two launches, no atomics of any kind, bitwise repeatable): grad_table_j[r, :] = sum of grad_out[v, :] over the
 *   rows v with idx[v, j] == r.  The rows are cut into n_slab = ceil(V / L) slabs of L = max(PNA_EMBED_SLAB_ROWS, ceil(V /
 *   PNA_EMBED_MAX_SLABS)) consecutive rows (so n_slab <= PNA_EMBED_MAX_SLABS whatever V is).  A workgroup owns one slab and keeps ONE fp32
 *   image of all tables, (sum_j rows_j, round4(F)), in LDS; a thread owns one column and a fixed subset of the tables (tables occupy
 *   disjoint rows of the image: no two threads touch the same word) and adds the slab's rows in row order; the image goes to the slab's
 *   slot of the workspace.  The second launch, one thread per table element, adds the slots in slab order in float64 and stores fp32:
 *   EVERY element of every grad_table_j is written (zeros included); nothing is accumulated into or assumed cleared.
 * Scope (PNA_E_INVALID outside it, pna_embed_sum_workspace_bytes returns -1): V >= 1, 1 <= n_table <= PNA_MAX_EMBED_TABLE,
 * 1 <= F <= 256, rows_j >= 1 and sum_j rows_j * round4(F) * 4 <= 128 KiB (the image beside the kernel's staging area in the CU's
 * 160 KiB of LDS).  An index outside [0, rows_j) is CLAMPED into range by both calls: no index reads or writes out of bounds.
 * idx is int64, (V, ld_idx >= n_table) in elements (a 1-D index of any stride when n_table == 1).  grad_table_j is (rows_j, F)
 * contiguous.  workspace: pna_embed_sum_workspace_bytes(...) bytes (backward only), 16-byte aligned, no initialisation: no launch reads
 * what the call has not written. */
#define PNA_EMBED_SLAB_ROWS 64
#define PNA_EMBED_MAX_SLABS 256
typedef struct pna_embed_sum_args {
  uint32_t struct_size;    /* sizeof(pna_embed_sum_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  int32_t V;
  int32_t n_table;
  int32_t F;
  int32_t _pad0;
  const int64_t* idx;      /* (V, ld_idx) */
  int64_t ld_idx;          /* in elements */
  const float* table[PNA_MAX_EMBED_TABLE];    /* first n_table: (rows_j, ld_table_j >= F) */
  int32_t rows[PNA_MAX_EMBED_TABLE];
  int64_t ld_table[PNA_MAX_EMBED_TABLE];
  float* out;              /* forward (V, ld_out >= F) */
  int64_t ld_out;
  const float* grad_out;   /* backward (V, ld_go >= F) */
  int64_t ld_go;
  float* grad_table[PNA_MAX_EMBED_TABLE];     /* backward, first n_table: (rows_j, F) contiguous */
  void* workspace;         /* backward */
  int64_t workspace_bytes;
} pna_embed_sum_args;

int64_t pna_embed_sum_workspace_bytes(int64_t V, int32_t n_table, const int32_t* rows /* host */, int32_t F);   /* -1 outside the scope */
int pna_embed_sum_fwd_f32(const pna_embed_sum_args* args, pna_stream_t stream);
int pna_embed_sum_bwd_f32(const pna_embed_sum_args* args, pna_stream_t stream);

/* pna_readout_fwd_f32 (one launch, one workgroup per graph, a thread per column walking the graph's rows in order):
 *   out[g, :] = sum / mean / max of h[offsets[g] .. offsets[g+1], :]; op = PNA_AGG_SUM, PNA_AGG_MEAN (sum / n) or PNA_AGG_MAX.  For max
 *   the launch also writes argmax (G, F): the row of the FIRST maximum, pna_segreduce_fwd_f32's strict comparison and sticky NaN (-1 where
 *   no row exceeds -inf), so values and indices are that call's bits over the identity edge list.
 * pna_readout_bwd_f32 (one launch, no atomics, EVERY element of grad_h's rows [offsets[0], offsets[G]) written):
 *   sum: grad_out[g]; mean: grad_out[g] / n; max: grad_out[g] in the arg row, 0 elsewhere.
 * Scope: G >= 1 segments given by G + 1 ascending int32 offsets, every segment non-empty, inside [0, V] (offsets are clamped to it: no
 * offset reads or writes out of bounds); 1 <= F <= 512. */
typedef struct pna_readout_args {
  uint32_t struct_size;    /* sizeof(pna_readout_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* offsets;  /* [G+1] */
  int32_t G;
  int32_t V;               /* rows of h / grad_h */
  int32_t F;
  int32_t op;              /* PNA_AGG_SUM, PNA_AGG_MEAN or PNA_AGG_MAX */
  const float* h;          /* forward (V, ldh >= F) */
  int64_t ldh;
  float* out;              /* forward (G, ld_out >= F) */
  int64_t ld_out;
  int32_t* argmax;         /* max only: (G, F) contiguous; forward writes, backward reads */
  const float* grad_out;   /* backward (G, ld_go >= F) */
  int64_t ld_go;
  float* grad_h;           /* backward (V, ld_gh >= F) */
  int64_t ld_gh;
} pna_readout_args;

int pna_readout_fwd_f32(const pna_readout_args* args, pna_stream_t stream);
int pna_readout_bwd_f32(const pna_readout_args* args, pna_stream_t stream);

/* ---- The GRU update between two message-passing steps: a GRU CELL over rows, one call each way ------------------------------------
 * replaces: realworld_benchmark/nets/gru.py:5-30 (PNANet / PNANetSuperpixels with gru=True: nn.GRU over a length-1 sequence with the
 * previous features as hidden state), models/layers.py:237-268 (the multitask GNN's GRU with its zero padding, shared by the N/2
 * convolutions of models/pytorch/gnn_framework.py:60,93-95), and what autograd derives from them.
 *
 * Semantics: torch.nn.GRU, one layer, one direction, bias, sequence length 1; gate order in the 3H weight rows r, z, n:
 *   gi = x W_ih^T + b_ih    gh = h W_hh^T + b_hh
 *   r = sigmoid(gi_r + gh_r)    z = sigmoid(gi_z + gh_z)    n = tanh(gi_n + r gh_n)    out = (1 - z) n + z h
 * x is (V, I) with 1 <= I <= input_size and h is (V, Hc) with 1 <= Hc <= hidden_size: the columns that are missing are the reference's
 * zero padding (layers.py:260-264) and are never materialised (the K loops end there; z h is 0 there).  out is (V, hidden_size).
 * sigmoid and tanh branch on the sign of their argument (1 / (1 + exp(-a)) or exp(a) / (1 + exp(a)); -m / (m + 2) with m = expm1(-2 |a|)):
 * no overflow, no cancellation, exactly saturated and finite at +-100; exp / expm1 are the full-precision library functions.
 *
 * pna_gru_cell_fwd_f32 (one launch): a workgroup owns 16 rows; the x and h tiles sit in LDS; the two projections run on
 *   v_mfma_f32_16x16x4_f32 (exact fp32 products) with B fragments read straight from the nn.GRU parameters (any row pitch); gi_n and gh_n
 *   keep separate accumulators.  saved != NULL: r, z, n, gh_n are stored as (4, V, hidden_size) contiguous for the backward; NULL (no
 *   gradient wanted): nothing is saved.
 * pna_gru_cell_bwd_f32 (at most three launches, no atomics of any kind, bitwise repeatable):
 *   (a) rows kernel: da_n = grad_out (1 - z) (1 - n)(1 + n), da_z = grad_out (h - n) z (1 - z), da_r = da_n gh_n r (1 - r);
 *       dgi = [da_r | da_z | da_n], dgh = [da_r | da_z | da_n r]; grad_x = dgi W_ih (first I columns), grad_h = dgh W_hh + grad_out z
 *       (first Hc columns): gradients of padded columns are not produced.
 *   (b) per slab of L = max(PNA_GRU_SLAB_ROWS, ceil(V / PNA_GRU_MAX_SLABS)) consecutive rows: grad_W_ih = dgi^T x, grad_W_hh = dgh^T h and
 *       the column sums grad_b_ih, grad_b_hh, into the slab's slot of the workspace.
 *   (c) one thread per parameter element adds the slots in slab order in float64 and stores fp32.  EVERY element of a wanted parameter
 *       gradient is written (grad_W_ih (3H, input_size) and grad_W_hh (3H, hidden_size) contiguous, zeros in the padded columns).
 *   A gradient whose need_* flag is 0 is not written; (b) and (c) are not launched when no parameter gradient is wanted.
 * Scope (PNA_E_INVALID outside it, pna_last_error names the clause; pna_gru_cell_workspace_bytes returns -1): fp32 only (dtype ==
 * PNA_GRU_F32), 1 <= input_size <= 128, 2 <= hidden_size <= 128, V >= 2, 1 <= I <= input_size, 1 <= Hc <= hidden_size.
 * workspace (backward only): pna_gru_cell_workspace_bytes(...) = 4 (V 4 hidden_size + n_slab 3 hidden_size (I + Hc + 2)) bytes, 16-byte
 * aligned, no initialisation: no launch reads what the call has not written. */
#define PNA_GRU_F32 0
#define PNA_GRU_SLAB_ROWS 64
#define PNA_GRU_MAX_SLABS 64
typedef struct pna_gru_cell_args {
  uint32_t struct_size;    /* sizeof(pna_gru_cell_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  int64_t V;               /* rows */
  int32_t I;               /* columns of x */
  int32_t Hc;              /* columns of h */
  int32_t input_size;      /* columns of w_ih */
  int32_t hidden_size;     /* H: columns of w_hh and of out; both weights have 3H rows */
  int32_t dtype;           /* PNA_GRU_F32 */
  int32_t _pad0;
  const float* x;          /* (V, ldx >= I) */
  int64_t ldx;
  const float* h;          /* (V, ldh >= Hc) */
  int64_t ldh;
  const float* w_ih;       /* (3H, ld_wih >= input_size): nn.GRU.weight_ih_l0 as it is */
  int64_t ld_wih;
  const float* w_hh;       /* (3H, ld_whh >= H): nn.GRU.weight_hh_l0 as it is */
  int64_t ld_whh;
  const float* b_ih;       /* [3H] (forward) */
  const float* b_hh;       /* [3H] (forward) */
  float* out;              /* forward (V, ld_out >= H) */
  int64_t ld_out;
  float* saved;            /* (4, V, H) contiguous: r | z | n | gh_n; forward writes (NULL = not kept), backward reads */
  const float* grad_out;   /* backward (V, ld_go >= H) */
  int64_t ld_go;
  float* grad_x;           /* backward (V, ld_gx >= I) */
  int64_t ld_gx;
  float* grad_h;           /* backward (V, ld_gh >= Hc) */
  int64_t ld_gh;
  float* grad_w_ih;        /* backward (3H, input_size) contiguous */
  float* grad_w_hh;        /* backward (3H, H) contiguous */
  float* grad_b_ih;        /* backward [3H] */
  float* grad_b_hh;        /* backward [3H] */
  int32_t need_x;          /* backward: 0 = that gradient is not computed and its buffer (may be NULL) is not written */
  int32_t need_h;
  int32_t need_w_ih;
  int32_t need_w_hh;
  int32_t need_b_ih;
  int32_t need_b_hh;
  void* workspace;         /* backward */
  int64_t workspace_bytes;
} pna_gru_cell_args;

int64_t pna_gru_cell_workspace_bytes(int64_t V, int32_t I, int32_t Hc, int32_t hidden_size);   /* -1 outside the scope */
/* Host only.  1 when the shapes are inside the scope above (the entry points' own check, input_size included), else 0. */
int32_t pna_gru_cell_in_scope(int64_t V, int32_t I, int32_t Hc, int32_t input_size, int32_t hidden_size);
int pna_gru_cell_fwd_f32(const pna_gru_cell_args* args, pna_stream_t stream);
int pna_gru_cell_bwd_f32(const pna_gru_cell_args* args, pna_stream_t stream);

/* ---- The dense heads of the nets: 1 to 4 Linear layers with their activations over rows, one call each way --------------------------
 * replaces: realworld_benchmark/nets/mlp_readout_layer.py:14-29 (MLPReadout: the tail of the molecule, HIV and superpixel nets),
 * models/layers.py:101-234 (FCLayer / MLP without dropout and batch-norm: the multitask GNN's nodes_read_out), the two nn.Linear
 * embeddings of nets/superpixels_graph_classification/pna_net.py:38-41 as one-layer calls, and what autograd derives from them.
 *
 * Semantics: y = f_L(... f_1(x)), f_l(h) = act_l(h W_l^T + b_l), l = 1 .. n_layers.  widths[0] is the width of x, widths[l] the
 * output width of layer l; W_l = w[l - 1] is (widths[l], ldw >= widths[l - 1]) row-major as nn.Linear keeps it, b_l = b[l - 1] may be
 * NULL (bias=False).  act[l - 1] is PNA_MLP_ACT_NONE, _RELU (max(a, 0); derivative 0 at a <= 0) or _LEAKY (a > 0 ? a : a slope[l - 1];
 * derivative slope at a <= 0): torch's values, the point a == 0 included.  x and y are fp32 with unit column stride and any row pitch
 * >= their width; columns past a width are never read.  Rows are independent: a NaN or Inf in a row of x stays in that row of y and
 * of grad_x.
 *
 * pna_mlp_head_fwd_f32 (one launch): a workgroup owns 16 rows; the x tile sits in LDS zero-filled to the K pitch; every layer runs on
 *   v_mfma_f32_16x16x4_f32 (exact fp32 products, -ffp-contract=off) with B fragments read straight from the parameters; a wavefront
 *   owns 16 output columns and its activation epilogue writes the next layer's A tile into the other of two LDS buffers; only the last
 *   layer's rows are stored.  Nothing is saved: the same bits whether a backward follows or not.
 * pna_mlp_head_bwd_f32 (at most three launches, no atomics of any kind, bitwise repeatable):
 *   (a) rows kernel over the same tiles: rebuilds the pre-activations a_1 .. a_L of its rows in LDS from x, then walks down with
 *       dz_l = grad_l act_l'(a_l) and grad_(l-1) = dz_l W_l on the MFMA; stores grad_x; when a parameter gradient is wanted, stores
 *       h_1 .. h_(L-1) and dz_1 .. dz_L once to the workspace.
 *   (b) per slab of max(PNA_MLP_SLAB_ROWS, ceil(V / PNA_MLP_MAX_SLABS)) consecutive rows and per wanted layer: grad_W_l = dz_l^T h_(l-1)
 *       on the MFMA and the column sums grad_b_l (a ones column), into the slab's slot of the workspace.
 *   (c) one thread per parameter element adds the slots in slab order in float64 and stores fp32: grad_w[l - 1] (widths[l],
 *       widths[l - 1]) contiguous, grad_b[l - 1] [widths[l]].
 *   A gradient whose need_* flag is 0 is neither computed into nor written (its pointer may be NULL); (b) and (c) are not launched when
 *   no parameter gradient is wanted, and nothing at all when no gradient is.
 * Scope (PNA_E_INVALID outside it, pna_last_error names the clause, nothing is launched; pna_mlp_head_workspace_bytes returns -1 and
 * pna_mlp_head_in_scope 0): 1 <= n_layers <= PNA_MAX_MLP_LAYERS, every width in 1 .. PNA_MLP_MAX_WIDTH, 1 <= V < 2^31, every act a
 * PNA_MLP_ACT_* code.
 * workspace (backward only): 4 (V (2 sum_(l=1..L) widths[l] - widths[L]) + n_slab sum_(l=1..L) widths[l] (widths[l - 1] + 1)) bytes,
 * 16-byte aligned, no initialisation: no launch reads what the call has not written. */
#define PNA_MAX_MLP_LAYERS 4
#define PNA_MAX_MLP_WIDTHS 5  /* PNA_MAX_MLP_LAYERS + 1 */
#define PNA_MLP_MAX_WIDTH 128
#define PNA_MLP_ACT_NONE 0
#define PNA_MLP_ACT_RELU 1
#define PNA_MLP_ACT_LEAKY 2
#define PNA_MLP_SLAB_ROWS 64
#define PNA_MLP_MAX_SLABS 64
typedef struct pna_mlp_head_args {
  uint32_t struct_size;    /* sizeof(pna_mlp_head_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  int64_t V;               /* rows */
  int32_t n_layers;        /* L */
  int32_t widths[PNA_MAX_MLP_WIDTHS];       /* widths[0]: columns of x; widths[l]: outputs of layer l */
  int32_t act[PNA_MAX_MLP_LAYERS];          /* PNA_MLP_ACT_* of layer l + 1 */
  float slope[PNA_MAX_MLP_LAYERS];          /* the LeakyReLU slope of layer l + 1 (read for PNA_MLP_ACT_LEAKY only) */
  int32_t need_x;          /* backward: 0 = that gradient is not computed and its buffer (may be NULL) is not written */
  int32_t need_w[PNA_MAX_MLP_LAYERS];
  int32_t need_b[PNA_MAX_MLP_LAYERS];
  int32_t _pad0;
  const float* x;          /* (V, ldx >= widths[0]) */
  int64_t ldx;
  const float* w[PNA_MAX_MLP_LAYERS];       /* (widths[l + 1], ldw[l] >= widths[l]): nn.Linear.weight as it is */
  int64_t ldw[PNA_MAX_MLP_LAYERS];
  const float* b[PNA_MAX_MLP_LAYERS];       /* [widths[l + 1]] or NULL */
  float* y;                /* forward (V, ldy >= widths[L]) */
  int64_t ldy;
  const float* grad_out;   /* backward (V, ld_go >= widths[L]) */
  int64_t ld_go;
  float* grad_x;           /* backward (V, ld_gx >= widths[0]) */
  int64_t ld_gx;
  float* grad_w[PNA_MAX_MLP_LAYERS];        /* backward (widths[l + 1], widths[l]) contiguous */
  float* grad_b[PNA_MAX_MLP_LAYERS];        /* backward [widths[l + 1]] */
  void* workspace;         /* backward */
  int64_t workspace_bytes;
} pna_mlp_head_args;

/* widths: n_layers + 1 entries.  -1 outside the scope. */
int64_t pna_mlp_head_workspace_bytes(int64_t V, int32_t n_layers, const int32_t* widths);
/* Host only, launches nothing.  1 when the shapes and activation codes are inside the scope above (the entry points' own check), else 0. */
int32_t pna_mlp_head_in_scope(int64_t V, int32_t n_layers, const int32_t* widths, const int32_t* acts);
int pna_mlp_head_fwd_f32(const pna_mlp_head_args* args, pna_stream_t stream);
int pna_mlp_head_bwd_f32(const pna_mlp_head_args* args, pna_stream_t stream);

/* ---- The dense-adjacency PNALayer (the multitask GNN's convolution), one call each way ------------------------------------------------
 * replaces: models/pytorch/pna/layer.py:33-49,99-109 (PNATower / PNALayer with 1-layer pretrans and posttrans and the Linear + LeakyReLU
 * mixing network), aggregators.py:17-73 (mean, max, min, std), scalers.py:7-38 (the five scalers), and what autograd derives from them.
 *
 * x (B, N, in_dim) and adj (B, N, N) contiguous; in_dim = n_tower Fi (divide_input: tower t reads columns [t Fi, (t + 1) Fi)) or Fi.
 * Per tower t: w_pre (Fi, 2 Fi) = [W_p | W_q], b_pre [Fi], w_post (Fo, (1 + A S) Fi) = [W_h | W_(s, a) scaler-major], b_post [Fo];
 * w_mix (C, C), b_mix [C], C = n_tower Fo -- all read as the optimiser leaves them, no packed image.  out (B, N, C).
 * avg_log / avg_lin point to ONE float each ON THE DEVICE (avg_d["log"], avg_d["lin"]); one that no listed scaler reads may be NULL.
 *
 * Per graph: P = W_p x_t, Q = W_q x_t + b_pre, message m[i,j] = P[i] + Q[j]; a' = adj + I when self_loop (the aggregators only: the scalers'
 * D_i = sum_j adj_ij is taken from adj as passed).  mean_i = P_i + (sum_j a'_ij Q_j) / D'_i; std_i = sqrt(relu(var_i) + 1e-5) with var_i the
 * a'-weighted variance of Q_j about its weighted mean (the shift by P_i does not change it; never E[m^2] - E[m]^2); max_j = Q_j + max of
 * P_i over {i : a'_ij > 0}, min alike -- the FIRST extremal i wins (strict comparison in ascending i: pna_segreduce_fwd_f32's tie rule on
 * the by-column order).  A row (mean, std) or column (max, min) without an entry gives 0.  z_t = b_post + W_h x_t + sum_s f_s(D_i) W_s a_t
 * with f of PNA_DENSE_SCALER_*; out = leaky(W_mix cat_t z_t + b_mix, slope).
 *
 * pna_dense_layer_fwd_f32: ONE launch; a workgroup owns a slab of ceil(B / PNA_DENSE_MAX_SLABS) consecutive graphs and holds one graph's
 *   block, messages, aggregates and rows in LDS at a time.
 * pna_dense_layer_bwd_f32: at most TWO launches, nothing saved but x and adj: (a) the same workgroups rebuild the forward with the forward's
 *   device functions (so the LeakyReLU mask and the arg indices are the forward's), write grad_x (NULL: skipped) and add each graph's
 *   parameter gradients into the slab's image of the workspace in graph order; (b) the images are added in slab order in float64.  A NULL
 *   gradient pointer is skipped; adj gets no gradient.  Every sum has a fixed order and there are no atomics: bitwise repeatable.
 * Scope (PNA_E_INVALID outside it, pna_last_error names the clause; pna_dense_layer_workspace_bytes returns -1): 1 <= N <=
 * PNA_DENSE_MAX_NODES, 1 <= n_tower <= PNA_MAX_TOWER, Fi, Fo >= 1 with n_tower Fi <= 64 and n_tower Fo <= 64, 1-4 distinct aggregators
 * (PNA_AGG_MEAN, _MAX, _MIN, _STD), 1-3 distinct scalers, B >= 1, B N < 2^31, and pna_dense_layer_lds_bytes(...) <= 160 KiB:
 *   4 N ((N | 1) + 5 T Fi + A T Fi + 2 T Fo + 3 + S) + 2 N T Fi rounded up to 16.
 * workspace (backward only): min(B, PNA_DENSE_MAX_SLABS) images of T (2 Fi^2 + Fi + Fo (1 + A S) Fi + Fo) + C^2 + C floats, 16-byte aligned,
 * no initialisation. */
#define PNA_DENSE_MAX_NODES 128
#define PNA_DENSE_MAX_SLABS 256
#define PNA_DENSE_SCALER_IDENTITY 0
#define PNA_DENSE_SCALER_AMPLIFICATION 1  /* log(D + 1) / avg_log */
#define PNA_DENSE_SCALER_ATTENUATION 2    /* avg_log / log(D + 1) */
#define PNA_DENSE_SCALER_LINEAR 3         /* D / avg_lin */
#define PNA_DENSE_SCALER_INVERSE_LINEAR 4 /* avg_lin / D */
typedef struct pna_dense_layer_args {
  uint32_t struct_size;    /* sizeof(pna_dense_layer_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  int64_t B;               /* graphs */
  int32_t N;               /* nodes per graph */
  int32_t in_dim;          /* columns of x */
  int32_t n_tower;
  int32_t Fi;              /* a tower's input width */
  int32_t Fo;              /* a tower's output width */
  int32_t divide_input;
  int32_t self_loop;
  int32_t n_aggr;
  int32_t aggr[PNA_MAX_AGGR];      /* PNA_AGG_MEAN / _MAX / _MIN / _STD in the caller's order */
  int32_t n_scaler;
  int32_t scaler[PNA_MAX_SCALER];  /* PNA_DENSE_SCALER_* in the caller's order */
  float slope;                     /* of the LeakyReLU */
  const float* x;
  const float* adj;
  const float* avg_log;            /* one device float */
  const float* avg_lin;            /* one device float */
  const float* w_pre[PNA_MAX_TOWER];
  const float* b_pre[PNA_MAX_TOWER];
  const float* w_post[PNA_MAX_TOWER];
  const float* b_post[PNA_MAX_TOWER];
  const float* w_mix;
  const float* b_mix;
  float* out;                      /* forward */
  const float* grad_out;           /* backward (B, N, C) contiguous */
  float* grad_x;                   /* backward (B, N, in_dim) contiguous, NULL = not wanted */
  float* grad_w_pre[PNA_MAX_TOWER];   /* backward, the parameters' shapes, contiguous; NULL = not wanted */
  float* grad_b_pre[PNA_MAX_TOWER];
  float* grad_w_post[PNA_MAX_TOWER];
  float* grad_b_post[PNA_MAX_TOWER];
  float* grad_w_mix;
  float* grad_b_mix;
  void* workspace;                 /* backward */
  int64_t workspace_bytes;
} pna_dense_layer_args;

int64_t pna_dense_layer_lds_bytes(int32_t N, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_aggr, int32_t n_scaler);  /* -1: bad widths */
int64_t pna_dense_layer_workspace_bytes(int64_t B, int32_t N, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_aggr,
                                        int32_t n_scaler);                                      /* -1 outside the scope */
int pna_dense_layer_fwd_f32(const pna_dense_layer_args* args, pna_stream_t stream);
int pna_dense_layer_bwd_f32(const pna_dense_layer_args* args, pna_stream_t stream);

/* ---- The Set2Set graph readout (the multitask GNN's graph head), one call each way ---------------------------------------------------
 * replaces: models/layers.py:22-98 (Set2Set: a one-step nn.LSTM, the scores x q, a softmax over the nodes and the weighted sum, repeated
 * `steps` times; the loop is :81-98), as S2SReadout (:271-289) and the GNN (models/pytorch/gnn_framework.py:83,108) use it, and what
 * autograd derives from it.
 *
 * x (B, N, D) contiguous; w_ih (4D, 2D), w_hh (4D, D), b_ih, b_hh [4D]: nn.LSTM(2D, D).{weight,bias}_{ih,hh}_l0 as the optimiser leaves them,
 * contiguous, gate order i, f, g, o; out (B, 2D).  Per graph b with rows x_n:
 *   h = c = 0 (D), q* = 0 (2D); `steps` times:
 *     z = W_ih q* + W_hh h + (b_ih + b_hh);   c = sigmoid(z_f) c + sigmoid(z_i) tanh(z_g);   h = sigmoid(z_o) tanh(c);   q = h
 *     e_n = x_n . q;   a = softmax_n(e) (the maximum subtracted);   r = sum_n a_n x_n;   q* = [q | r]
 *   out_b = q*.
 * Exact fp32 on the vector ALU; every sum has a fixed order (the k of a product row ascending, the nodes ascending, the two wavefronts of
 * a softmax reduction in wavefront order after a butterfly inside each).  sigmoid and tanh are pna_gru_cell's forms: no overflow, no
 * cancellation, finite and exactly saturated at +-100.
 *
 * pna_set2set_fwd_f32: ONE launch; a workgroup owns a slab of ceil(B / PNA_S2S_MAX_SLABS) consecutive graphs; both weight matrices, the bias
 *   sum and one graph's rows sit in LDS; the step loop runs inside the kernel with workgroup barriers only.  Nothing is saved but out.
 * pna_set2set_bwd_f32: at most TWO launches, no atomics of any kind, bitwise repeatable.  (a) the same workgroups rebuild each graph's
 *   forward with the forward's device function, writing per step the activated gates, c_t, q*_t and a_t (7D + N floats) to the slab's own
 *   region of the workspace, then walk the steps in reverse: the weighted sum, the softmax, the scores, the LSTM cell, W_ih^T dz and W_hh^T dz
 *   into the previous step.  grad_x is accumulated in LDS and written once per graph (NULL: skipped); grad W_ih, grad W_hh and ONE bias
 *   gradient are accumulated in LDS over the slab's graphs in graph order and written as the slab's image.  (b) one thread per parameter
 *   element adds the images in slab order in float64 and rounds once; grad_b_ih and grad_b_hh receive the same bits.  A NULL gradient
 *   pointer is skipped; (b) is not launched when no parameter gradient is wanted.
 * Scope (PNA_E_INVALID outside it, pna_last_error names the clause; pna_set2set_workspace_bytes returns -1): fp32 only (dtype ==
 * PNA_S2S_F32), 1 <= D <= PNA_S2S_MAX_WIDTH, 1 <= N <= PNA_S2S_MAX_NODES, 1 <= steps <= PNA_S2S_MAX_STEPS, B >= 1, B N < 2^31.
 * pna_set2set_lds_bytes(N, D) is the backward's footprint, the larger one (-1: N or D outside the scope), with PI = 2D | 1, PH = D | 1:
 *   4 (4D (PI + PH) + N PH + 12 D^2 + N D + 26 D + 2 N + 4) rounded up to 16: 136976 bytes at D = 32, N = 128, inside a CU's 160 KiB.
 * workspace (backward only): min(B, PNA_S2S_MAX_SLABS) (12 D^2 + 4D + steps (7D + N)) floats, 16-byte aligned, no initialisation. */
#define PNA_S2S_F32 0
#define PNA_S2S_MAX_WIDTH 32
#define PNA_S2S_MAX_NODES 128
#define PNA_S2S_MAX_STEPS 128
#define PNA_S2S_MAX_SLABS 256
typedef struct pna_set2set_args {
  uint32_t struct_size;    /* sizeof(pna_set2set_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  int64_t B;               /* graphs */
  int32_t N;               /* nodes per graph */
  int32_t D;               /* columns of x = the LSTM's hidden size; its input size is 2D */
  int32_t steps;
  int32_t dtype;           /* PNA_S2S_F32 */
  const float* x;          /* (B, N, D) contiguous */
  const float* w_ih;       /* (4D, 2D) contiguous */
  const float* w_hh;       /* (4D, D) contiguous */
  const float* b_ih;       /* [4D] */
  const float* b_hh;       /* [4D] */
  float* out;              /* forward (B, 2D) contiguous */
  const float* grad_out;   /* backward (B, 2D) contiguous */
  float* grad_x;           /* backward (B, N, D) contiguous, NULL = not wanted */
  float* grad_w_ih;        /* backward, the parameters' shapes, contiguous; NULL = not wanted */
  float* grad_w_hh;
  float* grad_b_ih;
  float* grad_b_hh;
  void* workspace;         /* backward */
  int64_t workspace_bytes;
} pna_set2set_args;

int64_t pna_set2set_lds_bytes(int32_t N, int32_t D);                                            /* -1: N or D outside the scope */
int64_t pna_set2set_workspace_bytes(int64_t B, int32_t N, int32_t D, int32_t steps);            /* -1 outside the scope */
int pna_set2set_fwd_f32(const pna_set2set_args* args, pna_stream_t stream);
int pna_set2set_bwd_f32(const pna_set2set_args* args, pna_stream_t stream);

/* ---- The batch plan: every index array a fresh batch of small graphs needs, one call ---------------------------------------------------
 * replaces: realworld_benchmark/data/molecules.py:153-164 (dgl.batch of the members and the snorm_n column) and what pna_amd built
 * from it lazily, array by array: Graph.collate_flat (pna_amd/graph.py: the node offsets, the global edge ids, pna_collate_csr_i32's radix
 * sort, the max-degree read), Graph.work_items / heavy_schedule / edge_ids32 / snorm_n / degree_scalers, nets._readout_offsets, and
 * autograd._transposed_whole_rows with _TowerTrainPlan's pos_t (pna_amd/autograd.py: a second Graph, a second sort, rank_t, items_t).
 *
 * Input: the members' edge lists with LOCAL node ids one after the other (src_local / dst_local [E]) and the members' edge and node counts
 * ON THE DEVICE (edge_count / node_count [B]).  Member g owns the node range [noff_g, noff_g + n_g) and the edge range [eoff_g, eoff_g +
 * e_g) of the batch; the rows of its nodes in the destination-sorted CSR lie exactly in its edge range, and so do its rows of the
 * transposed CSR.  No global sort is needed: every array below is produced member by member out of LDS.
 *
 * Three launches at most, no library sort, nothing waits for the device:
 *   (1) one workgroup scans the B counts into node and edge offsets (workspace; readout_offsets is the node scan), cuts the members
 *       into GROUPS of consecutive members and initialises `record`.  A member above 256 nodes or 1 024 edges is a group of its own;
 *       smaller consecutive members share a group while their first node stays in one window of 256 nodes, their first edge in one
 *       window of 1 024 edges and their index in one window of 128 members -- so a group of small members spans fewer than 512 nodes and
 *       2 048 edges and there are at most 1 + 3 (V / 256 + E / 1 024) + B / 128 groups (the grid; surplus workgroups return at once).
 *   (2) one 256-thread workgroup per group.  A group is a block of the batch's block-diagonal adjacency, so it is sorted as ONE small
 *       graph: each of the four wavefronts takes a quarter of the group's edges in the caller's order and counts its edges per
 *       destination (an integer LDS add: a count does not depend on arrival order); a scan over the group's nodes gives rowptr and,
 *       per wavefront and destination, the first free position; then every wavefront walks its quarter IN ORDER, 64 edges a step,
 *       and an edge's position is that base plus the number of LOWER lanes of the step with the same destination (64 lane reads), the
 *       last such lane storing the new base.  No position depends on the arrival order of an atomic: edges of one destination keep the
 *       caller's order (DGL's mailbox order, what pna_collate_csr_i32's stable radix sort gives).  With want_transposed the same
 *       walk runs once more over the CSR positions with the source as key: the transposed CSR, stable in the forward CSR's order.
 *       No workgroup reads what another workgroup of the launch wrote; offsets cross from launch (1) only.
 *   (3) is not needed.
 * Every local id is checked against its member's n_g BEFORE it indexes anything: an id outside [0, n_g) sets bit 0 of record[2] and its
 * edge is written nowhere (its CSR slot at the end of the member's range, and src / dst of that edge, keep what they held); every other
 * member's arrays are what they would be without it.  Bit 1 of record[2]: a negative count, counts that do not add up to V and E (then
 * nothing is planned), or a member larger than member_nodes_max / member_edges_max declared (that group is skipped).  The call never
 * faults on bad input.
 *
 * Outputs, each nullable (NULL = not written):
 *   src, dst int64 [E]            global ids (Graph.src / .dst)
 *   rowptr [V + 1], col, row, eid [E] int32, eid64 int64 [E]   the destination-sorted CSR (CSR.eid and Graph.edge_ids32())
 *   items [V, 4]                  {row, beg, end, -1}: Graph.work_items() of a batch without heavy rows, natural order
 *   readout_offsets [B + 1]       the members' node ranges
 *   snorm_n fp32 [V]              sqrt(1 / n_g): one IEEE division, one IEEE square root (data/molecules.py:157-159)
 *   amp, att fp32 [V]             with avg_log > 0: pna_degree_scalers_f32's values from the same device function
 *   with want_transposed: rowptr_t [V + 1], col_t [E] (the destination of every out-edge), row_t [E], pos_t [E] (the position of every
 *   transposed edge in the forward CSR) and pos_t64, rank_t [E] = pos_t - rowptr[col_t], items_t [V, 4], row64 / col64 int64 [E] (row
 *   and col once more as the transposed graph's edge list)
 *   record int32 [4], required    {max in-degree, max out-degree (0 without want_transposed), status, 0}
 * Scope (PNA_E_INVALID outside it, pna_last_error names the clause, nothing is launched; pna_batch_plan_workspace_bytes returns -1):
 * 1 <= B, 0 <= E, V < 2^31, and member_nodes_max / member_edges_max -- the caller's HOST knowledge of its largest member, which the
 * launch's LDS is sized by -- inside pna_batch_plan_limits.  The limits are what one workgroup's LDS holds: 4 (2 e + 7 n + 3) bytes for
 * a group of n nodes and e edges (two CSR columns, four wavefronts' counters and three scans), 122 892 of the 160 KiB at 2 048 nodes
 * and 8 192 edges.  workspace: 4 (3 (B + 1) + 4) bytes rounded up to 256, no initialisation. */
typedef struct pna_batch_plan_args {
  uint32_t struct_size;    /* sizeof(pna_batch_plan_args) of the CALLER's header: a shorter struct is refused with PNA_E_INVALID */
  uint32_t _abi_reserved;  /* 0 */
  const int32_t* src_local;      /* [E] */
  const int32_t* dst_local;      /* [E] */
  const int32_t* edge_count;     /* [B], device */
  const int32_t* node_count;     /* [B], device */
  int32_t B;
  int32_t E;
  int32_t V;
  int32_t want_transposed;       /* 0 / 1 */
  int32_t member_nodes_max;      /* host: no member has more nodes / edges than this (<= pna_batch_plan_limits) */
  int32_t member_edges_max;
  float avg_log;                 /* <= 0: no scalers */
  int32_t _pad0;
  int64_t* src;
  int64_t* dst;
  int32_t* rowptr;
  int32_t* col;
  int32_t* row;
  int32_t* eid;
  int64_t* eid64;
  int32_t* items;
  int32_t* readout_offsets;
  float* snorm_n;
  int32_t* rowptr_t;
  int32_t* col_t;
  int32_t* row_t;
  int32_t* pos_t;
  int64_t* pos_t64;
  int32_t* rank_t;
  int32_t* items_t;
  int64_t* row64;
  int64_t* col64;
  float* amp;
  float* att;
  int32_t* record;
  void* workspace;
  int64_t workspace_bytes;
} pna_batch_plan_args;

/* Host only, callable without a GPU: the largest member (nodes, edges) one workgroup's share of the LDS holds.  Returns PNA_OK. */
int pna_batch_plan_limits(int32_t* max_member_nodes, int32_t* max_member_edges);
int64_t pna_batch_plan_workspace_bytes(int32_t B, int64_t E, int64_t V);                          /* -1 outside the scope */
int pna_batch_plan_i32(const pna_batch_plan_args* args, pna_stream_t stream);

const char* pna_last_error(void);
int pna_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PNA_AMD_H */
