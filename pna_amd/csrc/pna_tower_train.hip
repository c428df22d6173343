// pna_tower_train.hip -- PNALayer's TRAINING forward and backward on molecule-sized batches (the ZINC workload:
// realworld_benchmark/README.md:61, realworld_benchmark/train/train_molecules_graph_regression.py:29-32) as ONE C call each for gfx950.
// Implements pna_tower_train_{workspace_bytes, fwd_f32, bwd_f32} of include/pna_amd.h (models/dgl/pna_layer.py:130-145 over :55-76 in
// train mode: T towers of 1-layer pretrans, update_all with mean | max | min | std and the degree scalers, 1-layer posttrans, graph
// norm, BatchNorm1d with batch statistics; then the mixing Linear + LeakyReLU and the residual).
//
// Why: at this size the generic training route (torch.stack of the weights, two projection GEMMs, AggregateFn, then PER TOWER a
// PosttransFn, a multiply, a library BatchNorm and a dropout node, then cat / Linear / LeakyReLU / residual) is bound by launch and
// host latency.  As in pna_simple_train.hip the work is cut by destination ROWS: a workgroup owns 16 rows and takes the towers one at a
// time, so the 16 x 4 Fi aggregate tile of ONE tower is all the LDS has to hold; products are exact fp32 on v_mfma_f32_16x16x4_f32.
// Every weight is read from the module's own tensor through a per-tower pointer (an optimiser rewrites them every step); tower blocks
// of 75 or 15 floats are not 16-byte aligned, so caller tensors are read with scalar loads and only LDS tiles with 16-byte ones.
//
// Determinism: no float atomics.  A row's messages x_src[u] + x_dst[v] are folded serially in CSR order (pna_segreduce_fwd_f32's order
// for in-degrees <= 128: same bits, same arg indices; the std block is that kernel's on x_src without the destination term); column
// sums are fp32 inside a 16-row tile and float64 across the tiles in a fixed order, in launches of their own (one workgroup per
// column: no row workgroup re-adds the partial sums).
//
// Dropout inside the towers (pna_tower_drop_train_*_f32, pna_dropout_mask_f32): the two mixing kernels have a DROP instantiation that
// applies a Philox4x32-10 mask (pna_philox.h) between the BatchNorms' output and the mixing Linear; the backward regenerates it from
// the call's (seed, offset).  Every other launch is shared with the calls without dropout.
//
// Any list of aggregators (pna_tower_aggr_train_*_f32: 1-4 distinct ones out of mean | sum | max | min | std | var in the layer's order,
// models/dgl/aggregators.py:6-26, 50-51 under pna_layer.py:55-76, 130-145 -- the MPNN rows of realworld_benchmark/README.md:54, 91-100
// and every aggregator ablation): KArgs carries the block index of each aggregator inside a tower's aggregate, -1 when it is not listed,
// read under wavefront-uniform branches.  The three entry pairs above fill it with {mean, max, min, std} and run the same kernels in the
// same arithmetic sequence.  That route's backward is always the per-edge one (k_tt_edge_dm + k_tt_edge_pull), with or without x_edge.
//
// PNAConv, the PyG formulation (pna_pyg_conv_train_*_f32: models/pytorch_geometric/pna.py:120-159): the same kernels in two modes of
// KArgs -- nobn (no BatchNorm: hcat = z, gz = g_hcat, no column sums, no finalise launches) and pyg (aggregators.py:25-32: var not
// clamped and not gated, std of a row without in-edges sqrt(1e-5)) -- behind k_pyg_pack, which turns the layer's [W_i | W_j | W_e] and its
// edge encoder into the tower call's [W_a | W_b | W_e W_enc], and in front of k_pyg_unpack, which turns that image's gradient back.
// Every other entry runs with both modes 0: the same branches taken, the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_philox.h"
#include "pna_rowstats.h"
#include "pna_train_dev.h"

namespace {

using namespace pna_train;      // f4, kRows, quads, pitch_of, quad_fma, bn_affine, fold_msg, bn_finalize_column

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxT = PNA_MAX_TOWER;
constexpr int kMaxC = 128;       // out_dim = T Fo
constexpr int kMaxFi = 128;      // a lane of the gather owns columns lane and lane + 64
constexpr int kMaxIn = 512;      // T Fi
constexpr int kEU = 4;           // edges of a row whose gathers are issued together
constexpr int kMaxED = 64;       // edge_dim of the route with edge features: the edge tile's K

struct KArgs {
  const int32_t* rowptr; const int32_t* col;
  int V, T, Fi, Fo, S, C, TFi, div, residual;
  int K;                                                    // A Fi: the width of one tower's aggregate, A listed aggregators
  int b_mean, b_sum, b_max, b_min, b_std, b_var;            // the aggregator's block inside a tower's aggregate, -1 = not listed
  float* rowmean;                                           // saved (V, T Fi) E[m0] where std / var is listed without mean, else NULL
  const float* h; long ldh;
  const float* snorm;                                       // [V] or NULL (graph norm off)
  const float* scale[3];
  const float* w_pre[kMaxT]; const float* b_pre[kMaxT];     // (Fi, 2 Fi) = [W_a | W_b], [Fi]
  const float* w_post[kMaxT]; const float* b_post[kMaxT];   // (Fo, (1 + A S) Fi) = [W_h | W_s0 | ..], [Fo]
  const float* gamma[kMaxT]; const float* beta[kMaxT];
  float* rmean[kMaxT]; float* rvar[kMaxT];
  const float* w_mix; const float* b_mix;                   // (C, C), [C]
  float slope, eps, momentum;
  float* xcat; float* a; int32_t* amx; int32_t* amn; float* z; float* p; float* mean; float* invstd;     // the saved state
  float* out; long ld_out;
  const float* go; long ld_go;
  float* part; int n_part;                                  // [tiles][2][C] column sums of a 16-row tile
  float* cm;                                                // backward [2][C]: mean g, mean g xhat
  float* gp; float* hcat; float* ghc; float* gz;            // backward (V, C) each
  float* gagg;                                              // backward (V, T K): the listed blocks' gradients per tower, a's layout
  float* gxs; float* gxd;                                   // backward (V, T Fi): the gradient of x_src, x_dst
  float* gh;                                                // backward (V, in_dim)
  float* ggamma[kMaxT]; float* gbeta[kMaxT];
  long ldw_pre;                                             // row pitch of w_pre[t]: 2 Fi, 2 Fi + ED with edge features
  // edge features (pna_tower_edge_train_*): message = (x_src[u] + x_dst[v]) + x_edge[k], x_edge,t[k] = W_e,t e[eid[k]]
  int E, ED;
  const float* e; long ld_e; const int32_t* eid;            // (E, ld_e) in ORIGINAL edge order; original id of CSR edge k
  float* xedge;                                             // saved (E, T Fi), CSR order
  const int32_t* pos_t; const int32_t* items_t;             // backward: CSR position of transposed edge j; {u, beg, end, -1} per source row
  float* dm; float* ecsr;                                   // backward (E, T Fi) message gradient, (E, ED) copy of e, both in CSR order
  float* ge; long ld_ge;                                    // backward (E, ld_ge), original edge order, or NULL
  pna_philox::Mask drop;                                    // pna_tower_drop_train_*: the dropout between the BatchNorms and the mixing Linear
  int nobn;                                                 // pna_pyg_conv_train_*: no BatchNorm at all -- hcat = z, gz = g_hcat [snorm]; no column sums
  int pyg;                                                  // the PyG statistics: var not clamped (no gate in its gradient), std of a row without in-edges sqrt(1e-5)
};

__device__ __forceinline__ float leaky(float p, float slope) { return p > 0.f ? p : p * slope; }

// var of one feature of one destination row (models/dgl/aggregators.py:22-26): pna_dev::row_stats' radicand before the + 1e-5, op by op
// raw (models/pytorch_geometric/aggregators.py:25-28): the same difference, NOT clamped
__device__ __forceinline__ float row_var(float s, float q, int deg, bool raw) {
  if (deg <= 0) return 0.f;
  const float D = (float)deg, invD = 1.0f / D;
  const float mean = pna_dev::div_rn(s, D, invD), msq = pna_dev::div_rn(q, D, invD);
  const float var = msq - mean * mean;
  return (var < 0.f && !raw) ? 0.f : var;
}

// ---- forward, launch 1: x_cat = [x_src | x_dst], x_src,t = W_a,t h_t, x_dst,t = W_b,t h_t + b_t, of 16 rows ----------------------
__global__ __launch_bounds__(kThreads) void k_tt_project(const KArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int Fi = g.Fi, T = g.T, TFi = g.TFi, in_dim = g.div ? TFi : Fi, PH = in_dim + 1;
  float* const H = lds;                                     // [16][PH] the rows' input features
  const int r0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.V - r0);
  for (int i = tid; i < kRows * in_dim; i += kThreads) {
    const int r = i / in_dim, k = i - r * in_dim;
    H[r * PH + k] = r < nrows ? g.h[(size_t)(r0 + r) * g.ldh + k] : 0.f;
  }
  __syncthreads();
  const int NT = (2 * Fi + 15) / 16, Q = quads(Fi);
  for (int u = wave; u < T * NT; u += kWaves) {
    const int t = u / NT, nt = u - t * NT;
    const int j = nt * 16 + li;                             // output column of the tower's [x_src | x_dst]
    const bool jok = j < 2 * Fi;
    const int half = j >= Fi ? 1 : 0, f = min(j - half * Fi, Fi - 1);
    const float* const wrow = g.w_pre[t] + (size_t)f * g.ldw_pre + half * Fi;
    const float* const hrow = H + li * PH + (g.div ? t * Fi : 0);
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int qd = 0; qd < Q; ++qd) {
      const int k = 16 * qd + 4 * lg;
      f4 a, b;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = k + i < Fi;
        const int kk = ok ? k + i : 0;
        const float hv = hrow[kk], wv = wrow[kk];
        a[i] = ok ? hv : 0.f;
        b[i] = (ok && jok) ? wv : 0.f;
      }
      quad_fma(acc, a, b);
    }
    const float bias = (jok && half) ? g.b_pre[t][f] : 0.f;
    if (jok) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lg + i;
        if (r < nrows) g.xcat[(size_t)(r0 + r) * 2 * TFi + half * TFi + t * Fi + f] = half ? acc[i] + bias : acc[i];
      }
    }
  }
}

// ---- forward with edge features, launch 2: x_edge,t[k] = W_e,t e[eid[k]] of 16 CSR edges, all towers.  The rows e[eid[k]] go to an LDS
// tile (zeros in the K padding and in the rows past E); the B fragments are scalar loads from the tower's own weight (the block
// starts at column 2 Fi of a row of 2 Fi + ED floats: not 16-byte aligned) ----
__global__ __launch_bounds__(kThreads) void k_tt_edge_project(const KArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int Fi = g.Fi, T = g.T, TFi = g.TFi, ED = g.ED, Q = quads(ED), P = pitch_of(Q);
  float* const EF = lds;                                    // [16][P] the edges' feature rows
  const int k0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.E - k0);
  for (int i = tid; i < kRows * P; i += kThreads) {
    const int r = i / P, k = i - r * P;
    EF[i] = (k < ED && r < nrows) ? g.e[(size_t)g.eid[k0 + r] * g.ld_e + k] : 0.f;
  }
  __syncthreads();
  const int NT = (Fi + 15) / 16;
  for (int u = wave; u < T * NT; u += kWaves) {
    const int t = u / NT, nt = u - t * NT;
    const int f = nt * 16 + li;                             // output column inside the tower
    const bool fok = f < Fi;
    const float* const wrow = g.w_pre[t] + (size_t)min(f, Fi - 1) * g.ldw_pre + 2 * Fi;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int qd = 0; qd < Q; ++qd) {
      const int k = 16 * qd + 4 * lg;
      const f4 a = *reinterpret_cast<const f4*>(EF + li * P + k);
      f4 b;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = fok && k + i < ED;
        const float wv = wrow[ok ? k + i : 0];
        b[i] = ok ? wv : 0.f;
      }
      quad_fma(acc, a, b);
    }
    if (fok) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lg + i;
        if (r < nrows) g.xedge[(size_t)(k0 + r) * TFi + t * Fi + f] = acc[i];
      }
    }
  }
}

// ---- forward, launch 2 (3 with edge features): per tower gather + reduce + contraction of 16 destination rows; the tile's BatchNorm
// partial sums.  EDGE: the message is (x_src[u] + x_dst[v]) + x_edge[k] (pna_segreduce.hip's order with dst_term and edge_term) and
// the std is that of x_src[u] + x_edge[k] ----
template <int S, bool EDGE>
__global__ __launch_bounds__(kThreads) void k_tt_rows_fwd(const KArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int Fi = g.Fi, Fo = g.Fo, T = g.T, TFi = g.TFi, C = g.C, K = g.K, Q = quads(K), P = pitch_of(Q), QH = quads(Fi), PH = pitch_of(QH);
  const int NT = (Fo + 15) / 16, PZ = C + 1;
  float* const A = lds;                                     // [16][P]  one tower's aggregate, the listed blocks ([mean | max | min | std])
  float* const H = A + kRows * P;                           // [16][PH] the tower's input slice
  float* const Z = H + kRows * PH;                          // [16][PZ] the rows' z, all towers
  float* const SC = Z + kRows * PZ;                         // [4][16]  scale_0..2 and the graph-norm factor of the tile's rows
  const int r0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.V - r0);
  if (tid < 4 * kRows) {
    const int s = tid >> 4, r = tid & 15;
    const float* p = s == 3 ? g.snorm : (s < S ? g.scale[s] : nullptr);
    SC[tid] = (p && r < nrows) ? p[r0 + r] : 1.f;
  }
  for (int t = 0; t < T; ++t) {
    // zeros in the K padding columns and in the rows past the matrix's end (they multiply weights; 0 * garbage would not be 0)
    for (int i = tid; i < kRows * P; i += kThreads) {
      const int r = i / P, k = i - r * P;
      if (k >= K || r >= nrows) A[i] = 0.f;
    }
    for (int i = tid; i < kRows * PH; i += kThreads) {
      const int r = i / PH, k = i - r * PH;
      H[i] = (k < Fi && r < nrows) ? g.h[(size_t)(r0 + r) * g.ldh + (g.div ? t * Fi : 0) + k] : 0.f;
    }
    // ---- gather: a wavefront owns rows wave, wave + 8; a lane owns columns lane and lane + 64; the row's edges in CSR order.
    // mean | max | min and the arg indices are those of the message x_src[u] + x_dst[v], as the standalone gather forms it (the
    // backward's rowprep subtracts x_dst from that mean); the std is that of x_src[u] alone: the same number, without the
    // cancellation of E[m^2] - E[m]^2 when x_dst dwarfs the neighbours' spread ----
    const float* const xs = g.xcat + t * Fi;
    for (int r = wave; r < nrows; r += kWaves) {
      const int row = r0 + r;
      const int beg = g.rowptr[row], end = g.rowptr[row + 1];
      const int cc[2] = {min(lane, Fi - 1), min(lane + 64, Fi - 1)};      // (lanes past the last column redo it; not stored)
      float s[2] = {0.f, 0.f}, q[2] = {0.f, 0.f}, mx[2] = {-INFINITY, -INFINITY}, mn[2] = {INFINITY, INFINITY}, dt[2];
      float s0[2] = {0.f, 0.f}, q0[2] = {0.f, 0.f};         // sums of x_src[u] alone: the std does not see the shift
      int ax[2] = {-1, -1}, an[2] = {-1, -1};
#pragma unroll
      for (int j = 0; j < 2; ++j) dt[j] = xs[(size_t)row * 2 * TFi + TFi + cc[j]];
      for (int e = beg; e < end; e += kEU) {
        float v[kEU][2], xe[kEU][2];
#pragma unroll
        for (int u = 0; u < kEU; ++u) {
          const int k = min(e + u, end - 1);
          const size_t o = (size_t)g.col[k] * 2 * TFi;
          v[u][0] = xs[o + cc[0]];
          v[u][1] = xs[o + cc[1]];
          if constexpr (EDGE) {
            const float* const xr = g.xedge + (size_t)k * TFi + t * Fi;
            xe[u][0] = xr[cc[0]];
            xe[u][1] = xr[cc[1]];
          }
        }
#pragma unroll
        for (int u = 0; u < kEU; ++u)
          if (e + u < end) {                                // (wavefront-uniform)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              if constexpr (EDGE) {
                const float m0 = v[u][j] + xe[u][j];        // the std's message: no destination term
                fold_msg((v[u][j] + dt[j]) + xe[u][j], e + u, s[j], q[j], mx[j], mn[j], ax[j], an[j]);
                s0[j] = s0[j] + m0;
                q0[j] = q0[j] + m0 * m0;
              } else {
                fold_msg(v[u][j] + dt[j], e + u, s[j], q[j], mx[j], mn[j], ax[j], an[j]);
                s0[j] = s0[j] + v[u][j];
                q0[j] = q0[j] + v[u][j] * v[u][j];
              }
            }
          }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        if (c < Fi) {
          float mean, omx, omn, sd, m0, x0, n0;
          pna_dev::row_stats(s[j], q[j], mx[j], mn[j], end - beg, mean, omx, omn, sd);     // mean | max | min of the shifted messages
          pna_dev::row_stats(s0[j], q0[j], mx[j], mn[j], end - beg, m0, x0, n0, sd);       // std of x_src alone
          if (g.pyg && end == beg) sd = sqrtf(1e-5f);       // (models/pytorch_geometric/aggregators.py:31-32 on an empty segment)
          float* const al = A + r * P + c;
          float* const ag = g.a + (size_t)row * T * K + (size_t)t * K + c;
          if (g.b_mean >= 0) { al[g.b_mean * Fi] = mean; ag[g.b_mean * Fi] = mean; }            // (every branch on the list is wavefront-uniform)
          if (g.b_max >= 0) { al[g.b_max * Fi] = omx; ag[g.b_max * Fi] = omx; g.amx[(size_t)row * TFi + t * Fi + c] = ax[j]; }
          if (g.b_min >= 0) { al[g.b_min * Fi] = omn; ag[g.b_min * Fi] = omn; g.amn[(size_t)row * TFi + t * Fi + c] = an[j]; }
          if (g.b_std >= 0) { al[g.b_std * Fi] = sd; ag[g.b_std * Fi] = sd; }
          if (g.b_sum >= 0) { al[g.b_sum * Fi] = s[j]; ag[g.b_sum * Fi] = s[j]; }               // the fold's own sum (0 without in-edges)
          if (g.b_var >= 0) {
            const float vr = row_var(s0[j], q0[j], end - beg, g.pyg != 0);
            al[g.b_var * Fi] = vr; ag[g.b_var * Fi] = vr;
          }
          if (g.rowmean) g.rowmean[(size_t)row * TFi + t * Fi + c] = m0;
        }
      }
    }
    __syncthreads();
    // ---- contraction: wavefront nt owns the tower's output columns [16 nt, 16 nt + 16); B fragments from the weight's rows ----
    for (int nt = wave; nt < NT; nt += kWaves) {
      const int n = nt * 16 + li;
      const bool nok = n < Fo;
      const float* const wrow = g.w_post[t] + (size_t)min(n, Fo - 1) * (Fi + S * K);
      f4 acch = {0.f, 0.f, 0.f, 0.f}, acc[S];
#pragma unroll
      for (int s = 0; s < S; ++s) acc[s] = (f4){0.f, 0.f, 0.f, 0.f};
      for (int qd = 0; qd < QH; ++qd) {                     // the self panel W_h h_t
        const int k = 16 * qd + 4 * lg;
        const f4 a = *reinterpret_cast<const f4*>(H + li * PH + k);
        f4 b;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool ok = nok && k + i < Fi;
          const float wv = wrow[ok ? k + i : 0];
          b[i] = ok ? wv : 0.f;
        }
        quad_fma(acch, a, b);
      }
      for (int qd = 0; qd < Q; ++qd) {
        const int k = 16 * qd + 4 * lg;
        const f4 a = *reinterpret_cast<const f4*>(A + li * P + k);
#pragma unroll
        for (int s = 0; s < S; ++s) {
          f4 b;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool ok = nok && k + i < K;
            const float wv = wrow[Fi + s * K + (ok ? k + i : 0)];
            b[i] = ok ? wv : 0.f;
          }
          quad_fma(acc[s], a, b);
        }
      }
      const float bn = nok ? g.b_post[t][n] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lg + i;
        float zt = bn + acch[i];
#pragma unroll
        for (int s = 0; s < S; ++s) zt = zt + SC[s * kRows + r] * acc[s][i];
        if (g.snorm) zt = zt * SC[3 * kRows + r];
        if (nok) {
          Z[r * PZ + t * Fo + n] = zt;
          if (r < nrows) g.z[(size_t)(r0 + r) * C + t * Fo + n] = zt;
        }
      }
    }
    __syncthreads();
  }
  // ---- the tile's BatchNorm column sums, shifted by the tile's first row (the finalize pass re-bases them in float64) ----
  if (g.nobn) return;                                       // (uniform: no BatchNorm, nobody reads the sums)
  for (int c = tid; c < C; c += kThreads) {
    const float kc = Z[c];
    float s0 = 0.f, s1 = 0.f;
    for (int r = 0; r < nrows; ++r) {
      const float d = Z[r * PZ + c] - kc;
      s0 = s0 + d;
      s1 = s1 + d * d;
    }
    g.part[((size_t)blockIdx.x * 2 + 0) * C + c] = s0;
    g.part[((size_t)blockIdx.x * 2 + 1) * C + c] = s1;
  }
}

// ---- forward, launch 3: one workgroup per column -- the tiles' sums in float64, the column's constants, its tower's running statistics ----
__global__ __launch_bounds__(256) void k_tt_bn_finalize(const KArgs g) {
  __shared__ double red[2][256];
  const int c = blockIdx.x, t = c / g.Fo, n = c - t * g.Fo;
  bn_finalize_column(g.z, g.C, c, g.V, g.part, g.n_part, g.eps, g.momentum, g.mean + c, g.invstd + c, g.rmean[t] ? g.rmean[t] + n : nullptr,
                     g.rmean[t] ? g.rvar[t] + n : nullptr, red);
}

// the BatchNorm's per-column multiplier and offset: gamma invstd, beta
__device__ __forceinline__ void bn_consts(const KArgs& g, int c, float& cm, float& ci, float& ca, float& cb) {
  const int t = c / g.Fo, n = c - t * g.Fo;
  cm = g.mean[c]; ci = g.invstd[c];
  ca = (g.gamma[t] ? g.gamma[t][n] : 1.f) * ci;
  cb = g.beta[t] ? g.beta[t][n] : 0.f;
}

// The dropout mask of a tile's rows [r0, r0 + nrows) x C: one Philox call per quad of four consecutive elements e = v C + c (a quad
// straddles a row end whenever C % 4 != 0), f(r, c, keep) for each of its elements inside the tile -- every element exactly once.
template <class F>
__device__ __forceinline__ void tile_mask_each(const KArgs& g, int r0, int nrows, int tid, F f) {
  const uint64_t e0 = (uint64_t)r0 * (uint64_t)g.C, e1 = e0 + (uint64_t)nrows * (uint64_t)g.C;
  for (uint64_t q = (e0 >> 2) + (uint64_t)tid; q <= ((e1 - 1) >> 2); q += kThreads) {
    uint32_t w[4];
    pna_philox::quad_words(g.drop, q, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint64_t e = 4 * q + i;
      if (e >= e0 && e < e1) {
        const int d = (int)(e - e0), r = d / g.C;
        f(r, d - r * g.C, w[i] >= g.drop.thr);
      }
    }
  }
}

// ---- forward, launch 4: hcat = (z - mean) (gamma invstd) + beta, p = W_mix hcat + b_mix (saved), out = [h +] leaky(p) of 16 rows.
// DROP (pna_tower_drop_train_fwd_f32): the tile holds mask * hcat -- a kept element times 1 / (1 - p), a dropped one exactly 0 ----
template <bool DROP>
__global__ __launch_bounds__(kThreads) void k_tt_mix_fwd(const KArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int C = g.C, Q = quads(C), P = pitch_of(Q), NT = (C + 15) / 16;
  float* const HC = lds;                                    // [16][P]
  const int r0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.V - r0);
  if constexpr (DROP) {
    for (int i = tid; i < kRows * P; i += kThreads) {       // the padding; the quads below write every element inside the tile
      const int r = i / P, c = i - r * P;
      if (c >= C || r >= nrows) HC[i] = 0.f;
    }
    tile_mask_each(g, r0, nrows, tid, [&](int r, int c, bool keep) {
      float cm, ci, ca, cb;
      bn_consts(g, c, cm, ci, ca, cb);
      const float v = bn_affine(g.z[(size_t)(r0 + r) * C + c], cm, ca, cb);
      HC[r * P + c] = keep ? v * g.drop.scale : 0.f;
    });
  } else {
    for (int i = tid; i < kRows * P; i += kThreads) {
      const int r = i / P, c = i - r * P;
      float v = 0.f;
      if (c < C && r < nrows) {
        if (g.nobn) {
          v = g.z[(size_t)(r0 + r) * C + c];
        } else {
          float cm, ci, ca, cb;
          bn_consts(g, c, cm, ci, ca, cb);
          v = bn_affine(g.z[(size_t)(r0 + r) * C + c], cm, ca, cb);
        }
      }
      HC[i] = v;
    }
  }
  __syncthreads();
  for (int nt = wave; nt < NT; nt += kWaves) {
    const int n = nt * 16 + li;
    const bool nok = n < C;
    const float* const wrow = g.w_mix + (size_t)min(n, C - 1) * C;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int qd = 0; qd < Q; ++qd) {
      const int k = 16 * qd + 4 * lg;
      const f4 a = *reinterpret_cast<const f4*>(HC + li * P + k);
      f4 b;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = nok && k + i < C;
        const float wv = wrow[ok ? k + i : 0];
        b[i] = ok ? wv : 0.f;
      }
      quad_fma(acc, a, b);
    }
    if (nok) {
      const float bn = g.b_mix ? g.b_mix[n] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lg + i;
        if (r < nrows) {
          const size_t row = (size_t)(r0 + r);
          const float p = acc[i] + bn;
          g.p[row * C + n] = p;
          float o = leaky(p, g.slope);
          if (g.residual) o = g.h[row * g.ldh + n] + o;
          g.out[row * g.ld_out + n] = o;
        }
      }
    }
  }
}

// ---- backward, launch 1: g_p = grad_out leaky'(p), hcat (both stored for the mixing weight's gradient), g_hcat = g_p W_mix (stored),
// the tile's column sums of g_hcat and g_hcat xhat.  DROP (pna_tower_drop_train_bwd_f32): the forward's mask, regenerated from the key --
// the stored hcat is the masked one, g_hcat = mask * (g_p W_mix) before it is stored and before the column sums ----
template <bool DROP>
__global__ __launch_bounds__(kThreads) void k_tt_mix_bwd(const KArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int C = g.C, Q = quads(C), P = pitch_of(Q), NT = (C + 15) / 16, PG = C + 1;
  float* const GP = lds;                                    // [16][P]  g_p
  float* const GH = GP + kRows * P;                         // [16][PG] g_hcat
  const int r0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.V - r0);
  for (int i = tid; i < kRows * P; i += kThreads) {
    const int r = i / P, c = i - r * P;
    float v = 0.f;
    if (c < C && r < nrows) {
      const size_t row = (size_t)(r0 + r);
      const float p = g.p[row * C + c], go = g.go[row * g.ld_go + c];
      v = p > 0.f ? go : go * g.slope;
      g.gp[row * C + c] = v;
      if constexpr (!DROP) {
        if (g.nobn) {
          g.hcat[row * C + c] = g.z[row * C + c];
        } else {
          float cm, ci, ca, cb;
          bn_consts(g, c, cm, ci, ca, cb);
          g.hcat[row * C + c] = bn_affine(g.z[row * C + c], cm, ca, cb);
        }
      }
    }
    GP[i] = v;
  }
  if constexpr (DROP) {
    // the masked hcat, and the mask's factor parked in GH where the g_hcat of the same element lands below
    tile_mask_each(g, r0, nrows, tid, [&](int r, int c, bool keep) {
      const size_t row = (size_t)(r0 + r);
      float cm, ci, ca, cb;
      bn_consts(g, c, cm, ci, ca, cb);
      const float v = bn_affine(g.z[row * C + c], cm, ca, cb);
      g.hcat[row * C + c] = keep ? v * g.drop.scale : 0.f;
      GH[r * PG + c] = keep ? g.drop.scale : 0.f;
    });
  }
  __syncthreads();
  // g_hcat tile (16 rows x 16 columns j): A = g_p (K = the mixing output n), B[k = n][j] = W_mix[n][j]
  for (int jt = wave; jt < NT; jt += kWaves) {
    const int j = jt * 16 + li;
    const bool jok = j < C;
    const int jj = min(j, C - 1);
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int qd = 0; qd < Q; ++qd) {
      const int k = 16 * qd + 4 * lg;
      const f4 a = *reinterpret_cast<const f4*>(GP + li * P + k);
      f4 b;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float wv = g.w_mix[(size_t)min(k + i, C - 1) * C + jj];
        b[i] = (jok && k + i < C) ? wv : 0.f;
      }
      quad_fma(acc, a, b);
    }
    if (jok) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lg + i;
        if constexpr (DROP) {
          const float gv = (r < nrows && GH[r * PG + j] > 0.f) ? acc[i] * g.drop.scale : 0.f;     // (rows past the end hold no factor)
          GH[r * PG + j] = gv;
          if (r < nrows) g.ghc[(size_t)(r0 + r) * C + j] = gv;
        } else {
          GH[r * PG + j] = acc[i];
          if (r < nrows) g.ghc[(size_t)(r0 + r) * C + j] = acc[i];
        }
      }
    }
  }
  if (g.nobn) return;                                       // (uniform: no mean terms, no grad_gamma / grad_beta)
  __syncthreads();
  for (int c = tid; c < C; c += kThreads) {
    const float cm = g.mean[c], ci = g.invstd[c];
    float s0 = 0.f, s1 = 0.f;
    for (int r = 0; r < nrows; ++r) {
      const float gv = GH[r * PG + c];
      s0 = s0 + gv;
      s1 = s1 + gv * ((g.z[(size_t)(r0 + r) * C + c] - cm) * ci);
    }
    g.part[((size_t)blockIdx.x * 2 + 0) * C + c] = s0;
    g.part[((size_t)blockIdx.x * 2 + 1) * C + c] = s1;
  }
}

// ---- backward, launch 2: one workgroup per column -- the tiles' sums in float64 in a fixed order: grad_beta, grad_gamma, the two means ----
__global__ __launch_bounds__(256) void k_tt_bwd_finalize(const KArgs g) {
  __shared__ double red[2][256];
  const int c = blockIdx.x, C = g.C;
  double t0 = 0.0, t1 = 0.0;
  for (int t = threadIdx.x; t < g.n_part; t += 256) {
    t0 += (double)g.part[((size_t)t * 2 + 0) * C + c];
    t1 += (double)g.part[((size_t)t * 2 + 1) * C + c];
  }
  red[0][threadIdx.x] = t0; red[1][threadIdx.x] = t1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { red[0][threadIdx.x] += red[0][threadIdx.x + s]; red[1][threadIdx.x] += red[1][threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const int t = c / g.Fo, n = c - t * g.Fo;
  g.cm[c] = (float)(red[0][0] / (double)g.V);
  g.cm[C + c] = (float)(red[1][0] / (double)g.V);
  if (g.gbeta[t]) g.gbeta[t][n] = (float)red[0][0];
  if (g.ggamma[t]) g.ggamma[t][n] = (float)red[1][0];
}

// ---- backward, launch 3: gz = n[v] gamma invstd (g - mean g - xhat mean(g xhat)) (stored) and, per tower, G = sum_s scale_s (gz_t W_s)
// of 16 rows into gagg's blocks, a's layout ([G_mean | G_max | G_min | G_std]) ----
template <int S>
__global__ __launch_bounds__(kThreads) void k_tt_rows_bwd(const KArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int Fi = g.Fi, Fo = g.Fo, T = g.T, C = g.C, K = g.K, QN = quads(Fo), PN = pitch_of(QN), NTJ = (K + 15) / 16;
  float* const GZ = lds;                                    // [T][16][PN] gz, a padded block per tower
  float* const SC = GZ + T * kRows * PN;                    // [4][16]
  const int r0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.V - r0);
  if (tid < 4 * kRows) {
    const int s = tid >> 4, r = tid & 15;
    const float* p = s == 3 ? g.snorm : (s < S ? g.scale[s] : nullptr);
    SC[tid] = (p && r < nrows) ? p[r0 + r] : 1.f;
  }
  __syncthreads();
  for (int i = tid; i < T * kRows * PN; i += kThreads) {
    const int t = i / (kRows * PN), rem = i - t * kRows * PN, r = rem / PN, n = rem - r * PN;
    float val = 0.f;
    if (n < Fo && r < nrows) {
      const int c = t * Fo + n;
      const size_t row = (size_t)(r0 + r);
      if (g.nobn) {
        val = g.ghc[row * C + c];
      } else {
        float cm, ci, ca, cb;
        bn_consts(g, c, cm, ci, ca, cb);
        // pna_bn_tail's backward apply, op by op; the graph-norm factor last
        val = ca * ((g.ghc[row * C + c] - g.cm[c]) - ((g.z[row * C + c] - cm) * ci) * g.cm[C + c]);
      }
      if (g.snorm) val = val * SC[3 * kRows + r];
      g.gz[row * C + c] = val;
    }
    GZ[i] = val;
  }
  __syncthreads();
  // G tile (16 rows x 16 columns of the tower's K) per wavefront: A = gz_t (K = Fo), B[k = n][j] = W_post,t[n][Fi + s K + j]
  for (int u = wave; u < T * NTJ; u += kWaves) {
    const int t = u / NTJ, jt = u - t * NTJ;
    const int j = jt * 16 + li;
    const bool jok = j < K;
    const int jj = min(j, K - 1);
    const float* const w = g.w_post[t] + Fi + jj;
    const long ldw = (long)Fi + (long)S * K;
    f4 acc[S];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = (f4){0.f, 0.f, 0.f, 0.f};
    for (int qd = 0; qd < QN; ++qd) {
      const int k = 16 * qd + 4 * lg;
      const f4 a = *reinterpret_cast<const f4*>(GZ + (t * kRows + li) * PN + k);
#pragma unroll
      for (int s = 0; s < S; ++s) {
        f4 b;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float wv = w[(size_t)min(k + i, Fo - 1) * ldw + (size_t)s * K];
          b[i] = (jok && k + i < Fo) ? wv : 0.f;
        }
        quad_fma(acc[s], a, b);
      }
    }
    if (jok) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lg + i;
        if (r < nrows) {
          float G = SC[r] * acc[0][i];
#pragma unroll
          for (int s = 1; s < S; ++s) G = G + SC[s * kRows + r] * acc[s][i];
          g.gagg[(size_t)(r0 + r) * T * K + (size_t)t * K + j] = G;
        }
      }
    }
  }
}

// ---- backward, after the pull: grad_h = [grad_out +] sum_t (gz_t W_h,t + gx_src,t W_a,t + gx_dst,t W_b,t) of 16 rows; a tower's slice
// when the input is divided, the towers added in tower order (in the accumulator) otherwise ----
__global__ __launch_bounds__(kThreads) void k_tt_grad_h(const KArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int Fi = g.Fi, Fo = g.Fo, T = g.T, TFi = g.TFi, C = g.C, KK = Fo + 2 * Fi, Q = quads(KK), P = pitch_of(Q);
  const int NTI = (Fi + 15) / 16;                           // <= 8: a wavefront owns at most one column tile
  const int in_dim = g.div ? TFi : Fi;
  float* const A = lds;                                     // [16][P] one tower's [gz_t | gx_src,t | gx_dst,t]
  const int r0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.V - r0);
  const int i0 = wave * 16 + li;                            // this lane's input column inside the tower
  const bool iok = wave < NTI && i0 < Fi;
  const int ii = min(i0, Fi - 1);
  f4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < T; ++t) {
    __syncthreads();
    for (int i = tid; i < kRows * P; i += kThreads) {
      const int r = i / P, k = i - r * P;
      float v = 0.f;
      if (k < KK && r < nrows) {
        const size_t row = (size_t)(r0 + r);
        v = k < Fo ? g.gz[row * C + t * Fo + k] : (k < Fo + Fi ? g.gxs[row * TFi + t * Fi + (k - Fo)] : g.gxd[row * TFi + t * Fi + (k - Fo - Fi)]);
      }
      A[i] = v;
    }
    __syncthreads();
    if (wave < NTI) {
      const float* const wpost = g.w_post[t] + ii;          // W_h,t[k][i]: row k of the posttrans weight, column i
      const float* const wpre = g.w_pre[t];
      const long ldpost = (long)Fi + (long)g.S * g.K;
      for (int qd = 0; qd < Q; ++qd) {
        const int k = 16 * qd + 4 * lg;
        const f4 a = *reinterpret_cast<const f4*>(A + li * P + k);
        f4 b;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int kk = min(k + i, KK - 1);
          float wv;
          if (kk < Fo) wv = wpost[(size_t)kk * ldpost];
          else if (kk < Fo + Fi) wv = wpre[(size_t)(kk - Fo) * g.ldw_pre + ii];
          else wv = wpre[(size_t)(kk - Fo - Fi) * g.ldw_pre + Fi + ii];
          b[i] = (iok && k + i < KK) ? wv : 0.f;
        }
        quad_fma(acc, a, b);
      }
      if (g.div || t == T - 1) {
        if (iok) {
          const int col = (g.div ? t * Fi : 0) + i0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * lg + i;
            if (r < nrows) {
              const size_t row = (size_t)(r0 + r);
              g.gh[row * in_dim + col] = g.residual ? g.go[row * g.ld_go + col] + acc[i] : acc[i];
            }
          }
        }
        acc = (f4){0.f, 0.f, 0.f, 0.f};
      }
    }
  }
}

// ---- backward, after the rows kernel (the routes with edge features and the one with an aggregator list): the message gradient per
// edge, destination row by destination row over the FORWARD CSR (a wavefront owns rows wave, wave + 8; a lane owns columns lane and
// lane + 64 of a tower).  Only the listed terms appear; m0[k] = x_src[u] [+ x_edge[k]] (EDGE), mean0 = the saved row mean of m0 where
// there is one, else mean[v] - x_dst[v]:
//   dm[k] = (G_mean[v] / D + G_sum[v]) + ([std^2 - 1e-5 > 0] G_std[v] / (std[v] D) + [var > 0] 2 G_var[v] / D) (m0[k] - mean0)
//           + [k = argmax[v]] G_max[v] + [k = argmin[v]] G_min[v]
// gx_dst[v] = G_mean + G_max + G_min + D G_sum (the variance terms sum to zero over a row; 0 for a row without in-edges), and with EDGE
// the CSR-ordered copy of e that the W_e weight gradient reads.  With {mean, max, min, std} the operations and their order are those
// of the route with edge features before the list existed ----
template <bool EDGE>
__global__ __launch_bounds__(kThreads) void k_tt_edge_dm(const KArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Fi = g.Fi, T = g.T, TFi = g.TFi, K = g.K, ED = g.ED;
  const bool spread = g.b_std >= 0 || g.b_var >= 0;         // whether any term reads the messages themselves
  const int r0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.V - r0);
  for (int r = wave; r < nrows; r += kWaves) {
    const int row = r0 + r;
    const int beg = g.rowptr[row], end = g.rowptr[row + 1], D = end - beg;
    if constexpr (EDGE) {
      if (lane < ED)
        for (int k = beg; k < end; ++k) g.ecsr[(size_t)k * ED + lane] = g.e[(size_t)g.eid[k] * g.ld_e + lane];
    }
    const float fD = (float)D, invD = D > 0 ? 1.0f / fD : 0.f;
    for (int t = 0; t < T; ++t) {
      const float* const xs = g.xcat + t * Fi;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j, cc = min(c, Fi - 1);   // (lanes past the last column redo it; not stored)
        const bool ok = c < Fi;
        if (j == 1 && Fi <= 64) continue;                   // (wavefront-uniform, like every branch on the list below)
        const size_t oa = (size_t)row * T * K + (size_t)t * K + cc, oc = (size_t)row * TFi + t * Fi + cc;
        float Gm = 0.f, Gx = 0.f, Gn = 0.f, Gs = 0.f, mean = 0.f, sd = 0.f;
        int ax = -1, an = -1;
        if (g.b_mean >= 0) { Gm = g.gagg[oa + g.b_mean * Fi]; mean = g.a[oa + g.b_mean * Fi]; }
        if (g.b_max >= 0) { Gx = g.gagg[oa + g.b_max * Fi]; ax = g.amx[oc]; }
        if (g.b_min >= 0) { Gn = g.gagg[oa + g.b_min * Fi]; an = g.amn[oc]; }
        if (g.b_std >= 0) { Gs = g.gagg[oa + g.b_std * Fi]; sd = g.a[oa + g.b_std * Fi]; }
        const float xd = xs[(size_t)row * 2 * TFi + TFi + cc];
        float r1 = Gm * invD;
        float r2 = (D > 0 && sd * sd - 1e-5f > 0.f) ? Gs / (sd * fD) : 0.f;
        float gd = (Gm + Gx) + Gn;
        if (g.b_sum >= 0) {
          const float Gu = g.gagg[oa + g.b_sum * Fi];
          r1 = r1 + Gu;
          gd = gd + fD * Gu;
        }
        if (g.b_var >= 0) {
          const float Gv = g.gagg[oa + g.b_var * Fi], vr = g.a[oa + g.b_var * Fi];
          r2 = r2 + ((D > 0 && (g.pyg || vr > 0.f)) ? (2.0f * Gv) / fD : 0.f);
        }
        const float sh = g.rowmean ? g.rowmean[oc] : mean - xd;     // the mean of m0 over the row
        if (ok) g.gxd[oc] = D > 0 ? gd : 0.f;
        for (int e = beg; e < end; e += kEU) {
          float m0[kEU] = {0.f, 0.f, 0.f, 0.f};
          if (spread) {
#pragma unroll
            for (int u = 0; u < kEU; ++u) {
              const int k = min(e + u, end - 1);
              m0[u] = xs[(size_t)g.col[k] * 2 * TFi + cc];
              if constexpr (EDGE) m0[u] = m0[u] + g.xedge[(size_t)k * TFi + t * Fi + cc];
            }
          }
#pragma unroll
          for (int u = 0; u < kEU; ++u)
            if (e + u < end) {                              // (wavefront-uniform)
              const int k = e + u;
              float d = r1;
              if (spread) d = r1 + r2 * (m0[u] - sh);
              d = d + (k == ax ? Gx : 0.f);
              d = d + (k == an ? Gn : 0.f);
              if (ok) g.dm[(size_t)k * TFi + t * Fi + c] = d;
            }
        }
      }
    }
  }
}

// ---- backward with edge features: gx_src[u] = sum of dm[pos_t[j]] over the source row's transposed edges in list order (one
// whole-row record {u, beg, end, -1} per source row: no segments, no atomics); a wavefront owns records wave, wave + 8 of 16, a lane
// one column of 64 at a time, four rows' loads in flight ----
__global__ __launch_bounds__(kThreads) void k_tt_edge_pull(const KArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int TFi = g.TFi;
  const int r0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.V - r0);
  for (int r = wave; r < nrows; r += kWaves) {
    const int32_t* const rec = g.items_t + 4 * (size_t)(r0 + r);
    const int u = rec[0], beg = rec[1], end = rec[2];
    for (int cb = 0; cb < TFi; cb += 64) {
      const int c = cb + lane, cc = min(c, TFi - 1);
      float acc = 0.f;
      for (int j = beg; j < end; j += kEU) {
        float v[kEU];
#pragma unroll
        for (int i = 0; i < kEU; ++i) v[i] = g.dm[(size_t)g.pos_t[min(j + i, end - 1)] * TFi + cc];
#pragma unroll
        for (int i = 0; i < kEU; ++i)
          if (j + i < end) acc = acc + v[i];                // (wavefront-uniform)
      }
      if (c < TFi) g.gxs[(size_t)u * TFi + c] = acc;
    }
  }
}

// ---- backward with edge features, when grad_e is wanted: grad_e[eid[k]] = sum_t dm_t[k] W_e,t of 16 CSR edges; the accumulator is
// kept across the towers; every row of grad_e is written exactly once, through the permutation ----
__global__ __launch_bounds__(kThreads) void k_tt_edge_grad_e(const KArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int Fi = g.Fi, T = g.T, TFi = g.TFi, ED = g.ED, Q = quads(Fi), P = pitch_of(Q);
  const int NTJ = (ED + 15) / 16;                           // <= 4: a wavefront owns at most one column tile
  float* const A = lds;                                     // [16][P] one tower's dm rows
  const int k0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.E - k0);
  const int j0 = wave * 16 + li;                            // this lane's column of e
  const bool jok = wave < NTJ && j0 < ED;
  const int jj = min(j0, ED - 1);
  f4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < T; ++t) {
    __syncthreads();
    for (int i = tid; i < kRows * P; i += kThreads) {
      const int r = i / P, k = i - r * P;
      A[i] = (k < Fi && r < nrows) ? g.dm[(size_t)(k0 + r) * TFi + t * Fi + k] : 0.f;
    }
    __syncthreads();
    if (wave < NTJ) {
      const float* const w = g.w_pre[t] + 2 * Fi + jj;      // W_e,t[k][j]: row k of the pretrans weight, column 2 Fi + j
      for (int qd = 0; qd < Q; ++qd) {
        const int k = 16 * qd + 4 * lg;
        const f4 a = *reinterpret_cast<const f4*>(A + li * P + k);
        f4 b;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float wv = w[(size_t)min(k + i, Fi - 1) * g.ldw_pre];
          b[i] = (jok && k + i < Fi) ? wv : 0.f;
        }
        quad_fma(acc, a, b);
      }
    }
  }
  if (jok) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * lg + i;
      if (r < nrows) g.ge[(size_t)g.eid[k0 + r] * g.ld_ge + j0] = acc[i];
    }
  }
}

// ---- a weight gradient outside pna_posttrans_dw_f32's shape limits: gw[n][k] = sum_v [scale[v]] gy[v][n] a[v][k], one thread per (n, k),
// the rows in sequence (fp32, a fixed order).  gb[n] = sum_v gy[v][n] from the threads of k = 0. ----
__global__ __launch_bounds__(256) void k_tt_dw_plain(const float* gy, long ldg, int N, const float* a, long lda, int K, const float* scale, int V,
                                                     float* gw, long ldw, float* gb) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * K) return;
  const int n = (int)(i / K), k = (int)(i - (long)n * K);
  float acc = 0.f, sb = 0.f;
  for (int v = 0; v < V; ++v) {
    const float gv = gy[(size_t)v * ldg + n], av = a[(size_t)v * lda + k];
    sb = sb + gv;
    acc = acc + ((scale ? scale[v] : 1.f) * gv) * av;
  }
  gw[(size_t)n * ldw + k] = acc;
  if (k == 0 && gb) gb[n] = sb;
}

inline int64_t up64(int64_t floats) { return (floats + 63) / 64 * 64; }     // workspace pieces at 256-byte boundaries

struct Layout {
  int64_t part_fwd, part_bwd, cm, gp, hcat, ghc, gz, gagg, gxs, gxd, packed, dm, ecsr, dw, total;      // offsets in floats
  int64_t pitch, dw_bytes;
  int n_tile;
};

bool in_scope(int64_t V, int64_t E, int T, int Fi, int Fo, int S, int div) {
  return V >= 2 && V < (1ll << 31) - kRows && E >= 0 && E < (1ll << 31) && T >= 1 && T <= kMaxT && Fi >= 4 && Fi <= kMaxFi && (int64_t)T * Fi <= kMaxIn &&
         Fo >= 1 && (int64_t)T * Fo <= kMaxC && S >= 1 && S <= 3 && (div == 0 || div == 1);
}

// pna_posttrans_dw_f32's shape limits and workspace (include/pna_amd.h: N <= 128, n_scaler N <= 240, K + Kh + 1 <= 384; one 240 x 384 fp32 partial
// per slab of >= 256 rows -- how many slabs depends on the device: room for the most it can ask for), restated here so that a call
// of this route asks the runtime nothing
bool dw_takes(int N, int S, int K, int Kh) { return N <= 128 && S * N <= 240 && K + Kh + 1 <= 384; }      // (every N of this file is <= 128)
int64_t dw_bytes_of(int64_t V, int N, int S, int K, int Kh) { return dw_takes(N, S, K, Kh) ? (int64_t)240 * 384 * 4 * ((V + 255) / 256) : 0; }

// The aggregator list of a call: how many, each one's block inside a tower's aggregate (-1 = not listed; indexed by PNA_AGG_MEAN ..
// PNA_AGG_VAR), and what pna_tower_aggr_train_args carries beside the three older blocks.  general: the call came through
// pna_tower_aggr_train_*_f32 -- its backward is the per-edge one whether there are edge features or not
struct Aggr {
  int A, b[6];
  bool general;
  float* row_mean;
  const int32_t* pos_t;
  bool pyg;                     // pna_pyg_conv_train_*: no BatchNorm and the PyG statistics
};
const Aggr kStandard = {4, {0, -1, 1, 2, 3, -1}, false, nullptr, nullptr, false};      // mean | max | min | std

// the list of a pna_tower_aggr_train call: 1..4 distinct codes out of PNA_AGG_MEAN .. PNA_AGG_VAR
bool read_list(int n_aggr, const int32_t* aggr, Aggr& ag) {
  if (n_aggr < 1 || n_aggr > 4 || !aggr) return false;
  ag.A = n_aggr;
  for (int i = 0; i < 6; ++i) ag.b[i] = -1;
  for (int i = 0; i < n_aggr; ++i) {
    if (aggr[i] < PNA_AGG_MEAN || aggr[i] > PNA_AGG_VAR || ag.b[aggr[i]] >= 0) return false;
    ag.b[aggr[i]] = i;
  }
  ag.general = true; ag.row_mean = nullptr; ag.pos_t = nullptr; ag.pyg = false;
  return true;
}
bool needs_row_mean(const Aggr& ag) { return (ag.b[PNA_AGG_STD] >= 0 || ag.b[PNA_AGG_VAR] >= 0) && ag.b[PNA_AGG_MEAN] < 0; }

// ED == 0: the route without edge features.  ED > 0: no packed rows (its pull reads dm), + dm (E, T Fi) and the CSR-ordered copy of e.
// A: the listed aggregators; per_edge: the backward forms dm also without edge features (no packed rows either way)
Layout layout_of(int64_t V, int T, int Fi, int Fo, int S, int64_t E = 0, int ED = 0, int A = 4, bool per_edge = false) {
  Layout l;
  const int64_t C = (int64_t)T * Fo, TFi = (int64_t)T * Fi;
  l.n_tile = (int)((V + kRows - 1) / kRows);
  l.pitch = (5 * TFi + 31) / 32 * 32;
  l.part_fwd = 0;
  l.part_bwd = l.part_fwd + up64((int64_t)l.n_tile * 2 * C);
  l.cm = l.part_bwd + up64((int64_t)l.n_tile * 2 * C);
  l.gp = l.cm + up64(2 * C);
  l.hcat = l.gp + up64(V * C);
  l.ghc = l.hcat + up64(V * C);
  l.gz = l.ghc + up64(V * C);
  l.gagg = l.gz + up64(V * C);
  l.gxs = l.gagg + up64(V * A * TFi);
  l.gxd = l.gxs + up64(V * TFi);
  l.packed = l.gxd + up64(V * TFi);
  l.dm = l.packed + ((ED > 0 || per_edge) ? 0 : up64(V * l.pitch));
  l.ecsr = l.dm + ((ED > 0 || per_edge) ? up64(E * TFi) : 0);
  l.dw = l.ecsr + (ED > 0 ? up64(E * ED) : 0);
  int64_t b = dw_bytes_of(V, Fo, S, A * Fi, Fi);
  const int64_t b1 = dw_bytes_of(V, Fi, 1, Fi, 0), b2 = dw_bytes_of(V, (int)C, 1, (int)C, 0), b3 = ED > 0 ? dw_bytes_of(E, Fi, 1, ED, 0) : 0;
  b = b > b1 ? b : b1;
  b = b > b2 ? b : b2;
  l.dw_bytes = b > b3 ? b : b3;
  l.total = l.dw + up64((l.dw_bytes + 3) / 4);
  return l;
}

// q != NULL: the call with edge features (pna_tower_edge_train_*): its own checks, the wider pretrans weight, the larger workspace.
// ag: the aggregator list (the three older entry pairs: kStandard)
int fill(const pna_tower_train_args* p, KArgs& g, Layout& l, bool bwd, const char* who, const pna_tower_edge_train_args* q = nullptr,
         const Aggr& ag = kStandard) {
  if (!p) return pna_set_error(PNA_E_INVALID, who);
  if (int rc_ss = pna_check_struct_size(bwd ? "pna_tower_train_bwd_f32" : "pna_tower_train_fwd_f32", p->struct_size, sizeof(*p))) return rc_ss;
  const int T = p->n_tower, Fi = p->Fi, Fo = p->Fo, S = p->n_scaler;
  if (!in_scope(p->V, p->E, T, Fi, Fo, S, p->divide_input)) return pna_set_error(PNA_E_INVALID, who);
  const int in_dim = p->divide_input ? T * Fi : Fi, C = T * Fo;
  if (p->residual && in_dim != C) return pna_set_error(PNA_E_INVALID, who);
  if (!p->rowptr || (p->E > 0 && !p->col) || !p->h || p->ldh < in_dim || !p->w_mix || !p->x_cat || !p->a || (ag.b[PNA_AGG_MAX] >= 0 && !p->argmax) || (ag.b[PNA_AGG_MIN] >= 0 && !p->argmin) || !p->z || !p->p ||
      (!ag.pyg && (!p->save_mean || !p->save_invstd)) || !p->workspace || ((uintptr_t)p->workspace & 255))
    return pna_set_error(PNA_E_INVALID, who);
  for (int t = 0; t < T; ++t)
    if (!p->w_pre[t] || !p->b_pre[t] || !p->w_post[t] || !p->b_post[t] || (p->gamma[t] == nullptr) != (p->beta[t] == nullptr) ||
        (p->gamma[t] == nullptr) != (p->gamma[0] == nullptr) || (p->running_mean[t] == nullptr) != (p->running_var[t] == nullptr))
      return pna_set_error(PNA_E_INVALID, who);
  if (!bwd && (!p->out || p->ld_out < C)) return pna_set_error(PNA_E_INVALID, who);
  if (bwd) {
    if (!p->grad_out || p->ld_go < C || !p->grad_h || !p->grad_w_mix || !p->grad_b_mix || !p->items_t || p->n_items_t != p->V)
      return pna_set_error(PNA_E_INVALID, who);
    if (!q && !ag.general && (!p->col_t || !p->rank_t)) return pna_set_error(PNA_E_INVALID, who);      // (the per-edge pull reads pos_t instead)
    if (!q && ag.general && p->E > 0 && !ag.pos_t) return pna_set_error(PNA_E_INVALID, who);
    for (int t = 0; t < T; ++t)
      if (!p->grad_w_pre[t] || !p->grad_b_pre[t] || !p->grad_w_post[t] || !p->grad_b_post[t] || (p->gamma[t] && (!p->grad_gamma[t] || !p->grad_beta[t])))
        return pna_set_error(PNA_E_INVALID, who);
  }
  const int ED = q ? q->edge_dim : 0;
  if (q) {
    if (ED < 1 || ED > kMaxED) return pna_set_error(PNA_E_INVALID, who);
    if (p->E > 0 && (!q->e || q->ld_e < ED || !q->eid || !q->x_edge || (bwd && !q->pos_t))) return pna_set_error(PNA_E_INVALID, who);
    if (bwd && q->grad_e && q->ld_ge < ED) return pna_set_error(PNA_E_INVALID, who);
  }
  if (ag.general && needs_row_mean(ag) && !ag.row_mean) return pna_set_error(PNA_E_INVALID, who);
  l = layout_of(p->V, T, Fi, Fo, S, p->E, ED, ag.A, ag.general);
  if (p->workspace_bytes < l.total * 4) return pna_set_error(PNA_E_INVALID, who);
  memset(&g, 0, sizeof(g));
  float* const ws = (float*)p->workspace;
  g.rowptr = p->rowptr; g.col = p->col; g.V = p->V; g.T = T; g.Fi = Fi; g.Fo = Fo; g.S = S; g.C = C; g.TFi = T * Fi;
  g.div = p->divide_input; g.residual = p->residual != 0;
  g.K = ag.A * Fi;
  g.b_mean = ag.b[PNA_AGG_MEAN]; g.b_sum = ag.b[PNA_AGG_SUM]; g.b_max = ag.b[PNA_AGG_MAX]; g.b_min = ag.b[PNA_AGG_MIN];
  g.b_std = ag.b[PNA_AGG_STD]; g.b_var = ag.b[PNA_AGG_VAR];
  g.rowmean = needs_row_mean(ag) ? ag.row_mean : nullptr;
  g.nobn = ag.pyg; g.pyg = ag.pyg;
  g.h = p->h; g.ldh = (long)p->ldh; g.snorm = p->snorm_n;
  for (int s = 0; s < 3; ++s) g.scale[s] = s < S ? p->row_scale[s] : nullptr;
  for (int t = 0; t < T; ++t) {
    g.w_pre[t] = p->w_pre[t]; g.b_pre[t] = p->b_pre[t]; g.w_post[t] = p->w_post[t]; g.b_post[t] = p->b_post[t];
    g.gamma[t] = p->gamma[t]; g.beta[t] = p->beta[t]; g.rmean[t] = p->running_mean[t]; g.rvar[t] = p->running_var[t];
    g.ggamma[t] = p->grad_gamma[t]; g.gbeta[t] = p->grad_beta[t];
  }
  g.w_mix = p->w_mix; g.b_mix = p->b_mix; g.slope = p->slope; g.eps = p->eps; g.momentum = p->momentum;
  g.xcat = p->x_cat; g.a = p->a; g.amx = p->argmax; g.amn = p->argmin; g.z = p->z; g.p = p->p; g.mean = p->save_mean; g.invstd = p->save_invstd;
  g.out = p->out; g.ld_out = (long)p->ld_out; g.go = p->grad_out; g.ld_go = (long)p->ld_go;
  g.part = ws + (bwd ? l.part_bwd : l.part_fwd); g.n_part = l.n_tile;
  g.cm = ws + l.cm; g.gp = ws + l.gp; g.hcat = ws + l.hcat; g.ghc = ws + l.ghc; g.gz = ws + l.gz; g.gagg = ws + l.gagg;
  g.gxs = ws + l.gxs; g.gxd = ws + l.gxd; g.gh = p->grad_h;
  g.ldw_pre = 2L * Fi + ED; g.E = p->E; g.ED = ED;
  if (q) {
    g.e = q->e; g.ld_e = (long)q->ld_e; g.eid = q->eid; g.xedge = q->x_edge; g.pos_t = q->pos_t; g.items_t = p->items_t;
    g.dm = ws + l.dm; g.ecsr = ws + l.ecsr; g.ge = q->grad_e; g.ld_ge = (long)q->ld_ge;
  } else if (ag.general) {
    g.pos_t = ag.pos_t; g.items_t = p->items_t; g.dm = ws + l.dm;
  }
  return PNA_OK;
}

// gw (N, ldw) [+ gb] = gy^T [h | scale_s a]: pna_posttrans_dw_f32's kernel where its shape limits hold (and the first scaler is the
// identity when it forms an h panel or a bias), the plain fp32 kernel otherwise
int weight_grad(const float* gy, int64_t ldg, int N, const float* a, int64_t lda, int K, const float* h, int64_t ldh, int Kh, int S,
                const float* const* scale, int64_t V, float* gw, int64_t ldw, float* gb, void* ws, int64_t ws_bytes, hipStream_t st) {
  if (V > 0 && dw_takes(N, S, K, Kh) && !(scale && scale[0])) {
    pna_posttrans_dw_args d;
    memset(&d, 0, sizeof(d));
    d.struct_size = (uint32_t)sizeof(d);
    d.gy = gy; d.ldg = ldg; d.M = V; d.N = N; d.n_scaler = S; d.a = a; d.lda = lda; d.K = K; d.Kh = Kh; d.h = h; d.ldh = ldh;
    for (int s = 0; s < S; ++s) d.row_scale[s] = scale ? scale[s] : nullptr;
    d.grad_w = gw; d.ldw = ldw; d.grad_b = gb;
    d.workspace = ws; d.workspace_bytes = ws_bytes;
    return pna_posttrans_dw_f32(&d, (pna_stream_t)st);
  }
  const dim3 bd(256);
  if (Kh > 0) {
    const long n = (long)N * Kh;
    hipLaunchKernelGGL(k_tt_dw_plain, dim3((unsigned)((n + 255) / 256)), bd, 0, st, gy, (long)ldg, N, h, (long)ldh, Kh, (const float*)nullptr, (int)V, gw, (long)ldw, gb);
  }
  const long n = (long)N * K;
  for (int s = 0; s < S; ++s)
    hipLaunchKernelGGL(k_tt_dw_plain, dim3((unsigned)((n + 255) / 256)), bd, 0, st, gy, (long)ldg, N, a, (long)lda, K, scale ? scale[s] : (const float*)nullptr, (int)V,
                       gw + Kh + (size_t)s * K, (long)ldw, (Kh == 0 && s == 0) ? gb : (float*)nullptr);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_tower_train_bwd_f32: launch failed");
  return PNA_OK;
}

template <bool EDGE, bool DROP = false>
int launch_fwd(const KArgs& g, const Layout& l, hipStream_t st, const char* failed) {
  const int Fi = g.Fi, C = g.C, in_dim = g.div ? g.TFi : Fi;
  const dim3 grid((unsigned)l.n_tile), block(kThreads);
  hipLaunchKernelGGL(k_tt_project, grid, block, (size_t)kRows * (in_dim + 1) * sizeof(float), st, g);                   // <= 33 KB
  if (EDGE && g.E > 0)
    hipLaunchKernelGGL(k_tt_edge_project, dim3((unsigned)((g.E + kRows - 1) / kRows)), block, (size_t)kRows * pitch_of(quads(g.ED)) * sizeof(float), st, g);
  const size_t lds = ((size_t)kRows * pitch_of(quads(g.K)) + (size_t)kRows * pitch_of(quads(Fi)) + (size_t)kRows * (C + 1) + 4 * kRows) * sizeof(float);   // <= 50 KB
  if (g.S == 1) hipLaunchKernelGGL((k_tt_rows_fwd<1, EDGE>), grid, block, lds, st, g);
  else if (g.S == 2) hipLaunchKernelGGL((k_tt_rows_fwd<2, EDGE>), grid, block, lds, st, g);
  else hipLaunchKernelGGL((k_tt_rows_fwd<3, EDGE>), grid, block, lds, st, g);
  if (!g.nobn) hipLaunchKernelGGL(k_tt_bn_finalize, dim3((unsigned)C), dim3(256), 0, st, g);
  hipLaunchKernelGGL(k_tt_mix_fwd<DROP>, grid, block, (size_t)kRows * pitch_of(quads(C)) * sizeof(float), st, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, failed);
  return PNA_OK;
}

// q != NULL: the backward with edge features -- the per-edge message gradient and its pull instead of rowprep + the ranked pull;
// per_edge: the same without edge features (the call with an aggregator list)
int launch_bwd(const pna_tower_train_args* p, const KArgs& g, const Layout& l, pna_stream_t stream, const pna_tower_edge_train_args* q, const char* failed,
               bool drop = false, bool per_edge = false) {
  hipStream_t st = (hipStream_t)stream;
  const int T = g.T, Fi = g.Fi, Fo = g.Fo, S = g.S, C = g.C, TFi = g.TFi, K = g.K;
  const dim3 grid((unsigned)l.n_tile), block(kThreads);
  // 1. the mixing network, 2. the column sums, 3. gz and the aggregate's gradient
  const size_t lds_mix = ((size_t)kRows * pitch_of(quads(C)) + (size_t)kRows * (C + 1)) * sizeof(float);
  if (drop) hipLaunchKernelGGL(k_tt_mix_bwd<true>, grid, block, lds_mix, st, g);
  else hipLaunchKernelGGL(k_tt_mix_bwd<false>, grid, block, lds_mix, st, g);
  if (!g.nobn) hipLaunchKernelGGL(k_tt_bwd_finalize, dim3((unsigned)C), dim3(256), 0, st, g);
  const size_t lds = ((size_t)T * kRows * pitch_of(quads(Fo)) + 4 * kRows) * sizeof(float);
  if (S == 1) hipLaunchKernelGGL(k_tt_rows_bwd<1>, grid, block, lds, st, g);
  else if (S == 2) hipLaunchKernelGGL(k_tt_rows_bwd<2>, grid, block, lds, st, g);
  else hipLaunchKernelGGL(k_tt_rows_bwd<3>, grid, block, lds, st, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, failed);
  float* const ws = (float*)p->workspace;
  int rc2;
  if (q) {
    // 4. the message gradient per edge (and gx_dst, the CSR-ordered e), then its pull per source row: gx_src; grad_e when wanted
    hipLaunchKernelGGL(k_tt_edge_dm<true>, grid, block, 0, st, g);
    hipLaunchKernelGGL(k_tt_edge_pull, grid, block, 0, st, g);
    if (g.ge && g.E > 0)
      hipLaunchKernelGGL(k_tt_edge_grad_e, dim3((unsigned)((g.E + kRows - 1) / kRows)), block, (size_t)kRows * pitch_of(quads(Fi)) * sizeof(float), st, g);
  } else if (per_edge) {
    // 4. the same two launches on the messages without an x_edge term: no copy of e, no grad_e
    hipLaunchKernelGGL(k_tt_edge_dm<false>, grid, block, 0, st, g);
    hipLaunchKernelGGL(k_tt_edge_pull, grid, block, 0, st, g);
  } else {
    // 4. rowprep + ranked pull over the transposed graph, all towers: gx_src; rowprep's grad_dst is gx_dst
    pna_segreduce_bwd_args b;
    memset(&b, 0, sizeof(b));
    b.struct_size = (uint32_t)sizeof(b);
    b.rowptr = p->rowptr; b.col = p->col; b.V = p->V; b.F = Fi;
    b.x = p->x_cat; b.ldx = 2 * (int64_t)TFi;
    b.dst_term = p->x_cat + TFi; b.ld_dst = 2 * (int64_t)TFi;
    b.n_tower = T; b.n_aggr = 4; b.tower_stride_in = Fi;
    b.aggr[0] = PNA_AGG_MEAN; b.aggr[1] = PNA_AGG_MAX; b.aggr[2] = PNA_AGG_MIN; b.aggr[3] = PNA_AGG_STD;
    b.gagg = g.gagg; b.ld_g = (int64_t)T * K; b.tower_stride_g = K;
    b.mean = p->a; b.stdv = p->a + 3 * (size_t)Fi; b.ld_stat = (int64_t)T * K; b.tower_stride_stat = K;
    b.argmax = p->argmax; b.argmin = p->argmin; b.ld_arg = TFi;
    b.grad_x = g.gxs; b.ld_gx = TFi;
    b.grad_dst = g.gxd; b.ld_gd = TFi;
    pna_segreduce_bwd_pull_args pl;
    memset(&pl, 0, sizeof(pl));
    pl.struct_size = (uint32_t)sizeof(pl);
    float* const packed = ws + l.packed;
    pl.base = &b; pl.table = packed; pl.ld_table = l.pitch;
    pl.col_t = p->col_t; pl.rank_t = p->rank_t; pl.items_t = p->items_t; pl.n_items_t = p->n_items_t; pl.run_rowprep = 1;
    pl.ranks = (uint16_t*)(packed + 4 * (size_t)TFi); pl.ld_rank = 2 * l.pitch;
    rc2 = pna_segreduce_bwd_pull_launch(&pl, nullptr, 0, stream);
    if (rc2 != PNA_OK) return rc2;
  }
  // 5. grad_h
  hipLaunchKernelGGL(k_tt_grad_h, grid, block, (size_t)kRows * pitch_of(quads(Fo + 2 * Fi)) * sizeof(float), st, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, failed);
  // 6. the weight and bias gradients, tower by tower, then the mixing network's
  void* const dws = ws + l.dw;
  const int64_t ldwp = (int64_t)g.ldw_pre;
  for (int t = 0; t < T; ++t) {
    const float* const ht = p->h + (g.div ? t * Fi : 0);
    rc2 = weight_grad(g.gz + t * Fo, C, Fo, p->a + (size_t)t * K, (int64_t)T * K, K, ht, p->ldh, Fi, S, p->row_scale, p->V, p->grad_w_post[t], (int64_t)Fi + (int64_t)S * K,
                      p->grad_b_post[t], dws, l.dw_bytes, st);
    if (rc2 != PNA_OK) return rc2;
    rc2 = weight_grad(g.gxs + t * Fi, TFi, Fi, ht, p->ldh, Fi, nullptr, 0, 0, 1, nullptr, p->V, p->grad_w_pre[t], ldwp, nullptr, dws, l.dw_bytes, st);
    if (rc2 != PNA_OK) return rc2;
    rc2 = weight_grad(g.gxd + t * Fi, TFi, Fi, ht, p->ldh, Fi, nullptr, 0, 0, 1, nullptr, p->V, p->grad_w_pre[t] + Fi, ldwp, p->grad_b_pre[t], dws, l.dw_bytes, st);
    if (rc2 != PNA_OK) return rc2;
    if (q) {                                                // grad_W_e,t = dm_t^T e_csr over the E edges (zeros when there are none)
      rc2 = weight_grad(g.dm + t * Fi, TFi, Fi, g.ecsr, g.ED, g.ED, nullptr, 0, 0, 1, nullptr, g.E, p->grad_w_pre[t] + 2 * Fi, ldwp, nullptr, dws, l.dw_bytes, st);
      if (rc2 != PNA_OK) return rc2;
    }
  }
  return weight_grad(g.gp, C, C, g.hcat, C, C, nullptr, 0, 0, 1, nullptr, p->V, p->grad_w_mix, C, p->grad_b_mix, dws, l.dw_bytes, st);
}

const char* const kEdgeNeeds =
    ": needs a base inside pna_tower_train_*_f32's scope whose w_pre / grad_w_pre are (Fi, 2 Fi + edge_dim) and whose 256-byte aligned workspace "
    "has pna_tower_edge_train_workspace_bytes(V, E, n_tower, Fi, Fo, n_scaler, divide_input, edge_dim) bytes (backward: items_t with "
    "n_items_t == V), 1 <= edge_dim <= 64, and with E > 0: e (ld_e >= edge_dim), eid, x_edge, in the backward pos_t (grad_e: ld_ge >= edge_dim)";

int fill_edge(const pna_tower_edge_train_args* q, KArgs& g, Layout& l, bool bwd) {
  static const std::string fwd_msg = std::string("pna_tower_edge_train_fwd_f32") + kEdgeNeeds, bwd_msg = std::string("pna_tower_edge_train_bwd_f32") + kEdgeNeeds;
  const char* const who = bwd ? bwd_msg.c_str() : fwd_msg.c_str();
  if (!q) return pna_set_error(PNA_E_INVALID, who);
  if (int rc_ss = pna_check_struct_size(bwd ? "pna_tower_edge_train_bwd_f32" : "pna_tower_edge_train_fwd_f32", q->struct_size, sizeof(*q))) return rc_ss;
  return fill(q->base, g, l, bwd, who, q);
}

// pna_tower_drop_train_*: its own checks, then the base route's (with or without edge features); the mask's constants into g.drop
int fill_drop(const pna_tower_drop_args* d, KArgs& g, Layout& l, bool bwd) {
  const char* const who = bwd ? "pna_tower_drop_train_bwd_f32: needs 0 <= p < 1, a base pna_tower_train_bwd_f32 accepts and edge == NULL, or an edge "
                                "pna_tower_edge_train_bwd_f32 accepts with edge->base == base"
                              : "pna_tower_drop_train_fwd_f32: needs 0 <= p < 1, a base pna_tower_train_fwd_f32 accepts and edge == NULL, or an edge "
                                "pna_tower_edge_train_fwd_f32 accepts with edge->base == base";
  if (!d) return pna_set_error(PNA_E_INVALID, who);
  if (int rc_ss = pna_check_struct_size(bwd ? "pna_tower_drop_train_bwd_f32" : "pna_tower_drop_train_fwd_f32", d->struct_size, sizeof(*d))) return rc_ss;
  if (!(d->p >= 0.f && d->p < 1.f) || !d->base) return pna_set_error(PNA_E_INVALID, who);      // (a NaN fails both comparisons)
  if (d->edge) {
    if (int rc_ss = pna_check_struct_size(bwd ? "pna_tower_drop_train_bwd_f32" : "pna_tower_drop_train_fwd_f32", d->edge->struct_size, sizeof(*d->edge)))
      return rc_ss;
    if (d->edge->base != d->base) return pna_set_error(PNA_E_INVALID, who);
  }
  const int rc = fill(d->base, g, l, bwd, who, d->edge);
  if (rc != PNA_OK) return rc;
  g.drop = pna_philox::make_mask(d->p, d->seed, d->offset);
  return PNA_OK;
}

// pna_tower_aggr_train_*: the list and the consistency of the blocks, then the base route's checks under that list
// who_pyg != NULL: the call came through pna_pyg_conv_train_*_f32 (its message; no BatchNorm, the PyG statistics)
int fill_aggr(const pna_tower_aggr_train_args* r, KArgs& g, Layout& l, bool bwd, const char* who_pyg = nullptr) {
  static const char* const needs =
      ": needs 1 <= n_aggr <= 4 distinct codes PNA_AGG_MEAN .. PNA_AGG_VAR in aggr; a base inside pna_tower_train_*_f32's scope whose a is (V, n_tower n_aggr Fi) "
      "and whose w_post / grad_w_post are (Fo, (1 + n_aggr n_scaler) Fi), argmax where max is listed, argmin where min is listed; edge == NULL, or an edge "
      "pna_tower_edge_train_*_f32 accepts with edge->base == base; drop == NULL, or 0 <= p < 1 with drop->base == base and drop->edge == edge; row_mean "
      "(V, n_tower Fi) where std or var is listed and mean is not; in the backward with E > 0 and edge == NULL pos_t; a 256-byte aligned workspace of "
      "pna_tower_aggr_train_workspace_bytes(V, E, n_tower, Fi, Fo, n_scaler, divide_input, edge_dim, n_aggr, aggr) bytes";
  static const std::string fwd_msg = std::string("pna_tower_aggr_train_fwd_f32") + needs, bwd_msg = std::string("pna_tower_aggr_train_bwd_f32") + needs;
  const char* const who = who_pyg ? who_pyg : (bwd ? bwd_msg.c_str() : fwd_msg.c_str());
  const char* const fn = bwd ? "pna_tower_aggr_train_bwd_f32" : "pna_tower_aggr_train_fwd_f32";
  if (!r) return pna_set_error(PNA_E_INVALID, who);
  if (int rc_ss = pna_check_struct_size(fn, r->struct_size, sizeof(*r))) return rc_ss;
  Aggr ag;
  if (!read_list(r->n_aggr, r->aggr, ag) || !r->base) return pna_set_error(PNA_E_INVALID, who);
  if (r->edge) {
    if (int rc_ss = pna_check_struct_size(fn, r->edge->struct_size, sizeof(*r->edge))) return rc_ss;
    if (r->edge->base != r->base) return pna_set_error(PNA_E_INVALID, who);
  }
  if (r->drop) {
    if (int rc_ss = pna_check_struct_size(fn, r->drop->struct_size, sizeof(*r->drop))) return rc_ss;
    if (r->drop->base != r->base || r->drop->edge != r->edge || !(r->drop->p >= 0.f && r->drop->p < 1.f)) return pna_set_error(PNA_E_INVALID, who);
  }
  ag.row_mean = r->row_mean; ag.pos_t = r->pos_t; ag.pyg = who_pyg != nullptr;
  const int rc = fill(r->base, g, l, bwd, who, r->edge, ag);
  if (rc != PNA_OK) return rc;
  if (r->drop) g.drop = pna_philox::make_mask(r->drop->p, r->drop->seed, r->drop->offset);
  return PNA_OK;
}

// out[v, c] = the factor of element (v, c) under the mask rule: 0 or 1 / (1 - p).  One thread per quad of four consecutive elements.
__global__ __launch_bounds__(256) void k_dropout_mask(float* out, long ld, uint64_t n, int C, const pna_philox::Mask m) {
  const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (4 * q >= n) return;
  uint32_t w[4];
  pna_philox::quad_words(m, q, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t e = 4 * q + i;
    if (e < n) {
      const uint64_t v = e / (uint64_t)C;
      out[v * (uint64_t)ld + (e - v * (uint64_t)C)] = w[i] >= m.thr ? m.scale : 0.f;
    }
  }
}

// ---- PNAConv (pna_pyg_conv_train_*): the layer's own tensors against the tower call's image ------------------------------------------
struct PygK {
  int T, Fi, ED;
  const float* w_pre[kMaxT]; const float* b_pre[kMaxT];     // the layer's: (Fi, (2 | 3) Fi) = [W_i | W_j | W_e], [Fi]
  const float* w_enc; const float* b_enc;                   // (Fi, ED), [Fi]
  float* img;                                               // T images (Fi, 2 Fi + ED) = [W_j | W_i | M], then T biases [Fi]
  const float* gimg;                                        // backward: the tower call's gradients in img's layout
  float* gw_pre[kMaxT]; float* gb_pre[kMaxT]; float* gw_enc; float* gb_enc;
};

// forward, launch 0: one thread per element of the image.  M_t[f][d] = sum_k W_e,t[f][k] W_enc[k][d] and b_t[f] + sum_k W_e,t[f][k] b_enc[k]
// in float64, k ascending, rounded once
__global__ __launch_bounds__(256) void k_pyg_pack(const PygK g) {
  const int Fi = g.Fi, ED = g.ED, ldw = 2 * Fi + ED, lds = (ED ? 3 : 2) * Fi, per = Fi * (ldw + 1);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)g.T * per) return;
  const int t = (int)(i / per), rem = (int)(i - (long)t * per), f = rem / (ldw + 1), c = rem - f * (ldw + 1);
  const float* const w = g.w_pre[t] + (size_t)f * lds;
  if (c < 2 * Fi) {
    g.img[(size_t)t * Fi * ldw + (size_t)f * ldw + c] = c < Fi ? w[Fi + c] : w[c - Fi];
    return;
  }
  double acc = c == ldw ? (double)g.b_pre[t][f] : 0.0;
  if (ED) {
    const int d = c - 2 * Fi;
    for (int k = 0; k < Fi; ++k) acc = __builtin_fma((double)w[2 * Fi + k], (double)(c == ldw ? g.b_enc[k] : g.w_enc[(size_t)k * ED + d]), acc);
  }
  if (c == ldw) g.img[(size_t)g.T * Fi * ldw + (size_t)t * Fi + f] = (float)acc;
  else g.img[(size_t)t * Fi * ldw + (size_t)f * ldw + c] = (float)acc;
}

// backward, last launch: one thread per element of grad_w_pre (T Fi lds), grad_b_pre (T Fi), grad_w_enc (Fi ED), grad_b_enc (Fi), in that
// order.  Sums in float64: d ascending; for the encoder t outermost, then f ascending
__global__ __launch_bounds__(256) void k_pyg_unpack(const PygK g) {
  const int T = g.T, Fi = g.Fi, ED = g.ED, ldw = 2 * Fi + ED, lds = (ED ? 3 : 2) * Fi;
  const long nA = (long)T * Fi * lds, nB = (long)T * Fi, nC = (long)Fi * ED, nD = ED ? Fi : 0;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  const float* const gbias = g.gimg + (size_t)T * Fi * ldw;
  if (i < nA) {
    const int t = (int)(i / ((long)Fi * lds)), rem = (int)(i - (long)t * Fi * lds), f = rem / lds, c = rem - f * lds;
    const float* const gw = g.gimg + (size_t)t * Fi * ldw + (size_t)f * ldw;
    float v;
    if (c < Fi) v = gw[Fi + c];
    else if (c < 2 * Fi) v = gw[c - Fi];
    else {
      const int k = c - 2 * Fi;
      double acc = 0.0;
      for (int d = 0; d < ED; ++d) acc = __builtin_fma((double)gw[2 * Fi + d], (double)g.w_enc[(size_t)k * ED + d], acc);
      acc = __builtin_fma((double)gbias[(size_t)t * Fi + f], (double)g.b_enc[k], acc);
      v = (float)acc;
    }
    g.gw_pre[t][(size_t)f * lds + c] = v;
    return;
  }
  i -= nA;
  if (i < nB) {
    const int t = (int)(i / Fi), f = (int)(i - (long)t * Fi);
    g.gb_pre[t][f] = gbias[i];
    return;
  }
  i -= nB;
  if (i < nC + nD) {
    const bool bias = i >= nC;
    const int k = bias ? (int)(i - nC) : (int)(i / ED), d = bias ? 0 : (int)(i - (long)k * ED);
    double acc = 0.0;
    for (int t = 0; t < T; ++t)
      for (int f = 0; f < Fi; ++f) {
        const float we = g.w_pre[t][(size_t)f * lds + 2 * Fi + k];
        const float gv = bias ? gbias[(size_t)t * Fi + f] : g.gimg[(size_t)t * Fi * ldw + (size_t)f * ldw + 2 * Fi + d];
        acc = __builtin_fma((double)we, (double)gv, acc);
      }
    if (bias) g.gb_enc[k] = (float)acc;
    else g.gw_enc[(size_t)k * ED + d] = (float)acc;
  }
}

int64_t pyg_img_floats(int T, int Fi, int ED) { return up64((int64_t)T * Fi * (2 * Fi + ED + 1)); }

// The blocks of a pna_pyg_conv_train call as the shared implementation takes them: copies of the caller's base / edge / list blocks whose
// pretrans pointers are the packed image (and, in the backward, its gradient in the workspace behind the tower call's own pieces)
struct PygCall {
  pna_tower_train_args base;
  pna_tower_edge_train_args edge;
  pna_tower_aggr_train_args aggr;
  PygK k;
};

int fill_pyg(const pna_pyg_conv_train_args* y, PygCall& c, KArgs& g, Layout& l, bool bwd) {
  static const char* const needs =
      ": needs aggr (drop == NULL) with a base inside pna_tower_aggr_train_*_f32's scope, snorm_n == NULL, residual == 0; edge and w_enc / b_enc "
      "together or not at all; every tower's w_pre (Fi, (2 | 3) Fi) and b_pre; packed of n_tower Fi (2 Fi + edge_dim + 1) floats; in the backward every "
      "tower's grad_w_pre / grad_b_pre (grad_w_enc / grad_b_enc with w_enc); a 256-byte aligned workspace of "
      "pna_pyg_conv_train_workspace_bytes(V, E, n_tower, Fi, Fo, n_scaler, divide_input, edge_dim, n_aggr, aggr) bytes";
  static const std::string fwd_msg = std::string("pna_pyg_conv_train_fwd_f32") + needs, bwd_msg = std::string("pna_pyg_conv_train_bwd_f32") + needs;
  const char* const who = bwd ? bwd_msg.c_str() : fwd_msg.c_str();
  const char* const fn = bwd ? "pna_pyg_conv_train_bwd_f32" : "pna_pyg_conv_train_fwd_f32";
  if (!y) return pna_set_error(PNA_E_INVALID, who);
  if (int rc_ss = pna_check_struct_size(fn, y->struct_size, sizeof(*y))) return rc_ss;
  const pna_tower_aggr_train_args* const r = y->aggr;
  if (!r) return pna_set_error(PNA_E_INVALID, who);
  if (int rc_ss = pna_check_struct_size(fn, r->struct_size, sizeof(*r))) return rc_ss;
  if (!r->base || r->drop) return pna_set_error(PNA_E_INVALID, who);
  if (int rc_ss = pna_check_struct_size(fn, r->base->struct_size, sizeof(*r->base))) return rc_ss;
  if (r->edge) {
    if (int rc_ss = pna_check_struct_size(fn, r->edge->struct_size, sizeof(*r->edge))) return rc_ss;
    if (r->edge->base != r->base) return pna_set_error(PNA_E_INVALID, who);
  }
  const pna_tower_train_args* const p = r->base;
  const int T = p->n_tower, Fi = p->Fi, ED = r->edge ? r->edge->edge_dim : 0;
  Aggr ag;
  if (!in_scope(p->V, p->E, T, Fi, p->Fo, p->n_scaler, p->divide_input) || (r->edge && (ED < 1 || ED > kMaxED)) || !read_list(r->n_aggr, r->aggr, ag))
    return pna_set_error(PNA_E_INVALID, who);
  if (p->snorm_n || p->residual || (y->w_enc == nullptr) != (r->edge == nullptr) || (y->w_enc == nullptr) != (y->b_enc == nullptr) || !y->packed ||
      !p->workspace || ((uintptr_t)p->workspace & 255))
    return pna_set_error(PNA_E_INVALID, who);
  if (bwd && y->w_enc && (!y->grad_w_enc || !y->grad_b_enc)) return pna_set_error(PNA_E_INVALID, who);
  for (int t = 0; t < T; ++t)
    if (!y->w_pre[t] || !y->b_pre[t] || (bwd && (!y->grad_w_pre[t] || !y->grad_b_pre[t]))) return pna_set_error(PNA_E_INVALID, who);
  const int64_t tower_floats = layout_of(p->V, T, Fi, p->Fo, p->n_scaler, p->E, ED, ag.A, true).total;
  if (p->workspace_bytes < (tower_floats + pyg_img_floats(T, Fi, ED)) * 4) return pna_set_error(PNA_E_INVALID, who);
  const int64_t ldw = 2 * (int64_t)Fi + ED;
  float* const gimg = (float*)p->workspace + tower_floats;
  c.base = *p;
  c.base.slope = 1.0f;
  memset(&c.k, 0, sizeof(c.k));
  c.k.T = T; c.k.Fi = Fi; c.k.ED = ED; c.k.w_enc = y->w_enc; c.k.b_enc = y->b_enc; c.k.img = y->packed; c.k.gimg = gimg;
  c.k.gw_enc = y->grad_w_enc; c.k.gb_enc = y->grad_b_enc;
  for (int t = 0; t < T; ++t) {
    c.k.w_pre[t] = y->w_pre[t]; c.k.b_pre[t] = y->b_pre[t]; c.k.gw_pre[t] = y->grad_w_pre[t]; c.k.gb_pre[t] = y->grad_b_pre[t];
    c.base.w_pre[t] = y->packed + (size_t)t * Fi * ldw;
    c.base.b_pre[t] = y->packed + (size_t)T * Fi * ldw + (size_t)t * Fi;
    c.base.grad_w_pre[t] = gimg + (size_t)t * Fi * ldw;
    c.base.grad_b_pre[t] = gimg + (size_t)T * Fi * ldw + (size_t)t * Fi;
    c.base.gamma[t] = c.base.beta[t] = nullptr;
    c.base.running_mean[t] = c.base.running_var[t] = nullptr;
    c.base.grad_gamma[t] = c.base.grad_beta[t] = nullptr;
  }
  c.aggr = *r;
  c.aggr.base = &c.base;
  if (r->edge) {
    c.edge = *r->edge;
    c.edge.base = &c.base;
    c.aggr.edge = &c.edge;
  }
  return fill_aggr(&c.aggr, g, l, bwd, who);
}

}  // namespace

extern "C" int64_t pna_tower_train_workspace_bytes(int64_t V, int64_t E, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_scaler, int32_t divide_input) {
  if (!in_scope(V, E, n_tower, Fi, Fo, n_scaler, divide_input)) return -1;
  return layout_of(V, n_tower, Fi, Fo, n_scaler).total * 4;
}

extern "C" int pna_tower_train_fwd_f32(const pna_tower_train_args* p, pna_stream_t stream) {
  KArgs g;
  Layout l;
  const int rc = fill(p, g, l, false, "pna_tower_train_fwd_f32: needs V >= 2, 1 <= n_tower <= 8, 4 <= Fi <= 128, n_tower Fi <= 512, 1 <= Fo, n_tower Fo <= 128, "
                                      "1 <= n_scaler <= 3, divide_input 0 / 1 (a residual: in_dim == n_tower Fo), rowptr / col, h (ld >= in_dim), every tower's "
                                      "w_pre / b_pre / w_post / b_post, gamma and beta together (all towers or none), running_mean and running_var together, w_mix, "
                                      "the saved tensors x_cat / a / argmax / argmin / z / p / save_mean / save_invstd, out (ld >= n_tower Fo), a 256-byte aligned "
                                      "workspace of pna_tower_train_workspace_bytes(V, E, n_tower, Fi, Fo, n_scaler, divide_input)");
  if (rc != PNA_OK) return rc;
  return launch_fwd<false>(g, l, (hipStream_t)stream, "pna_tower_train_fwd_f32: launch failed");
}

extern "C" int pna_tower_train_bwd_f32(const pna_tower_train_args* p, pna_stream_t stream) {
  KArgs g;
  Layout l;
  const int rc = fill(p, g, l, true, "pna_tower_train_bwd_f32: needs the forward's arguments and saved tensors, grad_out (ld >= n_tower Fo), grad_h, every tower's "
                                     "grad_w_pre / grad_b_pre / grad_w_post / grad_b_post (grad_gamma / grad_beta where it has gamma), grad_w_mix / grad_b_mix, the "
                                     "transposed graph (col_t, rank_t, one whole-row record per source row in items_t: n_items_t == V) and the forward's workspace size");
  if (rc != PNA_OK) return rc;
  return launch_bwd(p, g, l, stream, nullptr, "pna_tower_train_bwd_f32: launch failed");
}

extern "C" int64_t pna_tower_edge_train_workspace_bytes(int64_t V, int64_t E, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_scaler, int32_t divide_input,
                                                        int32_t edge_dim) {
  if (!in_scope(V, E, n_tower, Fi, Fo, n_scaler, divide_input) || edge_dim < 1 || edge_dim > kMaxED) return -1;
  return layout_of(V, n_tower, Fi, Fo, n_scaler, E, edge_dim).total * 4;
}

extern "C" int pna_tower_edge_train_fwd_f32(const pna_tower_edge_train_args* q, pna_stream_t stream) {
  KArgs g;
  Layout l;
  const int rc = fill_edge(q, g, l, false);
  if (rc != PNA_OK) return rc;
  return launch_fwd<true>(g, l, (hipStream_t)stream, "pna_tower_edge_train_fwd_f32: launch failed");
}

extern "C" int pna_tower_edge_train_bwd_f32(const pna_tower_edge_train_args* q, pna_stream_t stream) {
  KArgs g;
  Layout l;
  const int rc = fill_edge(q, g, l, true);
  if (rc != PNA_OK) return rc;
  return launch_bwd(q->base, g, l, stream, q, "pna_tower_edge_train_bwd_f32: launch failed");
}

extern "C" int pna_tower_drop_train_fwd_f32(const pna_tower_drop_args* d, pna_stream_t stream) {
  KArgs g;
  Layout l;
  const int rc = fill_drop(d, g, l, false);
  if (rc != PNA_OK) return rc;
  if (d->edge) return launch_fwd<true, true>(g, l, (hipStream_t)stream, "pna_tower_drop_train_fwd_f32: launch failed");
  return launch_fwd<false, true>(g, l, (hipStream_t)stream, "pna_tower_drop_train_fwd_f32: launch failed");
}

extern "C" int pna_tower_drop_train_bwd_f32(const pna_tower_drop_args* d, pna_stream_t stream) {
  KArgs g;
  Layout l;
  const int rc = fill_drop(d, g, l, true);
  if (rc != PNA_OK) return rc;
  return launch_bwd(d->base, g, l, stream, d->edge, "pna_tower_drop_train_bwd_f32: launch failed", true);
}

extern "C" int64_t pna_tower_aggr_train_workspace_bytes(int64_t V, int64_t E, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_scaler, int32_t divide_input,
                                                        int32_t edge_dim, int32_t n_aggr, const int32_t* aggr) {
  Aggr ag;
  if (!in_scope(V, E, n_tower, Fi, Fo, n_scaler, divide_input) || edge_dim < 0 || edge_dim > kMaxED || !read_list(n_aggr, aggr, ag)) return -1;
  return layout_of(V, n_tower, Fi, Fo, n_scaler, E, edge_dim, ag.A, true).total * 4;
}

extern "C" int pna_tower_aggr_train_fwd_f32(const pna_tower_aggr_train_args* r, pna_stream_t stream) {
  KArgs g;
  Layout l;
  const int rc = fill_aggr(r, g, l, false);
  if (rc != PNA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const char* const failed = "pna_tower_aggr_train_fwd_f32: launch failed";
  if (r->edge) return r->drop ? launch_fwd<true, true>(g, l, st, failed) : launch_fwd<true, false>(g, l, st, failed);
  return r->drop ? launch_fwd<false, true>(g, l, st, failed) : launch_fwd<false, false>(g, l, st, failed);
}

extern "C" int pna_tower_aggr_train_bwd_f32(const pna_tower_aggr_train_args* r, pna_stream_t stream) {
  KArgs g;
  Layout l;
  const int rc = fill_aggr(r, g, l, true);
  if (rc != PNA_OK) return rc;
  return launch_bwd(r->base, g, l, stream, r->edge, "pna_tower_aggr_train_bwd_f32: launch failed", r->drop != nullptr, true);
}

extern "C" int64_t pna_pyg_conv_train_workspace_bytes(int64_t V, int64_t E, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_scaler, int32_t divide_input,
                                                      int32_t edge_dim, int32_t n_aggr, const int32_t* aggr) {
  Aggr ag;
  if (!in_scope(V, E, n_tower, Fi, Fo, n_scaler, divide_input) || edge_dim < 0 || edge_dim > kMaxED || !read_list(n_aggr, aggr, ag)) return -1;
  return (layout_of(V, n_tower, Fi, Fo, n_scaler, E, edge_dim, ag.A, true).total + pyg_img_floats(n_tower, Fi, edge_dim)) * 4;
}

extern "C" int pna_pyg_conv_train_fwd_f32(const pna_pyg_conv_train_args* y, pna_stream_t stream) {
  PygCall c;
  KArgs g;
  Layout l;
  const int rc = fill_pyg(y, c, g, l, false);
  if (rc != PNA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const char* const failed = "pna_pyg_conv_train_fwd_f32: launch failed";
  const long n = (long)c.k.T * c.k.Fi * (2 * c.k.Fi + c.k.ED + 1);
  hipLaunchKernelGGL(k_pyg_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c.k);
  return c.k.ED ? launch_fwd<true, false>(g, l, st, failed) : launch_fwd<false, false>(g, l, st, failed);
}

extern "C" int pna_pyg_conv_train_bwd_f32(const pna_pyg_conv_train_args* y, pna_stream_t stream) {
  PygCall c;
  KArgs g;
  Layout l;
  int rc = fill_pyg(y, c, g, l, true);
  if (rc != PNA_OK) return rc;
  rc = launch_bwd(&c.base, g, l, stream, c.k.ED ? &c.edge : nullptr, "pna_pyg_conv_train_bwd_f32: launch failed", false, true);
  if (rc != PNA_OK) return rc;
  const int Fi = c.k.Fi, ED = c.k.ED;
  const long n = (long)c.k.T * Fi * ((ED ? 3 : 2) * Fi + 1) + (long)Fi * ED + (ED ? Fi : 0);
  hipLaunchKernelGGL(k_pyg_unpack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c.k);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_pyg_conv_train_bwd_f32: launch failed");
  return PNA_OK;
}

extern "C" int pna_dropout_mask_f32(float* out, int64_t ld, int64_t V, int32_t C, float p, uint64_t seed, uint64_t offset, pna_stream_t stream) {
  if (!out || V < 0 || C < 1 || ld < C || !(p >= 0.f && p < 1.f) || V > (int64_t)((1ull << 40) / (uint64_t)C))
    return pna_set_error(PNA_E_INVALID, "pna_dropout_mask_f32: needs out, V >= 0, C >= 1, ld >= C, V C <= 2^40, 0 <= p < 1");
  const uint64_t n = (uint64_t)V * (uint64_t)C;
  if (n == 0) return PNA_OK;
  const uint64_t quads4 = (n + 3) / 4;
  hipLaunchKernelGGL(k_dropout_mask, dim3((unsigned)((quads4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, (long)ld, n, (int)C,
                     pna_philox::make_mask(p, seed, offset));
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_dropout_mask_f32: launch failed");
  return PNA_OK;
}
