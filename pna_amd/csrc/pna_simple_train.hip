// pna_simple_train.hip -- PNASimpleLayer's TRAINING forward and backward on molecule-sized batches (the MolHIV workload:
// realworld_benchmark/train/train_HIV_graph_classification.py:4-26, nets/HIV_graph_classification/pna_net.py:42-60) as ONE C call
// each for gfx950.  Implements pna_simple_train_{workspace_bytes, fwd_f32, bwd_f32} of include/pna_amd.h
// (models/dgl/pna_layer.py:197-213 in train mode: update_all with mean | max | min | std and the degree scalers, the 1-layer
// posttrans, BatchNorm1d with batch statistics, ReLU, the residual).
//
// Why: at this size the generic training route (AggregateFn -> torch stack / reshape -> PosttransFn -> BnTailFn -> relu / residual)
// is bound by launch and host latency -- a dozen autograd nodes with allocator and Python work between them, and the (V, 12F) scaled
// aggregate written and read once each way.  As in pna_tower_fused.hip the work is cut by destination ROWS: a workgroup owns 16 rows,
// gathers and reduces them, keeps the 16 x 4F tile in LDS and multiplies it on v_mfma_f32_16x16x4_f32 (exact fp32 products) with the
// degree scalers applied to the accumulators, so the scaled aggregate never exists.  The weight is read directly from the Linear's
// (N, S 4F) matrix (an optimiser rewrites it every step: a packed image would cost a launch per call and never be reused).
//
// Determinism: no float atomics.  A row's messages are folded serially in CSR order (pna_segreduce_fwd_f32's order for in-degrees
// <= 128: same bits, same arg indices); column sums are fp32 inside a tile / slab and float64 across them in a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_rowstats.h"
#include "pna_train_dev.h"

namespace {

using namespace pna_train;      // f4, kRows, quads, pitch_of, quad_fma, bn_affine, fold_msg, bn_finalize_column

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kSlab = 128;       // rows per workgroup of the backward's column sums
constexpr int kMaxN = 128;
constexpr int kEU = 4;           // edges of a row whose gathers are issued together

struct KArgs {
  const int32_t* rowptr; const int32_t* col;
  int V, F, N, S, residual;
  const float* h; long ldh;
  const float* scale[3];
  const float* w; long ldw;
  const float* bias; const float* gamma; const float* beta;
  float eps, momentum;
  float* rmean; float* rvar;
  float* a; int32_t* amx; int32_t* amn; float* z;
  float* mean; float* invstd;
  float* out; long ld_out;
  const float* go; long ld_go;
  float* ggamma; float* gbeta;
  float* part;       // forward: [tiles][2][N] column sums of d, d^2 per 16-row tile; backward: [slabs][2][N] of g', g' xhat
  float* gz;         // backward (V, N)
  float* packed;     // backward (V, pitch): the pull's packed rows
  long pitch;
  int n_part;
};

// ---- forward, launch 1: gather + reduce + contraction + BatchNorm partial sums of 16 destination rows ----------------------------
template <int S>
__global__ __launch_bounds__(kThreads) void k_st_rows_fwd(const KArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int F = g.F, N = g.N, K = 4 * F, Q = quads(K), P = pitch_of(Q), NT = (N + 15) / 16, PZ = NT * 16 + 1;
  float* const A = lds;                                   // [16][P]  the rows' aggregate [mean | max | min | std]
  float* const Z = A + kRows * P;                         // [16][PZ] the rows' z
  float* const SC = Z + kRows * PZ;                       // [3][16]  scale_0..2 of the tile's rows
  const int r0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.V - r0);
  // zeros in the K padding columns and in the rows past the matrix's end (they multiply weights; 0 * garbage would not be 0)
  for (int i = tid; i < kRows * P; i += kThreads) {
    const int r = i / P, k = i - r * P;
    if (k >= K || r >= nrows) A[i] = 0.f;
  }
  if (tid < 3 * kRows) {
    const int s = tid >> 4, r = tid & 15;
    const float* p = s < S ? g.scale[s] : nullptr;
    SC[tid] = (p && r < nrows) ? p[r0 + r] : 1.f;
  }
  // ---- gather: a wavefront owns rows wave, wave + 8; a lane owns columns lane and lane + 64; the row's edges in CSR order ----
  for (int r = wave; r < nrows; r += kWaves) {
    const int row = r0 + r;
    const int beg = g.rowptr[row], end = g.rowptr[row + 1];
    const int cc[2] = {min(lane, F - 1), min(lane + 64, F - 1)};      // (lanes past the last column redo it; not stored)
    float s[2] = {0.f, 0.f}, q[2] = {0.f, 0.f}, mx[2] = {-INFINITY, -INFINITY}, mn[2] = {INFINITY, INFINITY};
    int ax[2] = {-1, -1}, an[2] = {-1, -1};
    for (int e = beg; e < end; e += kEU) {
      float v[kEU][2];
#pragma unroll
      for (int u = 0; u < kEU; ++u) {
        const size_t o = (size_t)g.col[min(e + u, end - 1)] * g.ldh;
        v[u][0] = g.h[o + cc[0]];
        v[u][1] = g.h[o + cc[1]];
      }
#pragma unroll
      for (int u = 0; u < kEU; ++u)
        if (e + u < end) {                                  // (wavefront-uniform)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            fold_msg(v[u][j], e + u, s[j], q[j], mx[j], mn[j], ax[j], an[j]);
          }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = lane + 64 * j;
      if (c < F) {
        float mean, omx, omn, sd;
        pna_dev::row_stats(s[j], q[j], mx[j], mn[j], end - beg, mean, omx, omn, sd);
        float* const al = A + r * P + c;
        al[0] = mean; al[F] = omx; al[2 * F] = omn; al[3 * F] = sd;
        float* const ag = g.a + (size_t)row * K + c;
        ag[0] = mean; ag[F] = omx; ag[2 * F] = omn; ag[3 * F] = sd;
        g.amx[(size_t)row * F + c] = ax[j];
        g.amn[(size_t)row * F + c] = an[j];
      }
    }
  }
  __syncthreads();
  // ---- contraction: wavefront nt owns output columns [16 nt, 16 nt + 16); B fragments straight from the weight's rows ----
  for (int nt = wave; nt < NT; nt += kWaves) {
    const int n = nt * 16 + li;
    const bool nok = n < N;
    const float* const wrow = g.w + (size_t)min(n, N - 1) * g.ldw;
    f4 acc[S];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = (f4){0.f, 0.f, 0.f, 0.f};
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int qd = 0; qd < Q; ++qd) {
      const int k = 16 * qd + 4 * lg;
      const f4 a = *reinterpret_cast<const f4*>(A + li * P + k);
      const bool ok = nok && k < K;                       // (K is a multiple of 4: a fragment is inside or outside as a whole)
      const int kk = ok ? k : 0;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const f4 b = *reinterpret_cast<const f4*>(wrow + (size_t)s * K + kk);
        quad_fma(acc[s], a, ok ? b : zero);
      }
    }
    const float bn = (g.bias && nok) ? g.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * lg + i;
      float zt = SC[r] * acc[0][i];
#pragma unroll
      for (int s = 1; s < S; ++s) zt = zt + SC[s * kRows + r] * acc[s][i];
      zt = zt + bn;
      Z[r * PZ + nt * 16 + li] = zt;
      if (nok && r < nrows) g.z[(size_t)(r0 + r) * N + n] = zt;
    }
  }
  __syncthreads();
  // ---- the tile's BatchNorm column sums, shifted by the tile's first row (the finalize pass re-bases them in float64) ----
  for (int c = tid; c < N; c += kThreads) {
    const float kc = Z[c];
    float s0 = 0.f, s1 = 0.f;
    for (int r = 0; r < nrows; ++r) {
      const float d = Z[r * PZ + c] - kc;
      s0 = s0 + d;
      s1 = s1 + d * d;
    }
    g.part[((size_t)blockIdx.x * 2 + 0) * N + c] = s0;
    g.part[((size_t)blockIdx.x * 2 + 1) * N + c] = s1;
  }
}

// ---- forward, launch 2: one workgroup per column -- the tiles' sums in float64, the column's constants (pna_bn_tail's finalize) ----
__global__ __launch_bounds__(256) void k_st_bn_finalize(const KArgs g) {
  __shared__ double red[2][256];
  const int c = blockIdx.x;
  bn_finalize_column(g.z, g.N, c, g.V, g.part, g.n_part, g.eps, g.momentum, g.mean + c, g.invstd + c, g.rmean ? g.rmean + c : nullptr,
                     g.rmean ? g.rvar + c : nullptr, red);
}

// ---- forward, launch 3: out = residual + relu((z - mean) (gamma invstd) + beta) ----
__global__ __launch_bounds__(256) void k_st_bn_apply(const KArgs g) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)g.V * g.N) return;
  const long v = i / g.N;
  const int c = (int)(i - v * g.N);
  const float ci = g.invstd[c];
  const float ca = (g.gamma ? g.gamma[c] : 1.f) * ci, cb = g.beta ? g.beta[c] : 0.f;
  const float y = bn_affine(g.z[i], g.mean[c], ca, cb);
  float o = y > 0.f ? y : (y != y ? y : 0.f);               // (NaN stays NaN, like F.relu)
  if (g.residual) o = g.h[v * g.ldh + c] + o;
  g.out[v * g.ld_out + c] = o;
}

// ---- backward, launch 1: column sums of g' = grad_out [pre-activation > 0] and g' xhat over a slab of 128 rows ----
__global__ __launch_bounds__(256) void k_st_bwd_colsums(const KArgs g) {
  __shared__ float red[2][2][kMaxN];
  const int c = threadIdx.x & (kMaxN - 1), hf = threadIdx.x >> 7, N = g.N;
  const long r0 = (long)blockIdx.x * kSlab + hf * (kSlab / 2), r1 = min(r0 + kSlab / 2, (long)g.V);
  float s0 = 0.f, s1 = 0.f;
  if (c < N) {
    const float cm = g.mean[c], ci = g.invstd[c];
    const float ca = (g.gamma ? g.gamma[c] : 1.f) * ci, cb = g.beta ? g.beta[c] : 0.f;
    for (long r = r0; r < r1; ++r) {
      const float v = g.z[r * N + c];
      float go = g.go[r * g.ld_go + c];
      if (!(bn_affine(v, cm, ca, cb) > 0.f)) go = 0.f;
      s0 = s0 + go;
      s1 = s1 + go * ((v - cm) * ci);
    }
  }
  red[0][hf][c] = s0; red[1][hf][c] = s1;
  __syncthreads();
  if (hf == 0 && c < N) {
    g.part[((size_t)blockIdx.x * 2 + 0) * N + c] = red[0][0][c] + red[0][1][c];
    g.part[((size_t)blockIdx.x * 2 + 1) * N + c] = red[1][0][c] + red[1][1][c];
  }
}

// ---- backward, launch 2: gz and G = sum_s scale_s (gz W_s) of 16 rows, written as [G_mean | G_std | G_max | G_min] into the pull's rows ----
template <int S>
__global__ __launch_bounds__(kThreads) void k_st_rows_bwd(const KArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int F = g.F, N = g.N, K = 4 * F, QN = quads(N), PN = pitch_of(QN), NTJ = (K + 15) / 16;
  float* const GZ = lds;                                  // [16][PN]
  float* const SC = GZ + kRows * PN;                      // [3][16]
  float* const CC = SC + 3 * kRows;                       // [2][128] mean g', mean g' xhat
  const int r0 = blockIdx.x * kRows;
  const int nrows = min(kRows, g.V - r0);
  // the slabs' partial sums in float64, in slab order (every workgroup: the same values)
  for (int i = tid; i < 2 * N; i += kThreads) {
    const int w = i / N, c = i - w * N;
    double t = 0.0;
    for (int p = 0; p < g.n_part; ++p) t += (double)g.part[((size_t)p * 2 + w) * N + c];
    CC[w * kMaxN + c] = (float)(t / (double)g.V);
    if (blockIdx.x == 0) {
      if (w == 0 && g.gbeta) g.gbeta[c] = (float)t;
      if (w == 1 && g.ggamma) g.ggamma[c] = (float)t;
    }
  }
  for (int i = tid; i < kRows * PN; i += kThreads) {
    const int r = i / PN, k = i - r * PN;
    if (k >= N || r >= nrows) GZ[i] = 0.f;
  }
  if (tid < 3 * kRows) {
    const int s = tid >> 4, r = tid & 15;
    const float* p = s < S ? g.scale[s] : nullptr;
    SC[tid] = (p && r < nrows) ? p[r0 + r] : 1.f;
  }
  __syncthreads();
  // gz = gamma invstd (g' - mean g' - xhat mean(g' xhat)): pna_bn_tail's backward apply, op by op
  for (int i = tid; i < nrows * N; i += kThreads) {
    const int r = i / N, c = i - r * N;
    const size_t row = (size_t)(r0 + r);
    const float cm = g.mean[c], ci = g.invstd[c];
    const float ca = (g.gamma ? g.gamma[c] : 1.f) * ci, cb = g.beta ? g.beta[c] : 0.f;
    const float v = g.z[row * N + c];
    const float go = (bn_affine(v, cm, ca, cb) > 0.f) ? g.go[row * g.ld_go + c] : 0.f;
    const float val = ca * ((go - CC[c]) - ((v - cm) * ci) * CC[kMaxN + c]);
    GZ[r * PN + c] = val;
    g.gz[row * N + c] = val;
  }
  __syncthreads();
  // G tile (16 rows x 16 columns of 4F) per wavefront: A = gz (K = N), B[k = n][j] = W[n][s 4F + j]
  for (int jt = wave; jt < NTJ; jt += kWaves) {
    const int j = jt * 16 + li;
    const bool jok = j < K;
    const int jj = min(j, K - 1);
    f4 acc[S];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = (f4){0.f, 0.f, 0.f, 0.f};
    for (int qd = 0; qd < QN; ++qd) {
      const int k = 16 * qd + 4 * lg;
      const f4 a = *reinterpret_cast<const f4*>(GZ + li * PN + k);
#pragma unroll
      for (int s = 0; s < S; ++s) {
        f4 b;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float wv = g.w[(size_t)min(k + t, N - 1) * g.ldw + (size_t)s * K + jj];
          b[t] = (jok && k + t < N) ? wv : 0.f;
        }
        quad_fma(acc[s], a, b);
      }
    }
    if (jok) {
      const int blk = j / F, f = j - blk * F;               // the weight's block order mean | max | min | std -> the rows' mean | std | max | min
      const int dblk = blk == 0 ? 0 : (blk == 3 ? 1 : blk + 1);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lg + i;
        if (r < nrows) {
          float G = SC[r] * acc[0][i];
#pragma unroll
          for (int s = 1; s < S; ++s) G = G + SC[s * kRows + r] * acc[s][i];
          g.packed[(size_t)(r0 + r) * g.pitch + dblk * F + f] = G;
        }
      }
    }
  }
}

// ---- the weight gradient of the shapes pna_posttrans_dw_f32's kernel does not take (n_scaler N > 240 or 4F + 1 > 384; N <= 128 holds here): one thread per
// (n, k), the rows in sequence (fp32, a fixed order).  grad_b from the threads of k = 0. ----
template <int S>
__global__ __launch_bounds__(256) void k_st_dw_plain(const KArgs g, float* gw, float* gb) {
  const int K = 4 * g.F;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)g.N * K) return;
  const int n = (int)(i / K), k = (int)(i - (long)n * K);
  float acc[S], sb = 0.f;
#pragma unroll
  for (int s = 0; s < S; ++s) acc[s] = 0.f;
  for (int v = 0; v < g.V; ++v) {
    const float gy = g.gz[(size_t)v * g.N + n], av = g.a[(size_t)v * K + k];
    sb = sb + gy;
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = acc[s] + ((g.scale[s] ? g.scale[s][v] : 1.f) * gy) * av;
  }
#pragma unroll
  for (int s = 0; s < S; ++s) gw[(size_t)n * S * K + (size_t)s * K + k] = acc[s];
  if (k == 0 && gb) gb[n] = sb;
}

inline int64_t up64(int64_t floats) { return (floats + 63) / 64 * 64; }     // workspace pieces at 256-byte boundaries

struct Layout {
  int64_t part_fwd, part_bwd, gz, packed, dw, total;      // offsets in floats (dw: bytes reserved behind `packed`)
  int64_t pitch, dw_bytes;
  int n_tile, n_slab;
};

bool in_scope(int64_t V, int64_t E, int F, int N, int S) {
  return V >= 2 && V < (1ll << 31) - kSlab && E >= 0 && E < (1ll << 31) && F >= 4 && F <= 128 && N >= 1 && N <= kMaxN && S >= 1 && S <= 3;
}

bool dw_kernel_takes(int F, int N, int S) { return pna_posttrans_dw_workspace_bytes(256, N, S, 4 * F, 0) >= 0; }

Layout layout_of(int64_t V, int F, int N, int S) {
  Layout l;
  l.n_tile = (int)((V + kRows - 1) / kRows);
  l.n_slab = (int)((V + kSlab - 1) / kSlab);
  l.pitch = (5 * (int64_t)F + 31) / 32 * 32;
  l.part_fwd = 0;
  l.part_bwd = l.part_fwd + up64((int64_t)l.n_tile * 2 * N);
  l.gz = l.part_bwd + up64((int64_t)l.n_slab * 2 * N);
  l.packed = l.gz + up64(V * N);
  l.dw = l.packed + up64(V * l.pitch);
  // the weight-gradient kernel cuts the rows into slabs of >= 256 (how many depends on the device): room for the most it can ask for
  l.dw_bytes = dw_kernel_takes(F, N, S) ? pna_posttrans_dw_workspace_bytes(256, N, S, 4 * F, 0) * ((V + 255) / 256) : 0;
  l.total = l.dw + up64((l.dw_bytes + 3) / 4);
  return l;
}

int fill(const pna_simple_train_args* p, KArgs& g, Layout& l, bool bwd, const char* who) {
  if (!p) return pna_set_error(PNA_E_INVALID, who);
  if (int rc_ss = pna_check_struct_size(bwd ? "pna_simple_train_bwd_f32" : "pna_simple_train_fwd_f32", p->struct_size, sizeof(*p))) return rc_ss;
  const int F = p->F, N = p->N, S = p->n_scaler;
  if (!in_scope(p->V, p->E, F, N, S) || (p->residual && F != N)) return pna_set_error(PNA_E_INVALID, who);
  if (!p->rowptr || (p->E > 0 && !p->col) || !p->h || p->ldh < F || !p->w || p->ldw < (int64_t)S * 4 * F || (p->ldw & 3) || ((uintptr_t)p->w & 15) ||
      !p->a || !p->argmax || !p->argmin || !p->z || !p->save_mean || !p->save_invstd || !p->workspace || ((uintptr_t)p->workspace & 255) ||
      (p->gamma == nullptr) != (p->beta == nullptr) || (p->running_mean == nullptr) != (p->running_var == nullptr))
    return pna_set_error(PNA_E_INVALID, who);
  if (!bwd && (!p->out || p->ld_out < N)) return pna_set_error(PNA_E_INVALID, who);
  if (bwd && (!p->grad_out || p->ld_go < N || !p->grad_h || !p->grad_w || !p->grad_b || !p->col_t || !p->rank_t || !p->items_t || p->n_items_t != p->V))
    return pna_set_error(PNA_E_INVALID, who);
  l = layout_of(p->V, F, N, S);
  if (p->workspace_bytes < l.total * 4) return pna_set_error(PNA_E_INVALID, who);
  memset(&g, 0, sizeof(g));
  float* const ws = (float*)p->workspace;
  g.rowptr = p->rowptr; g.col = p->col; g.V = p->V; g.F = F; g.N = N; g.S = S; g.residual = p->residual != 0;
  g.h = p->h; g.ldh = (long)p->ldh;
  for (int s = 0; s < 3; ++s) g.scale[s] = s < S ? p->row_scale[s] : nullptr;
  g.w = p->w; g.ldw = (long)p->ldw; g.bias = p->bias; g.gamma = p->gamma; g.beta = p->beta; g.eps = p->eps; g.momentum = p->momentum;
  g.rmean = p->running_mean; g.rvar = p->running_var;
  g.a = p->a; g.amx = p->argmax; g.amn = p->argmin; g.z = p->z; g.mean = p->save_mean; g.invstd = p->save_invstd;
  g.out = p->out; g.ld_out = (long)p->ld_out; g.go = p->grad_out; g.ld_go = (long)p->ld_go;
  g.ggamma = p->grad_gamma; g.gbeta = p->grad_beta;
  g.part = ws + (bwd ? l.part_bwd : l.part_fwd); g.n_part = bwd ? l.n_slab : l.n_tile;
  g.gz = ws + l.gz; g.packed = ws + l.packed; g.pitch = (long)l.pitch;
  return PNA_OK;
}

}  // namespace

extern "C" int64_t pna_simple_train_workspace_bytes(int64_t V, int64_t E, int32_t F, int32_t N, int32_t n_scaler) {
  if (!in_scope(V, E, F, N, n_scaler)) return -1;
  return layout_of(V, F, N, n_scaler).total * 4;
}

extern "C" int pna_simple_train_fwd_f32(const pna_simple_train_args* p, pna_stream_t stream) {
  KArgs g;
  Layout l;
  const int rc = fill(p, g, l, false, "pna_simple_train_fwd_f32: needs V >= 2, 4 <= F <= 128, 1 <= N <= 128, 1 <= n_scaler <= 3 (a residual: F == N), rowptr / col, "
                                      "h (ld >= F), w (16-byte aligned, ld >= n_scaler 4F, a multiple of 4), the saved tensors a / argmax / argmin / z / save_mean / "
                                      "save_invstd, gamma and beta together, running_mean and running_var together, out (ld >= N), a 256-byte aligned workspace of "
                                      "pna_simple_train_workspace_bytes(V, E, F, N, n_scaler)");
  if (rc != PNA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int Q = quads(4 * g.F), NT = (g.N + 15) / 16;
  const size_t lds = ((size_t)kRows * pitch_of(Q) + (size_t)kRows * (NT * 16 + 1) + 3 * kRows) * sizeof(float);     // <= 42 KB
  const dim3 grid((unsigned)l.n_tile), block(kThreads);
  if (g.S == 1) hipLaunchKernelGGL(k_st_rows_fwd<1>, grid, block, lds, st, g);
  else if (g.S == 2) hipLaunchKernelGGL(k_st_rows_fwd<2>, grid, block, lds, st, g);
  else hipLaunchKernelGGL(k_st_rows_fwd<3>, grid, block, lds, st, g);
  hipLaunchKernelGGL(k_st_bn_finalize, dim3((unsigned)g.N), dim3(256), 0, st, g);
  const long n = (long)g.V * g.N;
  hipLaunchKernelGGL(k_st_bn_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_simple_train_fwd_f32: launch failed");
  return PNA_OK;
}

extern "C" int pna_simple_train_bwd_f32(const pna_simple_train_args* p, pna_stream_t stream) {
  KArgs g;
  Layout l;
  const int rc = fill(p, g, l, true, "pna_simple_train_bwd_f32: needs the forward's arguments and saved tensors, grad_out (ld >= N), grad_h / grad_w / grad_b, the "
                                     "transposed graph (col_t, rank_t, one whole-row record per source row in items_t: n_items_t == V) and the forward's workspace size");
  if (rc != PNA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int F = g.F, N = g.N, S = g.S, K = 4 * F;
  // 1. column sums, 2. the rows kernel
  hipLaunchKernelGGL(k_st_bwd_colsums, dim3((unsigned)l.n_slab), dim3(256), 0, st, g);
  const size_t lds = ((size_t)kRows * pitch_of(quads(N)) + 3 * kRows + 2 * kMaxN) * sizeof(float);
  const dim3 grid((unsigned)l.n_tile), block(kThreads);
  if (S == 1) hipLaunchKernelGGL(k_st_rows_bwd<1>, grid, block, lds, st, g);
  else if (S == 2) hipLaunchKernelGGL(k_st_rows_bwd<2>, grid, block, lds, st, g);
  else hipLaunchKernelGGL(k_st_rows_bwd<3>, grid, block, lds, st, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_simple_train_bwd_f32: launch failed");
  // 3, 4. rowprep + pull over the transposed graph on the packed rows, in place; the residual's grad_out joins in the pull's store
  pna_segreduce_bwd_args b;
  memset(&b, 0, sizeof(b));
  b.struct_size = (uint32_t)sizeof(b);
  b.rowptr = p->rowptr; b.col = p->col; b.V = p->V; b.F = F;
  b.x = p->h; b.ldx = p->ldh;
  b.n_tower = 1; b.n_aggr = 4; b.tower_stride_in = F;
  b.aggr[0] = PNA_AGG_MEAN; b.aggr[1] = PNA_AGG_STD; b.aggr[2] = PNA_AGG_MAX; b.aggr[3] = PNA_AGG_MIN;
  b.gagg = g.packed; b.ld_g = l.pitch; b.tower_stride_g = K;
  b.mean = p->a; b.stdv = p->a + 3 * (size_t)F; b.ld_stat = K; b.tower_stride_stat = K;
  b.argmax = p->argmax; b.argmin = p->argmin; b.ld_arg = F;
  b.grad_x = p->grad_h; b.ld_gx = F;
  pna_segreduce_bwd_pull_args q;
  memset(&q, 0, sizeof(q));
  q.struct_size = (uint32_t)sizeof(q);
  q.base = &b; q.table = g.packed; q.ld_table = l.pitch;
  q.col_t = p->col_t; q.rank_t = p->rank_t; q.items_t = p->items_t; q.n_items_t = p->n_items_t; q.run_rowprep = 1;
  q.ranks = (uint16_t*)(g.packed + 4 * (size_t)F); q.ld_rank = 2 * l.pitch;
  int rc2 = pna_segreduce_bwd_pull_launch(&q, g.residual ? p->grad_out : nullptr, (long)p->ld_go, stream);
  if (rc2 != PNA_OK) return rc2;
  // 5, 6. the weight and bias gradient
  if (l.dw_bytes > 0 && !p->row_scale[0]) {
    pna_posttrans_dw_args d;
    memset(&d, 0, sizeof(d));
    d.struct_size = (uint32_t)sizeof(d);
    d.gy = g.gz; d.ldg = N; d.M = p->V; d.N = N; d.n_scaler = S; d.a = p->a; d.lda = K; d.K = K; d.Kh = 0;
    for (int s = 0; s < S; ++s) d.row_scale[s] = p->row_scale[s];
    d.grad_w = p->grad_w; d.ldw = (int64_t)S * K; d.grad_b = p->grad_b;
    d.workspace = (float*)p->workspace + l.dw; d.workspace_bytes = l.dw_bytes;
    return pna_posttrans_dw_f32(&d, stream);
  }
  const long n = (long)N * K;
  const dim3 gd((unsigned)((n + 255) / 256)), bd(256);
  if (S == 1) hipLaunchKernelGGL(k_st_dw_plain<1>, gd, bd, 0, st, g, p->grad_w, p->grad_b);
  else if (S == 2) hipLaunchKernelGGL(k_st_dw_plain<2>, gd, bd, 0, st, g, p->grad_w, p->grad_b);
  else hipLaunchKernelGGL(k_st_dw_plain<3>, gd, bd, 0, st, g, p->grad_w, p->grad_b);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_simple_train_bwd_f32: launch failed");
  return PNA_OK;
}
