// pna_mlp_head.hip -- the dense heads of the nets for gfx950: 1 to 4 Linear layers with none / ReLU / LeakyReLU over rows, forward and
// backward as ONE C call each.  Implements pna_mlp_head_{in_scope, workspace_bytes, fwd_f32, bwd_f32} of include/pna_amd.h.  Replaces
// realworld_benchmark/nets/mlp_readout_layer.py:14-29 (MLPReadout), models/layers.py:101-234 (FCLayer / MLP without dropout and
// batch-norm: the multitask GNN's nodes_read_out) and the nn.Linear embeddings of the superpixel net with what autograd derives from them.
//
//   y = f_L(... f_1(x))      f_l(h) = act_l(h W_l^T + b_l)      widths[0] = columns of x, widths[l] = outputs of layer l
//
// Forward: one launch.  A workgroup owns 16 rows (the M of one v_mfma_f32_16x16x4_f32 tile, as the sibling one-call kernels); the x tile
// sits in LDS zero-filled to the K pitch; wavefront nt owns output columns [16 nt, 16 nt + 16) of every layer; B fragments are read
// straight from the nn.Linear parameters; the activation epilogue writes the next layer's A tile into the other of two LDS buffers; only
// the last layer's rows go to memory.
// Backward: (a) a rows kernel over the same tiles: the pre-activations a_1 .. a_L of its rows rebuilt in LDS (nothing is saved but x;
// h_l = act_l(a_l) is applied as the A fragment is read), then down the layers dz_l = g_l act_l'(a_l) in place of a_l and
// g_(l-1) = dz_l W_l on the MFMA; grad_x stored; h_1 .. h_(L-1) and dz_1 .. dz_L stored once to the workspace;  (b) weight and bias
// gradients of every layer per slab of consecutive rows on the MFMA (grad_W_l = dz_l^T h_(l-1), the bias sums as a ones column);
// (c) the slabs added in slab order in float64 (pna_gru.hip's scheme).  No atomics of any kind: bitwise repeatable.
// No kernel waits for another workgroup; every loop bound comes from the arguments.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_train_dev.h"

namespace {

using namespace pna_train;      // f4, kRows, quads, pitch_of, quad_fma

constexpr int kThreads = 512;   // rows kernels: 8 wavefronts, one per 16-column tile of the widest layer
constexpr int kWaves = kThreads / 64;
constexpr int kMaxL = PNA_MAX_MLP_LAYERS;
constexpr int kMaxWidth = PNA_MLP_MAX_WIDTH;
constexpr int kDwThreads = 256; // weight-gradient kernel: 4 wavefronts share the column tiles of one 16-row band of one layer's outputs

struct MArgs {
  long V;
  int L;
  int w[kMaxL + 1];
  int act[kMaxL];
  float slope[kMaxL];
  const float* x; long ldx;
  const float* W[kMaxL]; long ldw[kMaxL];
  const float* b[kMaxL];
  float* y; long ldy;
  const float* go; long ldgo;
  float* gx; long ldgx;
  float* gw[kMaxL]; float* gb[kMaxL];
  int need_x, need_w[kMaxL], need_b[kMaxL];
  int keep;                // a parameter gradient is wanted: (a) stores h and dz, (b) and (c) run
  float* hs[kMaxL];        // hs[l] (V, w[l]), l = 1 .. L - 1: the input of layer l + 1 (hs[0] is x itself)
  float* dz[kMaxL];        // dz[l] (V, w[l + 1]): the cotangent of layer l + 1's pre-activation
  float* part;             // [n_slab][S]: per layer grad_W (w[l + 1], w[l]) | grad_b [w[l + 1]]
  long S;                  // sum_l w[l + 1] (w[l] + 1)
  long slab;
  int n_slab;
};

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }

// torch's forms, the point a == 0 and NaN included: relu = threshold(a, 0, 0), leaky_relu = a > 0 ? a : a slope
__device__ __forceinline__ float act_fwd(float a, int act, float slope) {
  if (act == PNA_MLP_ACT_RELU) return a <= 0.f ? 0.f : a;
  if (act == PNA_MLP_ACT_LEAKY) return a > 0.f ? a : a * slope;
  return a;
}

// dz = g act'(a): threshold_backward (0 where a <= 0) and leaky_relu_backward (g slope where a <= 0)
__device__ __forceinline__ float act_bwd(float g, float a, int act, float slope) {
  if (act == PNA_MLP_ACT_RELU) return a <= 0.f ? 0.f : g;
  if (act == PNA_MLP_ACT_LEAKY) return a > 0.f ? g : g * slope;
  return g;
}

// One B fragment of four consecutive k of a row-major parameter row (any pitch: scalar loads), zero where masked.
__device__ __forceinline__ f4 wfrag_row(const float* wrow, int k, int K, bool ok) {
  f4 b;
  b.x = (ok && k + 0 < K) ? wrow[min(k + 0, K - 1)] : 0.f;
  b.y = (ok && k + 1 < K) ? wrow[min(k + 1, K - 1)] : 0.f;
  b.z = (ok && k + 2 < K) ? wrow[min(k + 2, K - 1)] : 0.f;
  b.w = (ok && k + 3 < K) ? wrow[min(k + 3, K - 1)] : 0.f;
  return b;
}

// The x tile of rows [r0, r0 + nrows) into T [16][P]: zeros in the K padding columns and in the rows past the matrix's end.
__device__ __forceinline__ void load_x_tile(const MArgs& g, float* T, int P, long r0, int nrows) {
  const int K = g.w[0];
  for (int i = threadIdx.x; i < kRows * P; i += kThreads) {
    const int r = i / P, k = i - r * P;
    T[i] = (r < nrows && k < K) ? g.x[(r0 + r) * g.ldx + k] : 0.f;
  }
}

// ---- forward: one launch -----------------------------------------------------------------------------------------------------------
// lds: two buffers [16][PM], PM = the pitch of the widest layer input; layer l reads buffer l & 1 and writes the other
__global__ __launch_bounds__(kThreads) void k_mlp_rows_fwd(const MArgs g, const int PM) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const long r0 = (long)blockIdx.x * kRows;
  const int nrows = (int)lmin(kRows, g.V - r0);
  load_x_tile(g, lds, PM, r0, nrows);
  __syncthreads();
  for (int l = 0; l < g.L; ++l) {
    const float* const A = lds + (l & 1) * kRows * PM;
    float* const Z = lds + ((l + 1) & 1) * kRows * PM;
    const int K = g.w[l], N = g.w[l + 1], QK = quads(K), NT = (N + 15) / 16;
    const int act = g.act[l];
    const float slope = g.slope[l];
    const bool last = l == g.L - 1;
    for (int nt = wave; nt < NT; nt += kWaves) {
      const int n = nt * 16 + li;
      const bool nok = n < N;
      const int nc = min(n, N - 1);
      const float* const wr = g.W[l] + (long)nc * g.ldw[l];
      f4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int qd = 0; qd < QK; ++qd) {
        const int k = 16 * qd + 4 * lg;
        quad_fma(acc, *reinterpret_cast<const f4*>(A + li * PM + k), wfrag_row(wr, k, K, nok));
      }
      const float bias = g.b[l] ? g.b[l][nc] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lg + i;
        const float h = act_fwd(g.b[l] ? acc[i] + bias : acc[i], act, slope);
        if (last) {
          if (nok && r < nrows) g.y[(r0 + r) * g.ldy + n] = h;
        } else {
          Z[r * PM + n] = nok ? h : 0.f;                               // (the tiles cover the next layer's K pitch: zeros past N)
        }
      }
    }
    __syncthreads();
  }
}

// ---- backward (a): the rows kernel ----------------------------------------------------------------------------------------------
// lds: X [16][P(w0)] | Z_1 [16][P(w1)] | .. | Z_L [16][P(wL)]: Z_l holds a_l, then dz_l in its place
__global__ __launch_bounds__(kThreads) void k_mlp_rows_bwd(const MArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const long r0 = (long)blockIdx.x * kRows;
  const int nrows = (int)lmin(kRows, g.V - r0);
  const int L = g.L;
  load_x_tile(g, lds, pitch_of(quads(g.w[0])), r0, nrows);
  __syncthreads();
  // the forward of these rows: a_l into Z_l; the A fragment of layer l + 1 is act_l(a_l) as it is read
  {
    const float* A = lds;
    for (int l = 0; l < L; ++l) {
      const int K = g.w[l], N = g.w[l + 1], QK = quads(K), PA = pitch_of(QK), PZ = pitch_of(quads(N)), NT = (N + 15) / 16;
      float* const Z = const_cast<float*>(A) + kRows * PA;
      const int pact = l > 0 ? g.act[l - 1] : PNA_MLP_ACT_NONE;
      const float pslope = l > 0 ? g.slope[l - 1] : 0.f;
      for (int nt = wave; nt < NT; nt += kWaves) {
        const int n = nt * 16 + li;
        const bool nok = n < N;
        const int nc = min(n, N - 1);
        const float* const wr = g.W[l] + (long)nc * g.ldw[l];
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int qd = 0; qd < QK; ++qd) {
          const int k = 16 * qd + 4 * lg;
          f4 a = *reinterpret_cast<const f4*>(A + li * PA + k);
          a.x = act_fwd(a.x, pact, pslope); a.y = act_fwd(a.y, pact, pslope); a.z = act_fwd(a.z, pact, pslope); a.w = act_fwd(a.w, pact, pslope);
          quad_fma(acc, a, wfrag_row(wr, k, K, nok));
        }
        const float bias = g.b[l] ? g.b[l][nc] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * lg + i;
          const float a = g.b[l] ? acc[i] + bias : acc[i];
          Z[r * PZ + n] = nok ? a : 0.f;                               // (act(0) = 0: zeros past N stay zeros as the next A)
          if (g.keep && l < L - 1 && nok && r < nrows) g.hs[l + 1][(r0 + r) * N + n] = act_fwd(a, g.act[l], g.slope[l]);
        }
      }
      __syncthreads();
      A = Z;
    }
  }
  // dz_L = grad_out act_L'(a_L) in place of a_L: zeros past the width and past the matrix's end
  float* Zl = lds;
  for (int l = 0; l <= L; ++l) Zl += l > 0 ? kRows * pitch_of(quads(g.w[l - 1])) : 0;     // Z_L
  {
    const int N = g.w[L], PZ = pitch_of(quads(N));
    const int act = g.act[L - 1];
    const float slope = g.slope[L - 1];
    for (int i = tid; i < kRows * PZ; i += kThreads) {
      const int r = i / PZ, n = i - r * PZ;
      float d = 0.f;
      if (r < nrows && n < N) {
        d = act_bwd(g.go[(r0 + r) * g.ldgo + n], Zl[i], act, slope);
        if (g.keep) g.dz[L - 1][(r0 + r) * N + n] = d;
      }
      Zl[i] = d;
    }
  }
  __syncthreads();
  // down the layers: g_(l-1) = dz_l W_l, K = the outputs of layer l; the result's columns are its inputs
  for (int l = L - 1; l >= 0; --l) {
    if (l == 0 && !g.need_x) break;
    const int K = g.w[l + 1], C = g.w[l], QK = quads(K), PD = pitch_of(QK), PC = pitch_of(quads(C)), NT = (C + 15) / 16;
    const float* const D = Zl;
    float* const Zp = Zl - kRows * PC;                                 // Z_(l): a_l (l >= 1), the x tile (l == 0, not written)
    const int act = l > 0 ? g.act[l - 1] : PNA_MLP_ACT_NONE;
    const float slope = l > 0 ? g.slope[l - 1] : 0.f;
    const long ld = g.ldw[l];
    for (int ct = wave; ct < NT; ct += kWaves) {
      const int c = ct * 16 + li;
      const bool cok = c < C;
      const float* const Wc = g.W[l] + min(c, C - 1);
      f4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int qd = 0; qd < QK; ++qd) {
        const int k = 16 * qd + 4 * lg;
        f4 b;                                                          // B[k][c] = W[k][c]: the lanes of a group read one row
        b.x = (cok && k + 0 < K) ? Wc[(long)min(k + 0, K - 1) * ld] : 0.f;
        b.y = (cok && k + 1 < K) ? Wc[(long)min(k + 1, K - 1) * ld] : 0.f;
        b.z = (cok && k + 2 < K) ? Wc[(long)min(k + 2, K - 1) * ld] : 0.f;
        b.w = (cok && k + 3 < K) ? Wc[(long)min(k + 3, K - 1) * ld] : 0.f;
        quad_fma(acc, *reinterpret_cast<const f4*>(D + li * PD + k), b);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lg + i;
        const bool live = cok && r < nrows;
        if (l == 0) {
          if (live) g.gx[(r0 + r) * g.ldgx + c] = acc[i];
          continue;
        }
        const float d = live ? act_bwd(acc[i], Zp[r * PC + c], act, slope) : 0.f;
        Zp[r * PC + c] = d;                                            // (this lane alone reads and writes the element)
        if (g.keep && live) g.dz[l - 1][(r0 + r) * C + c] = d;
      }
    }
    __syncthreads();
    Zl = Zp;
  }
}

// ---- backward (b): one slab's weight and bias gradients of every layer ------------------------------------------------------------
// grid (n_slab, sum_l ceil(w[l + 1] / 16)): the workgroup owns output rows [16 jt, 16 jt + 16) of one layer's weight over the slab's rows;
// a wavefront takes 16-column tiles.  A[j][v] = dz_l[v][j], B[v][c] = h_(l-1)[v][c], both straight from memory; the rows of a slab in
// order, 16 per step.  The job of column tile 0 also sums the band's bias gradient (B = 1).
__global__ __launch_bounds__(kDwThreads) void k_mlp_dw_slab(const MArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  int l = 0, jt = blockIdx.y;
  long off = 0;                                                        // the layer's offset inside a slab's image
  for (; l < g.L - 1; ++l) {
    const int bands = (g.w[l + 1] + 15) / 16;
    if (jt < bands) break;
    jt -= bands;
    off += (long)g.w[l + 1] * (g.w[l] + 1);
  }
  if (!(g.need_w[l] || g.need_b[l])) return;                            // (workgroup-uniform)
  const int C = g.w[l], J = g.w[l + 1];
  const long v0 = (long)blockIdx.x * g.slab;
  const long v1 = lmin(g.V, v0 + g.slab);
  const int ja = jt * 16 + li;                                         // the output this lane feeds as A
  const bool jok = ja < J;
  const float* const dcol = g.dz[l] + min(ja, J - 1);
  const float* const hsrc = l == 0 ? g.x : g.hs[l];
  const long ldh = l == 0 ? g.ldx : (long)C;
  float* const pw = g.part + (long)blockIdx.x * g.S + off;
  float* const pb = pw + (long)J * C;
  const int NT = (C + 15) / 16;
  for (int ct = wave; ct < NT; ct += kDwThreads / 64) {
    const int c = ct * 16 + li;
    const bool cok = c < C;
    const float* const src = hsrc + min(c, C - 1);
    f4 acc = {0.f, 0.f, 0.f, 0.f}, accb = acc;
    const f4 ones = {1.f, 1.f, 1.f, 1.f};
    for (long vb = v0; vb < v1; vb += 16) {
      const long v = vb + 4 * lg;
      f4 a, b;
      a.x = (jok && v + 0 < v1) ? dcol[lmin(v + 0, v1 - 1) * J] : 0.f;
      a.y = (jok && v + 1 < v1) ? dcol[lmin(v + 1, v1 - 1) * J] : 0.f;
      a.z = (jok && v + 2 < v1) ? dcol[lmin(v + 2, v1 - 1) * J] : 0.f;
      a.w = (jok && v + 3 < v1) ? dcol[lmin(v + 3, v1 - 1) * J] : 0.f;
      b.x = (cok && v + 0 < v1) ? src[lmin(v + 0, v1 - 1) * ldh] : 0.f;
      b.y = (cok && v + 1 < v1) ? src[lmin(v + 1, v1 - 1) * ldh] : 0.f;
      b.z = (cok && v + 2 < v1) ? src[lmin(v + 2, v1 - 1) * ldh] : 0.f;
      b.w = (cok && v + 3 < v1) ? src[lmin(v + 3, v1 - 1) * ldh] : 0.f;
      quad_fma(acc, a, b);
      if (ct == 0) quad_fma(accb, a, ones);                            // (wavefront-uniform)
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = jt * 16 + 4 * lg + i;                              // the result's row
      if (j >= J) continue;
      if (cok) pw[(long)j * C + c] = acc[i];
      if (ct == 0 && li == 0) pb[j] = accb[i];
    }
  }
}

// ---- backward (c): one thread per parameter element, the slabs added in slab order in float64 ------------------------------------
__device__ __forceinline__ float slab_sum(const float* p, long stride, int n_slab) {
  double acc = 0.0;
  int s = 0;
  for (; s + 8 <= n_slab; s += 8) {                                    // eight slabs' loads in flight, added in slab order
    float t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = p[(long)(s + k) * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += (double)t[k];
  }
  for (; s < n_slab; ++s) acc += (double)p[(long)s * stride];
  return (float)acc;
}

__global__ __launch_bounds__(256) void k_mlp_dw_final(const MArgs g) {
  long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= g.S) return;
  const float* const p = g.part + e;
  for (int l = 0; l < g.L; ++l) {
    const long nw = (long)g.w[l + 1] * g.w[l], nb = g.w[l + 1];
    if (e < nw) {                                                      // the slab's image of grad_W_l is the gradient's own layout
      if (g.need_w[l]) g.gw[l][e] = slab_sum(p, g.S, g.n_slab);
      return;
    }
    e -= nw;
    if (e < nb) {
      if (g.need_b[l]) g.gb[l][e] = slab_sum(p, g.S, g.n_slab);
      return;
    }
    e -= nb;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline long slab_rows(long V) {
  const long l = (V + PNA_MLP_MAX_SLABS - 1) / PNA_MLP_MAX_SLABS;
  return l > PNA_MLP_SLAB_ROWS ? l : PNA_MLP_SLAB_ROWS;
}

// NULL inside the scope, else the clause that refuses
const char* scope_clause(int64_t V, int L, const int32_t* widths, const int32_t* acts) {
  if (L < 1 || L > kMaxL) return "needs 1 <= n_layers <= 4";
  if (!widths) return "needs widths[n_layers + 1]";
  for (int l = 0; l <= L; ++l)
    if (widths[l] < 1 || widths[l] > kMaxWidth) return "needs every width in 1 .. 128";
  if (V < 1 || V > INT32_MAX) return "needs V >= 1 rows (and V < 2^31)";
  if (acts)
    for (int l = 0; l < L; ++l)
      if (acts[l] != PNA_MLP_ACT_NONE && acts[l] != PNA_MLP_ACT_RELU && acts[l] != PNA_MLP_ACT_LEAKY)
        return "needs every act one of PNA_MLP_ACT_NONE / _RELU / _LEAKY";
  return nullptr;
}

int64_t row_floats(int L, const int32_t* w) {                          // h_1 .. h_(L-1) and dz_1 .. dz_L of one row
  int64_t n = 0;
  for (int l = 1; l <= L; ++l) n += (l < L ? 2 : 1) * (int64_t)w[l];
  return n;
}

int64_t slab_floats(int L, const int32_t* w) {
  int64_t n = 0;
  for (int l = 1; l <= L; ++l) n += (int64_t)w[l] * (w[l - 1] + 1);
  return n;
}

int fill(const pna_mlp_head_args* p, MArgs& g, bool bwd, const char* fn) {
  if (!p) return pna_refuse(fn, "args is NULL");
  if (int rc_ss = pna_check_struct_size(fn, p->struct_size, sizeof(*p))) return rc_ss;
  if (const char* c = scope_clause(p->V, p->n_layers, p->widths, p->act)) return pna_refuse(fn, c);
  const int L = p->n_layers;
  if (!p->x || p->ldx < p->widths[0]) return pna_refuse(fn, "needs x (V, ldx >= widths[0])");
  for (int l = 0; l < L; ++l)
    if (!p->w[l] || p->ldw[l] < p->widths[l]) return pna_refuse(fn, "needs every w[l] (widths[l + 1], ldw[l] >= widths[l])");
  memset(&g, 0, sizeof(g));
  g.V = p->V; g.L = L;
  for (int l = 0; l <= L; ++l) g.w[l] = p->widths[l];
  for (int l = 0; l < L; ++l) {
    g.act[l] = p->act[l]; g.slope[l] = p->slope[l];
    g.W[l] = p->w[l]; g.ldw[l] = (long)p->ldw[l]; g.b[l] = p->b[l];
  }
  g.x = p->x; g.ldx = (long)p->ldx;
  if (!bwd) {
    if (!p->y || p->ldy < p->widths[L]) return pna_refuse(fn, "needs y (V, ldy >= widths[n_layers])");
    g.y = p->y; g.ldy = (long)p->ldy;
    return PNA_OK;
  }
  if (!p->grad_out || p->ld_go < p->widths[L]) return pna_refuse(fn, "needs grad_out (V, ld_go >= widths[n_layers])");
  if (p->need_x && (!p->grad_x || p->ld_gx < p->widths[0])) return pna_refuse(fn, "need_x needs grad_x (V, ld_gx >= widths[0])");
  for (int l = 0; l < L; ++l) {
    if ((p->need_w[l] && !p->grad_w[l]) || (p->need_b[l] && !p->grad_b[l]))
      return pna_refuse(fn, "every need_w / need_b flag needs its gradient buffer");
    g.need_w[l] = p->need_w[l] != 0; g.need_b[l] = p->need_b[l] != 0;
    g.gw[l] = p->grad_w[l]; g.gb[l] = p->grad_b[l];
    g.keep |= g.need_w[l] | g.need_b[l];
  }
  g.need_x = p->need_x != 0;
  g.go = p->grad_out; g.ldgo = (long)p->ld_go;
  g.gx = p->grad_x; g.ldgx = (long)p->ld_gx;
  if (!g.keep) return PNA_OK;                                          // grad_x alone needs no workspace
  const int64_t need = pna_mlp_head_workspace_bytes(p->V, L, p->widths);
  if (!p->workspace || ((uintptr_t)p->workspace & 15) || p->workspace_bytes < need)
    return pna_refuse(fn, "needs a 16-byte aligned workspace of pna_mlp_head_workspace_bytes(V, n_layers, widths)");
  g.slab = slab_rows(g.V);
  g.n_slab = (int)((g.V + g.slab - 1) / g.slab);
  g.S = slab_floats(L, p->widths);
  float* ws = (float*)p->workspace;
  for (int l = 1; l < L; ++l) { g.hs[l] = ws; ws += g.V * g.w[l]; }
  for (int l = 0; l < L; ++l) { g.dz[l] = ws; ws += g.V * g.w[l + 1]; }
  g.part = ws;
  return PNA_OK;
}

}  // namespace

extern "C" int32_t pna_mlp_head_in_scope(int64_t V, int32_t n_layers, const int32_t* widths, const int32_t* acts) {
  if (!acts) return 0;
  return !scope_clause(V, n_layers, widths, acts);
}

extern "C" int64_t pna_mlp_head_workspace_bytes(int64_t V, int32_t n_layers, const int32_t* widths) {
  if (scope_clause(V, n_layers, widths, nullptr)) return -1;
  const long slab = slab_rows(V);
  const int64_t n_slab = (V + slab - 1) / slab;
  return (V * row_floats(n_layers, widths) + n_slab * slab_floats(n_layers, widths)) * 4;
}

extern "C" int pna_mlp_head_fwd_f32(const pna_mlp_head_args* p, pna_stream_t stream) {
  MArgs g;
  const int rc = fill(p, g, false, "pna_mlp_head_fwd_f32");
  if (rc != PNA_OK) return rc;
  int wmax = 0;
  for (int l = 0; l < g.L; ++l) wmax = g.w[l] > wmax ? g.w[l] : wmax;  // the widest layer INPUT
  const int PM = pitch_of(quads(wmax));
  const size_t lds = (size_t)2 * kRows * PM * sizeof(float);           // <= 16.5 KiB
  hipLaunchKernelGGL(k_mlp_rows_fwd, dim3((unsigned)((g.V + kRows - 1) / kRows)), dim3(kThreads), lds, (hipStream_t)stream, g, PM);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_mlp_head_fwd_f32: launch failed");
  return PNA_OK;
}

extern "C" int pna_mlp_head_bwd_f32(const pna_mlp_head_args* p, pna_stream_t stream) {
  MArgs g;
  const int rc = fill(p, g, true, "pna_mlp_head_bwd_f32");
  if (rc != PNA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!(g.need_x || g.keep)) return PNA_OK;
  size_t lds = 0;
  int bands = 0;
  for (int l = 0; l <= g.L; ++l) lds += (size_t)kRows * pitch_of(quads(g.w[l])) * sizeof(float);      // <= 41.25 KiB
  for (int l = 1; l <= g.L; ++l) bands += (g.w[l] + 15) / 16;
  hipLaunchKernelGGL(k_mlp_rows_bwd, dim3((unsigned)((g.V + kRows - 1) / kRows)), dim3(kThreads), lds, st, g);
  if (g.keep) {
    hipLaunchKernelGGL(k_mlp_dw_slab, dim3((unsigned)g.n_slab, (unsigned)bands), dim3(kDwThreads), 0, st, g);
    hipLaunchKernelGGL(k_mlp_dw_final, dim3((unsigned)((g.S + 255) / 256)), dim3(256), 0, st, g);
  }
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_mlp_head_bwd_f32: launch failed");
  return PNA_OK;
}
