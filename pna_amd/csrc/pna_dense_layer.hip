// pna_dense_layer.hip -- the dense-adjacency PNALayer (the multitask GNN's convolution) for gfx950, forward and backward as ONE C call each.
// Implements pna_dense_layer_{lds_bytes, workspace_bytes, fwd_f32, bwd_f32} of include/pna_amd.h.  Replaces models/pytorch/pna/layer.py:33-49,99-109 with
// aggregators.py:17-73 and scalers.py:7-38, and what autograd derives from them.
//
// A graph is at most PNA_DENSE_MAX_NODES nodes: its adjacency block, its factorised messages m[i,j] = P[i] + Q[j] (P = W_p x, Q = W_q x + b per
// tower), its aggregates and its posttrans rows all sit in ONE workgroup's LDS.  mean / std reduce over the second node index and max / min over
// the first: on the block in LDS that is a row walk and a column walk -- no CSR, no sort, no second edge order.
//
// lds (floats; pna_dense_layer_lds_bytes is the one formula, functional.dense_layer_fits its mirror):
//   ADJ [N][N | 1]   the block as stored (+ I on the diagonal when self_loop, after the scalers' degrees are taken); the odd pitch keeps the
//                    row walk -- lanes of a wavefront on different rows, one column -- off a shared bank
//   X   [N][in_dim]  (budgeted as N T Fi)
//   P, Q [N][T Fi]   backward: dP and dQ take their place once the forward is rebuilt
//   MU, HS [N][T Fi] the weighted mean of Q over the row; 1 / (2 std), 0 where var <= 0 or the row is empty
//   AGG [N][T][A][Fi] backward: G = d loss / d aggregate takes its place
//   Y   [N][T Fo]    the towers' outputs side by side; backward: g_y takes its place
//   GP  [N][T Fo]    backward: grad_out leaky'(p)
//   DEG [3 + S][N]   D = sum_j adj, D' = sum_j a', row-has-an-entry, the S scaler factors
//   ARG [2][N][T Fi] bytes: the winning first index of max and of min, 255 = empty column
// Forward: one launch, a workgroup per slab of consecutive graphs (one graph each up to PNA_DENSE_MAX_SLABS graphs).  Backward: (a) the same
// workgroups rebuild the forward with the SAME device functions (the LeakyReLU mask and the arg indices are the forward's by construction),
// form grad_x and add the graph's parameter gradients into the slab's image of the workspace, graph after graph; (b) the images are added in
// slab order in float64.  Every sum has a fixed order; no atomics of any kind: bitwise repeatable.  No kernel waits for another workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "pna_amd.h"
#include "pna_internal.h"

namespace {

constexpr int kThreads = 512;
constexpr int kLdsBudget = 160 * 1024;      // one workgroup may hold the CU's whole LDS
constexpr int kMaxWide = 64;                // T Fi and T Fo
constexpr int kEmpty = 255;

struct DArgs {
  long B;
  int N, IN, T, Fi, Fo, divide, self_loop, A, S;
  int ia_mean, ia_max, ia_min, ia_std;      // position in the caller's aggregator list, -1 = absent
  int scaler[3];
  float slope;
  const float* x; const float* adj; const float* avg_log; const float* avg_lin;
  const float* w_pre[PNA_MAX_TOWER]; const float* b_pre[PNA_MAX_TOWER];
  const float* w_post[PNA_MAX_TOWER]; const float* b_post[PNA_MAX_TOWER];
  const float* w_mix; const float* b_mix;
  float* out;
  const float* go;
  float* gx;
  float* g_w_pre[PNA_MAX_TOWER]; float* g_b_pre[PNA_MAX_TOWER];
  float* g_w_post[PNA_MAX_TOWER]; float* g_b_post[PNA_MAX_TOWER];
  float* g_w_mix; float* g_b_mix;
  float* part;                               // [n_slab][image]
  long slab;                                 // graphs per slab
  int n_slab;
};

// ---- the one LDS layout ----------------------------------------------------------------------------------------------------------------
struct Lay {
  int PA, TF, C, KA, Kp;
  int adj, x, p, q, mu, hs, agg, y, gp, deg, arg;      // float offsets
  long bytes;
};

__host__ __device__ inline Lay layout(int N, int T, int Fi, int Fo, int A, int S) {
  Lay l;
  l.PA = N | 1; l.TF = T * Fi; l.C = T * Fo; l.KA = A * l.TF; l.Kp = (1 + A * S) * Fi;
  int o = 0;
  l.adj = o; o += N * l.PA;
  l.x = o; o += N * l.TF;
  l.p = o; o += N * l.TF;
  l.q = o; o += N * l.TF;
  l.mu = o; o += N * l.TF;
  l.hs = o; o += N * l.TF;
  l.agg = o; o += N * l.KA;
  l.y = o; o += N * l.C;
  l.gp = o; o += N * l.C;
  l.deg = o; o += N * (3 + S);
  l.arg = o;
  l.bytes = 4L * o + ((2L * N * l.TF + 15) / 16) * 16;
  return l;
}

// floats of one slab's image: per tower w_pre (Fi, 2 Fi) | b_pre | w_post (Fo, Kp) | b_post, then w_mix (C, C) | b_mix
__host__ __device__ inline long image_floats(int T, int Fi, int Fo, int A, int S) {
  const long Kp = (1L + (long)A * S) * Fi, C = (long)T * Fo;
  return T * (2L * Fi * Fi + Fi + Fo * Kp + Fo) + C * C + C;
}

struct Img { long wpre, bpre, wpost, bpost, wmix, bmix; };
__host__ __device__ inline Img image_offsets(int T, int Fi, int Fo, int A, int S) {
  const long Kp = (1L + (long)A * S) * Fi, C = (long)T * Fo;
  Img m;
  m.wpre = 0;
  m.bpre = m.wpre + T * 2L * Fi * Fi;
  m.wpost = m.bpre + (long)T * Fi;
  m.bpost = m.wpost + T * Fo * Kp;
  m.wmix = m.bpost + (long)T * Fo;
  m.bmix = m.wmix + C * C;
  return m;
}

struct Lds {
  float *adj, *x, *p, *q, *mu, *hs, *agg, *y, *gp, *deg;
  unsigned char* arg;
  int PA, TF, C, KA, Kp;
};

__device__ __forceinline__ Lds carve(float* base, const DArgs& g) {
  const Lay l = layout(g.N, g.T, g.Fi, g.Fo, g.A, g.S);
  Lds L;
  L.adj = base + l.adj; L.x = base + l.x; L.p = base + l.p; L.q = base + l.q; L.mu = base + l.mu; L.hs = base + l.hs;
  L.agg = base + l.agg; L.y = base + l.y; L.gp = base + l.gp; L.deg = base + l.deg;
  L.arg = reinterpret_cast<unsigned char*>(base + l.arg);
  L.PA = l.PA; L.TF = l.TF; L.C = l.C; L.KA = l.KA; L.Kp = l.Kp;
  return L;
}

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }

// ---- the forward of one graph, phase by phase (shared by the forward kernel and by the backward's rebuild) ---------------------------------
__device__ __forceinline__ void fwd_load(const DArgs& g, const Lds& L, long b) {
  const int N = g.N, tid = threadIdx.x;
  const float* const adj = g.adj + b * N * N;
  for (int e = tid; e < N * N; e += kThreads) {
    const int i = e / N, j = e - i * N;
    L.adj[i * L.PA + j] = adj[e];
  }
  const float* const x = g.x + b * N * g.IN;
  for (int e = tid; e < N * g.IN; e += kThreads) L.x[e] = x[e];
  __syncthreads();
}

// degrees (of the ORIGINAL adjacency: the scalers never see the self loop), the scaler factors, a' = adj + I in place, and P, Q
__device__ __forceinline__ void fwd_nodes(const DArgs& g, const Lds& L) {
  const int N = g.N, tid = threadIdx.x, TF = L.TF, Fi = g.Fi;
  const float avg_log = g.avg_log ? *g.avg_log : 1.f, avg_lin = g.avg_lin ? *g.avg_lin : 1.f;
  for (int i = tid; i < N; i += kThreads) {
    float* const row = L.adj + i * L.PA;
    float d = 0.f, dp = 0.f;
    int any = 0;
    for (int j = 0; j < N; ++j) {
      const float a = row[j];
      const float ap = (g.self_loop && j == i) ? a + 1.f : a;
      d += a;
      dp += ap;
      any |= (ap != 0.f);
    }
    if (g.self_loop) row[i] = row[i] + 1.f;
    L.deg[i] = d;
    L.deg[N + i] = dp;
    L.deg[2 * N + i] = any ? 1.f : 0.f;
    for (int s = 0; s < g.S; ++s) {
      float f = 1.f;
      switch (g.scaler[s]) {
        case PNA_DENSE_SCALER_AMPLIFICATION: f = logf(d + 1.f) / avg_log; break;
        case PNA_DENSE_SCALER_ATTENUATION: f = avg_log / logf(d + 1.f); break;
        case PNA_DENSE_SCALER_LINEAR: f = d / avg_lin; break;
        case PNA_DENSE_SCALER_INVERSE_LINEAR: f = avg_lin / d; break;
        default: break;
      }
      L.deg[(3 + s) * N + i] = f;
    }
  }
  for (int e = tid; e < N * TF; e += kThreads) {
    const int i = e / TF, c = e - i * TF, t = c / Fi, f = c - t * Fi;
    const float* const w = g.w_pre[t] + (long)f * 2 * Fi;
    const float* const xr = L.x + i * g.IN + (g.divide ? t * Fi : 0);
    float p = 0.f, q = 0.f;
    for (int k = 0; k < Fi; ++k) {
      p += w[k] * xr[k];
      q += w[Fi + k] * xr[k];
    }
    L.p[e] = p;
    L.q[e] = q + g.b_pre[t][f];
  }
  __syncthreads();
}

// the aggregates of node n, tower-feature c: the row walk (mean, std) and the column walk (max, min)
__device__ __forceinline__ void fwd_aggregate(const DArgs& g, const Lds& L) {
  const int N = g.N, tid = threadIdx.x, TF = L.TF, Fi = g.Fi, PA = L.PA;
  for (int e = tid; e < N * TF; e += kThreads) {
    const int n = e / TF, c = e - n * TF, t = c / Fi, f = c - t * Fi;
    float* const out = L.agg + n * L.KA + t * g.A * Fi + f;
    if (g.ia_mean >= 0 || g.ia_std >= 0) {
      const float* const row = L.adj + n * PA;
      const float dp = L.deg[N + n];
      const bool any = L.deg[2 * N + n] != 0.f;
      float s = 0.f;
      for (int j = 0; j < N; ++j) s += row[j] * L.q[j * TF + c];
      const float mu = any ? s / dp : 0.f;
      L.mu[e] = mu;
      if (g.ia_mean >= 0) out[g.ia_mean * Fi] = any ? L.p[e] + mu : 0.f;
      if (g.ia_std >= 0) {
        float v = 0.f;                                     // the weighted variance of Q alone, centred: the shift by P[n] does not change it
        for (int j = 0; j < N; ++j) {
          const float d = L.q[j * TF + c] - mu;
          v += row[j] * (d * d);
        }
        v = any ? v / dp : 0.f;
        const float sd = sqrtf((v > 0.f ? v : 0.f) + 1e-5f);
        out[g.ia_std * Fi] = any ? sd : 0.f;
        L.hs[e] = (any && v > 0.f) ? 0.5f / sd : 0.f;
      }
    }
    if (g.ia_max >= 0 || g.ia_min >= 0) {
      float mx = 0.f, mn = 0.f;
      int imx = kEmpty, imn = kEmpty;
      for (int i = 0; i < N; ++i) {
        if (!(L.adj[i * PA + n] > 0.f)) continue;
        const float pv = L.p[i * TF + c];
        if (imx == kEmpty || pv > mx) { mx = pv; imx = i; }        // strict: the first extremal i wins, as the existing route's by_col order
        if (imn == kEmpty || pv < mn) { mn = pv; imn = i; }
      }
      const float qv = L.q[e];
      if (g.ia_max >= 0) out[g.ia_max * Fi] = imx == kEmpty ? 0.f : qv + mx;
      if (g.ia_min >= 0) out[g.ia_min * Fi] = imn == kEmpty ? 0.f : qv + mn;
      L.arg[e] = (unsigned char)imx;
      L.arg[N * TF + e] = (unsigned char)imn;
    }
  }
  __syncthreads();
}

// z_t = b_post + W_h x_t + sum_s f_s(D) W_s a_t: the scaled operand is never formed
__device__ __forceinline__ void fwd_post(const DArgs& g, const Lds& L) {
  const int N = g.N, tid = threadIdx.x, C = L.C, Fi = g.Fi, Fo = g.Fo, AF = g.A * Fi;
  for (int e = tid; e < N * C; e += kThreads) {
    const int i = e / C, cc = e - i * C, t = cc / Fo, o = cc - t * Fo;
    const float* const w = g.w_post[t] + (long)o * L.Kp;
    const float* const xr = L.x + i * g.IN + (g.divide ? t * Fi : 0);
    const float* const ag = L.agg + i * L.KA + t * AF;
    float h = 0.f;
    for (int k = 0; k < Fi; ++k) h += w[k] * xr[k];
    float z = g.b_post[t][o] + h;
    for (int s = 0; s < g.S; ++s) {
      const float* const ws = w + Fi + s * AF;
      float u = 0.f;
      for (int m = 0; m < AF; ++m) u += ws[m] * ag[m];
      z += g.scaler[s] == PNA_DENSE_SCALER_IDENTITY ? u : L.deg[(3 + s) * N + i] * u;
    }
    L.y[e] = z;
  }
  __syncthreads();
}

// the mixing Linear's output before the LeakyReLU
__device__ __forceinline__ float mix_p(const DArgs& g, const Lds& L, int i, int co) {
  const float* const w = g.w_mix + (long)co * L.C;
  const float* const y = L.y + i * L.C;
  float p = 0.f;
  for (int c = 0; c < L.C; ++c) p += w[c] * y[c];
  return p + g.b_mix[co];
}

__global__ __launch_bounds__(kThreads) void k_dense_layer_fwd(const DArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L = carve(lds, g);
  const int N = g.N, tid = threadIdx.x, C = L.C;
  const long b0 = (long)blockIdx.x * g.slab, b1 = lmin(g.B, b0 + g.slab);
  for (long b = b0; b < b1; ++b) {
    fwd_load(g, L, b);
    fwd_nodes(g, L);
    fwd_aggregate(g, L);
    fwd_post(g, L);
    float* const out = g.out + b * N * C;
    for (int e = tid; e < N * C; e += kThreads) {
      const float p = mix_p(g, L, e / C, e % C);
      out[e] = p > 0.f ? p : p * g.slope;
    }
    __syncthreads();
  }
}

// ---- backward (a) -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put(float* img, long idx, float v, bool first) {
  if (first) img[idx] = v;
  else img[idx] = img[idx] + v;                   // the same thread every graph: the slab's graphs are added in order
}

__global__ __launch_bounds__(kThreads) void k_dense_layer_bwd(const DArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds L = carve(lds, g);
  const int N = g.N, tid = threadIdx.x, C = L.C, TF = L.TF, Fi = g.Fi, Fo = g.Fo, A = g.A, AF = g.A * Fi, KA = L.KA, Kp = L.Kp, PA = L.PA, T = g.T;
  const Img off = image_offsets(T, Fi, Fo, A, g.S);
  float* const img = g.part + (long)blockIdx.x * image_floats(T, Fi, Fo, A, g.S);
  const long b0 = (long)blockIdx.x * g.slab, b1 = lmin(g.B, b0 + g.slab);
  for (long b = b0; b < b1; ++b) {
    const bool first = b == b0;
    fwd_load(g, L, b);
    fwd_nodes(g, L);
    fwd_aggregate(g, L);
    fwd_post(g, L);
    // g_p = grad_out leaky'(p)
    const float* const go = g.go + b * N * C;
    for (int e = tid; e < N * C; e += kThreads) {
      const float p = mix_p(g, L, e / C, e % C);
      L.gp[e] = p > 0.f ? go[e] : go[e] * g.slope;
    }
    __syncthreads();
    // grad w_mix = g_p^T y, grad b_mix
    for (int e = tid; e < C * C + C; e += kThreads) {
      float v = 0.f;
      if (e < C * C) {
        const int co = e / C, c = e - co * C;
        for (int i = 0; i < N; ++i) v += L.gp[i * C + co] * L.y[i * C + c];
      } else {
        const int co = e - C * C;
        for (int i = 0; i < N; ++i) v += L.gp[i * C + co];
      }
      put(img, off.wmix + e, v, first);
    }
    __syncthreads();
    // g_y = g_p W_mix, in y's place
    for (int e = tid; e < N * C; e += kThreads) {
      const int i = e / C, c = e - i * C;
      float v = 0.f;
      for (int co = 0; co < C; ++co) v += L.gp[i * C + co] * g.w_mix[(long)co * C + c];
      L.y[e] = v;
    }
    __syncthreads();
    // grad w_post = g_y,t^T [x_t | f_s(D) a_t], grad b_post
    const int n_wpost = T * Fo * Kp;
    for (int e = tid; e < n_wpost + T * Fo; e += kThreads) {
      float v = 0.f;
      if (e < n_wpost) {
        const int t = e / (Fo * Kp), r = e - t * Fo * Kp, o = r / Kp, k = r - o * Kp;
        const float* const gy = L.y + t * Fo + o;
        if (k < Fi) {
          const float* const xc = L.x + (g.divide ? t * Fi : 0) + k;
          for (int i = 0; i < N; ++i) v += gy[i * C] * xc[i * g.IN];
        } else {
          const int m = k - Fi, s = m / AF, ra = m - s * AF;
          const float* const ag = L.agg + t * AF + ra;
          if (g.scaler[s] == PNA_DENSE_SCALER_IDENTITY) {
            for (int i = 0; i < N; ++i) v += gy[i * C] * ag[i * KA];
          } else {
            const float* const fs = L.deg + (3 + s) * N;
            for (int i = 0; i < N; ++i) v += gy[i * C] * (fs[i] * ag[i * KA]);
          }
        }
        put(img, off.wpost + e, v, first);
      } else {
        const int cc = e - n_wpost;                            // t Fo + o
        for (int i = 0; i < N; ++i) v += L.y[i * C + cc];
        put(img, off.bpost + cc, v, first);
      }
    }
    __syncthreads();
    // G = sum_s f_s(D) (g_y,t W_s), in the aggregates' place; through the std; 0 where the aggregate was the constant of an empty row / column
    for (int e = tid; e < N * KA; e += kThreads) {
      const int i = e / KA, r = e - i * KA, t = r / AF, m = r - t * AF, a = m / Fi, f = m - a * Fi;
      const float* const gy = L.y + i * C + t * Fo;
      float acc = 0.f;
      for (int s = 0; s < g.S; ++s) {
        const float* const w = g.w_post[t] + Fi + s * AF + m;
        float u = 0.f;
        for (int o = 0; o < Fo; ++o) u += gy[o] * w[(long)o * Kp];
        acc += g.scaler[s] == PNA_DENSE_SCALER_IDENTITY ? u : L.deg[(3 + s) * N + i] * u;
      }
      const int c = t * Fi + f;
      if (a == g.ia_mean && L.deg[2 * N + i] == 0.f) acc = 0.f;
      if (a == g.ia_std) acc = L.hs[i * TF + c] != 0.f ? acc * L.hs[i * TF + c] : 0.f;          // d loss / d var
      if (a == g.ia_max && L.arg[i * TF + c] == kEmpty) acc = 0.f;
      if (a == g.ia_min && L.arg[N * TF + i * TF + c] == kEmpty) acc = 0.f;
      L.agg[e] = acc;
    }
    __syncthreads();
    // dP and dQ of node n, in P's and Q's place (each thread reads no P and only its own Q)
    for (int e = tid; e < N * TF; e += kThreads) {
      const int n = e / TF, c = e - n * TF, t = c / Fi, f = c - t * Fi;
      const float* const G = L.agg + t * AF + f;               // + i KA + a Fi
      float dP = 0.f, dQ = 0.f;
      if (g.ia_mean >= 0) {
        dP += G[n * KA + g.ia_mean * Fi];
        for (int i = 0; i < N; ++i) {
          if (L.deg[2 * N + i] == 0.f) continue;
          dQ += (L.adj[i * PA + n] / L.deg[N + i]) * G[i * KA + g.ia_mean * Fi];
        }
      }
      if (g.ia_std >= 0) {
        const float qn = L.q[e];
        for (int i = 0; i < N; ++i) {
          if (L.deg[2 * N + i] == 0.f) continue;
          dQ += G[i * KA + g.ia_std * Fi] * ((2.f * L.adj[i * PA + n] * (qn - L.mu[i * TF + c])) / L.deg[N + i]);
        }
      }
      if (g.ia_max >= 0) {
        dQ += G[n * KA + g.ia_max * Fi];
        for (int j = 0; j < N; ++j)
          if (L.arg[j * TF + c] == n) dP += G[j * KA + g.ia_max * Fi];
      }
      if (g.ia_min >= 0) {
        dQ += G[n * KA + g.ia_min * Fi];
        for (int j = 0; j < N; ++j)
          if (L.arg[N * TF + j * TF + c] == n) dP += G[j * KA + g.ia_min * Fi];
      }
      L.p[e] = dP;
      L.q[e] = dQ;
    }
    __syncthreads();
    // grad_x = g_y,t W_h + dP W_p + dQ W_q: tower t's slice when the input is divided, else the towers added in order
    if (g.gx) {
      float* const gx = g.gx + b * N * g.IN;
      for (int e = tid; e < N * g.IN; e += kThreads) {
        const int i = e / g.IN, col = e - i * g.IN;
        const int t0 = g.divide ? col / Fi : 0, t1 = g.divide ? t0 + 1 : T, k = g.divide ? col - t0 * Fi : col;
        float v = 0.f;
        for (int t = t0; t < t1; ++t) {
          float u = 0.f;
          const float* const wpo = g.w_post[t] + k;
          const float* const gy = L.y + i * C + t * Fo;
          for (int o = 0; o < Fo; ++o) u += gy[o] * wpo[(long)o * Kp];
          const float* const wpr = g.w_pre[t] + k;
          const float* const dP = L.p + i * TF + t * Fi;
          const float* const dQ = L.q + i * TF + t * Fi;
          for (int f = 0; f < Fi; ++f) u += dP[f] * wpr[(long)f * 2 * Fi];
          for (int f = 0; f < Fi; ++f) u += dQ[f] * wpr[(long)f * 2 * Fi + Fi];
          v = t == t0 ? u : v + u;
        }
        gx[e] = v;
      }
    }
    // grad w_pre = [dP^T x_t | dQ^T x_t], grad b_pre = the column sums of dQ
    const int n_wpre = T * Fi * 2 * Fi;
    for (int e = tid; e < n_wpre + TF; e += kThreads) {
      float v = 0.f;
      if (e < n_wpre) {
        const int t = e / (2 * Fi * Fi), r = e - t * 2 * Fi * Fi, f = r / (2 * Fi), k2 = r - f * 2 * Fi;
        const float* const d = (k2 < Fi ? L.p : L.q) + t * Fi + f;
        const float* const xc = L.x + (g.divide ? t * Fi : 0) + (k2 < Fi ? k2 : k2 - Fi);
        for (int i = 0; i < N; ++i) v += d[i * TF] * xc[i * g.IN];
        put(img, off.wpre + e, v, first);
      } else {
        const int c = e - n_wpre;
        for (int i = 0; i < N; ++i) v += L.q[i * TF + c];
        put(img, off.bpre + c, v, first);
      }
    }
    __syncthreads();
  }
}

// ---- backward (b): one thread per parameter element, the slabs' images added in slab order in float64 ----------------------------------
__global__ __launch_bounds__(256) void k_dense_layer_final(const DArgs g) {
  const int T = g.T, Fi = g.Fi, Fo = g.Fo;
  const long image = image_floats(T, Fi, Fo, g.A, g.S);
  const Img off = image_offsets(T, Fi, Fo, g.A, g.S);
  const long Kp = (1L + (long)g.A * g.S) * Fi;
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= image) return;
  float* dst = nullptr;
  if (e < off.bpre) { const long per = 2L * Fi * Fi; const int t = (int)(e / per); if (g.g_w_pre[t]) dst = g.g_w_pre[t] + (e - t * per); }
  else if (e < off.wpost) { const long r = e - off.bpre; const int t = (int)(r / Fi); if (g.g_b_pre[t]) dst = g.g_b_pre[t] + (r - (long)t * Fi); }
  else if (e < off.bpost) { const long r = e - off.wpost, per = Fo * Kp; const int t = (int)(r / per); if (g.g_w_post[t]) dst = g.g_w_post[t] + (r - t * per); }
  else if (e < off.wmix) { const long r = e - off.bpost; const int t = (int)(r / Fo); if (g.g_b_post[t]) dst = g.g_b_post[t] + (r - (long)t * Fo); }
  else if (e < off.bmix) { if (g.g_w_mix) dst = g.g_w_mix + (e - off.wmix); }
  else { if (g.g_b_mix) dst = g.g_b_mix + (e - off.bmix); }
  if (!dst) return;
  double acc = 0.0;
  for (int s = 0; s < g.n_slab; ++s) acc += (double)g.part[(long)s * image + e];
  *dst = (float)acc;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
inline long slab_graphs(long B) { return (B + PNA_DENSE_MAX_SLABS - 1) / PNA_DENSE_MAX_SLABS; }

// NULL inside the scope, else the clause that refuses
const char* scope_clause(int64_t B, int N, int T, int Fi, int Fo, int A, int S) {
  if (N < 1 || N > PNA_DENSE_MAX_NODES) return "needs 1 <= N <= 128 nodes per graph";
  if (T < 1 || T > PNA_MAX_TOWER) return "needs 1 <= n_tower <= PNA_MAX_TOWER";
  if (Fi < 1 || (long)T * Fi > kMaxWide) return "needs 1 <= Fi and n_tower Fi <= 64";
  if (Fo < 1 || (long)T * Fo > kMaxWide) return "needs 1 <= Fo and n_tower Fo <= 64";
  if (A < 1 || A > 4) return "needs 1 to 4 distinct aggregators out of mean, max, min, std";
  if (S < 1 || S > 3) return "needs 1 to 3 distinct scalers";
  if (B < 1 || B * N > INT32_MAX) return "needs B >= 1 graphs and B N < 2^31";
  if (layout(N, T, Fi, Fo, A, S).bytes > kLdsBudget) return "the graph does not fit the LDS budget (pna_dense_layer_lds_bytes > 160 KiB)";
  return nullptr;
}

int fill(const pna_dense_layer_args* p, DArgs& g, bool bwd, const char* fn) {
  if (!p) return pna_refuse(fn, "args is NULL");
  if (int rc_ss = pna_check_struct_size(fn, p->struct_size, sizeof(*p))) return rc_ss;
  if (p->n_aggr < 0 || p->n_aggr > PNA_MAX_AGGR || p->n_scaler < 0 || p->n_scaler > PNA_MAX_SCALER)
    return pna_refuse(fn, "needs 1 to 4 distinct aggregators and 1 to 3 distinct scalers");
  if (const char* c = scope_clause(p->B, p->N, p->n_tower, p->Fi, p->Fo, p->n_aggr, p->n_scaler)) return pna_refuse(fn, c);
  memset(&g, 0, sizeof(g));
  g.ia_mean = g.ia_max = g.ia_min = g.ia_std = -1;
  for (int a = 0; a < p->n_aggr; ++a) {
    int* slot = p->aggr[a] == PNA_AGG_MEAN ? &g.ia_mean : p->aggr[a] == PNA_AGG_MAX ? &g.ia_max : p->aggr[a] == PNA_AGG_MIN ? &g.ia_min
              : p->aggr[a] == PNA_AGG_STD ? &g.ia_std : nullptr;
    if (!slot || *slot >= 0) return pna_refuse(fn, "needs 1 to 4 distinct aggregators out of mean, max, min, std");
    *slot = a;
  }
  bool need_log = false, need_lin = false;
  for (int s = 0; s < p->n_scaler; ++s) {
    const int code = p->scaler[s];
    if (code < PNA_DENSE_SCALER_IDENTITY || code > PNA_DENSE_SCALER_INVERSE_LINEAR) return pna_refuse(fn, "unknown scaler code");
    for (int r = 0; r < s; ++r)
      if (p->scaler[r] == code) return pna_refuse(fn, "needs 1 to 3 distinct scalers");
    need_log |= code == PNA_DENSE_SCALER_AMPLIFICATION || code == PNA_DENSE_SCALER_ATTENUATION;
    need_lin |= code == PNA_DENSE_SCALER_LINEAR || code == PNA_DENSE_SCALER_INVERSE_LINEAR;
    g.scaler[s] = code;
  }
  const int T = p->n_tower, Fi = p->Fi;
  if (p->in_dim != (p->divide_input ? T * Fi : Fi)) return pna_refuse(fn, "in_dim must be n_tower Fi (divide_input) or Fi");
  if (!p->x || !p->adj) return pna_refuse(fn, "needs x (B, N, in_dim) and adj (B, N, N)");
  if ((need_log && !p->avg_log) || (need_lin && !p->avg_lin)) return pna_refuse(fn, "the scalers need avg_log / avg_lin (one device float each)");
  for (int t = 0; t < T; ++t)
    if (!p->w_pre[t] || !p->b_pre[t] || !p->w_post[t] || !p->b_post[t]) return pna_refuse(fn, "needs w_pre, b_pre, w_post, b_post of every tower");
  if (!p->w_mix || !p->b_mix) return pna_refuse(fn, "needs w_mix and b_mix");
  g.B = p->B; g.N = p->N; g.IN = p->in_dim; g.T = T; g.Fi = Fi; g.Fo = p->Fo; g.divide = p->divide_input != 0; g.self_loop = p->self_loop != 0;
  g.A = p->n_aggr; g.S = p->n_scaler; g.slope = p->slope;
  g.x = p->x; g.adj = p->adj; g.avg_log = p->avg_log; g.avg_lin = p->avg_lin; g.w_mix = p->w_mix; g.b_mix = p->b_mix;
  for (int t = 0; t < T; ++t) { g.w_pre[t] = p->w_pre[t]; g.b_pre[t] = p->b_pre[t]; g.w_post[t] = p->w_post[t]; g.b_post[t] = p->b_post[t]; }
  g.slab = slab_graphs(g.B);
  g.n_slab = (int)((g.B + g.slab - 1) / g.slab);
  if (!bwd) {
    if (!p->out) return pna_refuse(fn, "needs out (B, N, n_tower Fo)");
    g.out = p->out;
    return PNA_OK;
  }
  if (!p->grad_out) return pna_refuse(fn, "needs grad_out (B, N, n_tower Fo)");
  const int64_t need = pna_dense_layer_workspace_bytes(p->B, p->N, T, Fi, p->Fo, p->n_aggr, p->n_scaler);
  if (!p->workspace || ((uintptr_t)p->workspace & 15) || p->workspace_bytes < need)
    return pna_refuse(fn, "needs a 16-byte aligned workspace of pna_dense_layer_workspace_bytes(...)");
  g.go = p->grad_out; g.gx = p->grad_x; g.g_w_mix = p->grad_w_mix; g.g_b_mix = p->grad_b_mix;
  for (int t = 0; t < T; ++t) {
    g.g_w_pre[t] = p->grad_w_pre[t]; g.g_b_pre[t] = p->grad_b_pre[t]; g.g_w_post[t] = p->grad_w_post[t]; g.g_b_post[t] = p->grad_b_post[t];
  }
  g.part = (float*)p->workspace;
  return PNA_OK;
}

}  // namespace

extern "C" int64_t pna_dense_layer_lds_bytes(int32_t N, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_aggr, int32_t n_scaler) {
  if (N < 1 || N > PNA_DENSE_MAX_NODES || n_tower < 1 || n_tower > PNA_MAX_TOWER || Fi < 1 || (long)n_tower * Fi > kMaxWide || Fo < 1 ||
      (long)n_tower * Fo > kMaxWide || n_aggr < 1 || n_aggr > 4 || n_scaler < 1 || n_scaler > 3)
    return -1;
  return layout(N, n_tower, Fi, Fo, n_aggr, n_scaler).bytes;
}

extern "C" int64_t pna_dense_layer_workspace_bytes(int64_t B, int32_t N, int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_aggr, int32_t n_scaler) {
  if (scope_clause(B, N, n_tower, Fi, Fo, n_aggr, n_scaler)) return -1;
  const int64_t images = B < PNA_DENSE_MAX_SLABS ? B : PNA_DENSE_MAX_SLABS;        // (>= the slabs in use: monotone in B)
  return images * image_floats(n_tower, Fi, Fo, n_aggr, n_scaler) * 4;
}

extern "C" int pna_dense_layer_fwd_f32(const pna_dense_layer_args* p, pna_stream_t stream) {
  DArgs g;
  const int rc = fill(p, g, false, "pna_dense_layer_fwd_f32");
  if (rc != PNA_OK) return rc;
  const size_t lds = (size_t)layout(g.N, g.T, g.Fi, g.Fo, g.A, g.S).bytes;
  if (pna_raise_lds((const void*)k_dense_layer_fwd, lds, "pna_dense_layer_fwd_f32: the LDS size was refused")) return PNA_E_LAUNCH;
  hipLaunchKernelGGL(k_dense_layer_fwd, dim3((unsigned)g.n_slab), dim3(kThreads), lds, (hipStream_t)stream, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_dense_layer_fwd_f32: launch failed");
  return PNA_OK;
}

extern "C" int pna_dense_layer_bwd_f32(const pna_dense_layer_args* p, pna_stream_t stream) {
  DArgs g;
  const int rc = fill(p, g, true, "pna_dense_layer_bwd_f32");
  if (rc != PNA_OK) return rc;
  bool params = g.g_w_mix || g.g_b_mix;
  for (int t = 0; t < g.T; ++t) params = params || g.g_w_pre[t] || g.g_b_pre[t] || g.g_w_post[t] || g.g_b_post[t];
  if (!g.gx && !params) return PNA_OK;
  const size_t lds = (size_t)layout(g.N, g.T, g.Fi, g.Fo, g.A, g.S).bytes;
  if (pna_raise_lds((const void*)k_dense_layer_bwd, lds, "pna_dense_layer_bwd_f32: the LDS size was refused")) return PNA_E_LAUNCH;
  hipLaunchKernelGGL(k_dense_layer_bwd, dim3((unsigned)g.n_slab), dim3(kThreads), lds, (hipStream_t)stream, g);
  if (params) {
    const long n = image_floats(g.T, g.Fi, g.Fo, g.A, g.S);
    hipLaunchKernelGGL(k_dense_layer_final, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g);
  }
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_dense_layer_bwd_f32: launch failed");
  return PNA_OK;
}
