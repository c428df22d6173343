// pna_set2set.hip -- the Set2Set graph readout of the multitask GNN for gfx950, forward and backward as ONE C call each.  Implements
// pna_set2set_{lds_bytes, workspace_bytes, fwd_f32, bwd_f32} of include/pna_amd.h.  Replaces models/layers.py:22-98 (the loop is :81-98)
// as S2SReadout (:271-289) and the GNN (models/pytorch/gnn_framework.py:83,108) use it, with what autograd derives from it.
//
//   h = c = 0 (D), q* = 0 (2D); `steps` times:
//     z = W_ih q* + W_hh h + (b_ih + b_hh)          (4D, gate order i, f, g, o)
//     c = sigmoid(z_f) c + sigmoid(z_i) tanh(z_g);   h = sigmoid(z_o) tanh(c);   q = h
//     e_n = x_n . q;   a = softmax_n(e) (max subtracted);   r = sum_n a_n x_n;   q* = [q | r]
//   out_b = q*
//
// A workgroup owns a slab of consecutive graphs, one graph at a time: both weight matrices (odd row pitches: a thread per row reads without
// bank conflicts), the bias sum and the graph's rows sit in LDS and the step loop runs inside the kernel with workgroup barriers only.
// Exact fp32 on the vector ALU (the build's -ffp-contract=off): a 4D x 3D matrix-vector product has nothing for the matrix pipe.  Every sum
// has a fixed order -- a product row's k ascending, the nodes ascending, the softmax reductions a butterfly inside a wavefront and then the
// two wavefronts in order -- so results are bitwise repeatable.
// Backward: (a) the same workgroups rebuild each graph's forward with set2set_graph_fwd (the forward kernel's function), which records per
// step [activated gates 4D | c D | q* 2D | a N] in the slab's own region of the workspace, then walk the steps in reverse; grad_x accumulates
// in LDS and is written once per graph; grad W_ih, grad W_hh and one bias gradient accumulate in LDS over the slab's graphs and leave as the
// slab's image;  (b) the images added in slab order in float64 (pna_dense_layer.hip's scheme).  No atomics of any kind.
// No kernel waits for another workgroup; every loop bound comes from the arguments.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "pna_amd.h"
#include "pna_internal.h"

namespace {

constexpr int kThreads = 256;       // 4 wavefronts; the rows of z (<= 128) and the nodes (<= 128) take the first two
constexpr int kRedThreads = 128;    // the threads (whole wavefronts 0 and 1) that take part in a reduction over the nodes
constexpr long kLdsBudget = 160 * 1024;

static_assert(4 * PNA_S2S_MAX_WIDTH <= kRedThreads && PNA_S2S_MAX_NODES <= kRedThreads, "a thread per gate row and per node");
static_assert(kRedThreads + 2 * PNA_S2S_MAX_WIDTH <= kThreads, "the threads that stage q*_(t-1) sit behind the reduction's");

struct SArgs {
  long B;
  int N, D, T;
  const float* x; const float* wih; const float* whh; const float* bih; const float* bhh;
  float* out;
  const float* go;
  float* gx; float* gwih; float* gwhh; float* gbih; float* gbhh;
  float* part;             // [n_image][12 D^2 + 4D]: grad W_ih | grad W_hh | grad b of one slab
  float* rec;              // [n_image][T][7D + N]: the steps of the graph a slab is working on
  long slab;
  int n_slab;
};

// offsets in floats; the forward kernel allocates [0, fwd_end), the backward [0, end)
struct Lay {
  int PI, PH;              // row pitches of W_ih (2D | 1) and of W_hh and x (D | 1)
  int wih, whh, bs, x, act, c, qs, a, red, fwd_end;
  int gwih, gwhh, gb, gx, dz, dqs, dhc, de, qb, end;
};

__host__ __device__ inline Lay layout(int N, int D) {
  Lay L;
  L.PI = (2 * D) | 1; L.PH = D | 1;
  int o = 0;
  L.wih = o; o += 4 * D * L.PI;
  L.whh = o; o += 4 * D * L.PH;
  L.bs = o; o += 4 * D;
  L.x = o; o += N * L.PH;
  L.act = o; o += 4 * D;
  L.c = o; o += D;
  L.qs = o; o += 2 * D;
  L.a = o; o += N;
  L.red = o; o += 4;
  L.fwd_end = o;
  L.gwih = o; o += 8 * D * D;
  L.gwhh = o; o += 4 * D * D;
  L.gb = o; o += 4 * D;
  L.gx = o; o += N * D;
  L.dz = o; o += 4 * D;
  L.dqs = o; o += 2 * D;
  L.dhc = o; o += D;
  L.de = o; o += N;
  L.qb = o; o += 4 * D;
  L.end = o;
  return L;
}

inline long round16(long b) { return (b + 15) / 16 * 16; }
__host__ __device__ inline long image_floats(int D) { return 12L * D * D + 4 * D; }
__host__ __device__ inline long record_floats(int N, int D) { return 7L * D + N; }

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }

// ---- the gates: pna_gru.hip's forms, neither overflow nor cancellation; exp / expm1 are the full-precision library functions -------------
__device__ __forceinline__ float sigmoid_stable(float a) {
  if (a >= 0.f) return 1.f / (1.f + expf(-a));
  const float e = expf(a);
  return e / (1.f + e);
}

__device__ __forceinline__ float tanh_stable(float a) {
  const float m = expm1f(-2.f * fabsf(a));                // in [-1, 0]: -1 exactly when saturated
  const float t = -m / (m + 2.f);
  return a < 0.f ? -t : t;
}

// butterflies over the 64 lanes of a wavefront: every lane ends with the same bits (a + b == b + a), in an order the lane count fixes
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// both matrices to their pitched rows and the bias sum, once per workgroup: read as the optimiser left them
__device__ void load_weights(const SArgs& g, const Lay& L, float* lds) {
  const int tid = threadIdx.x, D = g.D;
  for (int i = tid; i < 8 * D * D; i += kThreads) {
    const int j = i / (2 * D), k = i - j * 2 * D;
    lds[L.wih + j * L.PI + k] = g.wih[i];
  }
  for (int i = tid; i < 4 * D * D; i += kThreads) {
    const int j = i / D, k = i - j * D;
    lds[L.whh + j * L.PH + k] = g.whh[i];
  }
  for (int i = tid; i < 4 * D; i += kThreads) lds[L.bs + i] = g.bih[i] + g.bhh[i];
}

__device__ void load_graph(const SArgs& g, const Lay& L, float* lds, long b) {
  const int tid = threadIdx.x, N = g.N, D = g.D;
  const float* const xb = g.x + b * N * D;
  for (int i = tid; i < N * D; i += kThreads) {
    const int n = i / D, d = i - n * D;
    lds[L.x + n * L.PH + d] = xb[i];
  }
}

// The forward of the graph whose rows are in LDS: q*_T is left in lds[L.qs, + 2D).  rec != NULL: step t's [act 4D | c D | q* 2D | a N] is
// written to rec + t (7D + N).  Begins and ends with a barrier of its own, so the caller may load before and read after without one.
__device__ void set2set_graph_fwd(const SArgs& g, const Lay& L, float* lds, float* rec) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = g.N, D = g.D;
  const long R = record_floats(N, D);
  float* const act = lds + L.act;
  float* const c = lds + L.c;
  float* const qs = lds + L.qs;
  float* const a = lds + L.a;
  float* const red = lds + L.red;
  if (tid < D) c[tid] = 0.f;
  if (tid < 2 * D) qs[tid] = 0.f;
  __syncthreads();
  for (int t = 0; t < g.T; ++t) {
    float* const rt = rec ? rec + t * R : nullptr;
    if (tid < 4 * D) {                                               // a gate row each: k ascending, W_ih's columns, then W_hh's
      const float* const wi = lds + L.wih + tid * L.PI;
      const float* const wh = lds + L.whh + tid * L.PH;
      float z = lds[L.bs + tid];
      for (int k = 0; k < 2 * D; ++k) z += wi[k] * qs[k];
      for (int k = 0; k < D; ++k) z += wh[k] * qs[k];                // h = q = q*[0, D)
      const float v = (tid >= 2 * D && tid < 3 * D) ? tanh_stable(z) : sigmoid_stable(z);
      act[tid] = v;
      if (rt) rt[tid] = v;
    }
    __syncthreads();
    if (tid < D) {
      const float cc = act[D + tid] * c[tid] + act[tid] * act[2 * D + tid];
      const float h = act[3 * D + tid] * tanh_stable(cc);
      c[tid] = cc;
      qs[tid] = h;
      if (rt) { rt[4 * D + tid] = cc; rt[5 * D + tid] = h; }
    }
    __syncthreads();
    float e = -INFINITY, p = 0.f;
    if (tid < kRedThreads) {                                         // (whole wavefronts: the shuffles see every lane)
      if (tid < N) {
        const float* const xr = lds + L.x + tid * L.PH;
        e = 0.f;
        for (int d = 0; d < D; ++d) e += xr[d] * qs[d];
      }
      const float m = wave_max(e);
      if (lane == 0) red[wave] = m;
    }
    __syncthreads();
    if (tid < kRedThreads) {
      const float m = fmaxf(red[0], red[1]);
      if (tid < N) p = expf(e - m);                                   // <= 1; the maximum's own is exactly 1
      const float s = wave_sum(p);
      if (lane == 0) red[2 + wave] = s;
    }
    __syncthreads();
    if (tid < N) {
      const float av = p / (red[2] + red[3]);
      a[tid] = av;
      if (rt) rt[7 * D + tid] = av;
    }
    __syncthreads();
    if (tid < D) {
      const float* const xc = lds + L.x + tid;
      float r = 0.f;
      for (int n = 0; n < N; ++n) r += a[n] * xc[n * L.PH];
      qs[D + tid] = r;
      if (rt) rt[6 * D + tid] = r;
    }
    __syncthreads();
  }
}

// ---- forward: one launch ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_set2set_fwd(const SArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lay L = layout(g.N, g.D);
  const int tid = threadIdx.x, D = g.D;
  const long b0 = (long)blockIdx.x * g.slab, b1 = lmin(g.B, b0 + g.slab);
  load_weights(g, L, lds);
  for (long b = b0; b < b1; ++b) {
    load_graph(g, L, lds, b);
    set2set_graph_fwd(g, L, lds, nullptr);
    if (tid < 2 * D) g.out[b * 2 * D + tid] = lds[L.qs + tid];
    __syncthreads();                                                 // q* is read before the next graph clears it
  }
}

// ---- backward (a): the slab's graphs, forward rebuilt, steps in reverse ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_set2set_bwd(const SArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lay L = layout(g.N, g.D);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = g.N, D = g.D, T = g.T;
  const long R = record_floats(N, D), image = image_floats(D);
  const long b0 = (long)blockIdx.x * g.slab, b1 = lmin(g.B, b0 + g.slab);
  float* const rec = g.rec + (long)blockIdx.x * T * R;
  float* const a = lds + L.a;
  float* const red = lds + L.red;
  float* const gwih = lds + L.gwih;
  float* const gwhh = lds + L.gwhh;
  float* const gb = lds + L.gb;
  float* const gx = lds + L.gx;
  float* const dz = lds + L.dz;
  float* const dqs = lds + L.dqs;
  float* const dhc = lds + L.dhc;
  float* const de = lds + L.de;
  const bool params = g.gwih || g.gwhh || g.gbih || g.gbhh;
  load_weights(g, L, lds);
  for (int i = tid; i < 12 * D * D + 4 * D; i += kThreads) gwih[i] = 0.f;      // gwih | gwhh | gb are adjacent
  for (long b = b0; b < b1; ++b) {
    load_graph(g, L, lds, b);
    set2set_graph_fwd(g, L, lds, rec);                               // (its last barrier also orders the records before the reads below)
    for (int i = tid; i < N * D; i += kThreads) gx[i] = 0.f;
    if (tid < 2 * D) {
      dqs[tid] = g.go[b * 2 * D + tid];
      lds[L.qb + ((T - 1) & 1) * 2 * D + tid] = rec[(long)(T - 1) * R + 5 * D + tid];
    }
    if (tid < D) dhc[tid] = 0.f;
    float dcc = 0.f;                                                 // thread d < D: the gradient of c_t carried into step t - 1
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
      const float* const rt = rec + (long)t * R;
      const float* const rp = t > 0 ? rt - R : rt;                   // (read only where t > 0)
      const float* const cur = lds + L.qb + (t & 1) * 2 * D;         // q*_t
      float* const prv = lds + L.qb + ((t + 1) & 1) * 2 * D;         // q*_(t-1)
      // r = sum_n a_n x_n: da_n = dr . x_n; the softmax's sum_m a_m da_m
      float av = 0.f, da = 0.f;
      if (tid < kRedThreads) {
        if (tid < N) {
          const float* const xr = lds + L.x + tid * L.PH;
          av = rt[7 * D + tid];
          for (int d = 0; d < D; ++d) da += dqs[D + d] * xr[d];
          a[tid] = av;
        }
        const float s = wave_sum(av * da);
        if (lane == 0) red[wave] = s;
      } else if (tid < kRedThreads + 2 * D) {
        const int k = tid - kRedThreads;
        prv[k] = t > 0 ? rp[5 * D + k] : 0.f;
      }
      float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f, ct = 0.f, cp = 0.f;
      if (tid < D) {
        gi = rt[tid]; gf = rt[D + tid]; gg = rt[2 * D + tid]; go = rt[3 * D + tid]; ct = rt[4 * D + tid];
        cp = t > 0 ? rp[4 * D + tid] : 0.f;
      }
      __syncthreads();
      if (tid < N) de[tid] = av * (da - (red[0] + red[1]));
      __syncthreads();
      // e_n = x_n . q and r: grad_x_n += a_n dr + de_n q
      for (int i = tid; i < N * D; i += kThreads) {
        const int n = i / D, d = i - n * D;
        gx[i] += a[n] * dqs[D + d] + de[n] * cur[d];
      }
      if (tid < D) {                                                 // dq, then the LSTM cell
        const float* const xc = lds + L.x + tid;
        float dq = 0.f;
        for (int n = 0; n < N; ++n) dq += de[n] * xc[n * L.PH];
        const float dh = (dqs[tid] + dq) + dhc[tid];
        const float tc = tanh_stable(ct);
        const float dc = dh * go * ((1.f - tc) * (1.f + tc)) + dcc;
        dz[tid] = (dc * gg) * (gi * (1.f - gi));
        dz[D + tid] = (dc * cp) * (gf * (1.f - gf));
        dz[2 * D + tid] = (dc * gi) * ((1.f - gg) * (1.f + gg));
        dz[3 * D + tid] = (dh * tc) * (go * (1.f - go));
        dcc = dc * gf;
      }
      __syncthreads();
      if (tid < 4 * D) gb[tid] += dz[tid];
      if (t > 0) {                                                   // (step 0 starts from zeros: no product, nothing to pass on)
        if (params) {
          for (int i = tid; i < 8 * D * D; i += kThreads) {
            const int j = i / (2 * D), k = i - j * 2 * D;
            gwih[i] += dz[j] * prv[k];
          }
          for (int i = tid; i < 4 * D * D; i += kThreads) {
            const int j = i / D, k = i - j * D;
            gwhh[i] += dz[j] * prv[k];                               // h_(t-1) = q*_(t-1)[0, D)
          }
        }
        if (tid < 2 * D) {                                           // W_ih^T dz -> the gradient of q*_(t-1)
          const float* const w = lds + L.wih + tid;
          float s = 0.f;
          for (int j = 0; j < 4 * D; ++j) s += w[j * L.PI] * dz[j];
          dqs[tid] = s;
        } else if (tid < 3 * D) {                                    // W_hh^T dz -> the gradient of h_(t-1)
          const float* const w = lds + L.whh + (tid - 2 * D);
          float s = 0.f;
          for (int j = 0; j < 4 * D; ++j) s += w[j * L.PH] * dz[j];
          dhc[tid - 2 * D] = s;
        }
      }
      __syncthreads();
    }
    if (g.gx) {
      float* const gxb = g.gx + b * N * D;
      for (int i = tid; i < N * D; i += kThreads) gxb[i] = gx[i];
    }
    __syncthreads();
  }
  if (params) {
    float* const img = g.part + (long)blockIdx.x * image;
    for (int i = tid; i < image; i += kThreads) img[i] = gwih[i];
  }
}

// ---- backward (b): one thread per parameter element, the slabs' images added in slab order in float64 ----------------------------------
__global__ __launch_bounds__(256) void k_set2set_final(const SArgs g) {
  const int D = g.D;
  const long image = image_floats(D), n_ih = 8L * D * D, n_hh = 4L * D * D;
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= image) return;
  float* d0 = nullptr;
  float* d1 = nullptr;
  if (e < n_ih) { if (g.gwih) d0 = g.gwih + e; }
  else if (e < n_ih + n_hh) { if (g.gwhh) d0 = g.gwhh + (e - n_ih); }
  else { if (g.gbih) d0 = g.gbih + (e - n_ih - n_hh); if (g.gbhh) d1 = g.gbhh + (e - n_ih - n_hh); }
  if (!d0 && !d1) return;
  double acc = 0.0;
  for (int s = 0; s < g.n_slab; ++s) acc += (double)g.part[(long)s * image + e];
  if (d0) *d0 = (float)acc;
  if (d1) *d1 = (float)acc;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
inline long slab_graphs(long B) { return (B + PNA_S2S_MAX_SLABS - 1) / PNA_S2S_MAX_SLABS; }

const char* shape_clause(int N, int D) {
  if (D < 1 || D > PNA_S2S_MAX_WIDTH) return "needs 1 <= D <= 32 columns (PNA_S2S_MAX_WIDTH)";
  if (N < 1 || N > PNA_S2S_MAX_NODES) return "needs 1 <= N <= 128 nodes per graph (PNA_S2S_MAX_NODES)";
  return nullptr;
}

// NULL inside the scope, else the clause that refuses
const char* scope_clause(int64_t B, int N, int D, int steps) {
  if (const char* c = shape_clause(N, D)) return c;
  if (steps < 1 || steps > PNA_S2S_MAX_STEPS) return "needs 1 <= steps <= 128 (PNA_S2S_MAX_STEPS)";
  if (B < 1 || B * N > INT32_MAX) return "needs B >= 1 graphs and B N < 2^31";
  if (round16(4L * layout(N, D).end) > kLdsBudget) return "the graph does not fit the LDS budget (pna_set2set_lds_bytes > 160 KiB)";
  return nullptr;
}

int fill(const pna_set2set_args* p, SArgs& g, bool bwd, const char* fn) {
  if (!p) return pna_refuse(fn, "args is NULL");
  if (int rc_ss = pna_check_struct_size(fn, p->struct_size, sizeof(*p))) return rc_ss;
  if (p->dtype != PNA_S2S_F32) return pna_refuse(fn, "fp32 only (dtype must be PNA_S2S_F32)");
  if (const char* c = scope_clause(p->B, p->N, p->D, p->steps)) return pna_refuse(fn, c);
  if (!p->x) return pna_refuse(fn, "needs x (B, N, D)");
  if (!p->w_ih || !p->w_hh) return pna_refuse(fn, "needs w_ih (4D, 2D) and w_hh (4D, D)");
  if (!p->b_ih || !p->b_hh) return pna_refuse(fn, "needs b_ih and b_hh [4D] (bias=True)");
  memset(&g, 0, sizeof(g));
  g.B = p->B; g.N = p->N; g.D = p->D; g.T = p->steps;
  g.x = p->x; g.wih = p->w_ih; g.whh = p->w_hh; g.bih = p->b_ih; g.bhh = p->b_hh;
  g.slab = slab_graphs(g.B);
  g.n_slab = (int)((g.B + g.slab - 1) / g.slab);
  if (!bwd) {
    if (!p->out) return pna_refuse(fn, "needs out (B, 2D)");
    g.out = p->out;
    return PNA_OK;
  }
  if (!p->grad_out) return pna_refuse(fn, "needs grad_out (B, 2D)");
  const int64_t need = pna_set2set_workspace_bytes(p->B, p->N, p->D, p->steps);
  if (!p->workspace || ((uintptr_t)p->workspace & 15) || p->workspace_bytes < need)
    return pna_refuse(fn, "needs a 16-byte aligned workspace of pna_set2set_workspace_bytes(B, N, D, steps)");
  g.go = p->grad_out; g.gx = p->grad_x;
  g.gwih = p->grad_w_ih; g.gwhh = p->grad_w_hh; g.gbih = p->grad_b_ih; g.gbhh = p->grad_b_hh;
  const long images = g.B < PNA_S2S_MAX_SLABS ? g.B : PNA_S2S_MAX_SLABS;
  g.part = (float*)p->workspace;
  g.rec = g.part + images * image_floats(g.D);
  return PNA_OK;
}

}  // namespace

extern "C" int64_t pna_set2set_lds_bytes(int32_t N, int32_t D) {
  if (shape_clause(N, D)) return -1;
  return round16(4L * layout(N, D).end);
}

extern "C" int64_t pna_set2set_workspace_bytes(int64_t B, int32_t N, int32_t D, int32_t steps) {
  if (scope_clause(B, N, D, steps)) return -1;
  const int64_t images = B < PNA_S2S_MAX_SLABS ? B : PNA_S2S_MAX_SLABS;           // (>= the slabs in use: monotone in B)
  return images * (image_floats(D) + steps * record_floats(N, D)) * 4;
}

extern "C" int pna_set2set_fwd_f32(const pna_set2set_args* p, pna_stream_t stream) {
  SArgs g;
  const int rc = fill(p, g, false, "pna_set2set_fwd_f32");
  if (rc != PNA_OK) return rc;
  const size_t lds = (size_t)round16(4L * layout(g.N, g.D).fwd_end);
  if (pna_raise_lds((const void*)k_set2set_fwd, lds, "pna_set2set_fwd_f32: the LDS size was refused")) return PNA_E_LAUNCH;
  hipLaunchKernelGGL(k_set2set_fwd, dim3((unsigned)g.n_slab), dim3(kThreads), lds, (hipStream_t)stream, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_set2set_fwd_f32: launch failed");
  return PNA_OK;
}

extern "C" int pna_set2set_bwd_f32(const pna_set2set_args* p, pna_stream_t stream) {
  SArgs g;
  const int rc = fill(p, g, true, "pna_set2set_bwd_f32");
  if (rc != PNA_OK) return rc;
  const bool params = g.gwih || g.gwhh || g.gbih || g.gbhh;
  if (!g.gx && !params) return PNA_OK;
  const size_t lds = (size_t)round16(4L * layout(g.N, g.D).end);
  if (pna_raise_lds((const void*)k_set2set_bwd, lds, "pna_set2set_bwd_f32: the LDS size was refused")) return PNA_E_LAUNCH;
  hipLaunchKernelGGL(k_set2set_bwd, dim3((unsigned)g.n_slab), dim3(kThreads), lds, (hipStream_t)stream, g);
  if (params) {
    const long n = image_floats(g.D);
    hipLaunchKernelGGL(k_set2set_final, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g);
  }
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_set2set_bwd_f32: launch failed");
  return PNA_OK;
}
