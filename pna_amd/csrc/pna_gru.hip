// pna_gru.hip -- the GRU update between two message-passing steps for gfx950: torch.nn.GRU with one layer, one direction, bias, over a
// sequence of length 1 (a GRU CELL over rows), forward and backward as ONE C call each.  Implements pna_gru_cell_{workspace_bytes,
// fwd_f32, bwd_f32} of include/pna_amd.h.  Replaces realworld_benchmark/nets/gru.py:5-30 (PNANet / PNANetSuperpixels, gru=True) and
// models/layers.py:237-268 (the multitask GNN's shared GRU, models/pytorch/gnn_framework.py:60,95) with what autograd derives from them.
//
//   gi = x W_ih^T + b_ih        gh = h W_hh^T + b_hh                (gate order in the 3H weight rows: r, z, n)
//   r = sigmoid(gi_r + gh_r)    z = sigmoid(gi_z + gh_z)    n = tanh(gi_n + r gh_n)    out = (1 - z) n + z h
//
// x is (V, I <= input_size) and h is (V, Hc <= hidden_size): the missing columns are the reference's zero padding (layers.py:260-264),
// never materialised -- the K loops end at I / Hc and the z h term is 0 past Hc.
//
// Forward: one launch.  A workgroup owns 16 rows (the M of one v_mfma_f32_16x16x4_f32 tile, as the sibling one-call kernels); the x and h
// tiles sit in LDS zero-filled to the K pitch; wavefront nt owns hidden columns [16 nt, 16 nt + 16) and keeps the r, z, gi_n and gh_n
// accumulators (gi_n and gh_n apart: r multiplies gh_n only); B fragments are read straight from the nn.GRU parameters.
// Backward: (a) a rows kernel over the same tiles: da_r, da_z, da_n from grad_out and the saved r, z, n, gh_n; grad_x = dgi W_ih and
// grad_h = dgh W_hh + grad_out z on the MFMA; dgi / dgh stored once as (V, 4H) [da_r | da_z | da_n | da_n r];  (b) weight and bias
// gradients per slab of consecutive rows on the MFMA (grad_W_ih = dgi^T x, grad_W_hh = dgh^T h, the bias sums as a ones column);
// (c) the slabs added in slab order in float64 (pna_net_ends.hip's scheme).  No atomics of any kind: bitwise repeatable.
// No kernel waits for another workgroup; every loop bound comes from the arguments.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_train_dev.h"

namespace {

using namespace pna_train;      // f4, kRows, quads, pitch_of, quad_fma

constexpr int kThreads = 512;   // rows kernels: 8 wavefronts, one per 16-column tile of the widest hidden size
constexpr int kWaves = kThreads / 64;
constexpr int kMaxWidth = 128;
constexpr int kDwThreads = 256; // weight-gradient kernel: 4 wavefronts share the (matrix, column tile) jobs of one 16-row band of 3H

struct GArgs {
  long V;
  int I, Hc, IN, H;
  const float* x; long ldx;
  const float* h; long ldh;
  const float* wih; long ldwi;
  const float* whh; long ldwh;
  const float* bih; const float* bhh;
  float* out; long ldo;
  float* saved;            // (4, V, H): r | z | n | gh_n
  const float* go; long ldgo;
  float* gx; long ldgx;
  float* gh; long ldgh;
  float* gwih; float* gwhh; float* gbih; float* gbhh;
  int need_x, need_h, need_wih, need_whh, need_bih, need_bhh;
  float* dg;               // (V, 4H): da_r | da_z | da_n | da_n r
  float* part;             // [n_slab][3H (I + Hc + 2)]: grad_W_ih | grad_W_hh | grad_b_ih | grad_b_hh of one slab
  long slab;
  int n_slab;
};

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }

// ---- the gates: forms that neither overflow nor cancel; exp / expm1 are the full-precision library functions ----------------------
__device__ __forceinline__ float sigmoid_stable(float a) {
  if (a >= 0.f) return 1.f / (1.f + expf(-a));            // exp of a non-positive number: in (0, 1]
  const float e = expf(a);                                // (NaN takes this branch and stays NaN)
  return e / (1.f + e);
}

__device__ __forceinline__ float tanh_stable(float a) {
  const float m = expm1f(-2.f * fabsf(a));                // in [-1, 0]: no cancellation near 0, -1 exactly when saturated
  const float t = -m / (m + 2.f);
  return a < 0.f ? -t : t;
}

// The gate epilogue of one element, apart from the projections (an LSTM epilogue would take the same four pre-activations' place).
struct GruGates { float r, z, n, ghn, out; };
__device__ __forceinline__ GruGates gru_gates(float a_r, float a_z, float gi_n, float gh_n, float hprev) {
  GruGates q;
  q.r = sigmoid_stable(a_r);
  q.z = sigmoid_stable(a_z);
  q.ghn = gh_n;
  q.n = tanh_stable(gi_n + q.r * gh_n);
  q.out = (1.f - q.z) * q.n + q.z * hprev;
  return q;
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

// ---- forward: one launch -----------------------------------------------------------------------------------------------------------
// lds: X [16][PI] | Hh [16][PH]
__global__ __launch_bounds__(kThreads) void k_gru_rows_fwd(const GArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int I = g.I, Hc = g.Hc, H = g.H;
  const int QI = quads(I), QH = quads(Hc), PI = pitch_of(QI), PH = pitch_of(QH), NT = (H + 15) / 16;
  float* const X = lds;
  float* const Hh = X + kRows * PI;
  const long r0 = (long)blockIdx.x * kRows;
  const int nrows = (int)lmin(kRows, g.V - r0);
  // zeros in the K padding columns and in the rows past the matrix's end (they multiply weights)
  for (int i = tid; i < kRows * PI; i += kThreads) {
    const int r = i / PI, k = i - r * PI;
    X[i] = (r < nrows && k < I) ? g.x[(r0 + r) * g.ldx + k] : 0.f;
  }
  for (int i = tid; i < kRows * PH; i += kThreads) {
    const int r = i / PH, k = i - r * PH;
    Hh[i] = (r < nrows && k < Hc) ? g.h[(r0 + r) * g.ldh + k] : 0.f;
  }
  __syncthreads();
  const long plane = g.V * H;
  for (int nt = wave; nt < NT; nt += kWaves) {
    const int n = nt * 16 + li;
    const bool nok = n < H;
    const int nc = min(n, H - 1);
    f4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, gin = ar, ghn = ar;
    const float* const wi = g.wih + (long)nc * g.ldwi;
    const float* const wh = g.whh + (long)nc * g.ldwh;
    const long gi_step = (long)H * g.ldwi, gh_step = (long)H * g.ldwh;      // one gate's rows
    for (int qd = 0; qd < QI; ++qd) {
      const int k = 16 * qd + 4 * lg;
      const f4 a = *reinterpret_cast<const f4*>(X + li * PI + k);
      quad_fma(ar, a, wfrag_row(wi, k, I, nok));
      quad_fma(az, a, wfrag_row(wi + gi_step, k, I, nok));
      quad_fma(gin, a, wfrag_row(wi + 2 * gi_step, k, I, nok));
    }
    for (int qd = 0; qd < QH; ++qd) {
      const int k = 16 * qd + 4 * lg;
      const f4 a = *reinterpret_cast<const f4*>(Hh + li * PH + k);
      quad_fma(ar, a, wfrag_row(wh, k, Hc, nok));
      quad_fma(az, a, wfrag_row(wh + gh_step, k, Hc, nok));
      quad_fma(ghn, a, wfrag_row(wh + 2 * gh_step, k, Hc, nok));
    }
    const float br = g.bih[nc] + g.bhh[nc], bz = g.bih[H + nc] + g.bhh[H + nc], bin = g.bih[2 * H + nc], bhn = g.bhh[2 * H + nc];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * lg + i;
      if (!(nok && r < nrows)) continue;
      const float hprev = n < Hc ? Hh[r * PH + n] : 0.f;
      const GruGates q = gru_gates(ar[i] + br, az[i] + bz, gin[i] + bin, ghn[i] + bhn, hprev);
      g.out[(r0 + r) * g.ldo + n] = q.out;
      if (g.saved) {
        float* const sv = g.saved + (r0 + r) * H + n;
        sv[0] = q.r; sv[plane] = q.z; sv[2 * plane] = q.n; sv[3 * plane] = q.ghn;
      }
    }
  }
}

// ---- backward (a): the rows kernel ----------------------------------------------------------------------------------------------
// lds: D [4][16][PD]: da_r | da_z | da_n | da_n r of the tile's rows, zero past H and past the matrix's end
__global__ __launch_bounds__(kThreads) void k_gru_rows_bwd(const GArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int I = g.I, Hc = g.Hc, H = g.H;
  const int QD = quads(H), PD = pitch_of(QD), DP = kRows * PD;
  float* const D = lds;
  const long r0 = (long)blockIdx.x * kRows;
  const int nrows = (int)lmin(kRows, g.V - r0);
  const long plane = g.V * H;
  const bool keep = g.need_wih || g.need_whh || g.need_bih || g.need_bhh;
  for (int i = tid; i < DP; i += kThreads) {
    const int r = i / PD, n = i - r * PD;
    float d_r = 0.f, d_z = 0.f, d_n = 0.f, d_nr = 0.f;
    if (r < nrows && n < H) {
      const long row = r0 + r;
      const float* const sv = g.saved + row * H + n;
      const float rr = sv[0], zz = sv[plane], nn = sv[2 * plane], ghn = sv[3 * plane];
      const float go = g.go[row * g.ldgo + n];
      const float hprev = n < Hc ? g.h[row * g.ldh + n] : 0.f;
      d_n = (go * (1.f - zz)) * ((1.f - nn) * (1.f + nn));          // tanh' = (1 - n)(1 + n)
      d_z = (go * (hprev - nn)) * (zz * (1.f - zz));
      d_r = (d_n * ghn) * (rr * (1.f - rr));
      d_nr = d_n * rr;
      if (keep) {
        float* const dst = g.dg + row * 4 * H + n;
        dst[0] = d_r; dst[H] = d_z; dst[2 * H] = d_n; dst[3 * H] = d_nr;
      }
    }
    D[i] = d_r; D[DP + i] = d_z; D[2 * DP + i] = d_n; D[3 * DP + i] = d_nr;
  }
  __syncthreads();
  // jobs: the 16-column tiles of grad_x (first I columns) and of grad_h (first Hc columns); K = the 3H gate rows
  const int jx = g.need_x ? (I + 15) / 16 : 0, jh = g.need_h ? (Hc + 15) / 16 : 0;
  for (int job = wave; job < jx + jh; job += kWaves) {
    const bool isx = job < jx;
    const int ct = isx ? job : job - jx, C = isx ? I : Hc;
    const int c = ct * 16 + li;
    const bool cok = c < C;
    const int cc = min(c, C - 1);
    const float* const W = (isx ? g.wih : g.whh) + cc;
    const long ld = isx ? g.ldwi : g.ldwh;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int gate = 0; gate < 3; ++gate) {
      const float* const Dp = D + ((gate == 2 && !isx) ? 3 : gate) * DP + li * PD;
      const float* const Wg = W + (long)gate * H * ld;
      for (int qd = 0; qd < QD; ++qd) {
        const int k = 16 * qd + 4 * lg;
        const f4 a = *reinterpret_cast<const f4*>(Dp + k);
        f4 b;                                                      // B[k][c] = W[gate H + k][c]: the lanes of a group read one row
        b.x = (cok && k + 0 < H) ? Wg[(long)min(k + 0, H - 1) * ld] : 0.f;
        b.y = (cok && k + 1 < H) ? Wg[(long)min(k + 1, H - 1) * ld] : 0.f;
        b.z = (cok && k + 2 < H) ? Wg[(long)min(k + 2, H - 1) * ld] : 0.f;
        b.w = (cok && k + 3 < H) ? Wg[(long)min(k + 3, H - 1) * ld] : 0.f;
        quad_fma(acc, a, b);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * lg + i;
      if (!(cok && r < nrows)) continue;
      const long row = r0 + r;
      if (isx) g.gx[row * g.ldgx + c] = acc[i];
      else g.gh[row * g.ldgh + c] = acc[i] + g.go[row * g.ldgo + c] * g.saved[plane + row * H + c];
    }
  }
}

// ---- backward (b): one slab's weight and bias gradients --------------------------------------------------------------------------
// grid (n_slab, ceil(3H / 16)): the workgroup owns gate rows [16 jt, 16 jt + 16) of both matrices over the slab's rows; a wavefront takes
// (matrix, 16-column tile) jobs.  A[j][v] = dgi / dgh [v][j], B[v][c] = x / h [v][c], both straight from memory (the lanes of a group read
// one row); the rows of a slab in order, 16 per step.  The job of column tile 0 also sums the band's bias gradient (B = 1).
__global__ __launch_bounds__(kDwThreads) void k_gru_dw_slab(const GArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int I = g.I, Hc = g.Hc, H = g.H, J = 3 * H;
  const long v0 = (long)blockIdx.x * g.slab;
  const long v1 = lmin(g.V, v0 + g.slab);
  const int jt = blockIdx.y;
  const int ja = jt * 16 + li;                                     // the gate row this lane feeds as A
  const bool jok = ja < J;
  const int jc = min(ja, J - 1);
  const bool on_i = g.need_wih || g.need_bih, on_h = g.need_whh || g.need_bhh;
  const int ni = on_i ? (I + 15) / 16 : 0, nh = on_h ? (Hc + 15) / 16 : 0;
  float* const part = g.part + (long)blockIdx.x * J * (I + Hc + 2);
  for (int job = wave; job < ni + nh; job += kDwThreads / 64) {
    const bool isx = job < ni;
    const int ct = isx ? job : job - ni, C = isx ? I : Hc;
    const int c = ct * 16 + li;
    const bool cok = c < C;
    const float* const src = (isx ? g.x : g.h) + min(c, C - 1);
    const long ld = isx ? g.ldx : g.ldh;
    const float* const dcol = g.dg + ((!isx && jc >= 2 * H) ? jc + H : jc);
    f4 acc = {0.f, 0.f, 0.f, 0.f}, accb = acc;
    const f4 ones = {1.f, 1.f, 1.f, 1.f};
    for (long vb = v0; vb < v1; vb += 16) {
      const long v = vb + 4 * lg;
      f4 a, b;
      a.x = (jok && v + 0 < v1) ? dcol[lmin(v + 0, v1 - 1) * 4 * H] : 0.f;
      a.y = (jok && v + 1 < v1) ? dcol[lmin(v + 1, v1 - 1) * 4 * H] : 0.f;
      a.z = (jok && v + 2 < v1) ? dcol[lmin(v + 2, v1 - 1) * 4 * H] : 0.f;
      a.w = (jok && v + 3 < v1) ? dcol[lmin(v + 3, v1 - 1) * 4 * H] : 0.f;
      b.x = (cok && v + 0 < v1) ? src[lmin(v + 0, v1 - 1) * ld] : 0.f;
      b.y = (cok && v + 1 < v1) ? src[lmin(v + 1, v1 - 1) * ld] : 0.f;
      b.z = (cok && v + 2 < v1) ? src[lmin(v + 2, v1 - 1) * ld] : 0.f;
      b.w = (cok && v + 3 < v1) ? src[lmin(v + 3, v1 - 1) * ld] : 0.f;
      quad_fma(acc, a, b);
      if (ct == 0) quad_fma(accb, a, ones);                        // (wavefront-uniform)
    }
    float* const pw = part + (isx ? 0 : (long)J * I);
    float* const pb = part + (long)J * (I + Hc) + (isx ? 0 : J);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = jt * 16 + 4 * lg + i;                          // the result's row
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
  for (; s + 8 <= n_slab; s += 8) {                                // eight slabs' loads in flight, added in slab order
    float t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = p[(long)(s + k) * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += (double)t[k];
  }
  for (; s < n_slab; ++s) acc += (double)p[(long)s * stride];
  return (float)acc;
}

__global__ __launch_bounds__(256) void k_gru_dw_final(const GArgs g) {
  const int I = g.I, Hc = g.Hc, H = g.H, IN = g.IN, J = 3 * H;
  const long S = (long)J * (I + Hc + 2);
  const long n_i = (long)J * IN, n_h = (long)J * H;
  long e = blockIdx.x * 256L + threadIdx.x;
  if (e < n_i) {                                                   // grad_W_ih (3H, input_size): the padded columns' gradient is 0
    if (!g.need_wih) return;
    const int j = (int)(e / IN), c = (int)(e - (long)j * IN);
    g.gwih[e] = c < I ? slab_sum(g.part + (long)j * I + c, S, g.n_slab) : 0.f;
    return;
  }
  e -= n_i;
  if (e < n_h) {
    if (!g.need_whh) return;
    const int j = (int)(e / H), c = (int)(e - (long)j * H);
    g.gwhh[e] = c < Hc ? slab_sum(g.part + (long)J * I + (long)j * Hc + c, S, g.n_slab) : 0.f;
    return;
  }
  e -= n_h;
  if (e < J) {
    if (g.need_bih) g.gbih[e] = slab_sum(g.part + (long)J * (I + Hc) + e, S, g.n_slab);
    return;
  }
  e -= J;
  if (e < J && g.need_bhh) g.gbhh[e] = slab_sum(g.part + (long)J * (I + Hc) + J + e, S, g.n_slab);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline long slab_rows(long V) {
  const long l = (V + PNA_GRU_MAX_SLABS - 1) / PNA_GRU_MAX_SLABS;
  return l > PNA_GRU_SLAB_ROWS ? l : PNA_GRU_SLAB_ROWS;
}

// NULL inside the scope, else the clause that refuses
const char* scope_clause(int64_t V, int I, int Hc, int IN, int H) {
  if (IN < 1 || IN > kMaxWidth) return "needs 1 <= input_size <= 128";
  if (H < 2 || H > kMaxWidth) return "needs 2 <= hidden_size <= 128";
  if (V < 2 || V > INT32_MAX) return "needs V >= 2 rows (and V < 2^31)";
  if (I < 1 || I > IN) return "needs 1 <= I <= input_size columns of x";
  if (Hc < 1 || Hc > H) return "needs 1 <= Hc <= hidden_size columns of h";
  return nullptr;
}

int fill(const pna_gru_cell_args* p, GArgs& g, bool bwd, const char* fn) {
  if (!p) return pna_refuse(fn, "args is NULL");
  if (int rc_ss = pna_check_struct_size(fn, p->struct_size, sizeof(*p))) return rc_ss;
  if (p->dtype != PNA_GRU_F32) return pna_refuse(fn, "fp32 only (dtype must be PNA_GRU_F32)");
  if (const char* c = scope_clause(p->V, p->I, p->Hc, p->input_size, p->hidden_size)) return pna_refuse(fn, c);
  const int I = p->I, Hc = p->Hc, IN = p->input_size, H = p->hidden_size;
  if (!p->x || p->ldx < I) return pna_refuse(fn, "needs x (V, ldx >= I)");
  if (!p->h || p->ldh < Hc) return pna_refuse(fn, "needs h (V, ldh >= Hc)");
  if (!p->w_ih || p->ld_wih < IN) return pna_refuse(fn, "needs w_ih (3 hidden_size, ld_wih >= input_size)");
  if (!p->w_hh || p->ld_whh < H) return pna_refuse(fn, "needs w_hh (3 hidden_size, ld_whh >= hidden_size)");
  memset(&g, 0, sizeof(g));
  g.V = p->V; g.I = I; g.Hc = Hc; g.IN = IN; g.H = H;
  g.x = p->x; g.ldx = (long)p->ldx; g.h = p->h; g.ldh = (long)p->ldh;
  g.wih = p->w_ih; g.ldwi = (long)p->ld_wih; g.whh = p->w_hh; g.ldwh = (long)p->ld_whh;
  g.saved = p->saved;
  if (!bwd) {
    if (!p->b_ih || !p->b_hh) return pna_refuse(fn, "needs b_ih and b_hh [3 hidden_size] (bias=True)");
    if (!p->out || p->ld_out < H) return pna_refuse(fn, "needs out (V, ld_out >= hidden_size)");
    g.bih = p->b_ih; g.bhh = p->b_hh; g.out = p->out; g.ldo = (long)p->ld_out;
    return PNA_OK;
  }
  if (!p->saved) return pna_refuse(fn, "needs the forward's saved state (4, V, hidden_size)");
  if (!p->grad_out || p->ld_go < H) return pna_refuse(fn, "needs grad_out (V, ld_go >= hidden_size)");
  if (p->need_x && (!p->grad_x || p->ld_gx < I)) return pna_refuse(fn, "need_x needs grad_x (V, ld_gx >= I)");
  if (p->need_h && (!p->grad_h || p->ld_gh < Hc)) return pna_refuse(fn, "need_h needs grad_h (V, ld_gh >= Hc)");
  if ((p->need_w_ih && !p->grad_w_ih) || (p->need_w_hh && !p->grad_w_hh) || (p->need_b_ih && !p->grad_b_ih) || (p->need_b_hh && !p->grad_b_hh))
    return pna_refuse(fn, "every need_w_* / need_b_* flag needs its gradient buffer");
  const int64_t need = pna_gru_cell_workspace_bytes(p->V, I, Hc, H);
  if (!p->workspace || ((uintptr_t)p->workspace & 15) || p->workspace_bytes < need)
    return pna_refuse(fn, "needs a 16-byte aligned workspace of pna_gru_cell_workspace_bytes(V, I, Hc, hidden_size)");
  g.go = p->grad_out; g.ldgo = (long)p->ld_go;
  g.gx = p->grad_x; g.ldgx = (long)p->ld_gx; g.gh = p->grad_h; g.ldgh = (long)p->ld_gh;
  g.gwih = p->grad_w_ih; g.gwhh = p->grad_w_hh; g.gbih = p->grad_b_ih; g.gbhh = p->grad_b_hh;
  g.need_x = p->need_x != 0; g.need_h = p->need_h != 0;
  g.need_wih = p->need_w_ih != 0; g.need_whh = p->need_w_hh != 0; g.need_bih = p->need_b_ih != 0; g.need_bhh = p->need_b_hh != 0;
  g.slab = slab_rows(g.V);
  g.n_slab = (int)((g.V + g.slab - 1) / g.slab);
  g.dg = (float*)p->workspace;
  g.part = g.dg + g.V * 4 * H;
  return PNA_OK;
}

}  // namespace

extern "C" int32_t pna_gru_cell_in_scope(int64_t V, int32_t I, int32_t Hc, int32_t input_size, int32_t hidden_size) {
  return !scope_clause(V, I, Hc, input_size, hidden_size);
}

extern "C" int64_t pna_gru_cell_workspace_bytes(int64_t V, int32_t I, int32_t Hc, int32_t hidden_size) {
  if (scope_clause(V, I, Hc, kMaxWidth, hidden_size)) return -1;
  const long slab = slab_rows(V);
  const int64_t n_slab = (V + slab - 1) / slab;
  return (V * 4 * hidden_size + n_slab * 3 * hidden_size * (I + Hc + 2)) * 4;
}

extern "C" int pna_gru_cell_fwd_f32(const pna_gru_cell_args* p, pna_stream_t stream) {
  GArgs g;
  const int rc = fill(p, g, false, "pna_gru_cell_fwd_f32");
  if (rc != PNA_OK) return rc;
  const size_t lds = (size_t)kRows * (pitch_of(quads(g.I)) + pitch_of(quads(g.Hc))) * sizeof(float);     // <= 16.5 KiB
  hipLaunchKernelGGL(k_gru_rows_fwd, dim3((unsigned)((g.V + kRows - 1) / kRows)), dim3(kThreads), lds, (hipStream_t)stream, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_gru_cell_fwd_f32: launch failed");
  return PNA_OK;
}

extern "C" int pna_gru_cell_bwd_f32(const pna_gru_cell_args* p, pna_stream_t stream) {
  GArgs g;
  const int rc = fill(p, g, true, "pna_gru_cell_bwd_f32");
  if (rc != PNA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool weights = g.need_wih || g.need_whh || g.need_bih || g.need_bhh;
  if (!(g.need_x || g.need_h || weights)) return PNA_OK;
  const size_t lds = (size_t)4 * kRows * pitch_of(quads(g.H)) * sizeof(float);                           // <= 33 KiB
  hipLaunchKernelGGL(k_gru_rows_bwd, dim3((unsigned)((g.V + kRows - 1) / kRows)), dim3(kThreads), lds, st, g);
  if (weights) {
    hipLaunchKernelGGL(k_gru_dw_slab, dim3((unsigned)g.n_slab, (unsigned)((3 * g.H + 15) / 16)), dim3(kDwThreads), 0, st, g);
    const long n = 3L * g.H * (g.IN + g.H + 2);
    hipLaunchKernelGGL(k_gru_dw_final, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g);
  }
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_gru_cell_bwd_f32: launch failed");
  return PNA_OK;
}
