// pna_bf16.hip -- bf16 inference path of PNASimpleLayer for gfx950 (MI355X, CDNA4): pna_segreduce_fwd_bf16 (gather +
// aggregator statistics of bf16 rows, fp32 accumulation, bf16 aggregate) and pna_posttrans_bf16 (the posttrans contraction on
// v_mfma_f32_16x16x32_bf16 with the scalers, bias and the eval-mode BatchNorm / ReLU / residual epilogue).  See
// include/pna_amd.h for the arguments and the reference code each entry point replaces.
//
// Gather: a wavefront is cut into 64 / G lane groups of G = ceil(F / 8) lanes; a group owns one destination row
// and each lane owns 8 consecutive features, so a row is one 16-byte load per lane when the row pitch is a multiple of 8
// elements (2-byte loads otherwise).  Every lane keeps (sum, sum of squares, max, min) of its 8 features in fp32 registers:
// no cross-lane reduction, no atomics.  Hub rows are cut into the graph's heavy-row segments whose fp32 partials are combined
// in segment order by a second kernel, so results do not depend on the launch geometry.
//
// Contraction: workgroups of 4 wavefronts x 2 row tiles of 16 rows; the aggregate rows are read straight into the MFMA A
// fragments (lane l: row l & 15, columns 8 (l >> 4) .. + 8 of the 32-column chunk), the weight chunk of every scaler block is
// staged in LDS once per workgroup and chunk, and each scaler block keeps its own fp32 accumulators: the row scalers multiply
// the fp32 sums in the epilogue (the (M, S K) scaled operand exists nowhere, and no scaled value is rounded to bf16).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_bf16_dev.h"
#include "pna_rowstats.h"

namespace {

using namespace pna_bf16;

// the in-edges [beg, end) of one row folded in CSR order; four gathers in flight per lane
template <bool V8>
__device__ __forceinline__ void gather(const SegArgs& a, int beg, int end, int f0, int nf, Acc& c) {
  const u16* xb = a.x + f0;
  int k = beg;
  for (; k + 4 <= end; k += 4) {
    int id[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) id[u] = a.col[k + u];
    float v[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) load8<V8>(xb + (size_t)id[u] * a.ldx, nf, v[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) fold(c, v[u]);
  }
  for (; k < end; ++k) {
    float v[8];
    load8<V8>(xb + (size_t)a.col[k] * a.ldx, nf, v);
    fold(c, v);
  }
}

// light rows: one lane group per destination row (rows of the heavy schedule are skipped)
template <bool V8, bool VOUT>
__global__ __launch_bounds__(kBlock) void k_segreduce_bf16(SegArgs a) {
  const int lane = threadIdx.x & 63, per_wave = 64 / a.G, grp = lane / a.G, li = lane - grp * a.G;
  if (grp >= per_wave) return;
  const long row = ((long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * per_wave + grp;
  const int f0 = li * 8;
  if (row >= a.V) return;
  const int beg = a.rowptr[row], end = a.rowptr[row + 1], deg = end - beg;
  if (a.n_heavy > 0 && deg > a.heavy_threshold) return;
  Acc c;
  acc_init(c);
  gather<V8>(a, beg, end, f0, a.F - f0, c);
  finish_row<VOUT>(a, (int)row, deg, f0, c);
}

// heavy segments: one lane group per segment, fp32 partials
template <bool V8>
__global__ __launch_bounds__(kBlock) void k_segreduce_bf16_seg(SegArgs a) {
  const int lane = threadIdx.x & 63, per_wave = 64 / a.G, grp = lane / a.G, li = lane - grp * a.G;
  if (grp >= per_wave) return;
  const long seg = ((long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * per_wave + grp;
  if (seg >= a.n_seg) return;
  const int h = a.seg_heavy[seg], row = a.heavy_rows[h];
  const int rb = a.rowptr[row], re = a.rowptr[row + 1];
  const int beg = rb + (int)(seg - a.heavy_segptr[h]) * a.seg_len;
  const int end = beg + a.seg_len < re ? beg + a.seg_len : re;
  const int f0 = li * 8;
  Acc c;
  acc_init(c);
  gather<V8>(a, beg, end, f0, a.F - f0, c);
  store_partials(a, seg, f0, c);
}

// heavy rows: the partials of a row combined in segment order, then finalized like a light row
template <bool VOUT>
__global__ __launch_bounds__(kBlock) void k_segreduce_bf16_fin(SegArgs a) {
  const int lane = threadIdx.x & 63, per_wave = 64 / a.G, grp = lane / a.G, li = lane - grp * a.G;
  if (grp >= per_wave) return;
  const long h = ((long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * per_wave + grp;
  if (h >= a.n_heavy) return;
  finish_heavy_row<VOUT>(a, h, li * 8);
}

// ---------------------------------------------------------------------------------------------------------------------------
// contraction + epilogue
// ---------------------------------------------------------------------------------------------------------------------------
struct PtArgs {
  const u16* a; int64_t lda; int M, K;
  int N, Kp;
  const float* row_scale[3];
  const u16* w_img;
  const u16* bias;
  int epilogue, relu;
  const float* col_scale; const float* col_shift;
  const u16* residual; int64_t ld_res;
  u16* y; int64_t ldy;
};

constexpr int kRT = 2;                        // row tiles of 16 rows per wavefront
constexpr int kBM = (kBlock / 64) * kRT * 16; // rows per workgroup
constexpr int kLdsRow = 40;                   // 32 k + 8 elements of padding: 80-byte rows, 16-byte aligned fragment reads

template <int S, int NT>
__global__ __launch_bounds__(kBlock) void k_posttrans_bf16(PtArgs p) {
  constexpr int NP = NT * 16;
  constexpr int PIECES = S * NP * 4;                           // 16-byte pieces of one 32-column weight chunk
  constexpr int PER_THREAD = (PIECES + kBlock - 1) / kBlock;
  __shared__ __attribute__((aligned(16))) u16 wl[S * NP * kLdsRow];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row0 = (long)blockIdx.x * kBM + wave * kRT * 16;
  const int ka = 8 * (lane >> 4);

  f4 acc[kRT][S][NT];
#pragma unroll
  for (int r = 0; r < kRT; ++r)
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[r][s][n] = (f4){0.f, 0.f, 0.f, 0.f};

  auto load_a = [&](int k0, u4 (&av)[kRT]) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < kRT; ++r) {
      const long row = row0 + r * 16 + (lane & 15);
      const int k = k0 + ka;
      av[r] = (row < p.M && k < p.K) ? *reinterpret_cast<const u4*>(p.a + row * p.lda + k) : (u4){0u, 0u, 0u, 0u};
    }
  };
  auto load_w = [&](int k0, u4 (&wv)[PER_THREAD]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      const int pid = threadIdx.x + i * kBlock;
      if (pid < PIECES) wv[i] = *reinterpret_cast<const u4*>(p.w_img + (size_t)(pid >> 2) * p.Kp + k0 + 8 * (pid & 3));
    }
  };

  u4 av[kRT], wv[PER_THREAD];
  load_a(0, av);
  load_w(0, wv);
  const int nc = p.Kp / 32;
  for (int c = 0; c < nc; ++c) {
    __syncthreads();                                            // every wavefront is done with the previous chunk
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      const int pid = threadIdx.x + i * kBlock;
      if (pid < PIECES) *reinterpret_cast<u4*>(wl + (pid >> 2) * kLdsRow + 8 * (pid & 3)) = wv[i];
    }
    __syncthreads();
    bf8 A[kRT];
#pragma unroll
    for (int r = 0; r < kRT; ++r) A[r] = __builtin_bit_cast(bf8, av[r]);
    if (c + 1 < nc) {                                           // the next chunk's loads fly under this chunk's MFMAs
      load_a((c + 1) * 32, av);
      load_w((c + 1) * 32, wv);
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const bf8 B = __builtin_bit_cast(bf8, *reinterpret_cast<const u4*>(wl + (s * NP + n * 16 + (lane & 15)) * kLdsRow + ka));
#pragma unroll
        for (int r = 0; r < kRT; ++r) acc[r][s][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[r], B, acc[r][s][n], 0, 0, 0);
      }
  }

  // epilogue: C/D lane map col = lane & 15, row = 4 (lane >> 4) + i
#pragma unroll
  for (int r = 0; r < kRT; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long row = row0 + r * 16 + 4 * (lane >> 4) + i;
      if (row >= p.M) continue;
      float sc[S];
#pragma unroll
      for (int s = 0; s < S; ++s) sc[s] = p.row_scale[s] ? p.row_scale[s][row] : 1.f;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int col = n * 16 + (lane & 15);
        if (col >= p.N) continue;
        float z = sc[0] * acc[r][0][n][i];
#pragma unroll
        for (int s = 1; s < S; ++s) z = z + sc[s] * acc[r][s][n][i];
        if (p.bias) z = z + bf2f(p.bias[col]);
        if (p.epilogue) {
          if (p.col_scale) z = z * p.col_scale[col] + p.col_shift[col];
          if (p.relu) z = z < 0.f ? 0.f : z;
          if (p.residual) z = z + bf2f(p.residual[row * p.ld_res + col]);
        }
        p.y[row * p.ldy + col] = f2bf(z);
      }
    }
}

template <int S, int NT>
hipError_t launch_pt(const PtArgs& k, hipStream_t st) {
  const unsigned grid = (unsigned)((k.M + kBM - 1) / kBM);
  hipLaunchKernelGGL((k_posttrans_bf16<S, NT>), dim3(grid), dim3(kBlock), 0, st, k);
  return hipGetLastError();
}

template <int S>
hipError_t launch_pt_n(const PtArgs& k, int nt, hipStream_t st) {
  switch (nt) {
    case 2: return launch_pt<S, 2>(k, st);
    case 4: return launch_pt<S, 4>(k, st);
    case 5: return launch_pt<S, 5>(k, st);
    default: return launch_pt<S, 8>(k, st);
  }
}

}  // namespace

extern "C" int pna_posttrans_bf16_tiles(int32_t N) {
  return N <= 0 || N > 128 ? -1 : N <= 32 ? 2 : N <= 64 ? 4 : N <= 80 ? 5 : 8;
}

extern "C" int64_t pna_segreduce_bf16_partials_bytes(int32_t n_seg, int32_t F) {
  if (n_seg <= 0 || F <= 0) return 0;
  return (int64_t)n_seg * 4 * ((F + 7) / 8 * 8) * (int64_t)sizeof(float);
}

extern "C" int pna_segreduce_fwd_bf16(const pna_segreduce_bf16_args* p, pna_stream_t stream) {
  if (!p) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_bf16: null args");
  if (int rc_ss = pna_check_struct_size("pna_segreduce_fwd_bf16", p->struct_size, sizeof(*p))) return rc_ss;
  if (p->V < 0 || p->F <= 0 || p->F > 512) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_bf16: need V >= 0 and 1 <= F <= 512");
  if (p->V == 0) return PNA_OK;
  if (!p->rowptr || !p->col || !p->x || !p->out) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_bf16: rowptr/col/x/out must be non-null");
  if (p->n_aggr < 1 || p->n_aggr > PNA_MAX_AGGR) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_bf16: n_aggr out of range");
  for (int i = 0; i < p->n_aggr; ++i)
    if (p->aggr[i] < PNA_AGG_MEAN || p->aggr[i] > PNA_AGG_VAR)
      return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_bf16: aggregator code must be mean/sum/max/min/std/var");
  const int bs = p->block_stride > 0 ? p->block_stride : p->F;
  if (bs < p->F || p->ldx < p->F || p->ldo < (int64_t)(p->n_aggr - 1) * bs + p->F || p->ldo % 8 != 0 || ((uintptr_t)p->out & 15) != 0)
    return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_bf16: leading dimensions too small, or out / ldo not 16-byte aligned");
  if (p->n_heavy > 0 && (!p->heavy_rows || !p->heavy_segptr || !p->seg_heavy || !p->partials || p->n_seg <= 0 || p->seg_len <= 0 ||
                         p->heavy_threshold <= 0))
    return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_bf16: incomplete heavy-row schedule");

  SegArgs a{};
  a.rowptr = p->rowptr; a.col = p->col; a.x = reinterpret_cast<const u16*>(p->x); a.ldx = p->ldx;
  a.V = p->V; a.F = p->F; a.G = (p->F + 7) / 8; a.F8 = a.G * 8;
  a.n_aggr = p->n_aggr;
  for (int i = 0; i < PNA_MAX_AGGR; ++i) a.aggr[i] = i < p->n_aggr ? p->aggr[i] : 0;
  a.out = reinterpret_cast<u16*>(p->out); a.ldo = p->ldo; a.bs = bs;
  a.heavy_threshold = p->heavy_threshold; a.seg_len = p->seg_len;
  a.n_heavy = p->n_heavy > 0 ? p->n_heavy : 0; a.n_seg = a.n_heavy ? p->n_seg : 0;
  a.heavy_rows = p->heavy_rows; a.heavy_segptr = p->heavy_segptr; a.seg_heavy = p->seg_heavy; a.partials = p->partials;

  // 16-byte gathers: the row pitch keeps every row's first feature 16-byte aligned and the caller declares the columns up to the
  // next multiple of 8 readable (or there are none)
  const bool v8 = p->ldx % 8 == 0 && ((uintptr_t)p->x & 15) == 0 && (p->F % 8 == 0 || p->x_tail_readable);
  const bool vout = bs % 8 == 0;
  hipStream_t st = (hipStream_t)stream;
  const long per_block = (long)(kBlock / 64) * (64 / a.G);
  if (a.n_heavy > 0) {
    const unsigned gs = (unsigned)((a.n_seg + per_block - 1) / per_block);
    if (v8) hipLaunchKernelGGL((k_segreduce_bf16_seg<true>), dim3(gs), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((k_segreduce_bf16_seg<false>), dim3(gs), dim3(kBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  }
  const unsigned grid = (unsigned)((a.V + per_block - 1) / per_block);
  if (v8 && vout) hipLaunchKernelGGL((k_segreduce_bf16<true, true>), dim3(grid), dim3(kBlock), 0, st, a);
  else if (v8) hipLaunchKernelGGL((k_segreduce_bf16<true, false>), dim3(grid), dim3(kBlock), 0, st, a);
  else if (vout) hipLaunchKernelGGL((k_segreduce_bf16<false, true>), dim3(grid), dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL((k_segreduce_bf16<false, false>), dim3(grid), dim3(kBlock), 0, st, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  if (a.n_heavy > 0) {
    const unsigned gf = (unsigned)((a.n_heavy + per_block - 1) / per_block);
    if (vout) hipLaunchKernelGGL((k_segreduce_bf16_fin<true>), dim3(gf), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((k_segreduce_bf16_fin<false>), dim3(gf), dim3(kBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  }
  return PNA_OK;
}

extern "C" int pna_posttrans_bf16(const pna_posttrans_bf16_args* p, pna_stream_t stream) {
  if (!p) return pna_set_error(PNA_E_INVALID, "pna_posttrans_bf16: null args");
  if (int rc_ss = pna_check_struct_size("pna_posttrans_bf16", p->struct_size, sizeof(*p))) return rc_ss;
  if (p->M < 0 || p->K <= 0 || p->K % 8 != 0 || p->n_scaler < 1 || p->n_scaler > 3)
    return pna_set_error(PNA_E_INVALID, "pna_posttrans_bf16: need M >= 0, K > 0 a multiple of 8, 1 <= n_scaler <= 3");
  const int nt = pna_posttrans_bf16_tiles(p->N);
  if (nt < 0) return pna_set_error(PNA_E_INVALID, "pna_posttrans_bf16: need 1 <= N <= 128");
  if (p->M == 0) return PNA_OK;
  if (!p->a || !p->w_img || !p->y) return pna_set_error(PNA_E_INVALID, "pna_posttrans_bf16: a/w_img/y must be non-null");
  if (p->lda < p->K || p->lda % 8 != 0 || ((uintptr_t)p->a & 15) != 0 || ((uintptr_t)p->w_img & 15) != 0)
    return pna_set_error(PNA_E_INVALID, "pna_posttrans_bf16: a / w_img must be 16-byte aligned with lda >= K a multiple of 8");
  if (p->ldy < p->N || (p->residual && p->ld_res < p->N) || (p->col_scale && !p->col_shift))
    return pna_set_error(PNA_E_INVALID, "pna_posttrans_bf16: bad ldy / ld_res, or col_scale without col_shift");
  PtArgs k{};
  k.a = reinterpret_cast<const u16*>(p->a); k.lda = p->lda; k.M = p->M; k.K = p->K;
  k.N = p->N; k.Kp = (p->K + 31) / 32 * 32;
  for (int s = 0; s < 3; ++s) k.row_scale[s] = s < p->n_scaler ? p->row_scale[s] : nullptr;
  k.w_img = reinterpret_cast<const u16*>(p->w_img);
  k.bias = reinterpret_cast<const u16*>(p->bias);
  k.epilogue = p->epilogue != 0; k.relu = p->relu != 0;
  k.col_scale = p->col_scale; k.col_shift = p->col_shift;
  k.residual = reinterpret_cast<const u16*>(p->residual); k.ld_res = p->ld_res;
  k.y = reinterpret_cast<u16*>(p->y); k.ldy = p->ldy;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  switch (p->n_scaler) {
    case 1: e = launch_pt_n<1>(k, nt, st); break;
    case 2: e = launch_pt_n<2>(k, nt, st); break;
    default: e = launch_pt_n<3>(k, nt, st); break;
  }
  if (e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  return PNA_OK;
}
