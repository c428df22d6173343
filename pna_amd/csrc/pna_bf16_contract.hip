// pna_bf16_contract.hip -- the MFMA contraction of the bf16 inference paths for gfx950 (MI355X, CDNA4): pna_contract_bf16 (scaler
// blocks, an unscaled self operand, a per-row post factor and a leaky activation: one entry point for the pretrans projections, the
// posttrans of all towers and the mixing network of PNALayer / PNATower) and pna_posttrans_bf16 (the posttrans of PNASimpleLayer with
// the eval-mode BatchNorm / ReLU / residual epilogue) on k_posttrans_bf16, the same tiling specialised for it.  See include/pna_amd.h
// for the arguments and the reference code each entry point replaces, DESIGN.md 4.10 and 4.11 for the layout.
//
// Workgroups of 4 wavefronts x RT row tiles of 16 rows; the operand rows are read straight into the MFMA A fragments (lane l: row
// l & 15, columns 8 (l >> 4) .. + 8 of the 32-column chunk), the weight chunk of every scaler block is staged in LDS once per
// workgroup and chunk, and each scaler block keeps its own fp32 accumulators: the row scalers multiply the fp32 sums in the epilogue
// (the (M, S K) scaled operand exists nowhere, and no scaled value is rounded to bf16).  The self operand is a second pass over its
// own weight image into the accumulators of block 0 when that block's row scale is the identity, else into a set of its own (SA =
// S + 1 sets; one row tile per wavefront where two would not fit the registers).  More than 128 output columns: column slabs on
// blockIdx.y.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_bf16_dev.h"
#include "pna_rowstats.h"

namespace {

using namespace pna_bf16;

struct CtArgs {
  const u16* a; int64_t lda; int M, K, Kp, vec_a;
  const u16* h; int64_t ldh; int Kh, Khp, vec_h;
  int N, R;                                   // R: rows of one block of the weight images
  const float* row_scale[3];
  const u16* w_img; const u16* w_self;
  const u16* bias;
  const float* row_post; const float* col_scale; const float* col_shift;
  float slope;
  const u16* residual; int64_t ld_res;
  u16* y; int64_t ldy;
};

constexpr int kLdsRow = 40;                   // 32 k + 8 elements of padding: 80-byte rows, 16-byte aligned fragment reads

// One operand against NB weight blocks into the accumulator sets [SLOT0, SLOT0 + NB): chunks of 32 columns, the operand rows read
// straight into the MFMA A fragments (lane l: row l & 15, columns 8 (l >> 4) .. + 8 of the chunk), the weight chunk through LDS.
template <int RT, int SA, int NT, int NB, int SLOT0>
__device__ __forceinline__ void contract_pass(f4 (&acc)[RT][SA][NT], u16* wl, const u16* a, int64_t lda, int M, int K, int Kp,
                                              bool vec, const u16* img, int R, long row0, int n0) {
  constexpr int NP = NT * 16;
  constexpr int PIECES = NB * NP * 4;                          // 16-byte pieces of one 32-column weight chunk
  constexpr int PER_THREAD = (PIECES + kBlock - 1) / kBlock;
  const int lane = threadIdx.x & 63;
  const int ka = 8 * (lane >> 4);

  auto load_a = [&](int k0, u4 (&av)[RT]) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const long row = row0 + r * 16 + (lane & 15);
      const int k = k0 + ka;
      u4 w = (u4){0u, 0u, 0u, 0u};
      if (row < M && k < K) {
        const u16* q = a + row * lda + k;
        if (vec) {
          w = *reinterpret_cast<const u4*>(q);                  // (K is a multiple of 8 here: the piece lies inside the row)
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const unsigned lo = k + 2 * j < K ? q[2 * j] : 0u, hi = k + 2 * j + 1 < K ? q[2 * j + 1] : 0u;
            w[j] = lo | (hi << 16);
          }
        }
      }
      av[r] = w;
    }
  };
  auto load_w = [&](int k0, u4 (&wv)[PER_THREAD]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      const int pid = threadIdx.x + i * kBlock;
      if (pid < PIECES) {
        const int wr = pid >> 2, b = wr / NP, rr = wr - b * NP;
        wv[i] = *reinterpret_cast<const u4*>(img + ((size_t)b * R + n0 + rr) * Kp + k0 + 8 * (pid & 3));
      }
    }
  };

  u4 av[RT], wv[PER_THREAD];
  load_a(0, av);
  load_w(0, wv);
  const int nc = Kp / 32;
  for (int c = 0; c < nc; ++c) {
    __syncthreads();                                            // every wavefront is done with the previous chunk
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      const int pid = threadIdx.x + i * kBlock;
      if (pid < PIECES) *reinterpret_cast<u4*>(wl + (pid >> 2) * kLdsRow + 8 * (pid & 3)) = wv[i];
    }
    __syncthreads();
    bf8 A[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) A[r] = __builtin_bit_cast(bf8, av[r]);
    if (c + 1 < nc) {                                           // the next chunk's loads fly under this chunk's MFMAs
      load_a((c + 1) * 32, av);
      load_w((c + 1) * 32, wv);
    }
#pragma unroll
    for (int s = 0; s < NB; ++s)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const bf8 B = __builtin_bit_cast(bf8, *reinterpret_cast<const u4*>(wl + (s * NP + n * 16 + (lane & 15)) * kLdsRow + ka));
#pragma unroll
        for (int r = 0; r < RT; ++r)
          acc[r][SLOT0 + s][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[r], B, acc[r][SLOT0 + s][n], 0, 0, 0);
      }
  }
}

// S scaler blocks; OWN = 1: the self operand accumulates into a set of its own (no identity scaler), else into block 0
template <int S, int OWN, int NT>
struct CtShape {
  static constexpr int SA = S + OWN;
  static constexpr int RT = SA * NT <= 24 ? 2 : 1;              // at most 192 accumulator registers per lane
  static constexpr int BM = (kBlock / 64) * RT * 16;
};

template <int S, int OWN, int NT>
__global__ __launch_bounds__(kBlock) void k_contract_bf16(CtArgs p) {
  constexpr int SA = CtShape<S, OWN, NT>::SA, RT = CtShape<S, OWN, NT>::RT, NP = NT * 16;
  __shared__ __attribute__((aligned(16))) u16 wl[S * NP * kLdsRow];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row0 = (long)blockIdx.x * CtShape<S, OWN, NT>::BM + wave * RT * 16;
  const int n0 = blockIdx.y * NP;

  f4 acc[RT][SA][NT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int s = 0; s < SA; ++s)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[r][s][n] = (f4){0.f, 0.f, 0.f, 0.f};

  contract_pass<RT, SA, NT, S, 0>(acc, wl, p.a, p.lda, p.M, p.K, p.Kp, p.vec_a != 0, p.w_img, p.R, row0, n0);
  if (p.h) contract_pass<RT, SA, NT, 1, OWN ? S : 0>(acc, wl, p.h, p.ldh, p.M, p.Kh, p.Khp, p.vec_h != 0, p.w_self, p.R, row0, n0);

  // epilogue: C/D lane map col = lane & 15, row = 4 (lane >> 4) + i
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long row = row0 + r * 16 + 4 * (lane >> 4) + i;
      if (row >= p.M) continue;
      float sc[S];
#pragma unroll
      for (int s = 0; s < S; ++s) sc[s] = p.row_scale[s] ? p.row_scale[s][row] : 1.f;
      const float post = p.row_post ? p.row_post[row] : 1.f;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int col = n0 + n * 16 + (lane & 15);
        if (col >= p.N) continue;
        float z = sc[0] * acc[r][0][n][i];
#pragma unroll
        for (int s = 1; s < S; ++s) z = z + sc[s] * acc[r][s][n][i];
        if (OWN) z = z + acc[r][SA - 1][n][i];
        if (p.bias) z = z + bf2f(p.bias[col]);
        z = z * post;
        if (p.col_scale) z = z * p.col_scale[col] + p.col_shift[col];
        z = z < 0.f ? z * p.slope : z;
        if (p.residual) z = z + bf2f(p.residual[row * p.ld_res + col]);
        p.y[row * p.ldy + col] = f2bf(z);
      }
    }
}

template <int S, int OWN, int NT>
hipError_t launch_ct(const CtArgs& k, hipStream_t st) {
  constexpr int BM = CtShape<S, OWN, NT>::BM;
  const dim3 grid((unsigned)((k.M + BM - 1) / BM), (unsigned)(k.R / (NT * 16)));
  hipLaunchKernelGGL((k_contract_bf16<S, OWN, NT>), grid, dim3(kBlock), 0, st, k);
  return hipGetLastError();
}

template <int S, int OWN>
hipError_t launch_ct_n(const CtArgs& k, int nt, hipStream_t st) {
  switch (nt) {
    case 2: return launch_ct<S, OWN, 2>(k, st);
    case 4: return launch_ct<S, OWN, 4>(k, st);
    case 5: return launch_ct<S, OWN, 5>(k, st);
    default: return launch_ct<S, OWN, 8>(k, st);
  }
}

template <int S>
hipError_t launch_ct_s(const CtArgs& k, int own, int nt, hipStream_t st) {
  return own ? launch_ct_n<S, 1>(k, nt, st) : launch_ct_n<S, 0>(k, nt, st);
}

bool vec_ok(const void* p, int64_t ld, int K) { return ((uintptr_t)p & 15) == 0 && ld % 8 == 0 && K % 8 == 0; }

// ---------------------------------------------------------------------------------------------------------------------------
// pna_posttrans_bf16: k_contract_bf16<S, 0, NT> for N <= 128 (same weight image, same tiling, same bits: tests/
// test_gpu_bf16_kernel_family.py) without the self operand, the column slabs and the run-time choice of the operand load, and
// with relu (+0.0 for a negative z) where the contraction has slope (z * 0 = -0.0).  Kept as a kernel of its own because it is 3 to
// 4.5 % faster at the bench shapes than the general kernel on the same arguments.
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

extern "C" int pna_contract_bf16_tiles(int32_t N) {
  return N <= 0 || N > 4096 ? -1 : N <= 32 ? 2 : N <= 64 ? 4 : N <= 80 ? 5 : 8;
}

extern "C" int pna_contract_bf16(const pna_contract_bf16_args* p, pna_stream_t stream) {
  if (!p) return pna_set_error(PNA_E_INVALID, "pna_contract_bf16: null args");
  if (int rc_ss = pna_check_struct_size("pna_contract_bf16", p->struct_size, sizeof(*p))) return rc_ss;
  if (p->M < 0 || p->K <= 0 || p->n_scaler < 1 || p->n_scaler > 3)
    return pna_set_error(PNA_E_INVALID, "pna_contract_bf16: need M >= 0, K > 0, 1 <= n_scaler <= 3");
  const int nt = pna_contract_bf16_tiles(p->N);
  if (nt < 0) return pna_set_error(PNA_E_INVALID, "pna_contract_bf16: need 1 <= N <= 4096");
  if (p->N > 128 && (p->n_scaler > 1 || p->h_self))
    return pna_set_error(PNA_E_INVALID, "pna_contract_bf16: N > 128 only with one scaler block and no h_self");
  if (p->h_self && (p->Kh <= 0 || !p->w_self || p->ld_self < p->Kh))
    return pna_set_error(PNA_E_INVALID, "pna_contract_bf16: h_self needs Kh > 0, ld_self >= Kh and w_self");
  if (p->M == 0) return PNA_OK;
  if (!p->a || !p->w_img || !p->y) return pna_set_error(PNA_E_INVALID, "pna_contract_bf16: a/w_img/y must be non-null");
  if (p->lda < p->K || ((uintptr_t)p->w_img & 15) != 0 || ((uintptr_t)p->w_self & 15) != 0)
    return pna_set_error(PNA_E_INVALID, "pna_contract_bf16: lda < K, or a weight image that is not 16-byte aligned");
  if (p->ldy < p->N || (p->residual && p->ld_res < p->N) || (!p->col_scale != !p->col_shift))
    return pna_set_error(PNA_E_INVALID, "pna_contract_bf16: bad ldy / ld_res, or only one of col_scale / col_shift");
  if (!(p->slope >= 0.f && p->slope <= 1.f)) return pna_set_error(PNA_E_INVALID, "pna_contract_bf16: slope must be in [0, 1]");
  CtArgs k{};
  k.a = reinterpret_cast<const u16*>(p->a); k.lda = p->lda; k.M = p->M; k.K = p->K; k.Kp = (p->K + 31) / 32 * 32;
  k.vec_a = vec_ok(p->a, p->lda, p->K);
  k.h = reinterpret_cast<const u16*>(p->h_self); k.ldh = p->ld_self; k.Kh = p->h_self ? p->Kh : 0; k.Khp = (k.Kh + 31) / 32 * 32;
  k.vec_h = p->h_self && vec_ok(p->h_self, p->ld_self, p->Kh);
  k.N = p->N; k.R = (p->N + 16 * nt - 1) / (16 * nt) * (16 * nt);
  for (int s = 0; s < 3; ++s) k.row_scale[s] = s < p->n_scaler ? p->row_scale[s] : nullptr;
  k.w_img = reinterpret_cast<const u16*>(p->w_img); k.w_self = reinterpret_cast<const u16*>(p->w_self);
  k.bias = reinterpret_cast<const u16*>(p->bias);
  k.row_post = p->row_post; k.col_scale = p->col_scale; k.col_shift = p->col_shift; k.slope = p->slope;
  k.residual = reinterpret_cast<const u16*>(p->residual); k.ld_res = p->ld_res;
  k.y = reinterpret_cast<u16*>(p->y); k.ldy = p->ldy;
  const int own = p->h_self && p->row_scale[0] != nullptr;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  switch (p->n_scaler) {
    case 1: e = launch_ct_s<1>(k, own, nt, st); break;
    case 2: e = launch_ct_s<2>(k, own, nt, st); break;
    default: e = launch_ct_s<3>(k, own, nt, st); break;
  }
  if (e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
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
