// pna_bf16_tower.hip -- bf16 inference path of PNALayer / PNATower for gfx950 (MI355X, CDNA4): pna_gather_bf16 (the gather of
// pna_bf16.hip with the destination and edge terms of the factorised pretrans added to every message in fp32) and
// pna_contract_bf16 (the MFMA contraction with an unscaled self operand, a per-row post factor and a leaky activation: one entry
// point for the pretrans projections, the posttrans of all towers and the mixing network).  See include/pna_amd.h for the
// arguments and the reference code each entry point replaces, DESIGN.md 4.11 for the layout.
//
// Gather: the lane layout of pna_bf16.hip (a lane group of ceil(F / 8) lanes per destination row, 8 features per lane, fp32
// statistics in registers, hub rows through the heavy-row segments).  A lane loads its 8 columns of the destination row once and
// adds them, and the edge row of every edge, to the gathered source row in fp32: the message is never rounded and never stored.
//
// Contraction: the tiling of k_posttrans_bf16 (4 wavefronts x RT row tiles of 16 rows, the weight chunk of every scaler block
// staged in LDS, fp32 accumulators per scaler block).  The self operand is a second pass over its own weight image into the
// accumulators of block 0 when that block's row scale is the identity, else into a set of its own (SA = S + 1 sets; one row
// tile per wavefront where two would not fit the registers).  More than 128 output columns: column slabs on blockIdx.y.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_bf16_dev.h"
#include "pna_rowstats.h"

namespace {

using namespace pna_bf16;

// ---------------------------------------------------------------------------------------------------------------------------
// gather of x[src] + dst_term[dst] + edge term
// ---------------------------------------------------------------------------------------------------------------------------
struct MsgArgs {
  SegArgs s;
  const u16* dst; int64_t ldd;
  const u16* er; int64_t lde; int n_er;
  const int32_t* et;
};

// the in-edges [beg, end) of destination `row` folded in CSR order; four edges in flight per lane
template <bool V8>
__device__ __forceinline__ void gather_msg(const MsgArgs& a, int row, int beg, int end, int f0, int nf, Acc& c) {
  const u16* xb = a.s.x + f0;
  float d[8];
  if (a.dst) {
    load8<V8>(a.dst + (size_t)row * a.ldd + f0, nf, d);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = 0.f;
  }
  const u16* eb = a.er ? a.er + f0 : nullptr;
  auto edge_row = [&](int k) __attribute__((always_inline)) {
    if (!a.et) return (size_t)k;
    int t = a.et[k];
    t = t < 0 ? 0 : t >= a.n_er ? a.n_er - 1 : t;              // a type outside the table reads a row of the table, never beyond it
    return (size_t)t;
  };
  int k = beg;
  for (; k + 4 <= end; k += 4) {
    int id[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) id[u] = a.s.col[k + u];
    float v[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) load8<V8>(xb + (size_t)id[u] * a.s.ldx, nf, v[u]);
    if (eb) {
      float w[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) load8<V8>(eb + edge_row(k + u) * a.lde, nf, w[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[u][j] = (v[u][j] + d[j]) + w[u][j];
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[u][j] = v[u][j] + d[j];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) fold(c, v[u]);
  }
  for (; k < end; ++k) {
    float v[8];
    load8<V8>(xb + (size_t)a.s.col[k] * a.s.ldx, nf, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = v[j] + d[j];
    if (eb) {
      float w[8];
      load8<V8>(eb + edge_row(k) * a.lde, nf, w);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] + w[j];
    }
    fold(c, v);
  }
}

// light rows: one lane group per destination row (rows of the heavy schedule are skipped)
template <bool V8, bool VOUT>
__global__ __launch_bounds__(kBlock) void k_gather_bf16(MsgArgs a) {
  const int lane = threadIdx.x & 63, per_wave = 64 / a.s.G, grp = lane / a.s.G, li = lane - grp * a.s.G;
  if (grp >= per_wave) return;
  const long row = ((long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * per_wave + grp;
  const int f0 = li * 8;
  if (row >= a.s.V) return;
  const int beg = a.s.rowptr[row], end = a.s.rowptr[row + 1], deg = end - beg;
  if (a.s.n_heavy > 0 && deg > a.s.heavy_threshold) return;
  Acc c;
  acc_init(c);
  gather_msg<V8>(a, (int)row, beg, end, f0, a.s.F - f0, c);
  finish_row<VOUT>(a.s, (int)row, deg, f0, c);
}

// heavy segments: one lane group per segment, fp32 partials of the full messages
template <bool V8>
__global__ __launch_bounds__(kBlock) void k_gather_bf16_seg(MsgArgs a) {
  const int lane = threadIdx.x & 63, per_wave = 64 / a.s.G, grp = lane / a.s.G, li = lane - grp * a.s.G;
  if (grp >= per_wave) return;
  const long seg = ((long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * per_wave + grp;
  if (seg >= a.s.n_seg) return;
  const int h = a.s.seg_heavy[seg], row = a.s.heavy_rows[h];
  const int rb = a.s.rowptr[row], re = a.s.rowptr[row + 1];
  const int beg = rb + (int)(seg - a.s.heavy_segptr[h]) * a.s.seg_len;
  const int end = beg + a.s.seg_len < re ? beg + a.s.seg_len : re;
  const int f0 = li * 8;
  Acc c;
  acc_init(c);
  gather_msg<V8>(a, row, beg, end, f0, a.s.F - f0, c);
  store_partials(a.s, seg, f0, c);
}

// heavy rows: the partials of a row combined in segment order, then finalized like a light row
template <bool VOUT>
__global__ __launch_bounds__(kBlock) void k_gather_bf16_fin(SegArgs a) {
  const int lane = threadIdx.x & 63, per_wave = 64 / a.G, grp = lane / a.G, li = lane - grp * a.G;
  if (grp >= per_wave) return;
  const long h = ((long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * per_wave + grp;
  if (h >= a.n_heavy) return;
  finish_heavy_row<VOUT>(a, h, li * 8);
}

// ---------------------------------------------------------------------------------------------------------------------------
// contraction + epilogue
// ---------------------------------------------------------------------------------------------------------------------------
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

}  // namespace

extern "C" int pna_contract_bf16_tiles(int32_t N) {
  return N <= 0 || N > 4096 ? -1 : N <= 32 ? 2 : N <= 64 ? 4 : N <= 80 ? 5 : 8;
}

extern "C" int pna_gather_bf16(const pna_gather_bf16_args* p, pna_stream_t stream) {
  if (!p) return pna_set_error(PNA_E_INVALID, "pna_gather_bf16: null args");
  if (int rc_ss = pna_check_struct_size("pna_gather_bf16", p->struct_size, sizeof(*p))) return rc_ss;
  if (p->V < 0 || p->F <= 0 || p->F > 512) return pna_set_error(PNA_E_INVALID, "pna_gather_bf16: need V >= 0 and 1 <= F <= 512");
  if (p->V == 0) return PNA_OK;
  if (!p->rowptr || !p->col || !p->x || !p->out) return pna_set_error(PNA_E_INVALID, "pna_gather_bf16: rowptr/col/x/out must be non-null");
  if (p->n_aggr < 1 || p->n_aggr > PNA_MAX_AGGR) return pna_set_error(PNA_E_INVALID, "pna_gather_bf16: n_aggr out of range");
  for (int i = 0; i < p->n_aggr; ++i)
    if (p->aggr[i] < PNA_AGG_MEAN || p->aggr[i] > PNA_AGG_VAR)
      return pna_set_error(PNA_E_INVALID, "pna_gather_bf16: aggregator code must be mean/sum/max/min/std/var");
  const int bs = p->block_stride > 0 ? p->block_stride : p->F;
  if (bs < p->F || p->ldx < p->F || p->ldo < (int64_t)(p->n_aggr - 1) * bs + p->F || p->ldo % 8 != 0 || ((uintptr_t)p->out & 15) != 0)
    return pna_set_error(PNA_E_INVALID, "pna_gather_bf16: leading dimensions too small, or out / ldo not 16-byte aligned");
  if ((p->dst_term && p->ld_dst < p->F) || (p->edge_rows && p->ld_edge < p->F))
    return pna_set_error(PNA_E_INVALID, "pna_gather_bf16: ld_dst / ld_edge smaller than F");
  if (p->edge_type && (!p->edge_rows || p->n_edge_rows < 1))
    return pna_set_error(PNA_E_INVALID, "pna_gather_bf16: edge_type needs edge_rows with n_edge_rows >= 1");
  if (p->n_heavy > 0 && (!p->heavy_rows || !p->heavy_segptr || !p->seg_heavy || !p->partials || p->n_seg <= 0 || p->seg_len <= 0 ||
                         p->heavy_threshold <= 0))
    return pna_set_error(PNA_E_INVALID, "pna_gather_bf16: incomplete heavy-row schedule");

  MsgArgs m{};
  SegArgs& a = m.s;
  a.rowptr = p->rowptr; a.col = p->col; a.x = reinterpret_cast<const u16*>(p->x); a.ldx = p->ldx;
  a.V = p->V; a.F = p->F; a.G = (p->F + 7) / 8; a.F8 = a.G * 8;
  a.n_aggr = p->n_aggr;
  for (int i = 0; i < PNA_MAX_AGGR; ++i) a.aggr[i] = i < p->n_aggr ? p->aggr[i] : 0;
  a.out = reinterpret_cast<u16*>(p->out); a.ldo = p->ldo; a.bs = bs;
  a.heavy_threshold = p->heavy_threshold; a.seg_len = p->seg_len;
  a.n_heavy = p->n_heavy > 0 ? p->n_heavy : 0; a.n_seg = a.n_heavy ? p->n_seg : 0;
  a.heavy_rows = p->heavy_rows; a.heavy_segptr = p->heavy_segptr; a.seg_heavy = p->seg_heavy; a.partials = p->partials;
  m.dst = reinterpret_cast<const u16*>(p->dst_term); m.ldd = p->ld_dst;
  m.er = reinterpret_cast<const u16*>(p->edge_rows); m.lde = p->ld_edge; m.n_er = p->n_edge_rows;
  m.et = p->edge_type;

  // 16-byte gathers: every operand keeps its rows' first feature 16-byte aligned and the columns up to the next multiple of 8 readable
  auto wide = [&](const void* q, int64_t ld) { return !q || (ld % 8 == 0 && ((uintptr_t)q & 15) == 0); };
  const bool v8 = wide(p->x, p->ldx) && wide(p->dst_term, p->ld_dst) && wide(p->edge_rows, p->ld_edge) &&
                  (p->F % 8 == 0 || p->tails_readable);
  const bool vout = bs % 8 == 0;
  hipStream_t st = (hipStream_t)stream;
  const long per_block = (long)(kBlock / 64) * (64 / a.G);
  if (a.n_heavy > 0) {
    const unsigned gs = (unsigned)((a.n_seg + per_block - 1) / per_block);
    if (v8) hipLaunchKernelGGL((k_gather_bf16_seg<true>), dim3(gs), dim3(kBlock), 0, st, m);
    else hipLaunchKernelGGL((k_gather_bf16_seg<false>), dim3(gs), dim3(kBlock), 0, st, m);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  }
  const unsigned grid = (unsigned)((a.V + per_block - 1) / per_block);
  if (v8 && vout) hipLaunchKernelGGL((k_gather_bf16<true, true>), dim3(grid), dim3(kBlock), 0, st, m);
  else if (v8) hipLaunchKernelGGL((k_gather_bf16<true, false>), dim3(grid), dim3(kBlock), 0, st, m);
  else if (vout) hipLaunchKernelGGL((k_gather_bf16<false, true>), dim3(grid), dim3(kBlock), 0, st, m);
  else hipLaunchKernelGGL((k_gather_bf16<false, false>), dim3(grid), dim3(kBlock), 0, st, m);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  if (a.n_heavy > 0) {
    const unsigned gf = (unsigned)((a.n_heavy + per_block - 1) / per_block);
    if (vout) hipLaunchKernelGGL((k_gather_bf16_fin<true>), dim3(gf), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((k_gather_bf16_fin<false>), dim3(gf), dim3(kBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  }
  return PNA_OK;
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
