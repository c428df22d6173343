// pna_bf16_small.hip -- the bf16 tower layer of molecule-sized batches for gfx950 (MI355X, CDNA4): pna_tower_layer_bf16, one C call
// and at most two launches for PNALayer / PNATower / PNASimpleLayer in inference (the bf16 counterpart of pna_tower_layer_f32,
// pna_tower_fused.hip).  See include/pna_amd.h for the arguments and the arithmetic contract, DESIGN.md 4.12 for the layout.
//
// Launch 1 is pna_contract_bf16 (pna_bf16_contract.hip) on the projection image: x_cat = [x_src | x_dst] of every tower, each tower's
// block Fp = round8(Fi) columns wide so that every 8-feature piece is one 16-byte load.
// Launch 2, k_tower_rows_bf16: one workgroup (4 wavefronts) per 16 destination rows.
//   gather    one lane per (row, tower, 8 features): x_src[u] + x_dst[v] + edge row in fp32 (fold_edges and finish_stats of pna_bf16_dev.h), every
//             aggregate rounded to bf16 into the LDS tile agg[16][T][A][Fp]; the rows' own features h go to a second LDS tile
//   towers    one wavefront per (tower, 16 output columns): the tower's OWN weight blocks only (A Fp columns per scaler, Fi for the
//             self block), v_mfma_f32_16x16x32_bf16 with the A fragments from LDS and the B fragments straight from the weight image
//             (it is read once per workgroup and stays in L2); scalers, bias, graph norm and the folded BatchNorm in fp32, rounded
//             to bf16 into the LDS tile hc[16][T Fo] (or, without a mixing network, into y)
//   mixing    one wavefront per 16 output columns over hc; bias, activation, residual, rounded to bf16 into y
// No atomics, a fixed order of every sum: identical bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_bf16_dev.h"
#include "pna_rowstats.h"

namespace {

using namespace pna_bf16;

constexpr int kRows = 16;                     // destination rows per workgroup
constexpr int kLdsPad = 8;                    // elements of padding per LDS row: rows start 16 bytes further into the banks
constexpr size_t kLdsMax = 160 * 1024;

struct RArgs {
  const int32_t* rowptr; const int32_t* col; int V;
  int T, Fi, Fp, Fo, Fop, A, no_self, n_hblk;
  int aggr[PNA_MAX_AGGR];
  const u16* x; int64_t ldx; int dst_off;     // source rows; dst_off < 0: no destination term
  const int32_t* et; const u16* etab; int64_t lde; int n_et;
  const u16* h; int64_t ldh; int Khp;
  const float* rs[3];
  const u16* post; const u16* wself; int Kp;  // [T][S][Fop][Kp], [T][Fop][Khp]
  const u16* post_bias; const float* row_post; const float* cs; const float* ct;
  const u16* mix; const u16* mix_bias; int No, Nop, Kmp; float slope;
  const u16* res; int64_t ld_res;
  u16* y; int64_t ldy;
  int LA, LH, LC;                             // LDS row pitches (elements) of the three tiles
};

// acc[b] += A (16 LDS rows at `al`, pitch la) . B_b^T (16 rows of NB weight blocks `stride` elements apart at `w`, pitch kp) over kp
// columns: one A fragment per 32 columns for all blocks, their B fragments in flight together
template <int NB>
__device__ __forceinline__ void dot_tile(f4 (&acc)[NB], const u16* al, int la, const u16* w, size_t stride, int kp, int lane) {
  const int ka = 8 * (lane >> 4);
  const u16* ap = al + (lane & 15) * la + ka;
  const u16* wp = w + (size_t)(lane & 15) * kp + ka;
#pragma unroll 2
  for (int c = 0; c < kp; c += 32) {
    const bf8 A = __builtin_bit_cast(bf8, *reinterpret_cast<const u4*>(ap + c));
    bf8 B[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) B[b] = __builtin_bit_cast(bf8, *reinterpret_cast<const u4*>(wp + b * stride + c));
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B[b], acc[b], 0, 0, 0);
  }
}

template <int S, bool V8>
__global__ __launch_bounds__(kBlock) void k_tower_rows_bf16(const RArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  u16* agg = reinterpret_cast<u16*>(lds_raw);
  u16* hl = agg + kRows * a.LA;
  u16* hc = hl + kRows * a.LH;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * kRows;

  // the three tiles start as zeros: padding columns and rows beyond V take part in the MFMAs
  {
    const int n16 = kRows * (a.LA + a.LH + a.LC) / 8;
    u4* z = reinterpret_cast<u4*>(lds_raw);
    for (int i = tid; i < n16; i += kBlock) z[i] = (u4){0u, 0u, 0u, 0u};
  }
  __syncthreads();

  // ---- gather: one lane per (row, tower, 8 features)
  {
    const int G = a.Fp / 8, per_row = a.T * G, items = kRows * per_row;
    for (int it = tid; it < items; it += kBlock) {
      const int r = it / per_row, rest = it - r * per_row, t = rest / G, f0 = 8 * (rest - t * G);
      const int row = row0 + r;
      if (row >= a.V) continue;
      const int beg = a.rowptr[row], end = a.rowptr[row + 1];
      Acc c;
      acc_init(c);
      // x_src[u] + x_dst[row] + the edge type's table row: the terms are always whole 16-byte pieces
      const int c0 = t * a.Fp + f0;
      MsgTerm m;
      m.dst = a.dst_off >= 0 ? a.x + (size_t)row * a.ldx + a.dst_off + c0 : nullptr;
      m.er = a.et ? a.etab + c0 : nullptr;
      m.lde = a.lde; m.et = a.et; m.n_er = a.n_et;
      fold_edges<V8, true, true, true>(a.col, a.x + c0, a.ldx, beg, end, a.Fi - f0, m, c);
      u16* o = agg + r * a.LA + t * a.Kp + f0;                  // the A aggregator blocks of the LDS row
      finish_stats(end - beg, a.Fi - f0, c, a.A, a.aggr, [&](int ai, const u16 (&v)[8]) __attribute__((always_inline)) {
        store8(o + ai * a.Fp, v);
      });
    }
  }
  // ---- the rows' own features, one block of round32(Fi) columns per input slice
  if (!a.no_self) {
    const int per_row = a.n_hblk * a.Fi, n = kRows * per_row;
    for (int i = tid; i < n; i += kBlock) {
      const int r = i / per_row, rest = i - r * per_row, b = rest / a.Fi, f = rest - b * a.Fi;
      const int row = row0 + r;
      if (row < a.V) hl[r * a.LH + b * a.Khp + f] = a.h[(size_t)row * a.ldh + rest];
    }
  }
  __syncthreads();

  // ---- towers: one wavefront per (tower, 16 output columns)
  const int NTo = a.Fop / 16;
  for (int u = wave; u < a.T * NTo; u += kBlock / 64) {
    const int t = u / NTo, n = u - t * NTo;
    f4 acc[S], ownv[1];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = (f4){0.f, 0.f, 0.f, 0.f};
    ownv[0] = (f4){0.f, 0.f, 0.f, 0.f};
    dot_tile<S>(acc, agg + t * a.Kp, a.LA, a.post + ((size_t)t * S * a.Fop + n * 16) * a.Kp, (size_t)a.Fop * a.Kp, a.Kp, lane);
    if (!a.no_self)
      dot_tile<1>(ownv, hl + (a.n_hblk > 1 ? t : 0) * a.Khp, a.LH, a.wself + ((size_t)t * a.Fop + n * 16) * a.Khp, 0, a.Khp, lane);
    const f4 own = ownv[0];
    // C/D lane map: column lane & 15, rows 4 (lane >> 4) + i
    const int cl = n * 16 + (lane & 15), col = t * a.Fo + cl;
    if (cl < a.Fo) {
      const float bias = a.post_bias ? bf2f(a.post_bias[col]) : 0.f;
      const float cs = a.cs ? a.cs[col] : 1.f, ct = a.cs ? a.ct[col] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * (lane >> 4) + i;
        const long row = row0 + r;
        if (row >= a.V) continue;
        float z = (a.rs[0] ? a.rs[0][row] : 1.f) * acc[0][i];
#pragma unroll
        for (int s = 1; s < S; ++s) z = z + (a.rs[s] ? a.rs[s][row] : 1.f) * acc[s][i];
        z = z + own[i];
        z = z + bias;
        if (a.row_post) z = z * a.row_post[row];
        if (a.cs) z = z * cs + ct;
        if (a.mix) {
          hc[r * a.LC + col] = f2bf(z);
        } else {
          z = z < 0.f ? z * a.slope : z;
          if (a.res) z = z + bf2f(a.res[row * a.ld_res + col]);
          a.y[row * a.ldy + col] = f2bf(z);
        }
      }
    }
  }
  if (!a.mix) return;
  __syncthreads();

  // ---- mixing network: one wavefront per 16 output columns
  for (int n = wave; n < a.Nop / 16; n += kBlock / 64) {
    f4 accv[1] = {(f4){0.f, 0.f, 0.f, 0.f}};
    dot_tile<1>(accv, hc, a.LC, a.mix + (size_t)n * 16 * a.Kmp, 0, a.Kmp, lane);
    const f4 acc = accv[0];
    const int col = n * 16 + (lane & 15);
    if (col >= a.No) continue;
    const float bias = a.mix_bias ? bf2f(a.mix_bias[col]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long row = row0 + 4 * (lane >> 4) + i;
      if (row >= a.V) continue;
      float z = acc[i] + bias;
      z = z < 0.f ? z * a.slope : z;
      if (a.res) z = z + bf2f(a.res[row * a.ld_res + col]);
      a.y[row * a.ldy + col] = f2bf(z);
    }
  }
}

template <int S, bool V8>
hipError_t launch_rows(const RArgs& g, size_t lds, hipStream_t st) {
  auto* fn = k_tower_rows_bf16<S, V8>;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(fn, dim3((unsigned)((g.V + kRows - 1) / kRows)), dim3(kBlock), lds, st, g);
  return hipGetLastError();
}

template <int S>
hipError_t launch_rows_v(const RArgs& g, bool v8, size_t lds, hipStream_t st) {
  return v8 ? launch_rows<S, true>(g, lds, st) : launch_rows<S, false>(g, lds, st);
}

int round_up(int x, int m) { return (x + m - 1) / m * m; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Row pitches (bf16 elements) of the three panels of a 16-row tile: the aggregates of every tower, the rows' own features (n_hblk
// blocks: none, one, or one per tower) and, with a mixing network, the concatenated tower outputs.
struct Tile {
  int LA, LH, LC;
  size_t bytes() const { return (size_t)kRows * ((size_t)LA + LH + LC) * sizeof(u16); }
};

Tile tile_of(int T, int Fi, int Fo, int A, int n_hblk, bool mix) {
  const int Kp = round_up(A * round_up(Fi, 8), 32);
  return {T * Kp + kLdsPad, n_hblk ? n_hblk * round_up(Fi, 32) + kLdsPad : 0, mix ? round_up(T * Fo, 32) + kLdsPad : 0};
}

}  // namespace

extern "C" int64_t pna_tower_layer_bf16_lds_bytes(int32_t n_tower, int32_t Fi, int32_t Fo, int32_t n_aggr, int32_t divide_input, int32_t No,
                                                  int32_t no_self_panel) {
  if (n_tower < 1 || Fi < 1 || Fo < 1 || n_aggr < 1 || No < 0) return -1;
  return (int64_t)tile_of(n_tower, Fi, Fo, n_aggr, no_self_panel ? 0 : divide_input ? n_tower : 1, No > 0).bytes();
}

extern "C" int pna_tower_layer_bf16(const pna_tower_layer_bf16_args* p, pna_stream_t stream) {
  if (!p) return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: null args");
  if (int rc_ss = pna_check_struct_size("pna_tower_layer_bf16", p->struct_size, sizeof(*p))) return rc_ss;
  const int T = p->n_tower, Fi = p->Fi, Fo = p->Fo, S = p->n_scaler, A = p->n_aggr;
  if (p->V < 0 || T < 1 || T > 64 || Fi < 1 || Fi > 2048 || Fo < 1 || Fo > 2048 || S < 1 || S > 3 || A < 1 || A > PNA_MAX_AGGR)
    return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: need V >= 0, 1 <= n_tower <= 64, 1 <= Fi, Fo <= 2048, 1 <= n_scaler <= 3, 1 <= n_aggr <= 8");
  for (int i = 0; i < A; ++i)
    if (p->aggr[i] < PNA_AGG_MEAN || p->aggr[i] > PNA_AGG_STD_PYG)
      return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: aggregator code must be mean/sum/max/min/std/var/var_raw/std_pyg");
  const bool simple = p->no_self_panel != 0;
  if (simple && (T != 1 || p->mix_img || p->edge_type || p->divide_input))
    return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: no_self_panel is the one-tower form without mixing network and edge table");
  if (!(p->mix_slope >= 0.f && p->mix_slope <= 1.f)) return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: mix_slope must be in [0, 1]");
  if (!p->col_scale != !p->col_shift) return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: only one of col_scale / col_shift");
  if (p->mix_img && (p->No < 1 || p->No > 4096)) return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: need 1 <= No <= 4096 with mix_img");
  const int Fp = round_up(Fi, 8), Fop = round_up(Fo, 16), Kp = round_up(A * Fp, 32), Khp = round_up(Fi, 32);
  const int n_hblk = simple ? 0 : p->divide_input ? T : 1;
  const int Kin = p->divide_input ? T * Fi : Fi, width = p->mix_img ? p->No : T * Fo;
  const int Kmp = p->mix_img ? round_up(T * Fo, 32) : 0;
  const Tile tile = tile_of(T, Fi, Fo, A, n_hblk, p->mix_img != nullptr);
  RArgs g{};
  g.LA = tile.LA; g.LH = tile.LH; g.LC = tile.LC;
  const size_t lds = tile.bytes();
  if (lds > kLdsMax) return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: the 16-row tile does not fit 160 KiB of LDS");
  if (p->V == 0) return PNA_OK;
  if (!p->rowptr || !p->col || !p->h || !p->post_img || !p->y)
    return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: rowptr/col/h/post_img/y must be non-null");
  if (p->ldh < Kin || p->ldy < width || (p->residual && p->ld_res < width))
    return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: ldh / ldy / ld_res smaller than the rows they hold");
  if (!aligned16(p->post_img) || !aligned16(p->mix_img) || !aligned16(p->proj_img))
    return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: a weight image that is not 16-byte aligned");
  if (!simple && (!p->x_cat || !p->proj_img || !aligned16(p->x_cat) || p->ldx < 2 * T * Fp || p->ldx % 8 != 0))
    return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: x_cat / proj_img missing, or x_cat not 16-byte aligned rows of >= 2 T round8(Fi) columns");
  if (p->edge_type && (!p->edge_table || p->n_edge_types < 1 || p->n_edge_types > 4 || !aligned16(p->edge_table) ||
                       p->ld_edge_table < T * Fp || p->ld_edge_table % 8 != 0))
    return pna_set_error(PNA_E_INVALID, "pna_tower_layer_bf16: edge_type needs 1..4 16-byte aligned edge_table rows of >= T round8(Fi) columns");

  if (!simple) {                                               // launch 1: x_cat = bf16([W_a h | W_b h + b]) of every tower
    pna_contract_bf16_args c{};
    c.struct_size = sizeof(c);
    c.a = p->h; c.lda = p->ldh; c.M = p->V; c.K = Kin; c.N = 2 * T * Fp; c.n_scaler = 1;
    c.w_img = p->proj_img; c.bias = p->proj_bias; c.slope = 1.f;
    c.y = p->x_cat; c.ldy = p->ldx;
    if (int rc = pna_contract_bf16(&c, stream)) return rc;
  }

  g.rowptr = p->rowptr; g.col = p->col; g.V = p->V;
  g.T = T; g.Fi = Fi; g.Fp = Fp; g.Fo = Fo; g.Fop = Fop; g.A = A; g.no_self = simple; g.n_hblk = n_hblk;
  for (int i = 0; i < PNA_MAX_AGGR; ++i) g.aggr[i] = i < A ? p->aggr[i] : 0;
  bool v8 = true;
  if (simple) {
    g.x = reinterpret_cast<const u16*>(p->h); g.ldx = p->ldh; g.dst_off = -1;
    v8 = aligned16(p->h) && p->ldh % 8 == 0 && (Fi % 8 == 0 || p->h_tail_readable);
  } else {
    g.x = reinterpret_cast<const u16*>(p->x_cat); g.ldx = p->ldx; g.dst_off = T * Fp;
  }
  g.et = p->edge_type; g.etab = reinterpret_cast<const u16*>(p->edge_table); g.lde = p->ld_edge_table; g.n_et = p->n_edge_types;
  g.h = reinterpret_cast<const u16*>(p->h); g.ldh = p->ldh; g.Khp = Khp;
  for (int s = 0; s < 3; ++s) g.rs[s] = s < S ? p->row_scale[s] : nullptr;
  g.post = reinterpret_cast<const u16*>(p->post_img); g.Kp = Kp;
  g.wself = g.post + (size_t)T * S * Fop * Kp;
  g.post_bias = reinterpret_cast<const u16*>(p->post_bias);
  g.row_post = p->row_post; g.cs = p->col_scale; g.ct = p->col_shift;
  g.mix = reinterpret_cast<const u16*>(p->mix_img); g.mix_bias = reinterpret_cast<const u16*>(p->mix_bias);
  g.No = p->mix_img ? p->No : 0; g.Nop = round_up(g.No, 16); g.Kmp = Kmp; g.slope = p->mix_slope;
  g.res = reinterpret_cast<const u16*>(p->residual); g.ld_res = p->ld_res;
  g.y = reinterpret_cast<u16*>(p->y); g.ldy = p->ldy;

  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  switch (S) {
    case 1: e = launch_rows_v<1>(g, v8, lds, st); break;
    case 2: e = launch_rows_v<2>(g, v8, lds, st); break;
    default: e = launch_rows_v<3>(g, v8, lds, st); break;
  }
  if (e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  return PNA_OK;
}
