// pna_bf16_shard.hip -- bf16 inference on a shard of a destination-sharded graph for gfx950 (MI355X, CDNA4): pna_pack_rows_bf16 (the
// send-side packing of the halo all-to-all on bf16 rows) and pna_gather_rows_bf16 (the row-list, split-table member of the bf16
// gather family of pna_bf16_gather.hip).  See include/pna_amd.h for the arguments and what each entry point replaces, DESIGN.md
// 4.15 for the routes.
//
// The gather is pna_bf16_gather.hip's: 64 / G lane groups of G = ceil(F / 8) lanes per wavefront, one destination row per group, 8
// features per lane, (sum, sum of squares, max, min) in fp32 registers, hub rows as segments with fp32 partials combined in
// segment order.  Two things differ.  Lane group i reduces row rows[i] of a LIST, so that one aggregate is filled by two launches:
// the rows that read local sources only while the halo exchange is in flight, the others and the hub rows after it.  And a source
// id selects one of TWO tables: ids below n_local read the local rows, the others the halo rows, which were received into a
// buffer of their own -- a compare and a select of base and pitch per gathered edge (fold_edges<..., SPLIT> of pna_bf16_dev.h),
// no concatenated [local | halo] copy.  A call with one table runs the same kernels with n_local = INT32_MAX.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_bf16_dev.h"
#include "pna_rowstats.h"

namespace {

using namespace pna_bf16;

struct RowsArgs {
  SegArgs s;
  const u16* dst; int64_t ldd;                // the message terms (MSG kernels only)
  const u16* er; int64_t lde; int n_er;
  const int32_t* et;
  const int32_t* rows; int n_rows;            // the destination rows of the light-row launch (null: 0 .. n_rows - 1)
  const char* far; unsigned pitch_far, pitch_near; int n_local;   // the second source table (HaloTab of pna_bf16_dev.h)
};

// the in-edges [beg, end) of destination `row`, features [f0, f0 + 8)
template <bool V8, bool MSG>
__device__ __forceinline__ void fold_row(const RowsArgs& a, int row, int beg, int end, int f0, Acc& c) {
  MsgTerm t{};
  if (MSG) {
    t.dst = a.dst ? a.dst + (size_t)row * a.ldd + f0 : nullptr;
    t.er = a.er ? a.er + f0 : nullptr;
    t.lde = a.lde; t.et = a.et; t.n_er = a.n_er;
  }
  const HaloTab hb{a.far + 2 * f0, a.pitch_far, a.pitch_near, a.n_local};
  fold_edges<V8, V8, MSG, false, true>(a.s.col, a.s.x + f0, a.s.ldx, beg, end, a.s.F - f0, t, c, hb);
}

// light rows: one lane group per LISTED destination row (a listed row of the heavy schedule is skipped; an id outside [0, V) too)
template <bool V8, bool VOUT, bool MSG>
__global__ __launch_bounds__(kBlock) void k_gather_rows_bf16(RowsArgs a) {
  const int lane = threadIdx.x & 63, per_wave = 64 / a.s.G, grp = lane / a.s.G, li = lane - grp * a.s.G;
  if (grp >= per_wave) return;
  const long i = ((long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * per_wave + grp;
  const int f0 = li * 8;
  if (i >= a.n_rows) return;
  const int row = a.rows ? a.rows[i] : (int)i;
  if ((unsigned)row >= (unsigned)a.s.V) return;
  const int beg = a.s.rowptr[row], end = a.s.rowptr[row + 1], deg = end - beg;
  if (a.s.n_heavy > 0 && deg > a.s.heavy_threshold) return;
  Acc c;
  acc_init(c);
  fold_row<V8, MSG>(a, row, beg, end, f0, c);
  finish_row<VOUT>(a.s, row, deg, f0, c);
}

// heavy segments: one lane group per segment, fp32 partials.  (The table select costs up to 4 VGPRs: three instantiations sit one
// step of waves per SIMD below their whole-V counterparts; asking the compiler for the step spills.)
template <bool V8, bool MSG>
__global__ __launch_bounds__(kBlock) void k_gather_rows_bf16_seg(RowsArgs a) {
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
  fold_row<V8, MSG>(a, row, beg, end, f0, c);
  store_partials(a.s, seg, f0, c);
}

// heavy rows: the partials of a row combined in segment order, then finalized like a light row
template <bool VOUT>
__global__ __launch_bounds__(kBlock) void k_gather_rows_bf16_fin(SegArgs a) {
  const int lane = threadIdx.x & 63, per_wave = 64 / a.G, grp = lane / a.G, li = lane - grp * a.G;
  if (grp >= per_wave) return;
  const long h = ((long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * per_wave + grp;
  if (h >= a.n_heavy) return;
  finish_heavy_row<VOUT>(a, h, li * 8);
}

template <bool MSG>
hipError_t launch_rows(const RowsArgs& m, bool v8, bool vout, hipStream_t st) {
  const SegArgs& a = m.s;
  const long per_block = (long)(kBlock / 64) * (64 / a.G);
  auto blocks = [&](long n) { return dim3((unsigned)((n + per_block - 1) / per_block)); };
  if (a.n_heavy > 0) {
    if (v8) hipLaunchKernelGGL((k_gather_rows_bf16_seg<true, MSG>), blocks(a.n_seg), dim3(kBlock), 0, st, m);
    else hipLaunchKernelGGL((k_gather_rows_bf16_seg<false, MSG>), blocks(a.n_seg), dim3(kBlock), 0, st, m);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (m.n_rows > 0) {
    if (v8 && vout) hipLaunchKernelGGL((k_gather_rows_bf16<true, true, MSG>), blocks(m.n_rows), dim3(kBlock), 0, st, m);
    else if (v8) hipLaunchKernelGGL((k_gather_rows_bf16<true, false, MSG>), blocks(m.n_rows), dim3(kBlock), 0, st, m);
    else if (vout) hipLaunchKernelGGL((k_gather_rows_bf16<false, true, MSG>), blocks(m.n_rows), dim3(kBlock), 0, st, m);
    else hipLaunchKernelGGL((k_gather_rows_bf16<false, false, MSG>), blocks(m.n_rows), dim3(kBlock), 0, st, m);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (a.n_heavy > 0) {
    if (vout) hipLaunchKernelGGL((k_gather_rows_bf16_fin<true>), blocks(a.n_heavy), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((k_gather_rows_bf16_fin<false>), blocks(a.n_heavy), dim3(kBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

int fail(const char* what) {
  char msg[256];
  snprintf(msg, sizeof(msg), "pna_gather_rows_bf16: %s", what);
  return pna_set_error(PNA_E_INVALID, msg);
}

// out[i, 0:F] = x[idx[i], 0:F], out[i, F:ldo] = 0; one lane per 8 columns of the packed row, 16-byte moves.  The piece that holds
// column F - 1 of a row whose width is no multiple of 8 is read element by element: nothing beyond the F columns of a source row is touched.
__global__ __launch_bounds__(256) void k_pack_rows_bf16_v8(const u16* x, long ldx, const int32_t* idx, long n, int F, int L, u16* out, long ldo) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long row = gid / L;
  if (row >= n) return;
  const int c0 = (int)(gid - row * L) * 8;
  u4 w = {0u, 0u, 0u, 0u};
  if (c0 + 8 <= F) {
    w = *reinterpret_cast<const u4*>(x + (long)idx[row] * ldx + c0);
  } else if (c0 < F) {
    const u16* p = x + (long)idx[row] * ldx + c0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (c0 + j < F) w[j >> 1] |= (unsigned)p[j] << (16 * (j & 1));
  }
  __builtin_nontemporal_store(w, reinterpret_cast<u4*>(out + row * ldo + c0));
}

// the same with one lane per column: any alignment, any pitch
__global__ __launch_bounds__(256) void k_pack_rows_bf16_e(const u16* x, long ldx, const int32_t* idx, long n, int F, u16* out, long ldo) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long row = gid / ldo;
  if (row >= n) return;
  const int c = (int)(gid - row * ldo);
  const u16 v = c < F ? x[(long)idx[row] * ldx + c] : (u16)0;
  __builtin_nontemporal_store(v, out + row * ldo + c);
}

}  // namespace

extern "C" int pna_pack_rows_bf16(const void* x, int64_t ldx, const int32_t* idx, int64_t n, int32_t F, void* out, int64_t ldo,
                                  pna_stream_t stream) {
  if (n < 0 || F <= 0 || ldx < F || ldo < F) return pna_set_error(PNA_E_INVALID, "pna_pack_rows_bf16: bad n / F / leading dimensions");
  if (n == 0) return PNA_OK;
  if (!x || !idx || !out) return pna_set_error(PNA_E_INVALID, "pna_pack_rows_bf16: x / idx / out must be non-null");
  const bool v8 = ldx % 8 == 0 && ldo % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0;
  const long L = v8 ? ldo / 8 : ldo;
  const long blocks = ((long)n * L + 255) / 256;
  if (blocks > 0x7fffffffL) return pna_set_error(PNA_E_INVALID, "pna_pack_rows_bf16: too many rows for one launch");
  const u16* xs = reinterpret_cast<const u16*>(x);
  u16* o = reinterpret_cast<u16*>(out);
  if (v8) hipLaunchKernelGGL(k_pack_rows_bf16_v8, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, xs, (long)ldx, idx, (long)n, F, (int)L, o, (long)ldo);
  else hipLaunchKernelGGL(k_pack_rows_bf16_e, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, xs, (long)ldx, idx, (long)n, F, o, (long)ldo);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  return PNA_OK;
}

extern "C" int pna_gather_rows_bf16(const pna_gather_rows_bf16_args* p, pna_stream_t stream) {
  if (!p) return pna_set_error(PNA_E_INVALID, "pna_gather_rows_bf16: null args");
  if (int rc_ss = pna_check_struct_size("pna_gather_rows_bf16", p->struct_size, sizeof(*p))) return rc_ss;
  if (p->V < 0 || p->F <= 0 || p->F > 512) return fail("need V >= 0 and 1 <= F <= 512");
  if (p->n_rows < 0) return fail("n_rows must be >= 0");
  if (p->x_halo && p->n_local <= 0) return fail("x_halo needs n_local >= 1 (the rows of x)");
  if (p->x_halo && p->ld_halo < p->F) return fail("ld_halo smaller than F");
  if (p->ldx >= (1LL << 31) || (p->x_halo && p->ld_halo >= (1LL << 31))) return fail("ldx / ld_halo must be below 2^31 elements");
  const int n_heavy = p->n_heavy > 0 ? p->n_heavy : 0;
  const int n_rows = p->rows ? p->n_rows : p->V;
  if (p->V == 0 || (n_rows == 0 && n_heavy == 0)) return PNA_OK;
  if (!p->rowptr || !p->col || !p->x || !p->out) return fail("rowptr/col/x/out must be non-null");
  if (p->n_aggr < 1 || p->n_aggr > PNA_MAX_AGGR) return fail("n_aggr out of range");
  for (int i = 0; i < p->n_aggr; ++i)
    if (p->aggr[i] < PNA_AGG_MEAN || p->aggr[i] > PNA_AGG_STD_PYG) return fail("aggregator code must be mean/sum/max/min/std/var/var_raw/std_pyg");
  const int bs = p->block_stride > 0 ? p->block_stride : p->F;
  if (bs < p->F || p->ldx < p->F || p->ldo < (int64_t)(p->n_aggr - 1) * bs + p->F || p->ldo % 8 != 0 || ((uintptr_t)p->out & 15) != 0)
    return fail("leading dimensions too small, or out / ldo not 16-byte aligned");
  if ((p->dst_term && p->ld_dst < p->F) || (p->edge_rows && p->ld_edge < p->F)) return fail("ld_dst / ld_edge smaller than F");
  if (p->edge_type && (!p->edge_rows || p->n_edge_rows < 1)) return fail("edge_type needs edge_rows with n_edge_rows >= 1");
  if (n_heavy > 0 && (!p->heavy_rows || !p->heavy_segptr || !p->seg_heavy || !p->partials || p->n_seg <= 0 || p->seg_len <= 0 ||
                      p->heavy_threshold <= 0))
    return fail("incomplete heavy-row schedule");

  RowsArgs m{};
  SegArgs& a = m.s;
  a.rowptr = p->rowptr; a.col = p->col; a.x = reinterpret_cast<const u16*>(p->x); a.ldx = p->ldx;
  a.V = p->V; a.F = p->F; a.G = (p->F + 7) / 8; a.F8 = a.G * 8;
  a.n_aggr = p->n_aggr;
  for (int i = 0; i < PNA_MAX_AGGR; ++i) a.aggr[i] = i < p->n_aggr ? p->aggr[i] : 0;
  a.out = reinterpret_cast<u16*>(p->out); a.ldo = p->ldo; a.bs = bs;
  a.heavy_threshold = p->heavy_threshold; a.seg_len = p->seg_len;
  a.n_heavy = n_heavy; a.n_seg = n_heavy ? p->n_seg : 0;
  a.heavy_rows = p->heavy_rows; a.heavy_segptr = p->heavy_segptr; a.seg_heavy = p->seg_heavy; a.partials = p->partials;
  m.dst = reinterpret_cast<const u16*>(p->dst_term); m.ldd = p->ld_dst;
  m.er = reinterpret_cast<const u16*>(p->edge_rows); m.lde = p->ld_edge; m.n_er = p->n_edge_rows;
  m.et = p->edge_type;
  m.rows = p->rows; m.n_rows = n_rows;
  // the second table's row 0 moved back by n_local rows (HaloTab); one table: no id reaches n_local
  m.pitch_near = (unsigned)(2 * p->ldx);
  m.pitch_far = p->x_halo ? (unsigned)(2 * p->ld_halo) : m.pitch_near;
  m.n_local = p->x_halo ? p->n_local : INT32_MAX;
  m.far = p->x_halo ? reinterpret_cast<const char*>((uintptr_t)p->x_halo - (uintptr_t)p->n_local * m.pitch_far) : reinterpret_cast<const char*>(p->x);

  // 16-byte gathers: every operand -- BOTH source tables -- keeps its rows' first feature 16-byte aligned and the columns up to the next
  // multiple of 8 readable
  auto wide = [&](const void* q, int64_t ld) { return !q || (ld % 8 == 0 && ((uintptr_t)q & 15) == 0); };
  const bool v8 = wide(p->x, p->ldx) && wide(p->x_halo, p->ld_halo) && wide(p->dst_term, p->ld_dst) && wide(p->edge_rows, p->ld_edge) &&
                  (p->F % 8 == 0 || p->tails_readable);
  const bool vout = bs % 8 == 0;
  const bool msg = p->dst_term || p->edge_rows;
  const hipError_t e = msg ? launch_rows<true>(m, v8, vout, (hipStream_t)stream) : launch_rows<false>(m, v8, vout, (hipStream_t)stream);
  if (e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  return PNA_OK;
}
