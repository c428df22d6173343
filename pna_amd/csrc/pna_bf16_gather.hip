// pna_bf16_gather.hip -- the gather of the bf16 inference paths for gfx950 (MI355X, CDNA4): pna_segreduce_fwd_bf16 (gather +
// aggregator statistics of bf16 rows, fp32 accumulation, bf16 aggregate: PNASimpleLayer) and pna_gather_bf16 (the same gather with
// the destination and edge terms of the factorised pretrans added to every message in fp32: PNALayer / PNATower).  One kernel
// triple serves both: MSG = false is the plain gather.  See include/pna_amd.h for the arguments and the reference code each entry
// point replaces, DESIGN.md 4.10 and 4.11 for the layout.
//
// A wavefront is cut into 64 / G lane groups of G = ceil(F / 8) lanes; a group owns one destination row and each lane owns 8
// consecutive features, so a row is one 16-byte load per lane when the row pitch is a multiple of 8 elements (2-byte loads
// otherwise).  Every lane keeps (sum, sum of squares, max, min) of its 8 features in fp32 registers: no cross-lane reduction, no
// atomics.  With MSG a lane loads its 8 columns of the destination row once and adds them, and the edge row of every edge, to the
// gathered source row in fp32: the message is never rounded and never stored.  Hub rows are cut into the graph's heavy-row
// segments whose fp32 partials are combined in segment order by a second kernel, so results do not depend on the launch geometry.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_bf16_dev.h"
#include "pna_rowstats.h"

namespace {

using namespace pna_bf16;

struct MsgArgs {
  SegArgs s;
  const u16* dst; int64_t ldd;                // the message terms (MSG kernels only)
  const u16* er; int64_t lde; int n_er;
  const int32_t* et;
};

// the in-edges [beg, end) of destination `row`, features [f0, f0 + 8)
template <bool V8, bool MSG>
__device__ __forceinline__ void fold_row(const MsgArgs& a, int row, int beg, int end, int f0, Acc& c) {
  MsgTerm t{};
  if (MSG) {
    t.dst = a.dst ? a.dst + (size_t)row * a.ldd + f0 : nullptr;
    t.er = a.er ? a.er + f0 : nullptr;
    t.lde = a.lde; t.et = a.et; t.n_er = a.n_er;
  }
  fold_edges<V8, V8, MSG>(a.s.col, a.s.x + f0, a.s.ldx, beg, end, a.s.F - f0, t, c);
}

// light rows: one lane group per destination row (rows of the heavy schedule are skipped)
template <bool V8, bool VOUT, bool MSG>
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
  fold_row<V8, MSG>(a, (int)row, beg, end, f0, c);
  finish_row<VOUT>(a.s, (int)row, deg, f0, c);
}

// heavy segments: one lane group per segment, fp32 partials
template <bool V8, bool MSG>
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
  fold_row<V8, MSG>(a, row, beg, end, f0, c);
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

template <bool MSG>
hipError_t launch_gather(const MsgArgs& m, bool v8, bool vout, hipStream_t st) {
  const SegArgs& a = m.s;
  const long per_block = (long)(kBlock / 64) * (64 / a.G);
  auto blocks = [&](long n) { return dim3((unsigned)((n + per_block - 1) / per_block)); };
  if (a.n_heavy > 0) {
    if (v8) hipLaunchKernelGGL((k_gather_bf16_seg<true, MSG>), blocks(a.n_seg), dim3(kBlock), 0, st, m);
    else hipLaunchKernelGGL((k_gather_bf16_seg<false, MSG>), blocks(a.n_seg), dim3(kBlock), 0, st, m);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (v8 && vout) hipLaunchKernelGGL((k_gather_bf16<true, true, MSG>), blocks(a.V), dim3(kBlock), 0, st, m);
  else if (v8) hipLaunchKernelGGL((k_gather_bf16<true, false, MSG>), blocks(a.V), dim3(kBlock), 0, st, m);
  else if (vout) hipLaunchKernelGGL((k_gather_bf16<false, true, MSG>), blocks(a.V), dim3(kBlock), 0, st, m);
  else hipLaunchKernelGGL((k_gather_bf16<false, false, MSG>), blocks(a.V), dim3(kBlock), 0, st, m);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (a.n_heavy > 0) {
    if (vout) hipLaunchKernelGGL((k_gather_bf16_fin<true>), blocks(a.n_heavy), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((k_gather_bf16_fin<false>), blocks(a.n_heavy), dim3(kBlock), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

int fail(const char* who, const char* what) {
  char msg[256];
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  return pna_set_error(PNA_E_INVALID, msg);
}

// validation, kernel arguments and launches of both entry points (`who` names the one that was called); MSG kernels for msg
int run_gather(const char* who, const pna_gather_bf16_args* p, bool msg, pna_stream_t stream) {
  if (p->V < 0 || p->F <= 0 || p->F > 512) return fail(who, "need V >= 0 and 1 <= F <= 512");
  if (p->V == 0) return PNA_OK;
  if (!p->rowptr || !p->col || !p->x || !p->out) return fail(who, "rowptr/col/x/out must be non-null");
  if (p->n_aggr < 1 || p->n_aggr > PNA_MAX_AGGR) return fail(who, "n_aggr out of range");
  for (int i = 0; i < p->n_aggr; ++i)
    if (p->aggr[i] < PNA_AGG_MEAN || p->aggr[i] > PNA_AGG_STD_PYG) return fail(who, "aggregator code must be mean/sum/max/min/std/var/var_raw/std_pyg");
  const int bs = p->block_stride > 0 ? p->block_stride : p->F;
  if (bs < p->F || p->ldx < p->F || p->ldo < (int64_t)(p->n_aggr - 1) * bs + p->F || p->ldo % 8 != 0 || ((uintptr_t)p->out & 15) != 0)
    return fail(who, "leading dimensions too small, or out / ldo not 16-byte aligned");
  if ((p->dst_term && p->ld_dst < p->F) || (p->edge_rows && p->ld_edge < p->F)) return fail(who, "ld_dst / ld_edge smaller than F");
  if (p->edge_type && (!p->edge_rows || p->n_edge_rows < 1)) return fail(who, "edge_type needs edge_rows with n_edge_rows >= 1");
  if (p->n_heavy > 0 && (!p->heavy_rows || !p->heavy_segptr || !p->seg_heavy || !p->partials || p->n_seg <= 0 || p->seg_len <= 0 ||
                         p->heavy_threshold <= 0))
    return fail(who, "incomplete heavy-row schedule");

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
  const hipError_t e = msg ? launch_gather<true>(m, v8, vout, (hipStream_t)stream) : launch_gather<false>(m, v8, vout, (hipStream_t)stream);
  if (e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  return PNA_OK;
}

}  // namespace

extern "C" int64_t pna_segreduce_bf16_partials_bytes(int32_t n_seg, int32_t F) {
  if (n_seg <= 0 || F <= 0) return 0;
  return (int64_t)n_seg * 4 * ((F + 7) / 8 * 8) * (int64_t)sizeof(float);
}

extern "C" int pna_segreduce_fwd_bf16(const pna_segreduce_bf16_args* p, pna_stream_t stream) {
  if (!p) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_bf16: null args");
  if (int rc_ss = pna_check_struct_size("pna_segreduce_fwd_bf16", p->struct_size, sizeof(*p))) return rc_ss;
  pna_gather_bf16_args g{};                                     // the message gather's arguments without terms
  g.rowptr = p->rowptr; g.col = p->col; g.V = p->V; g.F = p->F;
  g.x = p->x; g.ldx = p->ldx; g.tails_readable = p->x_tail_readable;
  g.n_aggr = p->n_aggr; g.block_stride = p->block_stride;
  for (int i = 0; i < PNA_MAX_AGGR; ++i) g.aggr[i] = p->aggr[i];
  g.out = p->out; g.ldo = p->ldo;
  g.heavy_threshold = p->heavy_threshold; g.seg_len = p->seg_len; g.n_heavy = p->n_heavy; g.n_seg = p->n_seg;
  g.heavy_rows = p->heavy_rows; g.heavy_segptr = p->heavy_segptr; g.seg_heavy = p->seg_heavy; g.partials = p->partials;
  return run_gather("pna_segreduce_fwd_bf16", &g, false, stream);
}

extern "C" int pna_gather_bf16(const pna_gather_bf16_args* p, pna_stream_t stream) {
  if (!p) return pna_set_error(PNA_E_INVALID, "pna_gather_bf16: null args");
  if (int rc_ss = pna_check_struct_size("pna_gather_bf16", p->struct_size, sizeof(*p))) return rc_ss;
  return run_gather("pna_gather_bf16", p, true, stream);
}
