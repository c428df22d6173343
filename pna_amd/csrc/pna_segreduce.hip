// pna_segreduce.hip -- fused gather + {mean,sum,max,min,std,var} segment-reduce + degree scalers
// for gfx950 (MI355X, CDNA4).  Implements pna_segreduce_fwd_f32 / pna_degree_scalers_f32 of
// include/pna_amd.h; see that header for the reference code each entry point replaces.
//
// Execution model (DESIGN.md "segment-reduce kernel"):
//   * a 64-lane wavefront is cut into G = 64/L lane groups; one group owns one destination row
//     at a time and each of its L lanes owns VEC (=4) consecutive features, so a row gather is one
//     global_load_dwordx4 per lane and no cross-lane reduction is ever needed: every lane keeps
//     its own (sum, sum of squares, max, min) in registers for its features;
//   * the source ids of a row are fetched L at a time by the group's lanes (one coalesced load) and
//     broadcast with ds_bpermute, then U gathers are issued back to back before the first is used
//     (memory-level parallelism is what bounds this kernel, not VALU);
//   * features that do not fill the last dwordx4 are handled by sliding the last lane's window back
//     to [F-4, F): the overlap recomputes identical values, so no padding of x or out is required
//     and any 4-byte aligned leading dimension works;
//   * rows with more than `heavy_threshold` in-edges are cut into fixed segments that other lane
//     groups reduce in parallel (blocks at the front of the grid, so the long poles start first);
//     a second tiny kernel folds the per-segment partials in segment order => results are
//     independent of the launch geometry.
// All arithmetic is fp32 without FMA contraction (-ffp-contract=off), mirroring the op-by-op
// rounding of the reference's torch code (x*x rounded, then summed; mean*mean rounded, then
// subtracted).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_rowstats.h"
#include "pna_scalers_dev.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) f4u { f4 v; };   // dwordx4 at 4-byte alignment
typedef int i4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) i4u { i4 v; };

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kNQ = 7;   // partial quantities per heavy segment: s, q, mx, mn, amx, amn, wsum

// Bench-experiment knobs (tune.reserved[0]: bit0 = skip the output stores, bits 8.. = KB of dummy dynamic LDS per block to
// cap the blocks per CU) exist only in the separate experiments build (-DPNA_AMD_EXPERIMENTS, tools/build_experiments.sh);
// the shipped library ignores tune.reserved[0].
#ifdef PNA_AMD_EXPERIMENTS
#define PNA_STORES_ON(a, probe) (!(((a).dbg & 1) && (probe) != 12345.678f))
#define PNA_DBG_WORD(t) ((t).reserved[0])
#else
#define PNA_STORES_ON(a, probe) true
#define PNA_DBG_WORD(t) 0
#endif

struct KArgs {
  const int32_t* rowptr; const int32_t* col;
  const float* x; const float* dst_term; const float* edge_term; const float* ew;
  const int32_t* etype;       // nullable: edge_term has one row per edge TYPE, the term of CSR edge k is row etype[k]
  const float* row_scale[PNA_MAX_SCALER];
  float* out; int32_t* argmax; int32_t* argmin;
  const int32_t* heavy_rows; const int32_t* heavy_segptr; const int32_t* seg_heavy; float* partials;
  const int32_t* heavy_out;   // nullable: output row of heavy row i (pna_segreduce_args.heavy_out_rows), else the row itself
  long ldx, ld_dst, ld_edge, ldo, ld_arg, ts_in, ts_out;
  int V, F, n_aggr, n_scaler, block_stride;
  int aggr[PNA_MAX_AGGR];
  int heavy_threshold, seg_len, n_heavy, n_seg;
  int L, G, R, n_heavy_blocks, pstride, nt, T, tiles, pf, dbg;
};

template <int VEC> struct Ld;
template <> struct Ld<4> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
    f4 t = reinterpret_cast<const f4u*>(p)->v;
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&v)[4], bool nt) {
    f4 t = {v[0], v[1], v[2], v[3]};
    typedef f4 f4a4 __attribute__((aligned(4)));
    if (nt) __builtin_nontemporal_store(t, reinterpret_cast<f4a4*>(p));
    else reinterpret_cast<f4u*>(p)->v = t;
  }
  static __device__ __forceinline__ void store_i(int32_t* p, const int (&v)[4]) {
    i4 t = {v[0], v[1], v[2], v[3]};
    reinterpret_cast<i4u*>(p)->v = t;
  }
};
template <> struct Ld<1> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[1]) { v[0] = *p; }
  static __device__ __forceinline__ void store(float* p, const float (&v)[1], bool nt) {
    if (nt) __builtin_nontemporal_store(v[0], p); else *p = v[0];
  }
  static __device__ __forceinline__ void store_i(int32_t* p, const int (&v)[1]) { *p = v[0]; }
};

template <int VEC, bool EXTRA> struct Acc {
  float s[VEC], q[VEC], mx[VEC], mn[VEC];
  int amx[VEC], amn[VEC];   // only live when EXTRA (dead-code eliminated otherwise)
  float wsum;
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int k = 0; k < VEC; ++k) { s[k] = 0.f; q[k] = 0.f; mx[k] = -INFINITY; mn[k] = INFINITY; }
#pragma unroll
    for (int k = 0; k < VEC; ++k) { amx[k] = -1; amn[k] = -1; }
    wsum = 0.f;
  }
};

using pna_dev::div_rn;   // (pna_rowstats.h: the correctly rounded s / D, single-instruction max / min)
using pna_dev::vmax;
using pna_dev::vmin;

// One message m (already gathered) of CSR edge position e folded into the accumulators.
template <int VEC, bool EXTRA>
__device__ __forceinline__ void fold(Acc<VEC, EXTRA>& a, const float (&m)[VEC], int e, float w, bool has_w) {
  if constexpr (!EXTRA) {
    // Hot path: 14 VALU per dwordx4 (2 pk_add, 2 pk_mul, 2 pk_add, 4 v_max, 4 v_min).  v_max/v_min drop
    // NaN operands; torch.max/min propagate them, so NaN is restored at the end of the row from the sum
    // of squares (q is NaN iff some message is NaN: its terms are >= 0, so inf never cancels) -- see nan_fix().
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float v = m[k];
      a.s[k] = a.s[k] + v;
      a.q[k] = a.q[k] + v * v;
      a.mx[k] = vmax(a.mx[k], v);
      a.mn[k] = vmin(a.mn[k], v);
    }
  } else {
    const bool on = !has_w || w > 0.f;                     // max/min: adjacency is a mask (A.5)
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float v = m[k];
      if (has_w) {
        a.s[k] = a.s[k] + v * w;                           // torch.mul(X, adj) then sum
        a.q[k] = a.q[k] + (v * v) * w;                     // torch.mul(torch.mul(X, X), adj)
      } else {
        a.s[k] = a.s[k] + v;
        a.q[k] = a.q[k] + v * v;
      }
      const bool gx = on && (v > a.mx[k] || (v != v && a.mx[k] == a.mx[k]));
      const bool gn = on && (v < a.mn[k] || (v != v && a.mn[k] == a.mn[k]));
      a.mx[k] = gx ? v : a.mx[k]; a.amx[k] = gx ? e : a.amx[k];
      a.mn[k] = gn ? v : a.mn[k]; a.amn[k] = gn ? e : a.amn[k];
    }
    a.wsum = a.wsum + (has_w ? w : 1.f);
  }
}

// B consecutive edges [e0, e0+B) of one row: issue every gather first, then fold in edge order.
// PARTIAL: only the first `nvalid` (1 <= nvalid < B) edges exist; the other slots re-load the last valid
// edge (same cache lines, so no extra memory traffic and -- unlike loads under a branch -- all B loads
// still issue back to back) and are not folded.
template <int VEC, int B, bool EXTRA, bool PARTIAL, bool IDX32>
__device__ __forceinline__ void batch(const KArgs& a, Acc<VEC, EXTRA>& acc, int myidx, int src_lane0, int e0,
                                      long off, const float (&dterm)[VEC], int nvalid, bool gather) {
  int id[B];
  int ee[B];
  float v[B][VEC];
#pragma unroll
  for (int u = 0; u < B; ++u) {
    const int uu = PARTIAL ? min(u, nvalid - 1) : u;
    ee[u] = e0 + uu;
    id[u] = __shfl(myidx, src_lane0 + uu);          // (edge-resident x: myidx already holds cb + lane)
  }
  (void)gather;
  if constexpr (IDX32) {
    // feature table < 4 GiB: 32-bit byte offsets against the wave-uniform base (global_load ... v_off, s[base])
    const unsigned ldb = (unsigned)a.ldx * 4u, offb = (unsigned)off * 4u;
#pragma unroll
    for (int u = 0; u < B; ++u)
      Ld<VEC>::load(reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.x) + ((unsigned)id[u] * ldb + offb)), v[u]);
  } else {
#pragma unroll
    for (int u = 0; u < B; ++u) Ld<VEC>::load(a.x + (size_t)id[u] * a.ldx + off, v[u]);
  }
  if constexpr (!EXTRA) {
#pragma unroll
    for (int u = 0; u < B; ++u) {
      if constexpr (PARTIAL) {
        // Branch-free tail: an empty slot holds a copy of the last valid edge.  Folding that copy into
        // max/min is idempotent; for sum / sum-of-squares it is replaced by +0 (v*v of 0 is 0).
        const bool on = u < nvalid;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float vm = on ? v[u][k] : 0.f;
          acc.s[k] = acc.s[k] + vm;
          acc.q[k] = acc.q[k] + vm * vm;
          acc.mx[k] = vmax(acc.mx[k], v[u][k]);
          acc.mn[k] = vmin(acc.mn[k], v[u][k]);
        }
      } else {
        fold<VEC, false>(acc, v[u], ee[u], 1.f, false);
      }
    }
  } else {
    float et[B][VEC];
    float w[B];
    if (a.edge_term) {
#pragma unroll
      for (int u = 0; u < B; ++u) Ld<VEC>::load(a.edge_term + (size_t)(a.etype ? a.etype[ee[u]] : ee[u]) * a.ld_edge + off, et[u]);
    }
    if (a.ew) {
#pragma unroll
      for (int u = 0; u < B; ++u) w[u] = a.ew[ee[u]];
    }
#pragma unroll
    for (int u = 0; u < B; ++u) {
      if (PARTIAL && u >= nvalid) continue;
      float m[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        m[k] = v[u][k];
        if (a.dst_term) m[k] = m[k] + dterm[k];
        if (a.edge_term) m[k] = m[k] + et[u][k];
      }
      fold<VEC, true>(acc, m, ee[u], a.ew ? w[u] : 1.f, a.ew != nullptr);
    }
  }
}

// All lanes of a group walk CSR positions [beg, end) of destination `row`.  `pref` holds the row's first
// L source ids (lane c: col[beg + c]) when `have_pref` -- fetched one row ahead by the caller.
template <int VEC, int U, bool EXTRA, bool IDX32>
__device__ __forceinline__ void walk(const KArgs& a, Acc<VEC, EXTRA>& acc, int row, int beg, int end, int c,
                                     int grp_lane0, long off, int pref, bool have_pref) {
  float dterm[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) dterm[k] = 0.f;
  if (EXTRA && a.dst_term && end > beg) Ld<VEC>::load(a.dst_term + (size_t)row * a.ld_dst + off, dterm);
  const int L = a.L;
  for (int cb = beg; cb < end; cb += L) {
    const int nidx = min(L, end - cb);
    int myidx = pref;
    if (!(have_pref && cb == beg)) {
      myidx = cb + c;                                   // edge-resident x: message row = CSR position
      if (a.col) myidx = c < nidx ? a.col[cb + c] : 0;
    }
    int j = 0;
    for (; j + U <= nidx; j += U) batch<VEC, U, EXTRA, false, IDX32>(a, acc, myidx, grp_lane0 + j, cb + j, off, dterm, U, true);
    if (j < nidx) batch<VEC, U, EXTRA, true, IDX32>(a, acc, myidx, grp_lane0 + j, cb + j, off, dterm, nidx - j, true);
  }
}

// mean/std/... from the raw accumulators, times the row scalers, written in the reference's
// scaler-major / aggregator-minor block order.
template <int VEC, bool EXTRA>
__device__ __forceinline__ void finalize_store(const KArgs& a, const Acc<VEC, EXTRA>& acc, int row, int deg,
                                               long offi, long offo, int orow = -1) {
  if (orow < 0) orow = row;                                // (orow: where the row's aggregate goes when the caller re-orders rows)
  float mean[VEC], var[VEC], vraw[VEC], sd[VEC], mx[VEC], mn[VEC];
  const bool empty = deg <= 0;
  const float D = (EXTRA && a.ew) ? acc.wsum : (float)deg;
  // one IEEE division per row, then s / D and q / D correctly rounded from it (div_rn): the reference's formula bit for bit
  const float invD = 1.0f / D;
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    mean[k] = div_rn(acc.s[k], D, invD);
    const float msq = div_rn(acc.q[k], D, invD);
    const float t = msq - mean[k] * mean[k];
    vraw[k] = t;
    var[k] = (t < 0.f) ? 0.f : t;                         // relu (keeps NaN)
    sd[k] = sqrtf(var[k] + 1e-5f);
    // the fast fold's v_max/v_min ignore NaN; q != q <=> the row holds a NaN message (torch propagates it)
    const bool has_nan = !EXTRA && acc.q[k] != acc.q[k];
    mx[k] = has_nan ? acc.q[k] : acc.mx[k];
    mn[k] = has_nan ? acc.q[k] : acc.mn[k];
  }
  for (int s = 0; s < a.n_scaler; ++s) {
    const float sc = a.row_scale[s] ? a.row_scale[s][row] : 1.f;
    for (int i = 0; i < a.n_aggr; ++i) {
      float o[VEC];
      const int code = a.aggr[i];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float v;
        switch (code) {
          case PNA_AGG_MEAN: v = mean[k]; break;
          case PNA_AGG_SUM: v = acc.s[k]; break;
          case PNA_AGG_MAX: v = mx[k]; break;
          case PNA_AGG_MIN: v = mn[k]; break;
          case PNA_AGG_STD: v = sd[k]; break;
          case PNA_AGG_VAR_RAW: v = vraw[k]; break;
          default: v = var[k]; break;
        }
        o[k] = empty ? 0.f : v * sc;
      }
      Ld<VEC>::store(a.out + (size_t)orow * a.ldo + (size_t)(s * a.n_aggr + i) * a.block_stride + offo, o, a.nt != 0);
    }
  }
  if constexpr (EXTRA) {                                   // (re-ordered rows: the arg indices go where the aggregate goes)
    if (a.argmax) Ld<VEC>::store_i(a.argmax + (size_t)orow * a.ld_arg + offi, acc.amx);
    if (a.argmin) Ld<VEC>::store_i(a.argmin + (size_t)orow * a.ld_arg + offi, acc.amn);
  }
}

template <int VEC, int U, bool EXTRA, bool IDX32>
__global__ __launch_bounds__(kBlock) void k_segreduce(const KArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int L = a.L;
  const int grp = lane / L;
  if (grp >= a.G) return;                                  // spare lanes of the wavefront
  const int c = lane - grp * L;
  const int grp_lane0 = grp * L;
  const int nchunks = (a.F + VEC - 1) / VEC;
  const int tower = blockIdx.y / a.tiles;                  // independent feature slice (PNA tower)
  const int chunk = (blockIdx.y - tower * a.tiles) * L + c;
  const bool lane_ok = chunk < nchunks;
  int off = min(chunk, nchunks - 1) * VEC;
  if (VEC == 4) off = min(off, a.F - 4);                   // slide the last window back inside the row
  const long offi = (long)tower * a.ts_in + off;           // column in x / dst_term / edge_term / arg*
  const long offo = (long)tower * a.ts_out + off;          // column in out (before the block offset)
  const int NG = kWaves * a.G;
  const int gid = wave * a.G + grp;

  Acc<VEC, EXTRA> acc;
  if ((int)blockIdx.x < a.n_heavy_blocks) {
    // ---- heavy segments: one lane group per segment, raw partials to the workspace -------------
    const int seg = blockIdx.x * NG + gid;
    if (seg >= a.n_seg) return;
    const int hi = a.seg_heavy[seg];
    const int row = a.heavy_rows[hi];
    const int sidx = seg - a.heavy_segptr[hi];
    const int rbeg = a.rowptr[row], rend = a.rowptr[row + 1];
    const int beg = rbeg + sidx * a.seg_len;
    const int end = min(beg + a.seg_len, rend);
    acc.init();
    walk<VEC, U, EXTRA, IDX32>(a, acc, row, beg, end, c, grp_lane0, offi, 0, false);
    if (lane_ok) {
      float* p = a.partials + ((size_t)seg * a.T + tower) * kNQ * a.pstride + off;
      Ld<VEC>::store(p, acc.s, false);
      Ld<VEC>::store(p + a.pstride, acc.q, false);
      Ld<VEC>::store(p + 2 * a.pstride, acc.mx, false);
      Ld<VEC>::store(p + 3 * a.pstride, acc.mn, false);
      if constexpr (EXTRA) {
        Ld<VEC>::store_i(reinterpret_cast<int32_t*>(p + 4 * a.pstride), acc.amx);
        Ld<VEC>::store_i(reinterpret_cast<int32_t*>(p + 5 * a.pstride), acc.amn);
        if (chunk == 0) p[6 * a.pstride - off] = acc.wsum;
      }
    }
    return;
  }
  // ---- ordinary rows: R rows per lane group, interleaved across the block's groups -------------
  // Software pipeline across rows: while row k is being gathered, the first L source ids of row k+1
  // and the rowptr pair of row k+2 are already in flight, so the dependent chain per row is just its
  // gathers (rowptr -> col -> x would otherwise be three serial memory latencies for ~10 edges).
  const long base = (long)(blockIdx.x - a.n_heavy_blocks) * NG * a.R + gid;
  const int thr = a.heavy_threshold;
  const bool pf = a.pf != 0 && a.col != nullptr;
  if (base >= a.V) return;
  int beg_c = a.rowptr[base], end_c = a.rowptr[base + 1];
  int idx_c = 0;
  {
    const int d = end_c - beg_c;
    if (pf && c < d && !(thr > 0 && d > thr)) idx_c = a.col[beg_c + c];
  }
  int beg_n = 0, end_n = 0;
  if (a.R > 1 && base + NG < a.V) { beg_n = a.rowptr[base + NG]; end_n = a.rowptr[base + NG + 1]; }
  for (int r = 0; r < a.R; ++r) {
    const long row_l = base + (long)r * NG;
    if (row_l >= a.V) break;
    const int row = (int)row_l;
    // prefetch for the rows to come (issued before this row's gathers)
    int idx_n = 0, beg_nn = 0, end_nn = 0;
    const bool vn = r + 1 < a.R && row_l + NG < a.V;
    if (vn && pf) {
      const int dn = end_n - beg_n;
      if (c < dn && !(thr > 0 && dn > thr)) idx_n = a.col[beg_n + c];
    }
    if (r + 2 < a.R && row_l + 2 * NG < a.V) { beg_nn = a.rowptr[row_l + 2 * NG]; end_nn = a.rowptr[row_l + 2 * NG + 1]; }
    const int deg = end_c - beg_c;
    if (!(thr > 0 && deg > thr)) {                           // heavy rows are done by the segment blocks
      acc.init();
      walk<VEC, U, EXTRA, IDX32>(a, acc, row, beg_c, end_c, c, grp_lane0, offi, idx_c, pf);
      if (lane_ok && PNA_STORES_ON(a, acc.s[0])) finalize_store<VEC, EXTRA>(a, acc, row, deg, offi, offo);
    }
    idx_c = idx_n; beg_c = beg_n; end_c = end_n; beg_n = beg_nn; end_n = end_nn;
  }
}

// ================================================================================================
// Hand-scheduled hot path: VEC = 4, plain gather (col != NULL, no dst/edge terms, weights or arg
// outputs), feature table < 4 GiB and < 2^24 rows (32-bit byte offsets, v_mad_u32_u24 addressing).
//
// hipcc's own s_waitcnt placement cannot know that the prefetched source ids / rowptr pair of the
// NEXT row have landed (they were issued before the current row's gathers, and VMEM returns in
// order), so it drains the queue -- including the previous row's output stores -- with vmcnt(0)
// before every first ds_bpermute.  Here every load of the row loop is issued through inline asm and
// waited for with counted s_waitcnt, so that per row the wave only ever waits on its gathers, with
// the previous row's store acknowledgements and the next rows' prefetches in flight underneath.
// Rules kept (cdna_hip_programming.md 5.7): an asm-loaded register is only consumed through the
// "+v" operand of the asm statement that waits for it (or anchors it), so the compiler can neither
// hoist a use above the wait nor recycle the register early.
// ================================================================================================
typedef int i2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void aload32(int& dst, const void* base, unsigned voff) {
  asm volatile("global_load_dword %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(base) : "memory");
}
__device__ __forceinline__ void aload64(i2& dst, const void* base, unsigned voff) {
  asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(base) : "memory");
}
__device__ __forceinline__ void aload128(f4& dst, const void* base, unsigned voff) {
  asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(base) : "memory");
}
// 64-bit lane address (round 4: source tables >= 4 GiB / >= 2^24 rows -- a shard's [local | halo] table at BASELINE configs[4] x 8)
__device__ __forceinline__ void aload128x(f4& dst, const char* p) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
// The same behind five wait states ("VALU writes SGPR -> VMEM reads that SGPR": hipcc reloads a spilled base pointer with
// v_readlane_b32 directly in front of an inline-asm load and does not insert the s_nop itself -- pna_fused_degree.hip has the
// story; tools/isa_audit.py::sgpr_hazards checks every kernel).  For the once-per-item loads of the instantiations whose
// argument block no longer fits the scalar registers (ARG).
template <bool WS> __device__ __forceinline__ void aload32w(int& dst, const void* base, unsigned voff) {
  if constexpr (WS) asm volatile("s_nop 4\n\tglobal_load_dword %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(base) : "memory");
  else aload32(dst, base, voff);
}
template <bool WS> __device__ __forceinline__ void aload128w(f4& dst, const void* base, unsigned voff) {
  if constexpr (WS) asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(base) : "memory");
  else aload128(dst, base, voff);
}
template <int N> __device__ __forceinline__ void await(f4& v) {
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v) : "n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void await(int& v) {
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v) : "n"(N) : "memory");
}

struct AccF {   // fast-path accumulators of one lane: 4 features
  f4 s, q, mx, mn;
  __device__ __forceinline__ void init() {
    s = (f4){0.f, 0.f, 0.f, 0.f}; q = s;
    mx = (f4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    mn = (f4){INFINITY, INFINITY, INFINITY, INFINITY};
  }
  __device__ __forceinline__ void fold(const f4 v) {
    s = s + v;
    q = q + v * v;
    mx.x = vmax(mx.x, v.x); mx.y = vmax(mx.y, v.y); mx.z = vmax(mx.z, v.z); mx.w = vmax(mx.w, v.w);
    mn.x = vmin(mn.x, v.x); mn.y = vmin(mn.y, v.y); mn.z = vmin(mn.z, v.z); mn.w = vmin(mn.w, v.w);
  }
  __device__ __forceinline__ void fold_masked(const f4 v, bool on) {   // empty slot = copy of a folded edge
    const f4 z = (f4){0.f, 0.f, 0.f, 0.f};
    const f4 vm = on ? v : z;
    s = s + vm;
    q = q + vm * vm;
    mx.x = vmax(mx.x, v.x); mx.y = vmax(mx.y, v.y); mx.z = vmax(mx.z, v.z); mx.w = vmax(mx.w, v.w);
    mn.x = vmin(mn.x, v.x); mn.y = vmin(mn.y, v.y); mn.z = vmin(mn.z, v.z); mn.w = vmin(mn.w, v.w);
  }
};

// ARG kernels (training: the backward routes the max / min gradients through these): the CSR position of the edge that set the
// running max / min, with k_segreduce's fold -- strict comparison, so the FIRST extremal edge in edge order wins and a copy of an
// already folded edge never does; NaN is sticky in value and position (torch.max / min semantics).
struct ArgF {
  i4 amx, amn;
  __device__ __forceinline__ void init() { amx = (i4){-1, -1, -1, -1}; amn = amx; }
};
#define PNA_FOLD_ARG1(mx, mn, amx, amn, v, e)                          \
  {                                                                   \
    const bool gx_ = (v) > (mx) || ((v) != (v) && (mx) == (mx));     \
    const bool gn_ = (v) < (mn) || ((v) != (v) && (mn) == (mn));     \
    mx = gx_ ? (v) : (mx); amx = gx_ ? (e) : (amx);                   \
    mn = gn_ ? (v) : (mn); amn = gn_ ? (e) : (amn);                   \
  }
__device__ __forceinline__ void fold_arg(AccF& acc, ArgF& ag, const f4 v, bool on, int e) {
  const f4 z = (f4){0.f, 0.f, 0.f, 0.f};
  const f4 vm = on ? v : z;
  acc.s = acc.s + vm;
  acc.q = acc.q + vm * vm;
  if (on) {                                                  // (wave-divergent only in a row's last, partial batch)
    PNA_FOLD_ARG1(acc.mx.x, acc.mn.x, ag.amx.x, ag.amn.x, v.x, e) PNA_FOLD_ARG1(acc.mx.y, acc.mn.y, ag.amx.y, ag.amn.y, v.y, e)
    PNA_FOLD_ARG1(acc.mx.z, acc.mn.z, ag.amx.z, ag.amn.z, v.z, e) PNA_FOLD_ARG1(acc.mx.w, acc.mn.w, ag.amx.w, ag.amn.w, v.w, e)
  }
}

// ET (the tower layers WITH edge features, models/dgl/pna_layer.py:35-40: the W_e . ef part of the factorised pretrans):
//   1: one more 16-byte load per edge and lane from the per-edge term (rows in CSR order: a stream), issued right behind the
//      edge's gather, so edge I is complete once 2 (U - 1 - I) younger loads remain;
//   2: the term is a row of a table of <= 4 edge TYPES (bond types: the term of an embedding) held in 16 registers per lane; the
//      types of a row's edges are fetched like its source ids.
// The message is formed in k_segreduce's order, (x[src] + dst_term[row]) + edge_term[k]: the same bits.
struct EtF {
  f4 tab[4];                                                 // ET == 2: the lane's 4 features of every type's term
};
__device__ __forceinline__ f4 et_select(const EtF& t, int ty) {
  return ty == 0 ? t.tab[0] : ty == 1 ? t.tab[1] : ty == 2 ? t.tab[2] : t.tab[3];
}
template <int N> __device__ __forceinline__ void await2(f4& v, f4& w) {
  asm volatile("s_waitcnt vmcnt(%2)" : "+v"(v), "+v"(w) : "n"(N) : "memory");
}

template <int I, int U, bool DST, bool ARG, int ET> struct Drain {   // wait for gather I of U (U-1-I younger ones may stay in flight), fold it
  static __device__ __forceinline__ void run(AccF& acc, ArgF& ag, f4 (&v)[U], f4 (&w)[U], const int (&ty)[U], const EtF& tb,
                                             int nvalid, bool partial, const f4 dt, int e0) {
    if constexpr (ET == 1) await2<2 * (U - 1 - I)>(v[I], w[I]);
    else await<U - 1 - I>(v[I]);
    f4 m = DST ? v[I] + dt : v[I];                           // message = x[src] (+ dst_term[row]), as k_segreduce forms it
    if constexpr (ET == 1) m = m + w[I];
    if constexpr (ET == 2) m = m + et_select(tb, ty[I]);
    if constexpr (ARG) fold_arg(acc, ag, m, !partial || I < nvalid, e0 + I);
    else if (partial) acc.fold_masked(m, I < nvalid); else acc.fold(m);
    Drain<I + 1, U, DST, ARG, ET>::run(acc, ag, v, w, ty, tb, nvalid, partial, dt, e0);
  }
};
template <int U, bool DST, bool ARG, int ET> struct Drain<U, U, DST, ARG, ET> {
  static __device__ __forceinline__ void run(AccF&, ArgF&, f4 (&)[U], f4 (&)[U], const int (&)[U], const EtF&, int, bool, const f4, int) {}
};

// Slim argument block of the hand-scheduled kernel.  Everything the row loop touches fits in ~40 SGPRs; the full
// KArgs (scaler pointers, aggregator codes, heavy-row arrays) made hipcc spill SGPRs into VGPR lanes, which cost
// two waves per SIMD.  The kernel is therefore specialised to the configuration the layers issue -- aggregators
// (mean, max, min, std), identity scaler only (the degree scalers are applied in the posttrans epilogue) -- and
// everything else goes through the compiler-scheduled k_segreduce.
struct FArgs {
  const int32_t* items;   // [n_items][4] = {row, beg, end, slot}: slot < 0 -> whole row (finalise + store),
                          //                 slot >= 0 -> heavy segment: raw partials to partials[slot]
  const int32_t* col; const float* x; float* out; float* partials;
  const float* dst;       // per-destination additive term (the h_dst half of a factorised pretrans), DST kernels only
  const int32_t* orow;    // OROW kernels: output row of node v's aggregate (pna_segreduce_args.out_row_of)
  int32_t* argmax; int32_t* argmin; long ld_arg, ts_arg;     // ARG kernels: CSR position of the extremal edge per (row, feature)
  const float* et; const int32_t* etype; unsigned lde_b; int n_types;   // ET kernels: per-edge term (1) / per-type table + types (2)
  long ldo, ts_out;
  unsigned ldb, ts_in_b;  // x row pitch / tower stride in bytes
  unsigned ldd_b;         // dst_term row pitch in bytes
  int n_items, n_edges, F, L, G, R, T, tiles, pstride, block_stride, nt, dbg;
};

// mean | max | min | std blocks of one destination row (identity scaler), 4 features per lane.
__device__ __forceinline__ void fast_finalize_store(const FArgs& a, const AccF& acc, int row, int deg, long offo) {
  float* const orow = a.out + (size_t)row * a.ldo + offo;
  const unsigned bs = (unsigned)a.block_stride;
  const bool nt = a.nt != 0;
  typedef f4 f4a4 __attribute__((aligned(4)));
  auto put = [&](unsigned blk, const f4 v) {
    f4a4* p = reinterpret_cast<f4a4*>(orow + blk * bs);
    if (nt) __builtin_nontemporal_store(v, p); else *p = v;
  };
  if (deg <= 0) {                                          // no in-edges: every block is 0
    const f4 z = (f4){0.f, 0.f, 0.f, 0.f};
    put(0, z); put(1, z); put(2, z); put(3, z);
    return;
  }
  const float D = (float)deg, invD = 1.0f / D;             // one IEEE division per row (see finalize_store / div_rn)
  const f4 mean = (f4){div_rn(acc.s.x, D, invD), div_rn(acc.s.y, D, invD), div_rn(acc.s.z, D, invD), div_rn(acc.s.w, D, invD)};
  const f4 msq = (f4){div_rn(acc.q.x, D, invD), div_rn(acc.q.y, D, invD), div_rn(acc.q.z, D, invD), div_rn(acc.q.w, D, invD)};
  f4 var = msq - mean * mean;
  var.x = var.x < 0.f ? 0.f : var.x; var.y = var.y < 0.f ? 0.f : var.y;
  var.z = var.z < 0.f ? 0.f : var.z; var.w = var.w < 0.f ? 0.f : var.w;
  // v_max/v_min drop NaN; q is NaN iff the row holds a NaN message (torch propagates it)
  f4 mx, mn, sd;
  mx.x = acc.q.x != acc.q.x ? acc.q.x : acc.mx.x; mx.y = acc.q.y != acc.q.y ? acc.q.y : acc.mx.y;
  mx.z = acc.q.z != acc.q.z ? acc.q.z : acc.mx.z; mx.w = acc.q.w != acc.q.w ? acc.q.w : acc.mx.w;
  mn.x = acc.q.x != acc.q.x ? acc.q.x : acc.mn.x; mn.y = acc.q.y != acc.q.y ? acc.q.y : acc.mn.y;
  mn.z = acc.q.z != acc.q.z ? acc.q.z : acc.mn.z; mn.w = acc.q.w != acc.q.w ? acc.q.w : acc.mn.w;
  sd.x = sqrtf(var.x + 1e-5f); sd.y = sqrtf(var.y + 1e-5f); sd.z = sqrtf(var.z + 1e-5f); sd.w = sqrtf(var.w + 1e-5f);
  put(0, mean); put(1, mx); put(2, mn); put(3, sd);
}

// U gathers of one row issued back to back from the ids held by the group's lanes, then folded in order.
template <int U, bool PARTIAL, bool DST, bool ARG, int ET, bool X64>
__device__ __forceinline__ void fast_batch(const float* x, AccF& acc, ArgF& ag, int idx, int src_lane0, unsigned ldb,
                                           unsigned offb, int nvalid, const f4 dt, int e0, const float* et, unsigned lde_b,
                                           int ety, const EtF& tb) {
  int id[U], ty[U];
  f4 v[U], w[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    id[u] = __shfl(idx, src_lane0 + (PARTIAL ? min(u, nvalid - 1) : u));
    ty[u] = ET == 2 ? __shfl(ety, src_lane0 + (PARTIAL ? min(u, nvalid - 1) : u)) : 0;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if constexpr (X64) aload128x(v[u], reinterpret_cast<const char*>(x) + offb + (size_t)(unsigned)id[u] * ldb);
    else aload128(v[u], x, __umul24((unsigned)id[u], ldb) + offb);
    if constexpr (ET == 1) aload128(w[u], et, (unsigned)(e0 + (PARTIAL ? min(u, nvalid - 1) : u)) * lde_b + offb);
  }
  Drain<0, U, DST, ARG, ET>::run(acc, ag, v, w, ty, tb, nvalid, PARTIAL, dt, e0);
}

// The prefetch invariants: the first L source ids of item r+1 and the record of item r+2 are requested BEFORE
// item r's gathers; VMEM returns in order, so once the wave has waited for any gather of item r they have landed.
// DST: message = x[src] + dst_term[row] (the tower layers: models/dgl/pna_layer.py:35-40 with the 1-layer pretrans
// factorised to node level).  The row's term is one more dwordx4 per lane, fetched one item ahead like the source ids.
// OROW (with DST): a whole-row record's aggregate goes to row out_row_of[row] of `out` (the record's `row` stays the node: the
// dst_term needs it) -- the tower layers' aggregate written in degree order (ABI 12).  Fetched one item ahead like the ids.
// ARG: also writes argmax / argmin (see ArgF); heavy segments then write k_segreduce's seven-quantity partials and are finished by
// k_heavy_finalize<4, true>.
template <int U, bool DST, bool OROW = false, bool ARG = false, int ET = 0, bool X64 = false>
__global__ __launch_bounds__(kBlock) void k_segreduce_fast(const FArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int L = a.L;
  const int grp = lane / L;
  if (grp >= a.G) return;
  const int c = lane - grp * L;
  const int grp_lane0 = grp * L;
  const int nchunks = (a.F + 3) / 4;
  const int tower = blockIdx.y / a.tiles;
  const int chunk = (blockIdx.y - tower * a.tiles) * L + c;
  const bool lane_ok = chunk < nchunks;
  const int off = min(min(chunk, nchunks - 1) * 4, a.F - 4);
  const long offo = (long)tower * a.ts_out + off;
  const int NG = kWaves * a.G;
  const long NI = a.n_items;
  const long base = (long)blockIdx.x * NG * a.R + wave * a.G + grp;
  if (base >= NI) return;
  const unsigned ldb = a.ldb;
  const unsigned offb = (unsigned)tower * a.ts_in_b + (unsigned)off * 4u;
  auto issue_item = [&](i4& dst, long k) {
    if constexpr (ARG) asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"((unsigned)k * 16u), "s"(a.items) : "memory");
    else asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"((unsigned)k * 16u), "s"(a.items) : "memory");
  };

  // Every asm-loaded register below is written by an asm load on EVERY path (addresses are clamped instead of
  // guarded): an asm output that met another definition at a control-flow merge could be copied by the compiler
  // before the load has landed.
  const long last = NI - 1;
  const unsigned e_last = (unsigned)a.n_edges - 1u;          // n_edges >= 1 (launcher)
  auto ids_of = [&](int& dst, const i4 rec) {                // lane c <- col[beg + min(c, deg-1)], clamped into col[]
    const int d = rec.z - rec.y;
    const unsigned pos = (unsigned)rec.y + (unsigned)min(c, max(d - 1, 0));
    aload32w<ARG>(dst, a.col, min(pos, e_last) * 4u);
  };

  const unsigned ldd_b = a.ldd_b;
  auto dst_of = [&](f4& dst, const i4 rec) {                 // lane c <- dst_term[row][its 4 features] (row < V always)
    aload128w<ARG>(dst, a.dst, __umul24((unsigned)rec.x, ldd_b) + offb);
  };
  auto types_of = [&](int& dst, const i4 rec) {              // lane c <- etype[beg + min(c, deg-1)] (ET == 2), like ids_of
    const int d = rec.z - rec.y;
    const unsigned pos = (unsigned)rec.y + (unsigned)min(c, max(d - 1, 0));
    aload32w<true>(dst, a.etype, min(pos, e_last) * 4u);
  };
  EtF tb;
  if constexpr (ET == 2) {                                   // the lane's slice of the type table: ordinary loads, before any asm load
#pragma unroll
    for (int ty = 0; ty < 4; ++ty) {
      const float* r = a.et + (size_t)min(ty, a.n_types - 1) * (a.lde_b / 4u) + (size_t)tower * (a.ts_in_b / 4u) + off;
      tb.tab[ty] = (f4){r[0], r[1], r[2], r[3]};
    }
  }

  // prologue: record of item 0 -> its first ids and the record of item 1
  i4 cur;
  issue_item(cur, base);
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(cur) : : "memory");
  int idx_c;
  ids_of(idx_c, cur);
  f4 dt_c = (f4){0.f, 0.f, 0.f, 0.f};
  if constexpr (DST) dst_of(dt_c, cur);
  int orow_c = 0;
  if constexpr (OROW) aload32(orow_c, a.orow, (unsigned)cur.x * 4u);
  int ety_c = 0;
  if constexpr (ET == 2) { types_of(ety_c, cur); asm volatile("s_waitcnt vmcnt(0)" : "+v"(ety_c) : : "memory"); }
  i4 nxt;
  issue_item(nxt, min(base + NG, last));
  if constexpr (OROW) asm volatile("s_waitcnt vmcnt(0)" : "+v"(idx_c), "+v"(nxt), "+v"(dt_c), "+v"(orow_c) : : "memory");
  else if constexpr (DST) asm volatile("s_waitcnt vmcnt(0)" : "+v"(idx_c), "+v"(nxt), "+v"(dt_c) : : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" : "+v"(idx_c), "+v"(nxt) : : "memory");

  AccF acc;
  ArgF ag;
  ag.init();
  for (int r = 0; r < a.R; ++r) {
    const long item = base + (long)r * NG;
    if (item >= NI) break;
    // ---- prefetch (issued BEFORE this item's gathers): ids of item r+1, record of item r+2 (clamped to the last item)
    int idx_n;
    i4 nn;
    f4 dt_n = (f4){0.f, 0.f, 0.f, 0.f};
    ids_of(idx_n, nxt);
    if constexpr (DST) dst_of(dt_n, nxt);
    int orow_n = 0;
    if constexpr (OROW) aload32(orow_n, a.orow, (unsigned)nxt.x * 4u);
    int ety_n = 0;
    if constexpr (ET == 2) types_of(ety_n, nxt);
    issue_item(nn, min(item + 2 * NG, last));
    // ---- this item
    const int row = cur.x, beg = cur.y, end = cur.z, slot = cur.w;
    acc.init();
    if constexpr (ARG) ag.init();
    int idx = idx_c, ety = ety_c;
    for (int cb = beg; cb < end; cb += L) {
      const int nidx = min(L, end - cb);
      if (cb != beg) {                                       // longer than one id chunk (rare): fetch + wait
        aload32w<ARG>(idx, a.col, (unsigned)(cb + min(c, nidx - 1)) * 4u);
        if constexpr (ET == 2) { aload32w<true>(ety, a.etype, (unsigned)(cb + min(c, nidx - 1)) * 4u); await<0>(ety); }
        await<0>(idx);
      }
      int j = 0;
      for (; j + U <= nidx; j += U)
        fast_batch<U, false, DST, ARG, ET, X64>(a.x, acc, ag, idx, grp_lane0 + j, ldb, offb, U, dt_c, cb + j, a.et, a.lde_b, ety, tb);
      if (j < nidx)
        fast_batch<U, true, DST, ARG, ET, X64>(a.x, acc, ag, idx, grp_lane0 + j, ldb, offb, nidx - j, dt_c, cb + j, a.et, a.lde_b, ety, tb);
    }
    if (lane_ok && PNA_STORES_ON(a, acc.s.x)) {
      if (slot < 0) {
        fast_finalize_store(a, acc, OROW ? orow_c : row, end - beg, offo);
        if constexpr (ARG) {
          typedef i4 i4a4 __attribute__((aligned(4)));
          const size_t oa = (size_t)row * a.ld_arg + (size_t)tower * a.ts_arg + off;
          if (a.argmax) *reinterpret_cast<i4a4*>(a.argmax + oa) = ag.amx;
          if (a.argmin) *reinterpret_cast<i4a4*>(a.argmin + oa) = ag.amn;
        }
      } else {                                               // heavy segment: raw (s, q, max, min) to the workspace
        typedef f4 f4a4 __attribute__((aligned(4)));
        float* p = a.partials + ((size_t)slot * a.T + tower) * kNQ * a.pstride + off;
        *reinterpret_cast<f4a4*>(p) = acc.s;
        *reinterpret_cast<f4a4*>(p + a.pstride) = acc.q;
        *reinterpret_cast<f4a4*>(p + 2 * a.pstride) = acc.mx;
        *reinterpret_cast<f4a4*>(p + 3 * a.pstride) = acc.mn;
        if constexpr (ARG) {                                 // k_segreduce's partial record: + argmax, argmin (as bits), edge count
          typedef i4 i4a4 __attribute__((aligned(4)));
          *reinterpret_cast<i4a4*>(p + 4 * a.pstride) = ag.amx;
          *reinterpret_cast<i4a4*>(p + 5 * a.pstride) = ag.amn;
          if (chunk == 0) p[6 * a.pstride - off] = (float)(end - beg);
        }
      }
    }
    // The prefetches were issued before this item's gathers and VMEM returns in order, so once the wave has waited
    // for any gather they have landed.  Only if no lane group of the wave gathered anything: drain.
    if (__builtin_amdgcn_ballot_w64(end > beg) == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" : "+v"(idx_n), "+v"(nn));                 // anchor: consumers cannot move above this point
    if constexpr (DST) { asm volatile("" : "+v"(dt_n)); dt_c = dt_n; }
    if constexpr (OROW) { asm volatile("" : "+v"(orow_n)); orow_c = orow_n; }
    if constexpr (ET == 2) { asm volatile("" : "+v"(ety_n)); ety_c = ety_n; }
    idx_c = idx_n; cur = nxt; nxt = nn;
  }
}

// Fold the per-segment partials of each heavy row and finish the row.  One wavefront per heavy row: lane
// group g folds segments g, g+G, g+2G, ... in order, then the G group results are combined in group order
// (a fixed association, so results stay independent of the launch geometry of the main kernel).
template <int VEC, bool EXTRA>
__global__ __launch_bounds__(kBlock) void k_heavy_finalize(const KArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int L = a.L;
  const int grp = lane / L;
  if (grp >= a.G) return;
  const int c = lane - grp * L;
  const int nchunks = (a.F + VEC - 1) / VEC;
  const int tower = blockIdx.y / a.tiles;
  const int chunk = (blockIdx.y - tower * a.tiles) * L + c;
  int off = min(chunk, nchunks - 1) * VEC;
  if (VEC == 4) off = min(off, a.F - 4);
  const long offi = (long)tower * a.ts_in + off;
  const long offo = (long)tower * a.ts_out + off;
  const int hi = blockIdx.x * kWaves + wave;
  if (hi >= a.n_heavy) return;
  const int row = a.heavy_rows[hi];
  const int s0 = a.heavy_segptr[hi], s1 = a.heavy_segptr[hi + 1];
  Acc<VEC, EXTRA> acc;
  acc.init();
  auto merge = [&](const float (&ps)[VEC], const float (&pq)[VEC], const float (&pmx)[VEC], const float (&pmn)[VEC],
                   const int (&pax)[VEC], const int (&pan)[VEC], float pw) __attribute__((always_inline)) {
    if constexpr (EXTRA) acc.wsum = acc.wsum + pw;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      acc.s[k] = acc.s[k] + ps[k];
      acc.q[k] = acc.q[k] + pq[k];
      // ties keep the earlier edge (smaller CSR position), NaN is sticky
      bool gx = pmx[k] > acc.mx[k] || (pmx[k] != pmx[k] && acc.mx[k] == acc.mx[k]);
      bool gn = pmn[k] < acc.mn[k] || (pmn[k] != pmn[k] && acc.mn[k] == acc.mn[k]);
      if constexpr (EXTRA) {
        gx = gx || (pmx[k] == acc.mx[k] && pax[k] >= 0 && (acc.amx[k] < 0 || pax[k] < acc.amx[k]));
        gn = gn || (pmn[k] == acc.mn[k] && pan[k] >= 0 && (acc.amn[k] < 0 || pan[k] < acc.amn[k]));
        acc.amx[k] = gx ? pax[k] : acc.amx[k];
        acc.amn[k] = gn ? pan[k] : acc.amn[k];
      }
      acc.mx[k] = gx ? pmx[k] : acc.mx[k];
      acc.mn[k] = gn ? pmn[k] : acc.mn[k];
    }
  };
  // Partials are independent loads: fetch PB segments' worth before folding.
  constexpr int PB = 4;
  const int G = a.G;
  for (int sb = s0 + grp; sb < s1; sb += PB * G) {
    float ps[PB][VEC], pq[PB][VEC], pmx[PB][VEC], pmn[PB][VEC], pw[PB];
    int pax[PB][VEC], pan[PB][VEC];
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      const int seg = min(sb + i * G, s1 - 1);
      const float* p = a.partials + ((size_t)seg * a.T + tower) * kNQ * a.pstride + off;
      Ld<VEC>::load(p, ps[i]);
      Ld<VEC>::load(p + a.pstride, pq[i]);
      Ld<VEC>::load(p + 2 * a.pstride, pmx[i]);
      Ld<VEC>::load(p + 3 * a.pstride, pmn[i]);
      pw[i] = 0.f;
#pragma unroll
      for (int k = 0; k < VEC; ++k) { pax[i][k] = -1; pan[i][k] = -1; }
      if constexpr (EXTRA) {
        float t[VEC];
        Ld<VEC>::load(p + 4 * a.pstride, t);
#pragma unroll
        for (int k = 0; k < VEC; ++k) pax[i][k] = __float_as_int(t[k]);
        Ld<VEC>::load(p + 5 * a.pstride, t);
#pragma unroll
        for (int k = 0; k < VEC; ++k) pan[i][k] = __float_as_int(t[k]);
        pw[i] = p[6 * a.pstride - off];
      }
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {                       // (no `break`: it kept the loop rolled and the partial arrays in scratch)
      if (sb + i * G < s1) merge(ps[i], pq[i], pmx[i], pmn[i], pax[i], pan[i], pw[i]);
    }
  }
  // combine the lane groups' results into group 0, in group order
  for (int g2 = 1; g2 < G; ++g2) {
    float ps[VEC], pq[VEC], pmx[VEC], pmn[VEC];
    int pax[VEC], pan[VEC];
    const int src = lane + g2 * L;                          // only meaningful for lanes of group 0
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      ps[k] = __shfl(acc.s[k], src); pq[k] = __shfl(acc.q[k], src);
      pmx[k] = __shfl(acc.mx[k], src); pmn[k] = __shfl(acc.mn[k], src);
      pax[k] = EXTRA ? __shfl(acc.amx[k], src) : -1; pan[k] = EXTRA ? __shfl(acc.amn[k], src) : -1;
    }
    const float pw = EXTRA ? __shfl(acc.wsum, src) : 0.f;
    if (grp == 0) merge(ps, pq, pmx, pmn, pax, pan, pw);
  }
  if (grp == 0 && chunk < nchunks)
    finalize_store<VEC, EXTRA>(a, acc, row, a.rowptr[row + 1] - a.rowptr[row], offi, offo, a.heavy_out ? a.heavy_out[hi] : -1);
}

// models/dgl/scalers.py:12-19 with the reference's rounding sequence (see pna_amd.h).
__global__ void k_degree_scalers(const int32_t* rowptr, int V, float avg_log, float inv_avg, float* amp, float* att) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const int d = rowptr[v + 1] - rowptr[v];
  float fa, ft;
  pna_degree_scalers_row(d, avg_log, inv_avg, fa, ft);     // (pna_scalers_dev.h: shared with the batch plan)
  if (amp) amp[v] = fa;
  if (att) att[v] = ft;
}

template <int VEC, int U>
int launch_u(const KArgs& k, bool extra, bool idx32, dim3 grid, hipStream_t st) {
  if (extra) {
    if (idx32) hipLaunchKernelGGL((k_segreduce<VEC, U, true, true>), grid, dim3(kBlock), 0, st, k);
    else hipLaunchKernelGGL((k_segreduce<VEC, U, true, false>), grid, dim3(kBlock), 0, st, k);
  } else {
    if (idx32) hipLaunchKernelGGL((k_segreduce<VEC, U, false, true>), grid, dim3(kBlock), 0, st, k);
    else hipLaunchKernelGGL((k_segreduce<VEC, U, false, false>), grid, dim3(kBlock), 0, st, k);
  }
  return 0;
}

int launch_any(const KArgs& k, int vec, int U, bool extra, bool idx32, dim3 grid, hipStream_t st) {
  if (vec == 1) return launch_u<1, 4>(k, extra, idx32, grid, st);      // scalar path: one unroll only
  switch (U) {
    case 2: return launch_u<4, 2>(k, extra, idx32, grid, st);
    case 4: return launch_u<4, 4>(k, extra, idx32, grid, st);
    case 8: return launch_u<4, 8>(k, extra, idx32, grid, st);
  }
  return -1;
}

}  // namespace

extern "C" int64_t pna_segreduce_partials_bytes(int32_t n_seg, int32_t F, int32_t n_tower) {
  const int64_t ps = ((int64_t)F + 3) / 4 * 4;
  return (int64_t)n_seg * (n_tower > 1 ? n_tower : 1) * kNQ * ps * (int64_t)sizeof(float);
}

extern "C" int pna_segreduce_fwd_f32(const pna_segreduce_args* p, pna_stream_t stream) {
  if (!p) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: null args");
  if (int rc_ss = pna_check_struct_size("pna_segreduce_fwd_f32", p->struct_size, sizeof(*p))) return rc_ss;
  if (p->V < 0 || p->F <= 0) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: bad V/F");
  if (p->V == 0) return PNA_OK;
  if (!p->rowptr || !p->x || !p->out) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: rowptr/x/out must be non-null");
  if (p->n_aggr <= 0 || p->n_aggr > PNA_MAX_AGGR || p->n_scaler <= 0 || p->n_scaler > PNA_MAX_SCALER)
    return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: n_aggr/n_scaler out of range");
  for (int i = 0; i < p->n_aggr; ++i)
    if (p->aggr[i] < PNA_AGG_MEAN || p->aggr[i] > PNA_AGG_VAR_RAW)
      return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: unknown aggregator code");
  const int T = p->n_tower > 1 ? p->n_tower : 1;
  const int64_t ts_in = T > 1 ? p->tower_stride_in : 0, ts_out = T > 1 ? p->tower_stride_out : 0;
  if (T > 1 && (ts_in < p->F || ts_out < (int64_t)p->block_stride * (p->n_aggr * p->n_scaler - 1) + p->F))
    return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: tower strides too small");
  const int64_t in_w = ts_in * (T - 1) + p->F;             // columns touched in x / dst_term / edge_term
  const int64_t out_w = ts_out * (T - 1) + (int64_t)p->block_stride * (p->n_aggr * p->n_scaler - 1) + p->F;
  if (p->ldx < in_w || p->block_stride < p->F || p->ldo < out_w)
    return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: leading dimensions too small");
  if ((p->dst_term && p->ld_dst < in_w) || (p->edge_term && p->ld_edge < in_w) ||
      ((p->argmax || p->argmin) && p->ld_arg < in_w))
    return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: leading dimensions too small");
  if (p->edge_type && (!p->edge_term || p->n_edge_types < 1))
    return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: edge_type needs edge_term (the table) and n_edge_types >= 1");
  const bool heavy = p->heavy_threshold > 0 && p->n_heavy > 0;
  if (heavy && (!p->heavy_rows || !p->heavy_segptr || !p->seg_heavy || !p->partials || p->seg_len <= 0 || p->n_seg <= 0))
    return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: incomplete heavy-row schedule");

  KArgs k;
  memset(&k, 0, sizeof(k));
  k.rowptr = p->rowptr; k.col = p->col; k.x = p->x; k.dst_term = p->dst_term; k.edge_term = p->edge_term;
  k.ew = p->edge_weight; k.etype = p->edge_type;
  for (int s = 0; s < p->n_scaler; ++s) k.row_scale[s] = p->row_scale[s];
  k.out = p->out; k.argmax = p->argmax; k.argmin = p->argmin;
  k.heavy_rows = p->heavy_rows; k.heavy_segptr = p->heavy_segptr; k.seg_heavy = p->seg_heavy; k.partials = p->partials;
  k.heavy_out = p->heavy_out_rows;
  k.ldx = p->ldx; k.ld_dst = p->ld_dst; k.ld_edge = p->ld_edge; k.ldo = p->ldo; k.ld_arg = p->ld_arg;
  k.V = p->V; k.F = p->F; k.n_aggr = p->n_aggr; k.n_scaler = p->n_scaler; k.block_stride = p->block_stride;
  for (int i = 0; i < p->n_aggr; ++i) k.aggr[i] = p->aggr[i];
  k.heavy_threshold = heavy ? p->heavy_threshold : (p->heavy_threshold > 0 ? p->heavy_threshold : 0);
  k.seg_len = p->seg_len; k.n_heavy = heavy ? p->n_heavy : 0; k.n_seg = heavy ? p->n_seg : 0;
  // a threshold without a schedule would silently drop rows: only honour it when the lists exist
  if (!heavy) k.heavy_threshold = 0;

  const pna_tuning& t = p->tune;
  int vec = t.vec ? t.vec : (p->F >= 4 ? 4 : 1);
  if (vec != 1 && vec != 4) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: tune.vec must be 1 or 4");
  if (vec == 4 && p->F < 4) vec = 1;
  const int nchunks = (p->F + vec - 1) / vec;
  int L = t.lanes_per_row;
  int tiles;
  if (L <= 0) {
    tiles = (nchunks + 63) / 64;
    L = (nchunks + tiles - 1) / tiles;
  } else {
    if (L > 64) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: tune.lanes_per_row > 64");
    tiles = (nchunks + L - 1) / L;
  }
  k.L = L; k.G = 64 / L; k.T = T; k.tiles = tiles; k.ts_in = ts_in; k.ts_out = ts_out;
  int U = t.unroll ? t.unroll : 4;
  if (U < 2 || U > 8 || U == 7) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: tune.unroll must be 2..6 or 8");
  k.R = t.rows_per_group > 0 ? t.rows_per_group : 4;
  k.nt = t.nt_store >= 0 ? 1 : 0;
  k.pf = t.prefetch >= 0 ? 1 : 0;
  k.dbg = PNA_DBG_WORD(t);   // experiments build only (see PNA_STORES_ON)
  k.pstride = (p->F + 3) / 4 * 4;
  const int NG = kWaves * k.G;
  k.n_heavy_blocks = heavy ? (k.n_seg + NG - 1) / NG : 0;
  const long rows_per_block = (long)NG * k.R;
  const long light_blocks = (p->V + rows_per_block - 1) / rows_per_block;
  if (light_blocks + k.n_heavy_blocks > 0x7fffffffL) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: grid too large");
  const bool extra = p->dst_term || p->edge_term || p->edge_weight || p->argmax || p->argmin;
  const bool want_arg = p->argmax || p->argmin;
  // edge terms on the hand-scheduled kernel (ABI 14): with dst_term, default unroll, no position tracking / row map; per edge (32-bit
  // offsets into the term) or per edge type (<= 4 types: the table rides in registers)
  const int et_mode = !p->edge_term ? 0 : p->edge_type ? 2 : 1;
  const bool et_fast = et_mode == 0 || (p->dst_term && U == 4 && !want_arg && !p->out_row_of && p->ld_edge * 4 < (1ll << 24) &&
                                        (et_mode == 2 ? p->n_edge_types <= 4
                                                      : (double)p->n_edges * (double)p->ld_edge * 4.0 < 4294967296.0));
  // what the hand-scheduled kernel lacks (argmax / argmin: built for the default unroll, together)
  const bool extra_fast = !et_fast || p->edge_weight || (want_arg && !(U == 4 && p->argmax && p->argmin && !p->out_row_of));
  dim3 grid((unsigned)(light_blocks + k.n_heavy_blocks), (unsigned)(tiles * T));
  hipStream_t st = (hipStream_t)stream;
  // 32-bit gather offsets when the whole feature table is addressable with them
  const bool idx32 = p->x_rows > 0 && (double)p->x_rows * (double)p->ldx * 4.0 < 4294967296.0 && p->ldx < (1 << 28);
  // hand-scheduled kernel for the configuration the layers issue (see k_segreduce_fast / FArgs)
  const bool std4 = p->n_aggr == 4 && p->aggr[0] == PNA_AGG_MEAN && p->aggr[1] == PNA_AGG_MAX && p->aggr[2] == PNA_AGG_MIN &&
                    p->aggr[3] == PNA_AGG_STD && p->n_scaler == 1 && p->row_scale[0] == nullptr;
  // the source rows through 32-bit offsets (24-bit multiply) where the table allows, else through 64-bit lane addresses (round 4:
  // the instantiations the layers' large-graph paths issue: default unroll, no edge terms / argument tracking)
  const bool small_x = idx32 && p->x_rows < (1 << 24) && p->ldx * 4 < (1 << 24);
  const bool x64 = !small_x;
  const bool x64_ok = p->x_rows > 0 && p->x_rows < (1ll << 32) && p->ldx * 4 < (1ll << 31) && et_mode == 0 && !want_arg && U == 4;
  const bool fast_ok = vec == 4 && !extra_fast && std4 && p->col != nullptr && (small_x || x64_ok) &&
                       (int64_t)T * ts_in * 4 < (1 << 30) && p->work_items != nullptr &&
                       p->n_work_items > 0 && p->n_work_items < (1 << 27) && p->n_edges > 0 && p->n_edges < (1LL << 30) &&
                       (!p->dst_term || (p->V < (1 << 24) && p->ld_dst * 4 < (1 << 24) &&
                                         (double)p->V * (double)p->ld_dst * 4.0 < 4294967296.0)) &&
                       t.reserved[1] != 1;
  int rc = 0;
  if (!fast_ok && t.reserved[1] == 2)
    return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: the hand-scheduled kernel was required (tune.reserved[1] = 2) but this call does not qualify for it");
  if (!fast_ok && U != 2 && U != 4 && U != 8) U = 4;       // the compiler-scheduled kernel is built for 2, 4, 8
  if (fast_ok) {
    FArgs f;
    memset(&f, 0, sizeof(f));
    f.items = p->work_items; f.col = p->col; f.x = p->x; f.out = p->out; f.partials = p->partials;
    f.ldo = p->ldo; f.ts_out = ts_out; f.ldb = (unsigned)(p->ldx * 4); f.ts_in_b = (unsigned)(ts_in * 4);
    f.n_items = p->n_work_items; f.n_edges = (int)p->n_edges; f.F = p->F; f.L = k.L; f.G = k.G; f.R = k.R; f.T = T; f.tiles = tiles;
    f.pstride = k.pstride; f.block_stride = p->block_stride; f.nt = k.nt; f.dbg = k.dbg;
    f.dst = p->dst_term; f.ldd_b = (unsigned)(p->ld_dst * 4);
    f.orow = p->out_row_of;
    f.argmax = p->argmax; f.argmin = p->argmin; f.ld_arg = p->ld_arg; f.ts_arg = ts_in;
    f.et = p->edge_term; f.etype = p->edge_type; f.lde_b = (unsigned)(p->ld_edge * 4); f.n_types = p->n_edge_types;
    if (p->out_row_of && !(p->dst_term && U == 4))
      return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: out_row_of is honoured with dst_term and the default unroll only (without dst_term the work list's row field is the output row)");
    const long fb = (p->n_work_items + rows_per_block - 1) / rows_per_block;
    dim3 fgrid((unsigned)fb, (unsigned)(tiles * T));
    const unsigned dyn_lds = (unsigned)(k.dbg >> 8) * 1024u;   // 0 in the shipped build
    if (et_mode == 1) {
      hipLaunchKernelGGL((k_segreduce_fast<4, true, false, false, 1>), fgrid, dim3(kBlock), dyn_lds, st, f);
    } else if (et_mode == 2) {
      hipLaunchKernelGGL((k_segreduce_fast<4, true, false, false, 2>), fgrid, dim3(kBlock), dyn_lds, st, f);
    } else if (want_arg) {
      if (p->dst_term) hipLaunchKernelGGL((k_segreduce_fast<4, true, false, true>), fgrid, dim3(kBlock), dyn_lds, st, f);
      else hipLaunchKernelGGL((k_segreduce_fast<4, false, false, true>), fgrid, dim3(kBlock), dyn_lds, st, f);
    } else if (x64) {
      if (p->dst_term && p->out_row_of) hipLaunchKernelGGL((k_segreduce_fast<4, true, true, false, 0, true>), fgrid, dim3(kBlock), dyn_lds, st, f);
      else if (p->dst_term) hipLaunchKernelGGL((k_segreduce_fast<4, true, false, false, 0, true>), fgrid, dim3(kBlock), dyn_lds, st, f);
      else hipLaunchKernelGGL((k_segreduce_fast<4, false, false, false, 0, true>), fgrid, dim3(kBlock), dyn_lds, st, f);
    } else if (p->dst_term && p->out_row_of) {
      hipLaunchKernelGGL((k_segreduce_fast<4, true, true>), fgrid, dim3(kBlock), dyn_lds, st, f);
    } else if (p->dst_term) {
      switch (U) {
        case 2: hipLaunchKernelGGL((k_segreduce_fast<2, true>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
        case 3: hipLaunchKernelGGL((k_segreduce_fast<3, true>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
        case 4: hipLaunchKernelGGL((k_segreduce_fast<4, true>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
        case 5: hipLaunchKernelGGL((k_segreduce_fast<5, true>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
        case 6: hipLaunchKernelGGL((k_segreduce_fast<6, true>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
        default: hipLaunchKernelGGL((k_segreduce_fast<8, true>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
      }
    } else {
      switch (U) {
        case 2: hipLaunchKernelGGL((k_segreduce_fast<2, false>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
        case 3: hipLaunchKernelGGL((k_segreduce_fast<3, false>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
        case 4: hipLaunchKernelGGL((k_segreduce_fast<4, false>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
        case 5: hipLaunchKernelGGL((k_segreduce_fast<5, false>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
        case 6: hipLaunchKernelGGL((k_segreduce_fast<6, false>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
        default: hipLaunchKernelGGL((k_segreduce_fast<8, false>), fgrid, dim3(kBlock), dyn_lds, st, f); break;
      }
    }
  } else {
    rc = launch_any(k, vec, U, extra, idx32, grid, st);
  }
  if (rc != 0) return pna_set_error(PNA_E_INVALID, "pna_segreduce_fwd_f32: no kernel for this tuning");
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  if (heavy) {
    dim3 g2((unsigned)((k.n_heavy + kWaves - 1) / kWaves), (unsigned)(tiles * T));
    // the hand-scheduled kernel writes (s, q, max, min) partials with NaN-dropping max/min: finish them with the
    // plain finalize (NaN restored from q), also when a dst_term was added to the messages
    // (its ARG instantiation writes k_segreduce's full partial records -- NaN-sticky max / min with their positions -- and is
    // finished by the EXTRA finalize, which also stores argmax / argmin; the dst_term is already inside the partials)
    const bool extra = fast_ok ? want_arg : (p->dst_term || p->edge_term || p->edge_weight || p->argmax || p->argmin);
    if (vec == 4) {
      if (extra) hipLaunchKernelGGL((k_heavy_finalize<4, true>), g2, dim3(kBlock), 0, st, k);
      else hipLaunchKernelGGL((k_heavy_finalize<4, false>), g2, dim3(kBlock), 0, st, k);
    } else {
      if (extra) hipLaunchKernelGGL((k_heavy_finalize<1, true>), g2, dim3(kBlock), 0, st, k);
      else hipLaunchKernelGGL((k_heavy_finalize<1, false>), g2, dim3(kBlock), 0, st, k);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  }
  return PNA_OK;
}

extern "C" int pna_degree_scalers_f32(const int32_t* rowptr, int32_t V, float avg_log, float* amp, float* att,
                                      pna_stream_t stream) {
  if (V < 0 || (V > 0 && !rowptr)) return pna_set_error(PNA_E_INVALID, "pna_degree_scalers_f32: bad arguments");
  if (V == 0) return PNA_OK;
  const float inv = 1.0f / avg_log;                        // Tensor.reciprocal() in fp32
  hipLaunchKernelGGL(k_degree_scalers, dim3((V + 255) / 256), dim3(256), 0, (hipStream_t)stream, rowptr, V, avg_log, inv,
                     amp, att);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  return PNA_OK;
}
