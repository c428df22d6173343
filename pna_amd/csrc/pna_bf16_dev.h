// pna_bf16_dev.h -- device helpers shared by the bf16 inference kernels (pna_bf16_gather.hip, pna_bf16_shard.hip, pna_bf16_contract.hip,
// pna_bf16_small.hip, pna_bf16_edge_mlp.hip): the bf16 <-> fp32 conversions, the per-lane statistics of a gather (8 features per lane, fp32), the ONE fold
// over a row's in-edges (fold_edges) and the ONE finalisation of a row's statistics (finish_stats).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pna_amd.h"
#include "pna_rowstats.h"

namespace pna_bf16 {

typedef unsigned short u16;
typedef float f4 __attribute__((ext_vector_type(4)));
typedef short bf8 __attribute__((ext_vector_type(8)));   // 8 bf16 = one MFMA A/B fragment
typedef unsigned u4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;

__device__ __forceinline__ float bf2f(u16 b) { return __uint_as_float((unsigned)b << 16); }

// fp32 -> bf16, round to nearest even; NaN stays a (quiet) NaN
__device__ __forceinline__ u16 f2bf(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u16)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (u16)(u >> 16);
}

// ---------------------------------------------------------------------------------------------------------------------------
// gather + statistics
// ---------------------------------------------------------------------------------------------------------------------------
struct SegArgs {
  const int32_t* rowptr; const int32_t* col; const u16* x; int64_t ldx;
  int V, F, G;                 // G lanes per destination row
  int n_aggr; int aggr[PNA_MAX_AGGR];
  u16* out; int64_t ldo; int bs;
  int heavy_threshold, seg_len, n_heavy, n_seg;
  const int32_t* heavy_rows; const int32_t* heavy_segptr; const int32_t* seg_heavy;
  float* partials;             // [n_seg][4][F8] fp32: s, q, mx, mn
  int F8;
};

struct Acc { float s[8], q[8], mx[8], mn[8]; };

__device__ __forceinline__ void acc_init(Acc& c) {
#pragma unroll
  for (int j = 0; j < 8; ++j) { c.s[j] = 0.f; c.q[j] = 0.f; c.mx[j] = -INFINITY; c.mn[j] = INFINITY; }
}

// 8 features [f0, f0 + 8) of one source row; V8: one 16-byte load (the caller guarantees the whole piece is readable)
template <bool V8>
__device__ __forceinline__ void load8(const u16* p, int nf, float (&v)[8]) {
  if (V8) {
    const u4 w = *reinterpret_cast<const u4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[2 * j] = __uint_as_float(w[j] << 16); v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u); }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < nf ? bf2f(p[j]) : 0.f;
  }
}

__device__ __forceinline__ void fold(Acc& c, const float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c.s[j] = c.s[j] + v[j];
    c.q[j] = c.q[j] + v[j] * v[j];
    c.mx[j] = pna_dev::vmax(c.mx[j], v[j]);
    c.mn[j] = pna_dev::vmin(c.mn[j], v[j]);
  }
}

// The optional message term of fold_edges: message of CSR edge k = x[col[k]] + dst + edge row, formed in fp32.  dst: this lane's 8
// columns of the destination row (null: +0.0 is added, which turns a gathered -0.0 into +0.0); er: this lane's 8 columns of edge row
// 0 (null: no edge term), rows lde apart; et: the edge's row in a table of n_er rows (null: CSR edge k reads row k).
struct MsgTerm {
  const u16* dst; const u16* er; int64_t lde; const int32_t* et; int n_er;
};

// The two source tables of a split gather (fold_edges<..., SPLIT = true>): a source id c < n_local reads row c of the first table,
// any other id row c - n_local of the second.  far: this lane's 8 columns of the second table's row 0 moved back by n_local rows, so
// that both tables are addressed by the id itself; pitches in BYTES as 32-bit values (base + id * pitch is one 32 x 32 -> 64 bit
// multiply-add per gathered edge behind the compare and the select of base and pitch).
struct HaloTab {
  const char* far; unsigned pitch_far, pitch_near; int n_local;
};

// The in-edges [beg, end) of one destination row folded in CSR order for the 8 features at xb of every source row (nf of them
// exist); four edges in flight per lane.  V8 / VT: 16-byte loads of the source rows / of the term rows.  MSG = false: no term is
// read or added (not even a zero: -0.0 + 0.0 is +0.0, and max / min would see it).  TYPED: edge rows always come from the type table.
// SPLIT: the source rows live in two tables (HaloTab); one compare and a select of base and pitch per gathered edge.
template <bool V8, bool VT, bool MSG, bool TYPED = false, bool SPLIT = false>
__device__ __forceinline__ void fold_edges(const int32_t* col, const u16* xb, int64_t ldx, int beg, int end, int nf, const MsgTerm& t,
                                           Acc& c, const HaloTab& hb = HaloTab{}) {
  auto src_row = [&](int id) __attribute__((always_inline)) {
    if (!SPLIT) return xb + (size_t)id * ldx;
    const bool far = id >= hb.n_local;
    const char* base = far ? hb.far : reinterpret_cast<const char*>(xb);
    return reinterpret_cast<const u16*>(base + (uint64_t)(unsigned)id * (far ? hb.pitch_far : hb.pitch_near));
  };
  float d[8];
  if (MSG) {
    if (t.dst) {
      load8<VT>(t.dst, nf, d);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = 0.f;
    }
  }
  const u16* eb = MSG ? t.er : nullptr;
  auto edge_row = [&](int k) __attribute__((always_inline)) {
    if (!TYPED && !t.et) return (size_t)k;
    int r = t.et[k];
    r = r < 0 ? 0 : r >= t.n_er ? t.n_er - 1 : r;              // a type outside the table reads a row of the table, never beyond it
    return (size_t)r;
  };
  int k = beg;
  for (; k + 4 <= end; k += 4) {
    int id[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) id[u] = col[k + u];
    float v[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) load8<V8>(src_row(id[u]), nf, v[u]);
    if (MSG) {
      if (eb) {
        float w[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) load8<VT>(eb + edge_row(k + u) * t.lde, nf, w[u]);
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
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) fold(c, v[u]);
  }
  for (; k < end; ++k) {
    float v[8];
    load8<V8>(src_row(col[k]), nf, v);
    if (MSG) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] + d[j];
      if (eb) {
        float w[8];
        load8<VT>(eb + edge_row(k) * t.lde, nf, w);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] + w[j];
      }
    }
    fold(c, v);
  }
}

// One row's statistics of nf <= 8 features finalized (pna_rowstats.h: the fp32 kernel's formulas): store(ai, r) receives the eight
// values of aggregator block ai, each rounded to bf16 once (zeros for the features beyond nf; for deg <= 0 zeros too, except
// PNA_AGG_STD_PYG, whose empty row is sqrtf(1e-5f): the PyG rule).  PNA_AGG_VAR_RAW is the variance without the clamp at 0.
template <class Store>
__device__ __forceinline__ void finish_stats(int deg, int nf, const Acc& c, int n_aggr, const int* aggr, Store store) {
  float mean[8], msq[8];
  const float D = (float)deg, invD = 1.0f / D;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mean[j] = pna_dev::div_rn(c.s[j], D, invD);
    msq[j] = pna_dev::div_rn(c.q[j], D, invD);
  }
  for (int ai = 0; ai < n_aggr; ++ai) {
    const int code = aggr[ai];
    u16 r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float val;
      if (j >= nf) {
        val = 0.f;
      } else if (deg <= 0) {
        val = code == PNA_AGG_STD_PYG ? sqrtf(1e-5f) : 0.f;
      } else {
        const float raw = msq[j] - mean[j] * mean[j];
        const float var = raw < 0.f ? 0.f : raw;
        switch (code) {
          case PNA_AGG_MEAN: val = mean[j]; break;
          case PNA_AGG_SUM: val = c.s[j]; break;
          case PNA_AGG_MAX: val = c.q[j] != c.q[j] ? c.q[j] : c.mx[j]; break;
          case PNA_AGG_MIN: val = c.q[j] != c.q[j] ? c.q[j] : c.mn[j]; break;
          case PNA_AGG_STD:
          case PNA_AGG_STD_PYG: val = sqrtf(var + 1e-5f); break;
          case PNA_AGG_VAR_RAW: val = raw; break;
          default: val = var; break;                   // PNA_AGG_VAR
        }
      }
      r[j] = f2bf(val);
    }
    store(ai, r);
  }
}

// eight bf16 values as one 16-byte store
__device__ __forceinline__ void store8(u16* o, const u16 (&r)[8]) {
  u4 w;
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = (unsigned)r[2 * j] | ((unsigned)r[2 * j + 1] << 16);
  *reinterpret_cast<u4*>(o) = w;
}

// one row's aggregator blocks into a.out: 16-byte stores (VOUT), else element stores of the block's own features only
template <bool VOUT>
__device__ __forceinline__ void finish_row(const SegArgs& a, int row, int deg, int f0, const Acc& c) {
  u16* o = a.out + (size_t)row * a.ldo + f0;
  const int nf = a.F - f0, nw = nf < 8 ? nf : 8;
  finish_stats(deg, nf, c, a.n_aggr, a.aggr, [&](int ai, const u16 (&r)[8]) __attribute__((always_inline)) {
    u16* ob = o + (size_t)ai * a.bs;
    if (VOUT) {
      store8(ob, r);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < nw) ob[j] = r[j];
    }
  });
}

// the fp32 partials (s, q, mx, mn) of one heavy-row segment, [n_seg][4][F8]
__device__ __forceinline__ void store_partials(const SegArgs& a, long seg, int f0, const Acc& c) {
  float* p = a.partials + (size_t)seg * 4 * a.F8 + f0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    p[j] = c.s[j];
    p[a.F8 + j] = c.q[j];
    p[2 * a.F8 + j] = c.mx[j];
    p[3 * a.F8 + j] = c.mn[j];
  }
}

// heavy row h: the partials of its segments combined in segment order, then finalized like a light row
template <bool VOUT>
__device__ __forceinline__ void finish_heavy_row(const SegArgs& a, long h, int f0) {
  const int row = a.heavy_rows[h], deg = a.rowptr[row + 1] - a.rowptr[row];
  Acc c;
  acc_init(c);
  for (int seg = a.heavy_segptr[h]; seg < a.heavy_segptr[h + 1]; ++seg) {
    const float* p = a.partials + (size_t)seg * 4 * a.F8 + f0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      c.s[j] = c.s[j] + p[j];
      c.q[j] = c.q[j] + p[a.F8 + j];
      c.mx[j] = pna_dev::vmax(c.mx[j], p[2 * a.F8 + j]);
      c.mn[j] = pna_dev::vmin(c.mn[j], p[3 * a.F8 + j]);
    }
  }
  finish_row<VOUT>(a, row, deg, f0, c);
}

}  // namespace pna_bf16
