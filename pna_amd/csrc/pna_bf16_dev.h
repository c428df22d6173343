// pna_bf16_dev.h -- device helpers shared by the bf16 inference kernels (pna_bf16.hip, pna_bf16_tower.hip): the bf16 <-> fp32
// conversions, the per-lane statistics of the gather kernels (8 features per lane, fp32) and the finalisation of one row.
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

// finalize one row's statistics (pna_rowstats.h: the fp32 kernel's formulas) and store every aggregator block, rounded to bf16 once
template <bool VOUT>
__device__ __forceinline__ void finish_row(const SegArgs& a, int row, int deg, int f0, const Acc& c) {
  float mean[8], msq[8];
  const float D = (float)deg, invD = 1.0f / D;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mean[j] = pna_dev::div_rn(c.s[j], D, invD);
    msq[j] = pna_dev::div_rn(c.q[j], D, invD);
  }
  u16* o = a.out + (size_t)row * a.ldo + f0;
  const int nw = a.F - f0 < 8 ? a.F - f0 : 8;         // element stores: only the block's own features
  for (int ai = 0; ai < a.n_aggr; ++ai) {
    const int code = a.aggr[ai];
    u16 r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float val;
      if (deg <= 0 || f0 + j >= a.F) {
        val = 0.f;
      } else {
        float var = msq[j] - mean[j] * mean[j];
        var = var < 0.f ? 0.f : var;
        switch (code) {
          case PNA_AGG_MEAN: val = mean[j]; break;
          case PNA_AGG_SUM: val = c.s[j]; break;
          case PNA_AGG_MAX: val = c.q[j] != c.q[j] ? c.q[j] : c.mx[j]; break;
          case PNA_AGG_MIN: val = c.q[j] != c.q[j] ? c.q[j] : c.mn[j]; break;
          case PNA_AGG_STD: val = sqrtf(var + 1e-5f); break;
          default: val = var; break;                   // PNA_AGG_VAR
        }
      }
      r[j] = f2bf(val);
    }
    u16* ob = o + (size_t)ai * a.bs;
    if (VOUT) {
      u4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = (unsigned)r[2 * j] | ((unsigned)r[2 * j + 1] << 16);
      *reinterpret_cast<u4*>(ob) = w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < nw) ob[j] = r[j];
    }
  }
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
