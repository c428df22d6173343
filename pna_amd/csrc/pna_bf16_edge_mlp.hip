// pna_bf16_edge_mlp.hip -- the hidden layers of a deep pre_nn per edge for gfx950 (MI355X, CDNA4): pna_edge_mlp_bf16, the bf16
// inference of PNAConv(pre_layers >= 2) in the PyG front end.  See include/pna_amd.h for the arguments and the arithmetic contract,
// DESIGN.md 4.14 for the layout.
//
// One workgroup (4 wavefronts) serves one tower: its n_hidden weight matrices are copied into LDS once, then every wavefront walks
// tiles of 16 consecutive CSR edges on its own (no workgroup barrier after the copy).
//   layer 2   in v_mfma_f32_16x16x32_bf16 lane l holds A[row l & 15][k = 8 (l >> 4) + j]: the lane's three 16-byte loads of edge
//             k0 + (l & 15) -- x_src[col], x_dst[row], the edge row -- added in fp32, clamped at 0 and rounded ARE its A fragment.
//   B         the weight rows n0 + (l & 15), columns 32 c + 8 (l >> 4), read from LDS with ds_read_b128.  That instruction serves
//             the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...: all 16 rows, eight at column quad q and eight at
//             q + 1.  With a row pitch of m 16-byte slots the slot of (row r, quad q) is r m + q mod 16; the rows are round32(Fp)
//             elements = 4, 8, 12 or 16 slots wide, and a pad of TWO slots makes m = 2 (mod 4): r m takes the 8 even residues
//             twice, 8 rows apart, and rows 8 apart sit in different quads of a group -- one odd, one even.  16 slots, no conflict.
//   result    lane l holds C[row 4 (l >> 4) + i][col l & 15]: bias, ReLU and the rounding there, then one transpose through the
//             wavefront's own 16-row LDS tile gives the A fragments of the next layer or the 16-byte pieces of the output rows.
// A partial last tile re-reads the last valid edge and stores nothing for the rows beyond E.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_bf16_dev.h"

namespace {

using namespace pna_bf16;

constexpr int kTile = 16;                     // CSR edges per wavefront tile
constexpr int kWPad = 16;                     // elements of padding per weight row in LDS (two 16-byte slots: see above)
constexpr int kZPad = 8;                      // ... per row of a wavefront's tile
constexpr size_t kLdsMax = 160 * 1024;
constexpr int kMaxBlocks = 2048;              // workgroups of a launch over all towers: each copies its tower's weights once

struct EArgs {
  int E, F, Fp, Np, nh, n_er;
  long n_tiles;
  const int32_t* col; const int32_t* row;
  const u16* xs; int64_t lds; const u16* xd; int64_t ldd;
  const u16* er; int64_t lde; const int32_t* et;
  const u16* w; const u16* bias;
  u16* out; int64_t ldo;
};

int round_up(int x, int m) { return (x + m - 1) / m * m; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

size_t lds_bytes(int F, int nh) {
  const int Kp = round_up(round_up(F, 8), 32), Np = round_up(F, 16);
  return ((size_t)nh * Np * (Kp + kWPad) + (size_t)(kBlock / 64) * kTile * (Kp + kZPad)) * sizeof(u16);
}

// writes of this wavefront to its LDS tile are visible to its own later reads (the LDS serves a wavefront's accesses in order; this
// keeps the compiler from moving them across)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// NC = round32(Fp) / 32 column chunks of 32: the A fragments of a tile stay in registers under a compile-time index
template <int NC>
__global__ __launch_bounds__(kBlock) void k_edge_mlp_bf16(const EArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  constexpr int Kp = NC * 32, WP = Kp + kWPad, ZP = Kp + kZPad;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = blockIdx.y;
  u16* wl = reinterpret_cast<u16*>(lds_raw);                               // [nh][Np][WP]
  u16* zall = wl + (size_t)a.nh * a.Np * WP;                               // [4][16][ZP]
  u16* zt = zall + wave * kTile * ZP;
  {
    const u16* wg = a.w + (size_t)t * a.nh * a.Np * Kp;
    const int n16 = a.nh * a.Np * (Kp / 8);
    for (int i = tid; i < n16; i += kBlock) {
      const int r = i / (Kp / 8), c = i - r * (Kp / 8);
      *reinterpret_cast<u4*>(wl + (size_t)r * WP + c * 8) = *reinterpret_cast<const u4*>(wg + (size_t)r * Kp + c * 8);
    }
    // the tiles start as zeros: their columns [Np, Kp) are never written and take part in the MFMAs
    for (int i = tid; i < (kBlock / 64) * kTile * ZP / 8; i += kBlock) reinterpret_cast<u4*>(zall)[i] = (u4){0u, 0u, 0u, 0u};
  }
  __syncthreads();

  const int q = lane >> 4, r = lane & 15, c0 = t * a.Fp;
  for (long tile = (long)blockIdx.x * (kBlock / 64) + wave; tile < a.n_tiles; tile += (long)gridDim.x * (kBlock / 64)) {
    const long e0 = tile * kTile;
    const long e = e0 + r < a.E ? e0 + r : (long)a.E - 1;
    const u16* ps = a.xs + (size_t)a.col[e] * a.lds + c0;
    const u16* pd = a.xd + (size_t)a.row[e] * a.ldd + c0;
    const u16* pe = nullptr;
    if (a.er) {
      size_t er = (size_t)e;
      if (a.et) {
        int ty = a.et[e];
        ty = ty < 0 ? 0 : ty >= a.n_er ? a.n_er - 1 : ty;                // a type outside the table reads a row of the table
        er = (size_t)ty;
      }
      pe = a.er + er * a.lde + c0;
    }
    // ---- z_1: the A fragments of the first matrix layer
    bf8 A[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int k = c * 32 + 8 * q;
      u16 z[8];
      if (k < a.Fp) {
        float s[8], d[8];
        load8<true>(ps + k, 8, s);
        load8<true>(pd + k, 8, d);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = s[j] + d[j];
        if (pe) {
          load8<true>(pe + k, 8, d);
#pragma unroll
          for (int j = 0; j < 8; ++j) s[j] = s[j] + d[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = k + j < a.F ? f2bf(s[j] < 0.f ? 0.f : s[j]) : (u16)0;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = 0;
      }
      u4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = (unsigned)z[2 * j] | ((unsigned)z[2 * j + 1] << 16);
      A[c] = __builtin_bit_cast(bf8, w);
    }
    // ---- the matrix layers
    for (int li = 0; li < a.nh; ++li) {
      if (li > 0) {
        wave_sync();
#pragma unroll
        for (int c = 0; c < NC; ++c) A[c] = __builtin_bit_cast(bf8, *reinterpret_cast<const u4*>(zt + r * ZP + c * 32 + 8 * q));
        wave_sync();                                                      // (every lane holds its fragments before the tile is rewritten)
      }
      const u16* wli = wl + (size_t)li * a.Np * WP;
      const u16* bl = a.bias + ((size_t)t * a.nh + li) * a.F;
      const bool last = li == a.nh - 1;
      for (int nt = 0; nt < a.Np / 16; ++nt) {
        const int n = nt * 16 + r;
        const u16* wp = wli + (size_t)n * WP + 8 * q;
        f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c)
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[c], __builtin_bit_cast(bf8, *reinterpret_cast<const u4*>(wp + c * 32)), acc, 0, 0, 0);
        const float b = n < a.F ? bf2f(bl[n]) : 0.f;                     // (the weight rows [F, Np) are zero: those columns become 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float z = acc[i] + b;
          if (!last) z = z < 0.f ? 0.f : z;
          zt[(4 * q + i) * ZP + n] = f2bf(z);
        }
      }
    }
    // ---- the output rows, columns [0, Fp) of the tower's block, in 16-byte pieces
    wave_sync();
    if (e0 + r < a.E) {
      u16* o = a.out + (size_t)(e0 + r) * a.ldo + c0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int k = c * 32 + 8 * q;
        if (k < a.Fp) *reinterpret_cast<u4*>(o + k) = *reinterpret_cast<const u4*>(zt + r * ZP + k);
      }
    }
    wave_sync();
  }
}

template <int NC>
hipError_t launch(const EArgs& g, int T, size_t lds, hipStream_t st) {
  auto* fn = k_edge_mlp_bf16<NC>;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const long want = (g.n_tiles + kBlock / 64 - 1) / (kBlock / 64), cap = kMaxBlocks / T > 0 ? kMaxBlocks / T : 1;
  hipLaunchKernelGGL(fn, dim3((unsigned)(want < cap ? want : cap), (unsigned)T), dim3(kBlock), lds, st, g);
  return hipGetLastError();
}

int fail(const char* what) { return pna_set_error(PNA_E_INVALID, what); }

}  // namespace

extern "C" int64_t pna_edge_mlp_bf16_lds_bytes(int32_t F, int32_t n_hidden) {
  if (F < 1 || F > 128 || n_hidden < 1 || n_hidden > 64) return -1;
  return (int64_t)lds_bytes(F, n_hidden);
}

extern "C" int pna_edge_mlp_bf16(const pna_edge_mlp_bf16_args* p, pna_stream_t stream) {
  if (!p) return fail("pna_edge_mlp_bf16: null args");
  if (int rc_ss = pna_check_struct_size("pna_edge_mlp_bf16", p->struct_size, sizeof(*p))) return rc_ss;
  if (p->E < 0 || p->T < 1 || p->T > 64 || p->F < 1 || p->F > 128 || p->n_hidden < 1 || p->n_hidden > 64)
    return fail("pna_edge_mlp_bf16: need E >= 0, 1 <= T <= 64, 1 <= F <= 128, 1 <= n_hidden <= 64");
  const int Fp = round_up(p->F, 8), W = p->T * Fp;
  const size_t lds = lds_bytes(p->F, p->n_hidden);
  if (lds > kLdsMax) return fail("pna_edge_mlp_bf16: the hidden weights of one tower do not fit 160 KiB of LDS");
  if (p->edge_type && (!p->edge_rows || p->n_edge_rows < 1)) return fail("pna_edge_mlp_bf16: edge_type needs edge_rows with n_edge_rows >= 1");
  if (p->E == 0) return PNA_OK;
  if (!p->w_img || !p->bias || !aligned16(p->w_img)) return fail("pna_edge_mlp_bf16: w_img (16-byte aligned) and bias must be non-null");
  if (!p->out || !aligned16(p->out) || p->ld_out % 8 != 0 || p->ld_out < W)
    return fail("pna_edge_mlp_bf16: out must be 16-byte aligned rows of >= T round8(F) columns, ld_out a multiple of 8");
  if (!p->col || !p->row || !p->x_src || !p->x_dst) return fail("pna_edge_mlp_bf16: col/row/x_src/x_dst must be non-null");
  auto rows_ok = [&](const void* q, int64_t ld) { return aligned16(q) && ld % 8 == 0 && ld >= W; };
  if (!rows_ok(p->x_src, p->ld_src) || !rows_ok(p->x_dst, p->ld_dst) || (p->edge_rows && !rows_ok(p->edge_rows, p->ld_edge)))
    return fail("pna_edge_mlp_bf16: x_src / x_dst / edge_rows must be 16-byte aligned rows of >= T round8(F) columns, pitches multiples of 8");

  EArgs g{};
  g.E = p->E; g.F = p->F; g.Fp = Fp; g.Np = round_up(p->F, 16); g.nh = p->n_hidden; g.n_er = p->n_edge_rows;
  g.n_tiles = ((long)p->E + kTile - 1) / kTile;
  g.col = p->col; g.row = p->row;
  g.xs = reinterpret_cast<const u16*>(p->x_src); g.lds = p->ld_src;
  g.xd = reinterpret_cast<const u16*>(p->x_dst); g.ldd = p->ld_dst;
  g.er = reinterpret_cast<const u16*>(p->edge_rows); g.lde = p->ld_edge; g.et = p->edge_type;
  g.w = reinterpret_cast<const u16*>(p->w_img); g.bias = reinterpret_cast<const u16*>(p->bias);
  g.out = reinterpret_cast<u16*>(p->out); g.ldo = p->ld_out;

  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  switch (round_up(Fp, 32) / 32) {
    case 1: e = launch<1>(g, p->T, lds, st); break;
    case 2: e = launch<2>(g, p->T, lds, st); break;
    case 3: e = launch<3>(g, p->T, lds, st); break;
    default: e = launch<4>(g, p->T, lds, st); break;
  }
  if (e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  return PNA_OK;
}
