// pna_net_ends.hip -- the two ENDS of the molecule nets for gfx950: the sum of embedding tables that opens them (ogb's AtomEncoder as
// nets/HIV_graph_classification/pna_net.py:42 uses it, the single nn.Embedding of nets/molecules_graph_regression/pna_net.py:68-73)
// and the per-graph readout that closes them (dgl.sum_nodes / mean_nodes / max_nodes, pna_net.py:83-90), forward and backward as ONE
// C call each.  Implements pna_embed_sum_{workspace_bytes, fwd_f32, bwd_f32} and pna_readout_{fwd_f32, bwd_f32} of include/pna_amd.h.
//
// Why: as torch ops the encoder is nine index_select + nine adds forward and a one_hot, a cast, a transpose and a GEMM per table
// backward; the readout goes through the generic aggregate (an arg-tracking gather over an identity edge list, then the generic
// backward over the same list), although its segments are contiguous node ranges.  On a molecule batch most of it is launch latency.
//
// Determinism: no atomics of any kind.  The embedding backward adds a slab's rows in row order in fp32 into an LDS image that one
// workgroup owns (one thread per column and table subset: no word is shared), then the slabs in slab order in float64.  The readout
// walks a graph's rows in order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "pna_amd.h"
#include "pna_internal.h"

namespace {

constexpr int kMaxTable = PNA_MAX_EMBED_TABLE;
constexpr int kMaxF = 256;                       // embedding width
constexpr long kImageBytes = 128 * 1024;         // the LDS image of all tables
constexpr int kSlabThreads = 1024;
constexpr int kChunk = 64;                       // rows whose image offsets are staged in LDS at a time
constexpr int kMaxReadoutF = 512;

struct EArgs {
  long V;
  int T, F, F4, total_rows;
  const int64_t* idx; long ld_idx;
  const float* table[kMaxTable];
  long ldt[kMaxTable];
  int rows[kMaxTable];
  int base[kMaxTable];      // first image row of table j
  float* out; long ldo;
  const float* go; long ld_go;
  float* gt[kMaxTable];
  float* ws;
  long slab;                // rows per slab
  int n_slab;
};

__device__ __forceinline__ int clamp_index(long x, int rows) { return (int)(x < 0 ? 0 : (x >= rows ? rows - 1 : x)); }

// ---- embedding forward: one thread per output element, the tables added in table order ------------------------------------------
__global__ __launch_bounds__(256) void k_embed_sum_fwd(const EArgs g) {
  const long n = g.V * g.F;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += (long)gridDim.x * 256L) {
    const long v = e / g.F;
    const int f = (int)(e - v * g.F);
    const int64_t* const iv = g.idx + v * g.ld_idx;
    float acc = 0.f;
    for (int j = 0; j < g.T; ++j) {
      const int r = clamp_index(iv[j], g.rows[j]);
      acc = acc + g.table[j][(long)r * g.ldt[j] + f];
    }
    g.out[v * g.ldo + f] = acc;
  }
}

// ---- embedding backward, launch 1: one slab of consecutive rows into an LDS image of all tables ---------------------------------
// lds: image (total_rows, F4) fp32 | off [kChunk][T] int32 (image offset of the row table j's index selects, clamped)
__global__ __launch_bounds__(kSlabThreads) void k_embed_sum_bwd_slab(const EArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int F = g.F, T = g.T;
  const int img = g.total_rows * g.F4;
  int* const off = (int*)(lds + img);
  for (int i = tid; i < img; i += kSlabThreads) lds[i] = 0.f;
  const long v0 = (long)blockIdx.x * g.slab;
  const long v1 = v0 + g.slab < g.V ? v0 + g.slab : g.V;
  const int per = kSlabThreads / F;                    // >= 4: F <= 256
  const int groups = per < T ? per : T;                // table subsets: group q owns tables q, q + groups, ...
  const int c = tid % F, grp = tid / F;
  const bool active = grp < groups;
  for (long vb = v0; vb < v1; vb += kChunk) {
    const int nr = (int)(v1 - vb < kChunk ? v1 - vb : kChunk);
    __syncthreads();                                   // the image is cleared / the previous chunk's offsets are consumed
    for (int i = tid; i < nr * T; i += kSlabThreads) {
      const int r = i / T, j = i - r * T;
      off[i] = (g.base[j] + clamp_index(g.idx[(vb + r) * g.ld_idx + j], g.rows[j])) * g.F4;
    }
    __syncthreads();
    if (active) {
      const float* gp = g.go + vb * g.ld_go + c;
      int r = 0;
      for (; r + 4 <= nr; r += 4) {                    // four rows' loads in flight, added in row order
        const float g0 = gp[(long)r * g.ld_go], g1 = gp[(long)(r + 1) * g.ld_go], g2 = gp[(long)(r + 2) * g.ld_go], g3 = gp[(long)(r + 3) * g.ld_go];
        for (int j = grp; j < T; j += groups) {
          float* p0 = lds + off[r * T + j] + c;       *p0 = *p0 + g0;
          float* p1 = lds + off[(r + 1) * T + j] + c; *p1 = *p1 + g1;
          float* p2 = lds + off[(r + 2) * T + j] + c; *p2 = *p2 + g2;
          float* p3 = lds + off[(r + 3) * T + j] + c; *p3 = *p3 + g3;
        }
      }
      for (; r < nr; ++r) {
        const float g0 = gp[(long)r * g.ld_go];
        for (int j = grp; j < T; j += groups) {
          float* p0 = lds + off[r * T + j] + c;
          *p0 = *p0 + g0;
        }
      }
    }
  }
  __syncthreads();
  float* const dst = g.ws + (long)blockIdx.x * img;
  for (int i = tid; i < img; i += kSlabThreads) dst[i] = lds[i];
}

// ---- embedding backward, launch 2: one thread per table element, the slabs added in slab order in float64 ------------------------
__global__ __launch_bounds__(256) void k_embed_sum_bwd_final(const EArgs g) {
  const long n = (long)g.total_rows * g.F;
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= n) return;
  const int R = (int)(e / g.F), f = (int)(e - (long)R * g.F);
  int j = 0;
  while (j + 1 < g.T && R >= g.base[j + 1]) ++j;
  const long img = (long)g.total_rows * g.F4;
  const float* p = g.ws + (long)R * g.F4 + f;
  double acc = 0.0;
  int s = 0;
  for (; s + 8 <= g.n_slab; s += 8) {                 // eight slabs' loads in flight, added in slab order
    float t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = p[(long)(s + k) * img];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += (double)t[k];
  }
  for (; s < g.n_slab; ++s) acc += (double)p[(long)s * img];
  g.gt[j][(long)(R - g.base[j]) * g.F + f] = (float)acc;
}

// ---- readout ----------------------------------------------------------------------------------------------------------------------
struct RArgs {
  const int32_t* off;
  int G, V, F, op;
  const float* h; long ldh;
  float* out; long ldo;
  int32_t* arg;
  const float* go; long ld_go;
  float* gh; long ld_gh;
};

__device__ __forceinline__ void segment_of(const RArgs& g, int gi, int& b, int& e) {
  b = g.off[gi]; e = g.off[gi + 1];
  b = b < 0 ? 0 : (b > g.V ? g.V : b);
  e = e < b ? b : (e > g.V ? g.V : e);
}

// one workgroup per graph, a thread per column, the graph's rows in order
__global__ __launch_bounds__(256) void k_readout_fwd(const RArgs g) {
  const int gi = blockIdx.x;
  int b, e;
  segment_of(g, gi, b, e);
  for (int f = threadIdx.x; f < g.F; f += blockDim.x) {
    const float* p = g.h + f;
    if (g.op == PNA_AGG_MAX) {
      float mx = -INFINITY;
      int ax = -1;
      for (int v = b; v < e; ++v) {                     // pna_segreduce.hip's fold: strict, the first extremal row wins, NaN sticky
        const float m = p[(long)v * g.ldh];
        const bool gx = m > mx || (m != m && mx == mx);
        mx = gx ? m : mx; ax = gx ? v : ax;
      }
      g.out[(long)gi * g.ldo + f] = mx;
      g.arg[(long)gi * g.F + f] = ax;
    } else {
      float s = 0.f;
      for (int v = b; v < e; ++v) s = s + p[(long)v * g.ldh];
      if (g.op == PNA_AGG_MEAN) s = e > b ? s / (float)(e - b) : 0.f;
      g.out[(long)gi * g.ldo + f] = s;
    }
  }
}

__global__ __launch_bounds__(256) void k_readout_bwd(const RArgs g) {
  const int gi = blockIdx.x;
  int b, e;
  segment_of(g, gi, b, e);
  for (int f = threadIdx.x; f < g.F; f += blockDim.x) {
    const float go = g.go[(long)gi * g.ld_go + f];
    float* p = g.gh + f;
    if (g.op == PNA_AGG_MAX) {
      const int ax = g.arg[(long)gi * g.F + f];
      for (int v = b; v < e; ++v) p[(long)v * g.ld_gh] = v == ax ? go : 0.f;
    } else {
      const float t = g.op == PNA_AGG_MEAN ? go / (float)(e - b) : go;
      for (int v = b; v < e; ++v) p[(long)v * g.ld_gh] = t;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
inline int round4(int F) { return (F + 3) / 4 * 4; }
inline long slab_rows(long V) {
  const long l = (V + PNA_EMBED_MAX_SLABS - 1) / PNA_EMBED_MAX_SLABS;
  return l > PNA_EMBED_SLAB_ROWS ? l : PNA_EMBED_SLAB_ROWS;
}

// total image rows, or -1 outside the scope
long embed_scope(int64_t V, int n_table, const int32_t* rows, int F) {
  if (V < 1 || V > INT32_MAX || n_table < 1 || n_table > kMaxTable || F < 1 || F > kMaxF || !rows) return -1;
  long total = 0;
  for (int j = 0; j < n_table; ++j) {
    if (rows[j] < 1) return -1;
    total += rows[j];
    if (total * round4(F) * 4 > kImageBytes) return -1;
  }
  return total;
}

int fill_embed(const pna_embed_sum_args* p, EArgs& g, bool bwd, const char* fn, const char* who) {
  if (!p) return pna_set_error(PNA_E_INVALID, who);
  if (int rc_ss = pna_check_struct_size(fn, p->struct_size, sizeof(*p))) return rc_ss;
  const long total = embed_scope(p->V, p->n_table, p->rows, p->F);
  if (total < 0 || !p->idx || p->ld_idx < (p->n_table > 1 ? p->n_table : 0)) return pna_set_error(PNA_E_INVALID, who);
  memset(&g, 0, sizeof(g));
  g.V = p->V; g.T = p->n_table; g.F = p->F; g.F4 = round4(p->F); g.total_rows = (int)total;
  g.idx = p->idx; g.ld_idx = (long)p->ld_idx;
  int base = 0;
  for (int j = 0; j < g.T; ++j) {
    if (!p->table[j] || p->ld_table[j] < p->F || (bwd && !p->grad_table[j])) return pna_set_error(PNA_E_INVALID, who);
    g.table[j] = p->table[j]; g.ldt[j] = (long)p->ld_table[j]; g.rows[j] = p->rows[j]; g.base[j] = base; g.gt[j] = p->grad_table[j];
    base += p->rows[j];
  }
  g.slab = slab_rows(g.V);
  g.n_slab = (int)((g.V + g.slab - 1) / g.slab);
  if (!bwd) {
    if (!p->out || p->ld_out < p->F) return pna_set_error(PNA_E_INVALID, who);
    g.out = p->out; g.ldo = (long)p->ld_out;
  } else {
    const int64_t need = (int64_t)g.n_slab * total * g.F4 * 4;
    if (!p->grad_out || p->ld_go < p->F || !p->workspace || ((uintptr_t)p->workspace & 15) || p->workspace_bytes < need)
      return pna_set_error(PNA_E_INVALID, who);
    g.go = p->grad_out; g.ld_go = (long)p->ld_go; g.ws = (float*)p->workspace;
  }
  return PNA_OK;
}

int fill_readout(const pna_readout_args* p, RArgs& g, bool bwd, const char* fn, const char* who) {
  if (!p) return pna_set_error(PNA_E_INVALID, who);
  if (int rc_ss = pna_check_struct_size(fn, p->struct_size, sizeof(*p))) return rc_ss;
  if (p->G < 1 || p->V < 1 || p->F < 1 || p->F > kMaxReadoutF || !p->offsets ||
      (p->op != PNA_AGG_SUM && p->op != PNA_AGG_MEAN && p->op != PNA_AGG_MAX) || (p->op == PNA_AGG_MAX && !p->argmax))
    return pna_set_error(PNA_E_INVALID, who);
  if (!bwd && (!p->h || p->ldh < p->F || !p->out || p->ld_out < p->F)) return pna_set_error(PNA_E_INVALID, who);
  if (bwd && (!p->grad_out || p->ld_go < p->F || !p->grad_h || p->ld_gh < p->F)) return pna_set_error(PNA_E_INVALID, who);
  memset(&g, 0, sizeof(g));
  g.off = p->offsets; g.G = p->G; g.V = p->V; g.F = p->F; g.op = p->op;
  g.h = p->h; g.ldh = (long)p->ldh; g.out = p->out; g.ldo = (long)p->ld_out; g.arg = p->argmax;
  g.go = p->grad_out; g.ld_go = (long)p->ld_go; g.gh = p->grad_h; g.ld_gh = (long)p->ld_gh;
  return PNA_OK;
}

inline unsigned readout_threads(int F) { return (unsigned)(F >= 256 ? 256 : (F + 63) / 64 * 64); }

}  // namespace

extern "C" int64_t pna_embed_sum_workspace_bytes(int64_t V, int32_t n_table, const int32_t* rows, int32_t F) {
  const long total = embed_scope(V, n_table, rows, F);
  if (total < 0) return -1;
  const long slab = slab_rows(V);
  return (int64_t)((V + slab - 1) / slab) * total * round4(F) * 4;
}

extern "C" int pna_embed_sum_fwd_f32(const pna_embed_sum_args* p, pna_stream_t stream) {
  EArgs g;
  const int rc = fill_embed(p, g, false, "pna_embed_sum_fwd_f32",
                            "pna_embed_sum_fwd_f32: needs V >= 1, 1 <= n_table <= 16, 1 <= F <= 256, rows_j >= 1 with sum_j rows_j * round4(F) * 4 <= 128 KiB, "
                            "idx (ld >= n_table), every table (ld >= F), out (ld >= F)");
  if (rc != PNA_OK) return rc;
  const long n = g.V * g.F;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_embed_sum_fwd, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_embed_sum_fwd_f32: launch failed");
  return PNA_OK;
}

extern "C" int pna_embed_sum_bwd_f32(const pna_embed_sum_args* p, pna_stream_t stream) {
  EArgs g;
  const int rc = fill_embed(p, g, true, "pna_embed_sum_bwd_f32",
                            "pna_embed_sum_bwd_f32: needs the forward's scope, idx and tables, grad_out (ld >= F), every grad_table, a 16-byte aligned workspace "
                            "of pna_embed_sum_workspace_bytes(V, n_table, rows, F)");
  if (rc != PNA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = ((size_t)g.total_rows * g.F4 + (size_t)kChunk * g.T) * sizeof(float);       // <= 132 KiB of the CU's 160
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)k_embed_sum_bwd_slab, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return pna_set_error(PNA_E_LAUNCH, "pna_embed_sum_bwd_f32: LDS attribute refused");
  hipLaunchKernelGGL(k_embed_sum_bwd_slab, dim3((unsigned)g.n_slab), dim3(kSlabThreads), lds, st, g);
  const long n = (long)g.total_rows * g.F;
  hipLaunchKernelGGL(k_embed_sum_bwd_final, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_embed_sum_bwd_f32: launch failed");
  return PNA_OK;
}

extern "C" int pna_readout_fwd_f32(const pna_readout_args* p, pna_stream_t stream) {
  RArgs g;
  const int rc = fill_readout(p, g, false, "pna_readout_fwd_f32",
                              "pna_readout_fwd_f32: needs G >= 1, V >= 1, 1 <= F <= 512, op among sum / mean / max, offsets [G+1], h (ld >= F), out (ld >= F), "
                              "argmax (G, F) for max");
  if (rc != PNA_OK) return rc;
  hipLaunchKernelGGL(k_readout_fwd, dim3((unsigned)g.G), dim3(readout_threads(g.F)), 0, (hipStream_t)stream, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_readout_fwd_f32: launch failed");
  return PNA_OK;
}

extern "C" int pna_readout_bwd_f32(const pna_readout_args* p, pna_stream_t stream) {
  RArgs g;
  const int rc = fill_readout(p, g, true, "pna_readout_bwd_f32",
                              "pna_readout_bwd_f32: needs the forward's scope and offsets, grad_out (ld >= F), grad_h (ld >= F), the forward's argmax for max");
  if (rc != PNA_OK) return rc;
  hipLaunchKernelGGL(k_readout_bwd, dim3((unsigned)g.G), dim3(readout_threads(g.F)), 0, (hipStream_t)stream, g);
  if (hipGetLastError() != hipSuccess) return pna_set_error(PNA_E_LAUNCH, "pna_readout_bwd_f32: launch failed");
  return PNA_OK;
}
