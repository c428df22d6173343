// pna_batch_plan.hip -- every index array a fresh batch of small graphs needs, from one call.
// Implements pna_batch_plan_i32 / pna_batch_plan_limits / pna_batch_plan_workspace_bytes of include/pna_amd.h.
//
// The reference batches on the host (realworld_benchmark/data/molecules.py:153-164); pna_amd built the batch's arrays lazily, one chain
// of small launches and host reads per array (graph.py collate_flat / work_items / snorm_n / degree_scalers, autograd.py
// _transposed_whole_rows).  A batch of disjoint graphs is block diagonal: member g's CSR rows lie inside its own edge range, so a
// workgroup can sort a few consecutive members in LDS and never look at another workgroup's output.  Two launches: k_plan_scan (offsets,
// groups of members, the record) and k_plan_groups (one workgroup per group: counts, scans, an in-order placement per wavefront).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pna_amd.h"
#include "pna_internal.h"
#include "pna_scalers_dev.h"

namespace {

constexpr int kBlock = 256;          // k_plan_groups: four wavefronts
constexpr int kWaves = kBlock / 64;
constexpr int kScanBlock = 1024;     // k_plan_scan: one workgroup
constexpr int kSmallNodes = 256;     // a member above either is a group of its own; the windows of the smaller ones
constexpr int kSmallEdges = 1024;
constexpr int kGroupMembers = 128;   // members per group at most (their offsets are staged in LDS)
constexpr int kLimitNodes = 2048;    // pna_batch_plan_limits
constexpr int kLimitEdges = 8192;

constexpr int64_t lds_bytes(int64_t cap_n, int64_t cap_e) { return 4 * (2 * cap_e + kWaves * cap_n + 3 * (cap_n + 1)); }
static_assert(lds_bytes(kLimitNodes, kLimitEdges) + 4096 <= 160 * 1024, "the limits must fit one workgroup's LDS");
static_assert(kLimitNodes >= 512 && kLimitEdges >= 4096 && 2 * kSmallNodes <= kLimitNodes && 2 * kSmallEdges <= kLimitEdges, "limits");

__host__ __device__ inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct PlanK {
  const int32_t* src_local; const int32_t* dst_local;
  const int32_t* node_off; const int32_t* edge_off; const int32_t* group_first; const int32_t* n_groups;
  int32_t cap_n, cap_e, want_t;
  float avg_log, inv_avg;
  int64_t* src; int64_t* dst;
  int32_t* rowptr; int32_t* col; int32_t* row; int32_t* eid; int64_t* eid64; int32_t* items; float* snorm_n;
  int32_t* rowptr_t; int32_t* col_t; int32_t* row_t; int32_t* pos_t; int64_t* pos_t64; int32_t* rank_t; int32_t* items_t;
  int64_t* row64; int64_t* col64;
  float* amp; float* att;
  int32_t* record;
};

// ---- launch 1: offsets, groups, record -------------------------------------------------------------------------------------------------
// Inclusive scan of one value per thread over the workgroup (Hillis-Steele in LDS); returns the thread's inclusive value.
template <typename T, int N>
__device__ inline T block_inclusive(T v, T* buf) {
  const int t = threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (int off = 1; off < N; off <<= 1) {
    const T add = t >= off ? buf[t - off] : (T)0;
    __syncthreads();
    buf[t] += add;
    __syncthreads();
  }
  const T r = buf[t];
  __syncthreads();
  return r;
}

__device__ inline int clamp_count(int c) { return c < 0 ? 0 : c; }

__global__ __launch_bounds__(kScanBlock) void k_plan_scan(const int32_t* __restrict__ node_count, const int32_t* __restrict__ edge_count,
                                                         int B, int V, int E, int grid_groups, int32_t* node_off, int32_t* edge_off,
                                                         int32_t* group_first, int32_t* n_groups, int32_t* readout, int32_t* rowptr,
                                                         int32_t* rowptr_t, int32_t* record) {
  __shared__ long long bufn[kScanBlock];
  __shared__ long long bufe[kScanBlock];
  __shared__ int bufg[kScanBlock];
  __shared__ int s_bad;
  const int t = threadIdx.x;
  const long long per = ((long long)B + kScanBlock - 1) / kScanBlock;
  const int lo = (int)(t * per < B ? t * per : B);
  const int hi = (int)(lo + per < B ? lo + per : B);
  if (t == 0) s_bad = 0;
  __syncthreads();
  long long sn = 0, se = 0;
  int bad = 0;
  for (int g = lo; g < hi; ++g) {
    const int n = node_count[g], e = edge_count[g];
    bad |= (n < 0) | (e < 0);
    sn += clamp_count(n);
    se += clamp_count(e);
  }
  const long long in_n = block_inclusive<long long, kScanBlock>(sn, bufn);
  const long long in_e = block_inclusive<long long, kScanBlock>(se, bufe);
  const long long tot_n = bufn[kScanBlock - 1], tot_e = bufe[kScanBlock - 1];
  bad |= (tot_n != V) | (tot_e != E);
  if (bad) atomicOr(&s_bad, 1);
  __syncthreads();
  const bool consistent = s_bad == 0;            // offsets end at V and E: every range below lies inside the caller's buffers
  // a member starts a group when it or its predecessor is large, or when it leaves its predecessor's node / edge / index window
  auto walk = [&](int base_g, bool store) {
    long long no = in_n - sn, eo = in_e - se;
    int flags = 0;
    for (int g = lo; g < hi; ++g) {
      const int n = clamp_count(node_count[g]), e = clamp_count(edge_count[g]);
      bool f = g == 0 || (g % kGroupMembers) == 0 || n > kSmallNodes || e > kSmallEdges;
      if (g > 0 && !f) {
        const int pn = clamp_count(node_count[g - 1]), pe = clamp_count(edge_count[g - 1]);
        f = pn > kSmallNodes || pe > kSmallEdges || no / kSmallNodes != (no - pn) / kSmallNodes || eo / kSmallEdges != (eo - pe) / kSmallEdges;
      }
      if (store) {
        if (consistent) {
          node_off[g] = (int)no;
          edge_off[g] = (int)eo;
          if (readout) readout[g] = (int)no;
          if (f) group_first[base_g + flags] = g;
        }
      }
      flags += f ? 1 : 0;
      no += n;
      eo += e;
    }
    return flags;
  };
  const int nf = walk(0, false);
  const int in_g = block_inclusive<int, kScanBlock>(nf, bufg);
  const int ng = bufg[kScanBlock - 1];
  walk(in_g - nf, true);
  if (t == 0) {
    const bool fits = ng <= grid_groups;         // (cannot fail: the grid is the bound derived in include/pna_amd.h)
    if (consistent) {
      node_off[B] = V;
      edge_off[B] = E;
      group_first[ng] = B;
      if (readout) readout[B] = V;
      if (rowptr) rowptr[V] = E;
      if (rowptr_t) rowptr_t[V] = E;
    }
    n_groups[0] = consistent && fits ? ng : 0;
    record[0] = 0;
    record[1] = 0;
    record[2] = consistent && fits ? 0 : 2;
    record[3] = 0;
  }
}

// ---- launch 2: one workgroup per group --------------------------------------------------------------------------------------------------
// largest m in [0, nm) with ofs[m] <= x, for ofs[0] <= x < ofs[nm]: the member that owns node / edge x (empty members are skipped)
__device__ inline int member_of(const int* ofs, int nm, int x) {
  int lo = 0, hi = nm;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ofs[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// How many LOWER lanes of the wavefront hold `key`, and whether a higher lane does.  Called by all 64 lanes together.
__device__ inline void wave_rank(int key, int lane, int& lower, int& higher) {
  lower = 0;
  higher = 0;
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    const int eq = __builtin_amdgcn_readlane(key, j) == key;
    lower += (j < lane) & eq;
    higher |= (j > lane) & eq;
  }
}

// S[0 .. n] = exclusive scan over v of the four wavefronts' counters cnt[w n + v]; S[n] = the total.  Returns the largest count.
__device__ inline int scan_counts(const int* cnt, int n, int* S, int* part, int* s_max) {
  const int t = threadIdx.x;
  const int per = (n + kBlock - 1) / kBlock;
  const int lo = t * per < n ? t * per : n;
  const int hi = lo + per < n ? lo + per : n;
  int sum = 0, mx = 0;
  for (int v = lo; v < hi; ++v) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += cnt[w * n + v];
    sum += c;
    mx = c > mx ? c : mx;
  }
  if (t == 0) *s_max = 0;
  const int incl = block_inclusive<int, kBlock>(sum, part);
  if (mx > 0) atomicMax(s_max, mx);
  int run = incl - sum;
  for (int v = lo; v < hi; ++v) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += cnt[w * n + v];
    S[v] = run;
    run += c;
  }
  if (t == kBlock - 1) S[n] = incl;
  __syncthreads();
  return *s_max;
}

// R[v] = first CSR position (relative to the group) of row v: the scan restarted at every member's own edge offset, so that a
// member with a refused edge leaves its hole at the end of ITS range and its neighbours' rows stay where they are.  Then the
// wavefronts' counters become their first free positions.
__device__ inline void rows_and_bases(int* cnt, int n, int e, const int* S, int* R, const int* nofs, const int* eofs, int nm) {
  for (int v = threadIdx.x; v < n; v += kBlock) {
    const int m = member_of(nofs, nm, v);
    int run = S[v] - S[nofs[m]] + eofs[m];
    R[v] = run;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int c = cnt[w * n + v];
      cnt[w * n + v] = run;
      run += c;
    }
  }
  if (threadIdx.x == 0) R[n] = e;
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void k_plan_groups(const PlanK k) {
  extern __shared__ int lds[];
  __shared__ int nofs[kGroupMembers + 1];
  __shared__ int eofs[kGroupMembers + 1];
  __shared__ int part[kBlock];
  __shared__ int s_max;
  const int grp = blockIdx.x;
  if (grp >= k.n_groups[0]) return;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int gfirst = k.group_first[grp], gend = k.group_first[grp + 1];
  const int nm = gend - gfirst;
  const int nbase = k.node_off[gfirst], ebase = k.edge_off[gfirst];
  const int n = k.node_off[gend] - nbase, e = k.edge_off[gend] - ebase;
  if (nm < 1 || nm > kGroupMembers || n > k.cap_n || e > k.cap_e || n < 0 || e < 0) {      // larger than the caller declared: skipped
    if (t == 0) atomicOr(&k.record[2], 2);
    return;
  }
  int* colL = lds;                       // [e] source of the CSR edge at position p (group-local id), -1 = a refused edge's hole
  int* rowL = colL + k.cap_e;            // [e] its destination
  int* cnt = rowL + k.cap_e;             // [4, n] per wavefront and row: the count, then the first free position
  int* S = cnt + kWaves * k.cap_n;       // [n + 1]
  int* Rf = S + k.cap_n + 1;             // [n + 1] forward rowptr, relative to the group
  int* Rt = Rf + k.cap_n + 1;            // [n + 1] transposed rowptr
  for (int i = t; i <= nm; i += kBlock) {
    nofs[i] = k.node_off[gfirst + i] - nbase;
    eofs[i] = k.edge_off[gfirst + i] - ebase;
  }
  for (int i = t; i < kWaves * n; i += kBlock) cnt[i] = 0;
  for (int p = t; p < e; p += kBlock) colL[p] = -1;
  __syncthreads();
  // every wavefront owns a run of `chunk` consecutive edges (a multiple of 64)
  const int chunk = ((e + kWaves - 1) / kWaves + 63) & ~63;
  const int steps = chunk / 64;
  const int kbeg = w * chunk;
  const int kend = kbeg + chunk < e ? kbeg + chunk : e;
  // one edge: its member, the bounds check, group-local ids
  auto load_edge = [&](int kk, int& s, int& d) {
    const int sl = k.src_local[ebase + kk], dl = k.dst_local[ebase + kk];
    const int m = member_of(eofs, nm, kk);
    const int nn = nofs[m + 1] - nofs[m];
    const bool ok = (unsigned)sl < (unsigned)nn && (unsigned)dl < (unsigned)nn;
    s = nofs[m] + sl;
    d = nofs[m] + dl;
    return ok;
  };
  int bad = 0;
  for (int kk = kbeg + lane; kk < kend; kk += 64) {
    int s, d;
    if (load_edge(kk, s, d)) atomicAdd(&cnt[w * n + d], 1);
    else bad = 1;
  }
  if (bad) atomicOr(&k.record[2], 1);
  __syncthreads();
  const int max_in = scan_counts(cnt, n, S, part, &s_max);
  if (t == 0 && max_in > 0) atomicMax(&k.record[0], max_in);
  rows_and_bases(cnt, n, e, S, Rf, nofs, eofs, nm);
  // per-node outputs of the forward graph
  for (int v = t; v < n; v += kBlock) {
    const int gv = nbase + v;
    const int beg = ebase + Rf[v], end = ebase + Rf[v + 1];
    if (k.rowptr) k.rowptr[gv] = beg;
    if (k.items) reinterpret_cast<int4*>(k.items)[gv] = make_int4(gv, beg, end, -1);
    if (k.snorm_n) {
      const int m = member_of(nofs, nm, v);
      const float nf = (float)(nofs[m + 1] - nofs[m]);
      k.snorm_n[gv] = sqrtf(__fdiv_rn(1.0f, nf));           // correctly rounded both (not __fsqrt_rn: it is the bare v_sqrt_f32, 1 ulp low on one size in six)
    }
    if (k.amp || k.att) {
      float fa, ft;
      pna_degree_scalers_row(S[v + 1] - S[v], k.avg_log, k.inv_avg, fa, ft);
      if (k.amp) k.amp[gv] = fa;
      if (k.att) k.att[gv] = ft;
    }
  }
  // placement: in order, 64 edges of the wavefront's run a step
  for (int st = 0; st < steps; ++st) {
    const int kk = kbeg + st * 64 + lane;
    int s = 0, d = 0;
    const bool ok = kk < kend && load_edge(kk, s, d);
    int lower, higher;
    wave_rank(ok ? d : -1 - lane, lane, lower, higher);
    if (ok) {
      const int pos = cnt[w * n + d] + lower;
      if (pos < e) {
        const int64_t gp = (int64_t)ebase + pos, gk = (int64_t)ebase + kk;
        colL[pos] = s;
        rowL[pos] = d;
        if (k.col) k.col[gp] = nbase + s;
        if (k.row) k.row[gp] = nbase + d;
        if (k.eid) k.eid[gp] = (int32_t)gk;
        if (k.eid64) k.eid64[gp] = gk;
        if (k.row64) k.row64[gp] = nbase + d;
        if (k.col64) k.col64[gp] = nbase + s;
        if (k.src) k.src[gk] = nbase + s;
        if (k.dst) k.dst[gk] = nbase + d;
      }
      if (!higher) cnt[w * n + d] = pos + 1;
    }
    __syncthreads();
  }
  if (!k.want_t) return;
  // the transposed graph: CSR position p is the edge row[p] -> col[p]; the same walk over p with the source as key
  for (int i = t; i < kWaves * n; i += kBlock) cnt[i] = 0;
  __syncthreads();
  for (int p = kbeg + lane; p < kend; p += 64) {
    const int u = colL[p];
    if (u >= 0) atomicAdd(&cnt[w * n + u], 1);
  }
  __syncthreads();
  const int max_out = scan_counts(cnt, n, S, part, &s_max);
  if (t == 0 && max_out > 0) atomicMax(&k.record[1], max_out);
  rows_and_bases(cnt, n, e, S, Rt, nofs, eofs, nm);
  for (int v = t; v < n; v += kBlock) {
    const int gv = nbase + v;
    const int beg = ebase + Rt[v], end = ebase + Rt[v + 1];
    if (k.rowptr_t) k.rowptr_t[gv] = beg;
    if (k.items_t) reinterpret_cast<int4*>(k.items_t)[gv] = make_int4(gv, beg, end, -1);
  }
  for (int st = 0; st < steps; ++st) {
    const int p = kbeg + st * 64 + lane;
    const int u = p < kend ? colL[p] : -1;
    const bool ok = u >= 0;
    int lower, higher;
    wave_rank(ok ? u : -1 - lane, lane, lower, higher);
    if (ok) {
      const int q = cnt[w * n + u] + lower;
      if (q < e) {
        const int64_t gq = (int64_t)ebase + q, gp = (int64_t)ebase + p;
        const int v = rowL[p];
        if (k.col_t) k.col_t[gq] = nbase + v;
        if (k.row_t) k.row_t[gq] = nbase + u;
        if (k.pos_t) k.pos_t[gq] = (int32_t)gp;
        if (k.pos_t64) k.pos_t64[gq] = gp;
        if (k.rank_t) k.rank_t[gq] = p - Rf[v];
      }
      if (!higher) cnt[w * n + u] = q + 1;
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int pna_batch_plan_limits(int32_t* max_member_nodes, int32_t* max_member_edges) {
  if (max_member_nodes) *max_member_nodes = kLimitNodes;
  if (max_member_edges) *max_member_edges = kLimitEdges;
  return PNA_OK;
}

extern "C" int64_t pna_batch_plan_workspace_bytes(int32_t B, int64_t E, int64_t V) {
  if (B < 1 || E < 0 || V < 0 || E >= ((int64_t)1 << 31) || V >= ((int64_t)1 << 31)) return -1;
  return align256(4 * (3 * ((int64_t)B + 1) + 4));
}

extern "C" int pna_batch_plan_i32(const pna_batch_plan_args* a, pna_stream_t stream) {
  const char* fn = "pna_batch_plan_i32";
  if (!a) return pna_refuse(fn, "null args");
  if (int rc = pna_check_struct_size(fn, a->struct_size, sizeof(pna_batch_plan_args))) return rc;
  if (a->B < 1 || a->E < 0 || a->V < 0) return pna_refuse(fn, "outside the scope: 1 <= B, 0 <= E, 0 <= V");
  if (a->member_nodes_max < 0 || a->member_nodes_max > kLimitNodes || a->member_edges_max < 0 || a->member_edges_max > kLimitEdges)
    return pna_refuse(fn, "outside the scope: a member above pna_batch_plan_limits (2048 nodes, 8192 edges)");
  if (!a->edge_count || !a->node_count || !a->record || (a->E > 0 && (!a->src_local || !a->dst_local))) return pna_refuse(fn, "null pointer");
  const int64_t need = pna_batch_plan_workspace_bytes(a->B, a->E, a->V);
  if (!a->workspace || a->workspace_bytes < need) return pna_refuse(fn, "workspace too small");
  if (((uintptr_t)a->items | (uintptr_t)a->items_t) & 15) return pna_refuse(fn, "items / items_t must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int32_t* ws = (int32_t*)a->workspace;
  int32_t* node_off = ws;
  int32_t* edge_off = node_off + a->B + 1;
  int32_t* group_first = edge_off + a->B + 1;
  int32_t* n_groups = group_first + a->B + 1;
  const int64_t bound = 1 + 3 * ((int64_t)a->V / kSmallNodes + (int64_t)a->E / kSmallEdges) + a->B / kGroupMembers;
  const int grid = (int)(bound < a->B ? bound : a->B);
  const bool with_scalers = a->avg_log > 0.f;
  PlanK k{};
  k.src_local = a->src_local; k.dst_local = a->dst_local;
  k.node_off = node_off; k.edge_off = edge_off; k.group_first = group_first; k.n_groups = n_groups;
  k.cap_n = a->member_nodes_max > 2 * kSmallNodes ? a->member_nodes_max : 2 * kSmallNodes;
  k.cap_e = a->member_edges_max > 2 * kSmallEdges ? a->member_edges_max : 2 * kSmallEdges;
  k.want_t = a->want_transposed ? 1 : 0;
  k.avg_log = a->avg_log;
  k.inv_avg = with_scalers ? 1.0f / a->avg_log : 0.f;           // Tensor.reciprocal() in fp32, like pna_degree_scalers_f32
  k.src = a->src; k.dst = a->dst;
  k.rowptr = a->rowptr; k.col = a->col; k.row = a->row; k.eid = a->eid; k.eid64 = a->eid64; k.items = a->items; k.snorm_n = a->snorm_n;
  if (k.want_t) {
    k.rowptr_t = a->rowptr_t; k.col_t = a->col_t; k.row_t = a->row_t; k.pos_t = a->pos_t; k.pos_t64 = a->pos_t64; k.rank_t = a->rank_t;
    k.items_t = a->items_t; k.row64 = a->row64; k.col64 = a->col64;
  }
  if (with_scalers) { k.amp = a->amp; k.att = a->att; }
  k.record = a->record;
  const unsigned long lds = (unsigned long)lds_bytes(k.cap_n, k.cap_e);
  if (int rc = pna_raise_lds((const void*)k_plan_groups, lds, "pna_batch_plan_i32: the runtime refused the workgroup's LDS")) return rc;
  hipLaunchKernelGGL(k_plan_scan, dim3(1), dim3(kScanBlock), 0, st, a->node_count, a->edge_count, (int)a->B, (int)a->V, (int)a->E, grid, node_off,
                     edge_off, group_first, n_groups, a->readout_offsets, a->rowptr, k.rowptr_t, a->record);
  hipLaunchKernelGGL(k_plan_groups, dim3(grid), dim3(kBlock), lds, st, k);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pna_set_error(PNA_E_LAUNCH, hipGetErrorString(e));
  return PNA_OK;
}
