// Device helpers shared by the one-call training kernels (pna_simple_train.hip, pna_tower_train.hip): the exact-fp32 MFMA step, the
// message fold of a destination row with arg tracking, the BatchNorm affine expression and the per-column finalize of the tiles'
// shifted sums.  Not part of the C ABI.
#ifndef PNA_TRAIN_DEV_H
#define PNA_TRAIN_DEV_H
#include <hip/hip_runtime.h>

namespace pna_train {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kRows = 16;        // destination rows of a workgroup = the M of one MFMA tile

__host__ __device__ constexpr int quads(int k) { return (k + 15) / 16; }
__host__ __device__ constexpr int pitch_of(int q) { return q * 16 + 4; }   // LDS row pitch (floats): rows 16-byte aligned, banks staggered

// 16 values of K per call: v_mfma_f32_16x16x4_f32 four times, lane group lg holds k = 4 lg .. 4 lg + 3 of the 16
__device__ __forceinline__ void quad_fma(f4& acc, const f4 a, const f4 b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

// z = (y - mean) (gamma invstd) + beta: pna_bn_tail.hip's expression
__device__ __forceinline__ float bn_affine(float y, float mean, float a, float b) { return __builtin_fmaf(y - mean, a, b); }

// One message m at CSR position e into a row's running sums: pna_segreduce.hip's arg fold -- strict comparison (the FIRST extremal
// edge wins), NaN sticky.
__device__ __forceinline__ void fold_msg(float m, int e, float& s, float& q, float& mx, float& mn, int& ax, int& an) {
  s = s + m;
  q = q + m * m;
  const bool gx = m > mx || (m != m && mx == mx);
  const bool gn = m < mn || (m != m && mn == mn);
  mx = gx ? m : mx; ax = gx ? e : ax;
  mn = gn ? m : mn; an = gn ? e : an;
}

// One BatchNorm column from the 16-row tiles' sums of d = z - z[first row of the tile] and d^2 (part[tile][2][N]): re-based on
// z[0, c] and added over the tiles in float64 by a workgroup of 256 threads (the re-basing pna_bn_tail.hip applies to its row lanes'
// and workgroups' sums; its shift is a median of three rows, here it is the tile's first row); the batch mean, 1 / sqrt of
// the BIASED variance + eps, and the running statistics moved with the UNBIASED variance (torch.nn.functional.batch_norm).
// red: double[2][256] of LDS.  rmean == NULL or momentum < 0: running statistics not kept.
__device__ __forceinline__ void bn_finalize_column(const float* z, int N, int c, int V, const float* part, int n_part, float eps, float momentum,
                                                   float* mean_c, float* invstd_c, float* rmean_c, float* rvar_c, double (*red)[256]) {
  const double k0 = (double)z[c];                           // the shift of the whole column: z[0, c]
  double t0 = 0.0, t1 = 0.0;
  for (int t = threadIdx.x; t < n_part; t += 256) {
    const double nt = (double)min(kRows, V - t * kRows);
    const double dk = (double)z[(size_t)t * kRows * N + c] - k0;
    const double s = (double)part[((size_t)t * 2 + 0) * N + c], q = (double)part[((size_t)t * 2 + 1) * N + c];
    t0 += s + nt * dk;                                      // sum (z - k0)   = sum (z - k_t) + n_t (k_t - k0)
    t1 += q + 2.0 * dk * s + nt * dk * dk;                  // sum (z - k0)^2
  }
  red[0][threadIdx.x] = t0; red[1][threadIdx.x] = t1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { red[0][threadIdx.x] += red[0][threadIdx.x + s]; red[1][threadIdx.x] += red[1][threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double Sm = red[0][0], Qm = red[1][0], M = (double)V;
  const double md = Sm / M;
  double var = Qm / M - md * md;                            // biased, like nn.BatchNorm1d's normalisation
  if (var < 0.0) var = 0.0;
  const double mean = k0 + md;
  *mean_c = (float)mean;
  *invstd_c = (float)(1.0 / sqrt(var + (double)eps));
  if (rmean_c && momentum >= 0.f) {
    const double m = (double)momentum;
    *rmean_c = (float)((1.0 - m) * (double)*rmean_c + m * mean);
    *rvar_c = (float)((1.0 - m) * (double)*rvar_c + m * var * (M / (M - 1.0)));
  }
}

}  // namespace pna_train
#endif
