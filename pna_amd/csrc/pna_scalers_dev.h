// The per-row degree scalers of models/dgl/scalers.py:12-19 as ONE device function, shared by every kernel that produces them
// (k_degree_scalers of pna_segreduce.hip, the batch plan of pna_batch_plan.hip), so that their bits cannot drift apart.
#ifndef PNA_SCALERS_DEV_H
#define PNA_SCALERS_DEV_H
#include <hip/hip_runtime.h>

// d = in-degree of the row, avg_log = avg_d["log"], inv_avg = 1.0f / avg_log rounded once on the host (Tensor.reciprocal() in fp32).
// A row without in-edges gets 0 for both, like the reference's masked scalers.
__device__ __forceinline__ void pna_degree_scalers_row(int d, float avg_log, float inv_avg, float& amp, float& att) {
  amp = 0.f;
  att = 0.f;
  if (d > 0) {
    const float lg = (float)log((double)d + 1.0);          // np.log(D + 1) in float64, then fp32
    amp = inv_avg * lg;                                    // avg.reciprocal() * scalar
    att = avg_log / lg;                                    // avg / scalar
  }
}
#endif
