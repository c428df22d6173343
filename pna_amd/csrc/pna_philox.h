// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the dropout mask rule of the
// one-call tower training route with dropout (pna_tower_drop_train_*_f32, pna_dropout_mask_f32; include/pna_amd.h).  Counter-based: a
// word is a pure function of (element index, seed, offset), so a backward regenerates the forward's mask from the 128-bit key instead
// of reading a saved one.  Plain C++: 32-bit multiplies and __umulhi, no state, no atomics.  Host and device compile the same text
// (tests hold the device against a numpy restatement of it).  Not part of the C ABI.
#ifndef PNA_PHILOX_H
#define PNA_PHILOX_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pna_philox {

constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;     // the round multipliers
constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;     // the key increments (golden ratio, sqrt(3) - 1)

__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// ten rounds on counter c[4] with key (k0, k1), in place
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(kM0, c[0]), lo0 = kM0 * c[0], hi1 = mulhi32(kM1, c[2]), lo1 = kM1 * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += kW0; k1 += kW1;
  }
}

// what a call's elements share: the key, the threshold and the factor of a kept element
struct Mask {
  uint32_t seed_lo, seed_hi, off_lo, off_hi;
  uint32_t thr;       // an element is kept iff its word >= thr
  float scale;        // 1.0f / (1.0f - p), formed once in fp32
};

// thr = (uint32) min(floor((double) p 2^32), 2^32 - 1) for 0 <= p < 1
__host__ __device__ __forceinline__ Mask make_mask(float p, uint64_t seed, uint64_t offset) {
  Mask m;
  m.seed_lo = (uint32_t)seed; m.seed_hi = (uint32_t)(seed >> 32); m.off_lo = (uint32_t)offset; m.off_hi = (uint32_t)(offset >> 32);
  const double t = (double)p * 4294967296.0;                  // exact: a float times a power of two
  m.thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;     // (the conversion truncates = floor for t >= 0)
  m.scale = 1.0f / (1.0f - p);
  return m;
}

// the four words of quad q: elements 4 q .. 4 q + 3 of the (V, C) matrix in row-major order, e = v C + c
__host__ __device__ __forceinline__ void quad_words(const Mask& m, uint64_t q, uint32_t (&w)[4]) {
  w[0] = (uint32_t)q; w[1] = (uint32_t)(q >> 32); w[2] = m.off_lo; w[3] = m.off_hi;
  philox4x32_10(w, m.seed_lo, m.seed_hi);
}

}  // namespace pna_philox
#endif
