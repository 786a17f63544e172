// Counter-based random numbers of the dropout path: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as
// 1, 2, 3", SC'11) and the ONE mask rule every user of it follows -- the device kernels (csrc/dropout.hip) and the host
// entry points beside them are compiled from this header, so the mask a test computes on a machine without a GPU is
// the mask the step applies.
//
// Mask rule of element (global row r, column c) of hidden layer `layer` at draw `draw`:
//   counter = (r, c / 4, layer, draw), key = (seed low word, seed high word);
//   the four output words serve columns 4 (c / 4) ... 4 (c / 4) + 3;
//   kept  <=>  (word >> 8) < thr,  thr = round(keep * 2^24) computed ONCE on the host and passed as an integer;
//   a kept element is multiplied by float(1 / keep).
// Integer comparisons only: no float enters the decision, so host and device cannot disagree about an element.
// This draws from the distribution of tf.nn.dropout (base_model.py: _dropout), not from TensorFlow's random stream.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLSR_HD __host__ __device__ __forceinline__
#else
#define CLSR_HD inline
#endif

#define CLSR_PHILOX_M0 0xD2511F53u
#define CLSR_PHILOX_M1 0xCD9E8D57u
#define CLSR_PHILOX_W0 0x9E3779B9u
#define CLSR_PHILOX_W1 0xBB67AE85u

struct clsr_u32x4 {
  uint32_t x, y, z, w;
};

CLSR_HD clsr_u32x4 clsr_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)CLSR_PHILOX_M0 * c0, p1 = (uint64_t)CLSR_PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += CLSR_PHILOX_W0;
    k1 += CLSR_PHILOX_W1;
  }
  clsr_u32x4 o = {c0, c1, c2, c3};
  return o;
}

// the four words of columns 4 q ... 4 q + 3 of global row `row`
CLSR_HD clsr_u32x4 clsr_dropout_words(uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t layer, uint32_t row,
                                      uint32_t q) {
  return clsr_philox4x32_10(row, q, layer, draw, seed_lo, seed_hi);
}

CLSR_HD bool clsr_dropout_keep(uint32_t word, uint32_t thr) { return (word >> 8) < thr; }
