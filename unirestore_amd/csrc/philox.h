// Philox4x32-10 + the word -> uniform / Box-Muller maps shared by the keyed noise (noise.hip) and the corruptions (corrupt.hip).
// The bits are part of both specifications (include/unirestore_hip.h): change nothing here without their known-answer tests.
#pragma once
#include "common.h"

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // Weyl constants (key schedule)

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 known answers are in the tests)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t* w) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// word -> uniform in [2^-24, 1 - 2^-24]: (x >> 9) + 0.5 has 24 significant bits, so the product is exact in fp32
__device__ __forceinline__ float word_to_uniform(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// Box-Muller on one word pair with the precise fp32 logf / sqrtf / sincosf (the fast intrinsics lose orders of magnitude near
// theta = 2 pi): the even word's output is r cos(theta), the odd word's r sin(theta)
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float* even, float* odd) {
  const float r = sqrtf(-2.0f * logf(word_to_uniform(wa)));
  const float theta = 6.283185307179586f * word_to_uniform(wb);
  float s, c;
  sincosf(theta, &s, &c);
  *even = r * c;
  *odd = r * s;
}
