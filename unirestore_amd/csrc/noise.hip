// Counter-based noise keyed per image (Philox4x32-10 + Box-Muller) for gfx950: an image's noise is a pure function of its own
// 64-bit seed, the draw and the element index - not of the batch it sits in.  The keys are read from a device table, so one captured
// graph serves every seed.  One launch, no allocation, no synchronisation, no atomics.
#include "common.h"

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // Weyl constants (key schedule)
constexpr int NOISE_MAX_BLOCKS_X = 4096;                                  // counters beyond grid.x * 256 are grid-strided
constexpr int NOISE_MAX_BLOCKS_Y = 65535;                                 // images beyond grid.y likewise

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

// One thread per Philox counter = four consecutive elements of one image.  blockIdx.y walks the images, blockIdx.x the counters.
// BITS: store the raw words instead of the normals.
template <bool BITS>
__global__ __launch_bounds__(256) void keyed_noise_kernel(const uint32_t* __restrict__ keys, uint32_t draw, uint32_t* __restrict__ out,
                                                          int N, long long count) {
  const long long nctr = (count + 3) >> 2;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const uint32_t k0 = keys[2 * n], k1 = keys[2 * n + 1];
    uint32_t* o = out + (long long)n * count;
    for (long long q = blockIdx.x * 256LL + threadIdx.x; q < nctr; q += (long long)gridDim.x * 256) {
      uint32_t w[4];
      philox4x32_10((uint32_t)q, draw, 0u, 0u, k0, k1, w);
      if (!BITS) {
        float f[4];
        box_muller(w[0], w[1], &f[0], &f[1]);
        box_muller(w[2], w[3], &f[2], &f[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = __float_as_uint(f[j]);
      }
      const long long e = q << 2;
      uint32_t* p = o + e;
      if (e + 4 <= count && ((uintptr_t)p & 15) == 0) {
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);      // one 16-byte store
      } else {                                                                 // count % 4 tail, or an address off 16 bytes
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (e + j < count) p[j] = w[j];
      }
    }
  }
}

}  // namespace

extern "C" {

int ur_keyed_noise(const uint32_t* keys, uint32_t draw, void* out, int N, long long count, int kind, ur_stream_t stream) {
  UR_REQUIRE(keys && out, "null pointer");
  UR_REQUIRE(N > 0, "N must be positive");
  UR_REQUIRE(count > 0 && count <= (1LL << 34), "count must be in [1, 2^34] (the element index's counter word is 32 bits)");
  UR_REQUIRE(kind == 0 || kind == 1, "kind must be 0 (fp32 normals) or 1 (raw uint32 words)");
  UR_REQUIRE(((uintptr_t)out & 3) == 0, "out must be 4-byte aligned");
  const long long nctr = (count + 3) >> 2;
  const long long bx = (nctr + 255) / 256;
  const dim3 grid((unsigned)(bx < NOISE_MAX_BLOCKS_X ? bx : NOISE_MAX_BLOCKS_X), (unsigned)(N < NOISE_MAX_BLOCKS_Y ? N : NOISE_MAX_BLOCKS_Y));
  hipStream_t s = (hipStream_t)stream;
  const double elems = (double)N * (double)count;
  ur::ProfScope prof("keyed_noise", elems * (kind ? 20.0 : 60.0), 4.0 * elems, s);
  if (kind == 0)
    hipLaunchKernelGGL(keyed_noise_kernel<false>, grid, dim3(256), 0, s, keys, draw, (uint32_t*)out, N, count);
  else
    hipLaunchKernelGGL(keyed_noise_kernel<true>, grid, dim3(256), 0, s, keys, draw, (uint32_t*)out, N, count);
  return ur::check_launch("ur_keyed_noise");
}

}  // extern "C"
