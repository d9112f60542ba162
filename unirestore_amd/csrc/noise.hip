// Counter-based noise keyed per image (Philox4x32-10 + Box-Muller) for gfx950: an image's noise is a pure function of its own
// 64-bit seed, the draw and the element index - not of the batch it sits in.  The keys are read from a device table, so one captured
// graph serves every seed.  One launch, no allocation, no synchronisation, no atomics.
#include "common.h"
#include "philox.h"

namespace {

constexpr int NOISE_MAX_BLOCKS_X = 4096;                                  // counters beyond grid.x * 256 are grid-strided
constexpr int NOISE_MAX_BLOCKS_Y = 65535;                                 // images beyond grid.y likewise

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
