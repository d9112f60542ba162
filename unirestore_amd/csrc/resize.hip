// Antialiased resize of u8 images for gfx950: the bytes torch's CPU interpolate(uint8, antialias=True) gives (the specification is
// the ur_resize_u8 comment in include/unirestore_hip.h).  x u8 [N,H,W,3] contiguous HWC -> out u8 [N,oh,ow,3].  Two table-driven
// passes in int32, the filter is in the host-built tables (bilinear and bicubic are the same kernels):
//   1. along the width into the caller's workspace [N,H,ow,3]: one output pixel per thread, which reads the xsize * 3 contiguous
//      bytes of its source span once and keeps three accumulators,
//   2. along the height: one output byte per thread, so a wave reads 64 neighbouring bytes of each source row and every lane of
//      a row shares the row's bounds and weights.
// A pass between equal lengths is skipped (the other one then writes out directly); with both equal the image is copied.
// No allocation, no synchronisation, no atomics, no per-thread arrays; every workspace byte that is read was written by this call.
#include "common.h"

#include <climits>

namespace {

// Integer weights of at most 22 fractional bits on bytes: the sum wraps as the reference's int32 does (it never does for a
// normalised filter), which unsigned arithmetic states without undefined behaviour.
__device__ __forceinline__ uint8_t finish(uint32_t acc, int p) { return (uint8_t)min(max((int)acc >> p, 0), 255); }

// A table row that would leave [0, n_in) or hold more than K weights contributes nothing: the kernels never read outside x.
__device__ __forceinline__ int checked_size(int first, int size, int n_in, int K) {
  return (first >= 0 && size >= 0 && size <= K && first <= n_in - size) ? size : 0;
}

__global__ void __launch_bounds__(256) resize_width_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y, long long pixels, int W,
                                                           int ow, const int32_t* __restrict__ bounds, const int32_t* __restrict__ weights,
                                                           int K, int p) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= pixels) return;
  const int ox = (int)(i % ow);
  const long long row = i / ow;                                                     // n * H + y
  const int xmin = bounds[2 * ox];
  const int xsize = checked_size(xmin, bounds[2 * ox + 1], W, K);
  const uint8_t* src = x + (row * W + (xsize ? xmin : 0)) * 3;
  const int32_t* wt = weights + (long long)ox * K;
  uint32_t r = 1u << (p - 1), g = r, b = r;
  for (int j = 0; j < xsize; ++j) {
    const uint32_t w = (uint32_t)wt[j];
    r += w * src[3 * j];
    g += w * src[3 * j + 1];
    b += w * src[3 * j + 2];
  }
  y[3 * i] = finish(r, p);
  y[3 * i + 1] = finish(g, p);
  y[3 * i + 2] = finish(b, p);
}

__global__ void __launch_bounds__(256) resize_height_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y, long long bytes, int H,
                                                            int oh, int row_bytes, const int32_t* __restrict__ bounds,
                                                            const int32_t* __restrict__ weights, int K, int p) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= bytes) return;
  const int col = (int)(i % row_bytes);
  const long long row = i / row_bytes;                                              // n * oh + oy
  const int oy = (int)(row % oh);
  const long long n = row / oh;
  const int ymin = bounds[2 * oy];
  const int ysize = checked_size(ymin, bounds[2 * oy + 1], H, K);
  const uint8_t* src = x + (n * H + (ysize ? ymin : 0)) * row_bytes + col;
  const int32_t* wt = weights + (long long)oy * K;
  uint32_t acc = 1u << (p - 1);
  for (int j = 0; j < ysize; ++j) acc += (uint32_t)wt[j] * src[(long long)j * row_bytes];
  y[i] = finish(acc, p);
}

__global__ void __launch_bounds__(256) resize_copy_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y, long long bytes) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i < bytes) y[i] = x[i];
}

inline unsigned blocks_of(long long threads) { return (unsigned)((threads + 255) / 256); }

constexpr int MAX_K = 1 << 16;                     // a reduction by 2^14 with the cubic filter; far beyond any image

}  // namespace

extern "C" {

size_t ur_resize_u8_ws_bytes(int N, int H, int W, int oh, int ow) {
  if (N <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0) return 0;
  return ((size_t)N * H * ow * 3 + 7) & ~(size_t)7;
}

int ur_resize_u8(const uint8_t* x, uint8_t* out, int N, int H, int W, int oh, int ow, const int32_t* xbounds, const int32_t* xweights, int xK,
                 int xp, const int32_t* ybounds, const int32_t* yweights, int yK, int yp, void* ws, size_t ws_bytes, ur_stream_t stream) {
  UR_REQUIRE(x && out && ws && xbounds && xweights && ybounds && yweights, "null pointer");
  UR_REQUIRE(N > 0, "N must be positive");
  UR_REQUIRE(H >= 2 && W >= 2 && oh >= 2 && ow >= 2, "H, W, oh and ow must be >= 2");
  UR_REQUIRE((long long)N * H * W * 3 <= INT_MAX - 256 && (long long)N * oh * ow * 3 <= INT_MAX - 256 && (long long)N * H * ow * 3 <= INT_MAX - 256,
             "N * H * W * 3, N * oh * ow * 3 and N * H * ow * 3 must stay below 2^31");
  UR_REQUIRE(xK >= 1 && xK <= MAX_K && yK >= 1 && yK <= MAX_K, "K must be in [1, 65536]");
  UR_REQUIRE(xp >= 1 && xp <= 22 && yp >= 1 && yp <= 22, "p must be in [1, 22]");
  UR_REQUIRE(out != x, "out must not be x");
  UR_REQUIRE((((uintptr_t)xbounds | (uintptr_t)xweights | (uintptr_t)ybounds | (uintptr_t)yweights) & 3) == 0, "tables must be 4-byte aligned");
  UR_REQUIRE(((uintptr_t)ws & 7) == 0, "workspace must be 8-byte aligned");
  UR_REQUIRE(ws_bytes >= ur_resize_u8_ws_bytes(N, H, W, oh, ow), "workspace too small");
  const long long in_bytes = (long long)N * H * W * 3, mid_pixels = (long long)N * H * ow, out_bytes = (long long)N * oh * ow * 3;
  const bool along_w = ow != W, along_h = oh != H;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("resize_u8", (double)(along_w ? mid_pixels * 6.0 * xK : 0.0) + (double)(along_h ? out_bytes * 2.0 * yK : 0.0),
                     (double)in_bytes + (double)out_bytes + (along_w && along_h ? 6.0 * (double)mid_pixels : 0.0), s);
  if (!along_w && !along_h) {
    hipLaunchKernelGGL(resize_copy_kernel, dim3(blocks_of(in_bytes)), dim3(256), 0, s, x, out, in_bytes);
    return ur::check_launch("ur_resize_u8 (copy)");
  }
  const uint8_t* mid = x;
  if (along_w) {
    uint8_t* dst = along_h ? (uint8_t*)ws : out;
    hipLaunchKernelGGL(resize_width_kernel, dim3(blocks_of(mid_pixels)), dim3(256), 0, s, x, dst, mid_pixels, W, ow, xbounds, xweights, xK, xp);
    const int rc = ur::check_launch("ur_resize_u8 (width)");
    if (rc || !along_h) return rc;
    mid = dst;
  }
  hipLaunchKernelGGL(resize_height_kernel, dim3(blocks_of(out_bytes)), dim3(256), 0, s, mid, out, out_bytes, H, oh, ow * 3, ybounds, yweights, yK, yp);
  return ur::check_launch("ur_resize_u8 (height)");
}

}  // extern "C"
