// What the fp32 layer kernels (f32_layers.hip) share with the metric-specific kernels that sample or size maps the same way.
#pragma once

#include <hip/hip_runtime.h>

namespace {

inline int conv_out(int x, int k, int s, int p) { return (x + 2 * p - k) / s + 1; }
inline int pool_out(int x) { return (x - 3) / 2 + 1; }

// An align_corners=True axis table: idx[o] = the first source index of output o, wt[2 * o], wt[2 * o + 1] = the fp32 weights of
// source idx[o] and idx[o] + 1 (built on the host in fp64).  The kernels clamp both indices to the axis, so a wrong table gives
// wrong numbers, never an access outside the map.  A pixel is combined as torch's upsample_bilinear2d does:
// h0 * (w0 * x00 + w1 * x01) + h1 * (w0 * x10 + w1 * x11); with weights (1, 0) that is x00 bit for bit
// while the neighbours are finite (0 x NaN and 0 x inf are NaN, as in torch) - but for x00 = -0.0, which comes out as +0.0 unless
// the neighbours' products are -0.0 too.
__device__ __forceinline__ float bilerp(float x00, float x01, float x10, float x11, float w0, float w1, float h0, float h1) {
  const float top = fmaf(w1, x01, w0 * x00), bot = fmaf(w1, x11, w0 * x10);
  return fmaf(h1, bot, h0 * top);
}

}  // namespace
