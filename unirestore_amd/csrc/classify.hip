// The classifier's own kernels for gfx950, exact fp32: the evaluator's preprocess (antialiased bilinear resize to 224 x 224 from
// host-built tap tables + ImageNet normalisation, NCHW in, NHWC out) and top-1 with the per-class counts of the accuracy.  The
// convolutions (and the FC layer, a 1x1 convolution on a 1x1 map), the padded 3x3 / stride-2 max-pool and the global average
// pool are ur_conv2d_f32_res, ur_maxpool2d_pad_f32 and ur_avgpool_f32 of f32_layers.hip.  No atomics; every sum runs in a fixed
// order, so the same inputs give the same bits on every run, eagerly and under graph replay, and an image's results do not
// depend on its place in the batch.
#include "common.h"

#include <climits>
#include <cmath>

namespace {

constexpr int CL_OUT = 224;          // T.Resize((224, 224))
constexpr int CL_MAX_TAPS = 64;      // per output index; a 960 x 1664 crop needs 16

// ------------------------------------------------------------------------------------------ preprocess
// A resize table for one axis: first[o] = the first input index of output o, count[o] <= taps its tap count, wt[o * taps + j]
// the fp32 weight of input first[o] + j.  The kernels clamp what they read from a table to the axis, so a wrong table gives
// wrong numbers, never an access outside the image.
// Horizontal pass (torch resizes the last axis first): x [N*3*H][W] -> tmp [N*3*H][224], taps in ascending order.
__global__ __launch_bounds__(256) void classify_resize_w_kernel(const float* __restrict__ x, float* __restrict__ tmp, int rows, int W,
                                                                const int* __restrict__ first, const int* __restrict__ count,
                                                                const float* __restrict__ wt, int taps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * CL_OUT) return;
  const int row = i / CL_OUT, ox = i - row * CL_OUT;
  const int f = min(max(first[ox], 0), W - 1), cnt = min(min(count[ox], taps), W - f);
  const float* src = x + (long long)row * W + f;
  const float* wv = wt + ox * taps;
  float s = 0.f;
  for (int j = 0; j < cnt; ++j) s = fmaf(wv[j], src[j], s);
  tmp[i] = s;
}

// Vertical pass + (v - mean_c) / std_c: tmp [N][3][H][224] -> y [N][224][224][3].
__global__ __launch_bounds__(256) void classify_resize_h_kernel(const float* __restrict__ tmp, float* __restrict__ y, int N, int H,
                                                                const int* __restrict__ first, const int* __restrict__ count,
                                                                const float* __restrict__ wt, int taps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * CL_OUT * CL_OUT) return;
  const int ox = i % CL_OUT;
  const int r = i / CL_OUT;
  const int oy = r % CL_OUT, n = r / CL_OUT;
  const int f = min(max(first[oy], 0), H - 1), cnt = min(min(count[oy], taps), H - f);
  const float* wv = wt + oy * taps;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};      // IMAGENET_DEFAULT_MEAN / STD
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* src = tmp + (((long long)n * 3 + c) * H + f) * CL_OUT + ox;
    float s = 0.f;
    for (int j = 0; j < cnt; ++j) s = fmaf(wv[j], src[(long long)j * CL_OUT], s);
    y[(long long)i * 3 + c] = (s - mean[c]) / sd[c];
  }
}

// ------------------------------------------------------------------------------------------ top-1 and the accuracy's counts
// One wave per image.  `better`: a larger value, or the same value at a lower index - ties go to the lowest index, and a NaN
// counts as the maximum (the first one wins), as torch.argmax has it.
__device__ __forceinline__ bool top1_better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

__global__ __launch_bounds__(64) void top1_kernel(const float* __restrict__ logits, int C, long long* __restrict__ pred) {
  const int lane = threadIdx.x;
  const float* row = logits + (long long)blockIdx.x * C;
  float bv = -INFINITY;
  int bi = INT_MAX;                        // lanes beyond C keep (-inf, INT_MAX) and lose against every real entry
  for (int c = lane; c < C; c += 64) {
    const float v = row[c];
    if (bi == INT_MAX || top1_better(v, c, bv, bi)) {
      bv = v;
      bi = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi != INT_MAX && (bi == INT_MAX || top1_better(ov, oi, bv, bi))) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) pred[blockIdx.x] = bi;
}

// counts [3][C]: tp_c, targets_c, predicted_c of this batch; one thread per class scans the N predictions.
__global__ __launch_bounds__(256) void top1_counts_kernel(const long long* __restrict__ pred, const long long* __restrict__ labels, int N,
                                                          int C, long long* __restrict__ counts) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  long long tp = 0, tg = 0, pr = 0;
  for (int n = 0; n < N; ++n) {
    const bool p = pred[n] == c, t = labels[n] == c;
    tp += p && t;
    tg += t;
    pr += p;
  }
  counts[c] = tp;                          // (64-bit row offsets: 2 * C does not fit an int from C = 2^30 on)
  counts[(long long)C + c] = tg;
  counts[2ll * C + c] = pr;
}

}  // namespace

extern "C" {

int ur_classify_preprocess(const float* x, float* tmp, float* y, int N, int C, int H, int W, const int* first_w, const int* count_w,
                           const float* wt_w, int taps_w, const int* first_h, const int* count_h, const float* wt_h, int taps_h,
                           ur_stream_t stream) {
  UR_REQUIRE(x && tmp && y && first_w && count_w && wt_w && first_h && count_h && wt_h, "null pointer");
  UR_REQUIRE(N >= 1 && H >= 1 && W >= 1, "N, H and W must be >= 1");
  UR_REQUIRE(C == 3, "C must be 3 (RGB)");
  UR_REQUIRE(taps_w >= 1 && taps_w <= CL_MAX_TAPS && taps_h >= 1 && taps_h <= CL_MAX_TAPS, "taps_w and taps_h must be in [1, 64]");
  UR_REQUIRE((long long)N * 3 * H * W < ur::GRID_1D_LIMIT && (long long)N * 3 * H * CL_OUT < ur::GRID_1D_LIMIT &&
                 (long long)N * 3 * CL_OUT * CL_OUT < ur::GRID_1D_LIMIT,
             "too many pixels: N*3*H*max(W, 224) and N*3*224*224 must be below 2^31 - 256");
  hipStream_t s = (hipStream_t)stream;
  const int rows = N * 3 * H, t1 = rows * CL_OUT, t2 = N * CL_OUT * CL_OUT;
  UR_GRID_1D(blocks_w, t1, 256);
  UR_GRID_1D(blocks_h, t2, 256);
  hipLaunchKernelGGL(classify_resize_w_kernel, dim3(blocks_w), dim3(256), 0, s, x, tmp, rows, W, first_w, count_w, wt_w, taps_w);
  hipLaunchKernelGGL(classify_resize_h_kernel, dim3(blocks_h), dim3(256), 0, s, tmp, y, N, H, first_h, count_h, wt_h, taps_h);
  return ur::check_launch("ur_classify_preprocess");
}

int ur_top1_counts(const float* logits, const long long* labels, int N, int C, long long* pred, long long* counts, ur_stream_t stream) {
  UR_REQUIRE(logits && labels && pred && counts, "null pointer");
  UR_REQUIRE(N >= 1 && C >= 1, "N and C must be >= 1");
  UR_REQUIRE((long long)N * C < ur::GRID_1D_LIMIT, "too many logits: N*C must be below 2^31 - 256");
  hipStream_t s = (hipStream_t)stream;
  UR_GRID_1D(blocks, C, 256);                          // C alone reaches the limit for N = 1
  hipLaunchKernelGGL(top1_kernel, dim3(N), dim3(64), 0, s, logits, C, pred);
  hipLaunchKernelGGL(top1_counts_kernel, dim3(blocks), dim3(256), 0, s, (const long long*)pred, labels, N, C, counts);
  return ur::check_launch("ur_top1_counts");
}

}  // extern "C"
