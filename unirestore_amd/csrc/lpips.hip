// LPIPS's own kernels (AlexNet, v0.1 linear layers) for gfx950, exact fp32: input scaling and the per-tap distance
// (unit-normalise over channels, weighted squared difference, fixed-order sums).  The convolutions and the 3x3 / stride-2
// max-pool are ur_conv2d_f32_res and ur_maxpool2d_f32 of f32_layers.hip.  NHWC activations, no atomics:
// the same inputs give the same bits on every run, eagerly and under graph replay.
#include "common.h"
#include "f32_layers.h"

#include <climits>

namespace {

// ------------------------------------------------------------------------------------------ geometry shared with the planner
constexpr int LP_MIN_HW = 31;       // the smallest input at which the fifth tap still has one pixel
constexpr int LP_TAPS = 5;
constexpr int LP_PIX = 64;          // pixels per block of the layer kernel (16 per wave)

// size of tap `tap` (0..4) along one axis of an input of size x
inline int tap_size(int x, int tap) {
  int v = conv_out(x, 11, 4, 2);                 // conv1 -> tap 0
  if (tap >= 1) v = pool_out(v);                 // pool, conv2 (5x5 pad 2 keeps the size) -> tap 1
  if (tap >= 2) v = pool_out(v);                 // pool, conv3..5 (3x3 pad 1) -> taps 2, 3, 4
  return v;
}
inline long long layer_parts(long long P) { return (P + LP_PIX - 1) / LP_PIX; }

const char* bad_image_shape(int N, int C, int H, int W) {
  if (N < 1) return "N must be >= 1";
  if (C != 3) return "C must be 3 (RGB)";
  if (H < LP_MIN_HW || W < LP_MIN_HW) return "H and W must be >= 31";
  if ((long long)N * H * W > INT_MAX / 8) return "too many pixels: N*H*W must be below 2^28";
  return "";
}

// ------------------------------------------------------------------------------------------ input scaling
// NCHW [N,3,H,W] in [0,1] -> NHWC ((2x - 1) - shift_c) / scale_c.  Kept as its own pass: conv1 zero-pads in the SCALED space, so
// folding shift / scale into conv1's weights and bias would be wrong wherever the 11x11 window hangs over the border.
__global__ __launch_bounds__(256) void lpips_prep_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int HW) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int n = i / HW, hw = i - n * HW;
  const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = x[((long long)n * 3 + c) * HW + hw];
    y[(long long)i * 3 + c] = ((2.0f * v - 1.0f) - shift[c]) / scale[c];
  }
}

// ------------------------------------------------------------------------------------------ per-tap distance
// feat [2N][P][C]: images 0..N-1 are the predictions, N..2N-1 the targets.  One wave per pixel: lanes stride over the channels,
// n = sqrt(sum f^2) by the xor butterfly (every lane ends with the same bits), u = f / (n + 1e-10) - the eps is added to the norm,
// so an all-zero feature vector gives u = 0, not NaN - then sum_c w_c (u_pred - u_tgt)^2.  Block (chunk, image) adds its 64 pixels
// in a fixed order (wave g: pixels g, g+4, ... ascending; then the four waves left to right) into one fp64 partial.
__global__ __launch_bounds__(256) void lpips_layer_kernel(const float* __restrict__ feat, const float* __restrict__ lin, int N, int P,
                                                          int C, int chunks, double* __restrict__ part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunk = blockIdx.x, n = blockIdx.y;
  const float* f0 = feat + (long long)n * P * C;
  const float* f1 = feat + (long long)(n + N) * P * C;
  const int p_end = min(P, (chunk + 1) * LP_PIX);
  double acc = 0.0;
  for (int px = chunk * LP_PIX + wave; px < p_end; px += 4) {          // wave-uniform bounds
    const float* a = f0 + (long long)px * C;
    const float* b = f1 + (long long)px * C;
    float sa = 0.f, sb = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float va = a[c], vb = b[c];
      sa = fmaf(va, va, sa);
      sb = fmaf(vb, vb, sb);
    }
    const float na = sqrtf(wave_sum(sa)) + 1e-10f, nb = sqrtf(wave_sum(sb)) + 1e-10f;
    float d = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float u = a[c] / na - b[c] / nb;
      d = fmaf(lin[c], u * u, d);
    }
    acc += (double)wave_sum(d);
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(long long)n * chunks + chunk] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct FinishArgs {
  long long off[LP_TAPS];      // first partial of the tap, in doubles
  int chunks[LP_TAPS];
  double pixels[LP_TAPS];
};

// One thread per image: the tap's partials in ascending order, divided by its pixel count, the five taps in layer order.
__global__ __launch_bounds__(64) void lpips_finish_kernel(const double* __restrict__ ws, FinishArgs f, int N, double* __restrict__ out) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  double total = 0.0;
#pragma unroll
  for (int l = 0; l < LP_TAPS; ++l) {
    const double* part = ws + f.off[l] + (long long)n * f.chunks[l];
    double s = 0.0;
    for (int i = 0; i < f.chunks[l]; ++i) s += part[i];
    total += s / f.pixels[l];
  }
  out[n] = total;
}

FinishArgs finish_layout(int N, int H, int W, long long* total_doubles) {
  FinishArgs f;
  long long off = 0;
  for (int l = 0; l < LP_TAPS; ++l) {
    const long long P = (long long)tap_size(H, l) * tap_size(W, l);
    f.off[l] = off;
    f.chunks[l] = (int)layer_parts(P);
    f.pixels[l] = (double)P;
    off += (long long)N * f.chunks[l];
  }
  *total_doubles = off;
  return f;
}

}  // namespace

extern "C" {

int ur_lpips_tap_hw(int H, int W, int tap, int* oh, int* ow) {
  UR_REQUIRE(oh && ow, "null pointer");
  UR_REQUIRE(H >= LP_MIN_HW && W >= LP_MIN_HW, "H and W must be >= 31");
  UR_REQUIRE(tap >= 0 && tap < LP_TAPS, "tap must be 0..4");
  *oh = tap_size(H, tap);
  *ow = tap_size(W, tap);
  return 0;
}

long long ur_lpips_layer_parts(long long P) {
  if (P < 1 || P > INT_MAX) return ur::fail(UR_E_INVALID, "ur_lpips_layer_parts: P must be in [1, 2^31)");
  return layer_parts(P);
}

long long ur_lpips_ws_size(int N, int H, int W) {
  const char* why = bad_image_shape(N, 3, H, W);
  if (*why) return ur::fail(UR_E_INVALID, std::string("ur_lpips_ws_size: ") + why);
  long long doubles;
  finish_layout(N, H, W, &doubles);
  return doubles * (long long)sizeof(double);
}

int ur_lpips_prep(const float* x, float* y, int N, int C, int H, int W, ur_stream_t stream) {
  UR_REQUIRE(x && y, "null pointer");
  const char* why = bad_image_shape(N, C, H, W);
  UR_REQUIRE(!*why, why);
  const int total = N * H * W;                         // below 2^28 (bad_image_shape): far inside the launch margin
  UR_GRID_1D(blocks, total, 256);
  hipLaunchKernelGGL(lpips_prep_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, total, H * W);
  return ur::check_launch("ur_lpips_prep");
}

int ur_lpips_layer(const float* feat, const float* lin, int N, int P, int C, double* part, long long part_bytes, ur_stream_t stream) {
  UR_REQUIRE(feat && lin && part, "null pointer");
  UR_REQUIRE(N >= 1 && N <= 65535, "N must be in [1, 65535]");
  UR_REQUIRE(P >= 1 && C >= 1, "P and C must be >= 1");
  const long long chunks = layer_parts(P);
  UR_REQUIRE(chunks <= INT_MAX / 256, "too many pixels");
  const long long need = (long long)N * chunks * (long long)sizeof(double);
  UR_REQUIRE(part_bytes >= need, "workspace too small: " + std::to_string(part_bytes) + " < " + std::to_string(need) + " bytes");
  hipLaunchKernelGGL(lpips_layer_kernel, dim3((unsigned)chunks, (unsigned)N), dim3(256), 0, (hipStream_t)stream, feat, lin, N, P, C,
                     (int)chunks, part);
  return ur::check_launch("ur_lpips_layer");
}

int ur_lpips_finish(const void* ws, long long ws_bytes, int N, int H, int W, double* out, ur_stream_t stream) {
  UR_REQUIRE(ws && out, "null pointer");
  const char* why = bad_image_shape(N, 3, H, W);
  UR_REQUIRE(!*why, why);
  long long doubles;
  const FinishArgs f = finish_layout(N, H, W, &doubles);
  const long long need = doubles * (long long)sizeof(double);
  UR_REQUIRE(ws_bytes >= need, "workspace too small: " + std::to_string(ws_bytes) + " < " + std::to_string(need) + " bytes");
  UR_GRID_1D(blocks, N, 64);
  hipLaunchKernelGGL(lpips_finish_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, (const double*)ws, f, N, out);
  return ur::check_launch("ur_lpips_finish");
}

}  // extern "C"
