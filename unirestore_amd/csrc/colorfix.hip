// Colour correction of a restored image against the image the encoder saw (gfx950): a five-level a-trous wavelet fix and an
// AdaIN (per-channel mean / standard deviation) fix, at canvas resolution between the decoder's conv_out and the egress kernels.
// c fp32 NHWC [N,H,W,ld_c] (restored), s 16-bit NHWC [src_n,H,W,ld_s] (source, image n reads source n % src_n), out fp32 NHWC
// [N,H,W,ld_c]; channels 0..2 carry RGB, [3, ld) of the inputs are never used in arithmetic and are written as zeros.
// No atomics and no order that depends on scheduling: two calls on the same inputs give the same bits.
#include "common.h"

#include <climits>

namespace {

constexpr int CF_HALO = 31;                        // 1 + 2 + 4 + 8 + 16: what five dilated 3-tap levels eat on an interior side
// column pass (vertical levels): a workgroup owns CF_VR rows x CF_VC columns, its LDS window is CF_VR + 2 halos = 128 rows
constexpr int CF_VR = 66;
constexpr int CF_VC = 16;
constexpr int CF_VROWS = CF_VR + 2 * CF_HALO;
constexpr int CF_VIN = 3 * CF_VC;                  // one LDS row: channel-major, 3 x CF_VC floats
// row pass (horizontal levels): a workgroup owns CF_HR full rows and walks them left to right in steps of CF_HC columns
constexpr int CF_HR = 4;
constexpr int CF_HC = 66;
constexpr int CF_HSEG = 128;                       // one LDS line: CF_HC + 2 halos = 128 columns
static_assert(CF_HC + 2 * CF_HALO <= CF_HSEG && CF_HC >= CF_HALO, "row-pass window");
// AdaIN statistics: pixels per workgroup (64 per thread: the longest sequential fp64 chain of the statistics pass)
constexpr int CF_SPX = 16384;

// RGB of one pixel.  vec: the pixel is 16-byte (fp32) / 8-byte (16-bit) aligned and ld >= 4, so one vector load fetches it (the
// fourth lane is a padding channel and is dropped); else three scalar loads.
__device__ __forceinline__ void load_rgb_f32(const float* p, int vec, float* v) {
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z;
  } else {
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
  }
}
template <bool F16> __device__ __forceinline__ void load_rgb_16(const uint16_t* p, int vec, float* v) {
  if (vec) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    v[0] = Act<F16>::lo(t.x); v[1] = Act<F16>::hi(t.x); v[2] = Act<F16>::lo(t.y);
  } else {
    v[0] = Act<F16>::one(p[0]); v[1] = Act<F16>::one(p[1]); v[2] = Act<F16>::one(p[2]);
  }
}
// RGB + zeroed padding channels of one output pixel
__device__ __forceinline__ void store_px(float* p, int ld, int vec, float r, float g, float b) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = make_float4(r, g, b, 0.f);
    for (int k = 4; k < ld; k += 4) *reinterpret_cast<float4*>(p + k) = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    p[0] = r; p[1] = g; p[2] = b;
    for (int k = 3; k < ld; ++k) p[k] = 0.f;
  }
}

// One level: dst[p] = (src[p-r] + src[p+r]) / 4 + src[p] / 2 with the taps clamped to the window [0, len).  The window ends at the
// image edge wherever the strip touches one (replicate border, at every level); on an interior side the clamp only keeps the
// read inside LDS and spoils positions that the halo gives away anyway.  Two rounded additions; the scalings are exact.
__device__ __forceinline__ float cf_tap(float lo, float mid, float hi) { return 0.25f * (lo + hi) + 0.5f * mid; }

// ---- wavelet, pass 1: the five vertical levels of d = s - c -> out (RGB) -------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256) void cf_wavelet_cols_kernel(const float* __restrict__ c, int ld_c, const uint16_t* __restrict__ s, int ld_s,
                                                              float* __restrict__ out, int src_n, int H, int W, int tiles_x, int tiles_y,
                                                              int vec_c, int vec_s) {
  __shared__ float buf[2][CF_VROWS * CF_VIN];
  const int tile = blockIdx.x % (tiles_x * tiles_y), n = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = (tile % tiles_x) * CF_VC, y0 = (tile / tiles_x) * CF_VR;
  const int nc = min(CF_VC, W - x0);
  const int g0 = max(0, y0 - CF_HALO), g1 = min(H, y0 + CF_VR + CF_HALO);
  const int nr = g1 - g0;
  const float* cn = c + (long long)n * H * W * ld_c;
  const uint16_t* sn = s + (long long)(n % src_n) * H * W * ld_s;
  float* on = out + (long long)n * H * W * ld_c;

  for (int e = threadIdx.x; e < nr * CF_VC; e += 256) {
    const int p = e / CF_VC, q = e % CF_VC;
    float d[3] = {0.f, 0.f, 0.f};
    if (q < nc) {
      const long long px = (long long)(g0 + p) * W + x0 + q;
      float cv[3], sv[3];
      load_rgb_f32(cn + px * ld_c, vec_c, cv);
      load_rgb_16<F16>(sn + px * ld_s, vec_s, sv);
#pragma unroll
      for (int k = 0; k < 3; ++k) d[k] = sv[k] - cv[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) buf[0][p * CF_VIN + k * CF_VC + q] = d[k];
  }
  __syncthreads();
  int cur = 0;
#pragma unroll
  for (int r = 1; r <= 16; r <<= 1) {
    const float* a = buf[cur];
    float* b = buf[cur ^ 1];
    for (int e = threadIdx.x; e < nr * CF_VIN; e += 256) {
      const int p = e / CF_VIN, q = e - p * CF_VIN;
      b[e] = cf_tap(a[max(p - r, 0) * CF_VIN + q], a[e], a[min(p + r, nr - 1) * CF_VIN + q]);
    }
    __syncthreads();
    cur ^= 1;
  }
  const float* t = buf[cur];
  const int own = min(CF_VR, H - y0), lead = y0 - g0;
  for (int e = threadIdx.x; e < own * CF_VC; e += 256) {
    const int i = e / CF_VC, q = e % CF_VC;
    if (q < nc) {
      const float* tp = t + (lead + i) * CF_VIN + q;
      float* op = on + ((long long)(y0 + i) * W + x0 + q) * ld_c;
      if (vec_c) {
        *reinterpret_cast<float4*>(op) = make_float4(tp[0], tp[CF_VC], tp[2 * CF_VC], 0.f);
      } else {
        op[0] = tp[0]; op[1] = tp[CF_VC]; op[2] = tp[2 * CF_VC];
      }
    }
  }
}

// ---- wavelet, pass 2: the five horizontal levels, in place on out, then out = c + L(d) ---------------------------------------
// A workgroup owns whole rows, so no other workgroup reads what it overwrites.  It walks its rows left to right: the window of a
// step is its CF_HC columns plus a halo; the left halo's columns were overwritten by the previous step and come from `carry`
// (their pass-1 values, kept in LDS), the right halo's are still pass-1 values in memory.
__global__ __launch_bounds__(256) void cf_wavelet_rows_kernel(const float* __restrict__ c, int ld, float* out, int H, int W, int tiles_y,
                                                              int vec) {
  __shared__ float buf[2][CF_HR * 3 * CF_HSEG];
  __shared__ float carry[CF_HR * 3 * CF_HALO];
  const int n = blockIdx.x / tiles_y, y0 = (blockIdx.x % tiles_y) * CF_HR;
  const int rows = min(CF_HR, H - y0), lines = rows * 3;
  const long long base = ((long long)n * H + y0) * W;          // pixel index of (n, y0, 0)
  for (int x0 = 0; x0 < W; x0 += CF_HC) {
    const int g0 = max(0, x0 - CF_HALO), g1 = min(W, x0 + CF_HC + CF_HALO);
    const int len = g1 - g0, lead = x0 - g0, nload = g1 - x0;
    for (int e = threadIdx.x; e < lines * lead; e += 256) {
      const int line = e / lead, p = e - line * lead;
      buf[0][line * CF_HSEG + p] = carry[line * CF_HALO + p];
    }
    for (int e = threadIdx.x; e < rows * nload; e += 256) {
      const int row = e / nload, q = e - row * nload;
      float v[3];
      load_rgb_f32(out + (base + (long long)row * W + x0 + q) * ld, vec, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) buf[0][(row * 3 + k) * CF_HSEG + lead + q] = v[k];
    }
    __syncthreads();
    if (x0 + CF_HC < W)                                        // columns [x0 + HC - 31, x0 + HC): the next step's left halo
      for (int e = threadIdx.x; e < lines * CF_HALO; e += 256) {
        const int line = e / CF_HALO, p = e - line * CF_HALO;
        carry[e] = buf[0][line * CF_HSEG + lead + CF_HC - CF_HALO + p];
      }
    int cur = 0;
#pragma unroll
    for (int r = 1; r <= 16; r <<= 1) {
      const float* a = buf[cur];
      float* b = buf[cur ^ 1];
      for (int e = threadIdx.x; e < lines * CF_HSEG; e += 256) {
        const int p = e % CF_HSEG, l0 = e - p;
        if (p < len) b[e] = cf_tap(a[l0 + max(p - r, 0)], a[e], a[l0 + min(p + r, len - 1)]);
      }
      __syncthreads();
      cur ^= 1;
    }
    const float* t = buf[cur];
    const int own = min(CF_HC, W - x0);
    for (int e = threadIdx.x; e < rows * own; e += 256) {
      const int row = e / own, q = e - row * own;
      const long long off = (base + (long long)row * W + x0 + q) * ld;
      float cv[3];
      load_rgb_f32(c + off, vec, cv);
      const float* tp = t + row * 3 * CF_HSEG + lead + q;
      store_px(out + off, ld, vec, cv[0] + tp[0], cv[1] + tp[CF_HSEG], cv[2] + tp[2 * CF_HSEG]);
    }
    // no barrier here: the next step's loads write buf[0] and read carry, both last touched before the final level's barrier; its
    // level 1 writes buf[1] only behind the barrier that follows the loads, which every thread reaches after its stores above
  }
}

// ---- AdaIN -------------------------------------------------------------------------------------------------------------------
// pass 1: fp64 (sum, sum of squares) of RGB of c[n] and of s[n % src_n] over one block of CF_SPX pixels -> part[n][j][12]
// (c sums, c squares, s sums, s squares; 3 each).  Strided per thread, xor butterfly per wave, the four waves left to right.
template <bool F16>
__global__ __launch_bounds__(256) void cf_adain_stats_kernel(const float* __restrict__ c, int ld_c, const uint16_t* __restrict__ s, int ld_s,
                                                             int src_n, long long P, int parts, double* __restrict__ part, int vec_c,
                                                             int vec_s) {
  __shared__ double red[12][4];
  const int n = blockIdx.x / parts, j = blockIdx.x % parts;
  const float* cn = c + (long long)n * P * ld_c;
  const uint16_t* sn = s + (long long)(n % src_n) * P * ld_s;
  const long long p0 = (long long)j * CF_SPX, p1 = min(P, p0 + CF_SPX);
  double acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.0;
  for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
    float cv[3], sv[3];
    load_rgb_f32(cn + p * ld_c, vec_c, cv);
    load_rgb_16<F16>(sn + p * ld_s, vec_s, sv);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double a = cv[k], b = sv[k];
      acc[k] += a;
      acc[3 + k] += a * a;
      acc[6 + k] += b;
      acc[9 + k] += b * b;
    }
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 12) part[(long long)blockIdx.x * 12 + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// pass 2: one workgroup per image adds the parts in ascending order and writes fp32 (a, b) per channel:
// a = sigma_s / sigma_c, b = mu_s - a * mu_c, sigma = sqrt(unbiased variance + 1e-5), all in fp64 until the final rounding.
__global__ __launch_bounds__(64) void cf_adain_finalize_kernel(const double* __restrict__ part, int parts, double P, float* __restrict__ ab) {
  __shared__ double tot[12];
  if (threadIdx.x < 12) {
    const double* p = part + (long long)blockIdx.x * parts * 12 + threadIdx.x;
    double v = 0.0;
    for (int j = 0; j < parts; ++j) v += p[(long long)j * 12];
    tot[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    const double mu_c = tot[k] / P, mu_s = tot[6 + k] / P;
    const double var_c = fmax(tot[3 + k] - tot[k] * mu_c, 0.0) / (P - 1.0), var_s = fmax(tot[9 + k] - tot[6 + k] * mu_s, 0.0) / (P - 1.0);
    const double a = sqrt(var_s + 1e-5) / sqrt(var_c + 1e-5);
    ab[(blockIdx.x * 3 + k) * 2] = (float)a;
    ab[(blockIdx.x * 3 + k) * 2 + 1] = (float)(mu_s - a * mu_c);
  }
}

// pass 3: out = a * c + b per pixel and channel
__global__ __launch_bounds__(256) void cf_adain_apply_kernel(const float* __restrict__ c, int ld, const float* __restrict__ ab,
                                                             float* __restrict__ out, long long P, int blocks_per_image, int vec) {
  const int n = blockIdx.x / blocks_per_image;
  const long long p = (long long)(blockIdx.x % blocks_per_image) * 256 + threadIdx.x;
  if (p >= P) return;
  const float* k = ab + n * 6;
  const long long off = ((long long)n * P + p) * ld;
  float cv[3];
  load_rgb_f32(c + off, vec, cv);
  store_px(out + off, ld, vec, k[0] * cv[0] + k[1], k[2] * cv[1] + k[3], k[4] * cv[2] + k[5]);
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline int adain_parts(long long P) { return (int)((P + CF_SPX - 1) / CF_SPX); }

// argument rules shared by the entry points; "" when legal
const char* bad_args(const void* c, int ld_c, const void* s, int ld_s, const void* out, int N, int src_n, int H, int W, int dtype) {
  if (!c || !s || !out) return "null pointer";
  if (N <= 0 || src_n <= 0 || H <= 0 || W <= 0) return "N, src_n, H and W must be >= 1";
  if (N % src_n != 0) return "src_n must divide N";
  if (ld_c < 3 || ld_s < 3) return "ld_c and ld_s must be >= 3 (RGB)";
  if (dtype != UR_DT_BF16 && dtype != UR_DT_F16) return "dtype must be UR_DT_BF16 or UR_DT_F16";
  if (out == c) return "out must not be c (the passes read c after they begin to write out)";
  return "";
}

}  // namespace

extern "C" {

int ur_color_fix_wavelet(const void* c_f32, int ld_c, const void* src_16, int ld_s, float* out, int N, int src_n, int H, int W, int dtype,
                         ur_stream_t stream) {
  const char* why = bad_args(c_f32, ld_c, src_16, ld_s, out, N, src_n, H, W, dtype);
  UR_REQUIRE(!*why, why);
  const int tx = (W + CF_VC - 1) / CF_VC, ty = (H + CF_VR - 1) / CF_VR, hy = (H + CF_HR - 1) / CF_HR;
  // one 256-thread workgroup per tile; a launch's work-item count has to stay below 2^31
  UR_REQUIRE((long long)N * tx * ty <= INT_MAX / 256 && (long long)N * hy <= INT_MAX / 256, "too many tiles: N * H * W is too large");
  const float* c = (const float*)c_f32;
  const int vec_c = ld_c % 4 == 0 && aligned(c, 16) && aligned(out, 16);
  const int vec_s = ld_s % 4 == 0 && aligned(src_16, 8);
  hipStream_t s = (hipStream_t)stream;
  const double px = (double)N * H * W;
  ur::ProfScope prof("color_fix_wavelet", px * 3 * 10 * 4, px * (4.0 * ld_c * 4 + 2.0 * ld_s), s);
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(cf_wavelet_cols_kernel<F16>, dim3(N * tx * ty), dim3(256), 0, s, c, ld_c, (const uint16_t*)src_16,
                                         ld_s, out, src_n, H, W, tx, ty, vec_c, vec_s));
  int rc = ur::check_launch("ur_color_fix_wavelet (columns)");
  if (rc) return rc;
  hipLaunchKernelGGL(cf_wavelet_rows_kernel, dim3(N * hy), dim3(256), 0, s, c, ld_c, out, H, W, hy, vec_c);
  return ur::check_launch("ur_color_fix_wavelet (rows)");
}

size_t ur_color_fix_adain_ws_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * adain_parts((long long)H * W) * 12 * sizeof(double) + (size_t)N * 6 * sizeof(float);
}

int ur_color_fix_adain(const void* c_f32, int ld_c, const void* src_16, int ld_s, float* out, int N, int src_n, int H, int W, int dtype,
                       void* ws, size_t ws_bytes, ur_stream_t stream) {
  const char* why = bad_args(c_f32, ld_c, src_16, ld_s, out, N, src_n, H, W, dtype);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(ws, "null pointer");
  const long long P = (long long)H * W;
  UR_REQUIRE(P >= 2, "H * W must be >= 2 (unbiased variance)");
  const int parts = adain_parts(P);
  const long long apply_blocks = (P + 255) / 256;
  UR_REQUIRE((long long)N * apply_blocks <= INT_MAX / 256, "too many pixels: N * H * W must be below 2^31");
  const size_t need = ur_color_fix_adain_ws_bytes(N, H, W);
  UR_REQUIRE(ws_bytes >= need, "workspace too small: " + std::to_string(ws_bytes) + " < " + std::to_string(need) + " bytes");
  UR_REQUIRE(aligned(ws, 8), "workspace must be 8-byte aligned");
  const float* c = (const float*)c_f32;
  const int vec_c = ld_c % 4 == 0 && aligned(c, 16) && aligned(out, 16);
  const int vec_s = ld_s % 4 == 0 && aligned(src_16, 8);
  double* part = (double*)ws;
  float* ab = (float*)(part + (size_t)N * parts * 12);
  hipStream_t s = (hipStream_t)stream;
  const double px = (double)N * P;
  ur::ProfScope prof("color_fix_adain", px * 3 * 10, px * (3.0 * ld_c * 4 + 2.0 * ld_s), s);
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(cf_adain_stats_kernel<F16>, dim3(N * parts), dim3(256), 0, s, c, ld_c, (const uint16_t*)src_16, ld_s,
                                         src_n, P, parts, part, vec_c, vec_s));
  int rc = ur::check_launch("ur_color_fix_adain (statistics)");
  if (rc) return rc;
  hipLaunchKernelGGL(cf_adain_finalize_kernel, dim3(N), dim3(64), 0, s, part, parts, (double)P, ab);
  rc = ur::check_launch("ur_color_fix_adain (finalize)");
  if (rc) return rc;
  hipLaunchKernelGGL(cf_adain_apply_kernel, dim3((unsigned)(N * apply_blocks)), dim3(256), 0, s, c, ld_c, ab, out, P, (int)apply_blocks, vec_c);
  return ur::check_launch("ur_color_fix_adain (apply)");
}

}  // extern "C"
