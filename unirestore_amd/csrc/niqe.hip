// NIQE (no-reference image quality) block features for gfx950: fp64 throughout, fixed-order sums, no atomics, 64-bit element
// offsets.  Five kernels - luma, MSCN field, per-block moments of the five fields, the antialiased bicubic halving, and the AGGD
// fit - that unirestore_amd/niqe.py chains into the 36 features of every 96 x 96 block.  The conventions are written out in
// include/unirestore_hip.h; the 36-dimensional algebra of the score itself runs on the host.
#include "common.h"

#include <cmath>

// The host restatement this file is checked against evaluates every expression as written: no fused multiply-add anywhere here.
#pragma clang fp contract(off)

namespace {

constexpr int NQ_GRID = 9801;          // alpha = 0.2 + 0.001 * i, i in [0, 9801)
constexpr int NQ_FIELDS = 5;           // M and its four rolled products
constexpr int NQ_MOMENTS = 6;          // n-, sum v^2 over v < 0, n+, sum v^2 over v > 0, sum |v|, sum v^2
constexpr int NQ_FEATS = 18;           // features of one scale
constexpr long long NQ_LIMIT = ur::GRID_1D_LIMIT;

struct Gauss7 {
  double w[7];
};

__global__ __launch_bounds__(256) void niqe_luma_kernel(const float* __restrict__ x, double* __restrict__ y, int H, int W, int h, int w,
                                                        long long total, int ycbcr) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int xx = (int)(i % w);
  const long long t = i / w;
  const int yy = (int)(t % h);
  const long long n = t / h;
  const long long plane = (long long)H * W;
  const float* p = x + n * 3 * plane + (long long)yy * W + xx;
  const double r = p[0], g = p[plane], b = p[2 * plane];
  const double v = ycbcr ? ((16.0 + 65.481 * r) + 128.553 * g) + 24.966 * b : ((0.299 * r + 0.587 * g) + 0.114 * b) * 255.0;
  y[i] = rint(v);                                            // round half to even
}

constexpr int MS_T = 32;               // output tile edge
constexpr int MS_R = 3;                // halo of the 7-tap window
constexpr int MS_IN = MS_T + 2 * MS_R;

// One block per 32 x 32 output tile and image: the tile and its replicate halo in LDS, the horizontal 7-tap sums of Y and Y^2,
// then the vertical ones; taps ascending in both passes.
__global__ __launch_bounds__(256) void niqe_mscn_kernel(const double* __restrict__ y, double* __restrict__ m, int h, int w, int tiles_x,
                                                        int tiles_y, Gauss7 g) {
  __shared__ double tile[MS_IN][MS_IN + 1];
  __shared__ double h1[MS_IN][MS_T + 1];
  __shared__ double h2[MS_IN][MS_T + 1];
  const int T = tiles_x * tiles_y;
  const int t = blockIdx.x % T;
  const long long n = blockIdx.x / T;
  const int y0 = (t / tiles_x) * MS_T, x0 = (t % tiles_x) * MS_T;
  const double* src = y + n * h * w;
  for (int i = threadIdx.x; i < MS_IN * MS_IN; i += 256) {
    const int r = i / MS_IN, c = i - r * MS_IN;
    const int gy = min(max(y0 + r - MS_R, 0), h - 1), gx = min(max(x0 + c - MS_R, 0), w - 1);
    tile[r][c] = src[(long long)gy * w + gx];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < MS_IN * MS_T; i += 256) {
    const int r = i / MS_T, c = i - r * MS_T;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const double v = tile[r][c + k];
      s1 += g.w[k] * v;
      s2 += g.w[k] * (v * v);
    }
    h1[r][c] = s1;
    h2[r][c] = s2;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < MS_T * MS_T; i += 256) {
    const int r = i / MS_T, c = i - r * MS_T;
    double mu = 0.0, e2 = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      mu += g.w[k] * h1[r + k][c];
      e2 += g.w[k] * h2[r + k][c];
    }
    if (y0 + r < h && x0 + c < w) {
      const double sigma = sqrt(fabs(e2 - mu * mu));
      m[n * h * w + (long long)(y0 + r) * w + x0 + c] = (tile[r + MS_R][c + MS_R] - mu) / (sigma + 1.0);
    }
  }
}

// One workgroup per bs x bs block (dynamic LDS: bs * bs doubles).  Thread t owns pixels t, t + 256, ... of the block in row-major
// order and adds them ascending; the 30 sums then go through the xor butterfly of each wave and the four wave totals left to
// right.  The rolled neighbours wrap inside the block: rolled(s)[i][j] = M[(i - s0) mod bs][(j - s1) mod bs].
__global__ __launch_bounds__(256) void niqe_moments_kernel(const double* __restrict__ f, double* __restrict__ out, int h, int w, int bs,
                                                           int blocks_x, int blocks_y) {
  extern __shared__ double blk[];
  __shared__ double red[NQ_FIELDS * NQ_MOMENTS][4];
  const int B = blocks_x * blocks_y;
  const int b = blockIdx.x % B;
  const long long n = blockIdx.x / B;
  const int by = b / blocks_x, bx = b - by * blocks_x;
  const double* src = f + n * h * w + (long long)by * bs * w + (long long)bx * bs;
  const int P = bs * bs;
  for (int i = threadIdx.x; i < P; i += 256) {
    const int r = i / bs, c = i - r * bs;
    blk[i] = src[(long long)r * w + c];
  }
  __syncthreads();
  double acc[NQ_FIELDS][NQ_MOMENTS];
#pragma unroll
  for (int k = 0; k < NQ_FIELDS; ++k)
#pragma unroll
    for (int j = 0; j < NQ_MOMENTS; ++j) acc[k][j] = 0.0;
  for (int i = threadIdx.x; i < P; i += 256) {
    const int r = i / bs, c = i - r * bs;
    const int rm = (r == 0 ? bs - 1 : r - 1) * bs;
    const int cm = c == 0 ? bs - 1 : c - 1, cp = c == bs - 1 ? 0 : c + 1;
    const double v0 = blk[i];
    const double v[NQ_FIELDS] = {v0, v0 * blk[r * bs + cm], v0 * blk[rm + c], v0 * blk[rm + cm], v0 * blk[rm + cp]};
#pragma unroll
    for (int k = 0; k < NQ_FIELDS; ++k) {
      const double a = v[k], a2 = a * a;
      acc[k][0] += a < 0.0 ? 1.0 : 0.0;
      acc[k][1] += a < 0.0 ? a2 : 0.0;
      acc[k][2] += a > 0.0 ? 1.0 : 0.0;
      acc[k][3] += a > 0.0 ? a2 : 0.0;
      acc[k][4] += fabs(a);
      acc[k][5] += a2;
    }
  }
#pragma unroll
  for (int k = 0; k < NQ_FIELDS; ++k)
#pragma unroll
    for (int j = 0; j < NQ_MOMENTS; ++j) {
      double s = acc[k][j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if ((threadIdx.x & 63) == 0) red[k * NQ_MOMENTS + j][threadIdx.x >> 6] = s;
    }
  __syncthreads();
  if (threadIdx.x < NQ_FIELDS * NQ_MOMENTS) {
    const double* q = red[threadIdx.x];
    out[(long long)blockIdx.x * (NQ_FIELDS * NQ_MOMENTS) + threadIdx.x] = ((q[0] + q[1]) + q[2]) + q[3];
  }
}

__device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

// One thread per output: the eight rows' taps of each of the eight columns (ascending), then the eight column taps.
__global__ __launch_bounds__(256) void niqe_halve_kernel(const double* __restrict__ y, double* __restrict__ out, int h, int w,
                                                         long long total) {
  constexpr double K[8] = {-0.0234375 / 2, -0.0703125 / 2, 0.2265625 / 2, 0.8671875 / 2, 0.8671875 / 2, 0.2265625 / 2, -0.0703125 / 2,
                           -0.0234375 / 2};
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ow = w / 2, oh = h / 2;
  const int ox = (int)(i % ow);
  const long long t = i / ow;
  const int oy = (int)(t % oh);
  const long long n = t / oh;
  const double* src = y + n * h * w;
  long long rows[8];
  int cols[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    rows[k] = (long long)mirror(2 * oy - 3 + k, h) * w;
    cols[k] = mirror(2 * ox - 3 + k, w);
  }
  double res = 0.0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += K[k] * (src[rows[k] + cols[c]] / 255.0);
    res += K[c] * s;
  }
  out[i] = res * 255.0;
}

// One thread per (block, field).  rho is strictly increasing: the first table entry >= R and its left neighbour are the only
// candidates of the argmin of (rho - R)^2; on equal distance the lower index (the first minimum) wins.
__global__ __launch_bounds__(256) void niqe_fit_kernel(const double* __restrict__ mom, const double* __restrict__ rho,
                                                       const double* __restrict__ scale, const double* __restrict__ mean_ratio,
                                                       double* __restrict__ feat, int* __restrict__ alpha_index, long long total, double P,
                                                       int ld, int col_off) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % NQ_FIELDS);
  const long long row = i / NQ_FIELDS;
  const double* q = mom + i * NQ_MOMENTS;
  const double l = sqrt(q[1] / q[0]), r = sqrt(q[3] / q[2]);
  const double gam = l / r, g2 = gam * gam;
  const double ma = q[4] / P;
  const double rhat = (ma * ma) / (q[5] / P);
  const double R = ((rhat * (g2 * gam + 1.0)) * (gam + 1.0)) / ((g2 + 1.0) * (g2 + 1.0));
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  int pick = -1;
  double alpha = nan, bl = nan, br = nan, mr = nan;
  if (R == R) {
    int lo = 0, hi = NQ_GRID;                                // first index with rho[index] >= R
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (rho[mid] < R) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) pick = 0;
    else if (lo == NQ_GRID) pick = NQ_GRID - 1;
    else {
      const double d0 = rho[lo - 1] - R, d1 = rho[lo] - R;
      pick = d1 * d1 < d0 * d0 ? lo : lo - 1;
    }
    alpha = 0.2 + 0.001 * (double)pick;
    bl = l * scale[pick];
    br = r * scale[pick];
    mr = mean_ratio[pick];
  }
  if (alpha_index) alpha_index[i] = pick;
  double* o = feat + row * ld + col_off;
  if (k == 0) {
    o[0] = alpha;
    o[1] = (bl + br) / 2.0;
  } else {
    o += 2 + 4 * (k - 1);
    o[0] = alpha;
    o[1] = (br - bl) * mr;
    o[2] = bl;
    o[3] = br;
  }
}

int unsupported(const char* who, const std::string& msg) { return ur::fail(UR_E_UNSUPPORTED, std::string(who) + ": " + msg); }

}  // namespace

#define NQ_LIMIT_CHECK(count, what)                                                                                    \
  do {                                                                                                                 \
    if ((count) >= NQ_LIMIT) return unsupported(__func__, std::string(what) + " must be below 2^31 - 256, got " + std::to_string(count)); \
  } while (0)

extern "C" {

int ur_niqe_luma(const float* x, double* y, int N, int H, int W, int h, int w, int color_space, ur_stream_t stream) {
  UR_REQUIRE(x && y, "null pointer");
  UR_REQUIRE(N >= 1 && H >= 1 && W >= 1, "N, H and W must be >= 1");
  UR_REQUIRE(h >= 1 && w >= 1 && h <= H && w <= W, "the crop h x w must lie inside H x W");
  UR_REQUIRE(color_space == 0 || color_space == 1, "color_space must be 0 (yiq) or 1 (ycbcr)");
  const long long total = (long long)N * h * w;
  NQ_LIMIT_CHECK(total, "N*h*w");
  UR_GRID_1D(blocks, total, 256);
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("niqe_luma", 6.0 * total, 20.0 * total, s);
  hipLaunchKernelGGL(niqe_luma_kernel, dim3(blocks), dim3(256), 0, s, x, y, H, W, h, w, total, color_space);
  return ur::check_launch("ur_niqe_luma");
}

int ur_niqe_mscn(const double* y, double* m, int N, int h, int w, ur_stream_t stream) {
  UR_REQUIRE(y && m, "null pointer");
  UR_REQUIRE(y != m, "m must not be y");
  UR_REQUIRE(N >= 1 && h >= 1 && w >= 1, "N, h and w must be >= 1");
  const long long tx = ((long long)w + MS_T - 1) / MS_T, ty = ((long long)h + MS_T - 1) / MS_T;
  const long long blocks = (long long)N * tx * ty;
  NQ_LIMIT_CHECK(blocks, "N*tiles (32 x 32 tiles)");
  Gauss7 g;
  double sum = 0.0;
  const double sigma = 7.0 / 6.0;
  for (int k = 0; k < 7; ++k) sum += g.w[k] = std::exp(-(double)((k - 3) * (k - 3)) / (2.0 * sigma * sigma));
  for (int k = 0; k < 7; ++k) g.w[k] /= sum;
  hipStream_t s = (hipStream_t)stream;
  const double px = (double)N * h * w;
  ur::ProfScope prof("niqe_mscn", 60.0 * px, 16.0 * px, s);
  hipLaunchKernelGGL(niqe_mscn_kernel, dim3((unsigned)blocks), dim3(256), 0, s, y, m, h, w, (int)tx, (int)ty, g);
  return ur::check_launch("ur_niqe_mscn");
}

int ur_niqe_block_moments(const double* field, double* moments, int N, int h, int w, int bs, ur_stream_t stream) {
  UR_REQUIRE(field && moments, "null pointer");
  UR_REQUIRE(bs == 96 || bs == 48, "bs must be 96 or 48");
  UR_REQUIRE(N >= 1 && h >= bs && w >= bs && h % bs == 0 && w % bs == 0, "N must be >= 1, h and w positive multiples of bs");
  const long long bx = w / bs, by = h / bs;
  const long long blocks = (long long)N * bx * by;
  NQ_LIMIT_CHECK(blocks, "N*blocks");
  const int lds = bs * bs * (int)sizeof(double);
  static ur::DeviceOnce attr_once;      // the attribute is per device
  if (auto once_guard = attr_once.first()) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(&niqe_moments_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 96 * (int)sizeof(double));
  }
  hipStream_t s = (hipStream_t)stream;
  const double px = (double)N * h * w;
  ur::ProfScope prof("niqe_block_moments", 40.0 * px, 8.0 * px, s);
  hipLaunchKernelGGL(niqe_moments_kernel, dim3((unsigned)blocks), dim3(256), lds, s, field, moments, h, w, bs, (int)bx, (int)by);
  return ur::check_launch("ur_niqe_block_moments");
}

int ur_niqe_halve(const double* y, double* out, int N, int h, int w, ur_stream_t stream) {
  UR_REQUIRE(y && out, "null pointer");
  UR_REQUIRE(y != out, "out must not be y");
  UR_REQUIRE(N >= 1 && h >= 4 && w >= 4 && h % 2 == 0 && w % 2 == 0, "N must be >= 1, h and w even and >= 4");
  const long long total = (long long)N * (h / 2) * (w / 2);
  NQ_LIMIT_CHECK((long long)N * h * w, "N*h*w");
  UR_GRID_1D(blocks, total, 256);
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("niqe_halve", 200.0 * total, 40.0 * total, s);
  hipLaunchKernelGGL(niqe_halve_kernel, dim3(blocks), dim3(256), 0, s, y, out, h, w, total);
  return ur::check_launch("ur_niqe_halve");
}

int ur_niqe_fit(const double* moments, const double* rho, const double* scale, const double* mean_ratio, double* features,
                int* alpha_index, long long rows, int block_pixels, int ld, int col_off, ur_stream_t stream) {
  UR_REQUIRE(moments && rho && scale && mean_ratio && features, "null pointer");
  UR_REQUIRE(rows >= 1, "rows must be >= 1");
  UR_REQUIRE(block_pixels >= 1, "block_pixels must be >= 1");
  UR_REQUIRE(col_off >= 0 && ld >= NQ_FEATS && col_off <= ld - NQ_FEATS, "the 18 features must fit a row: 0 <= col_off <= ld - 18");
  NQ_LIMIT_CHECK(rows, "rows");                              // (before the product below: it cannot overflow then)
  const long long total = rows * NQ_FIELDS;
  NQ_LIMIT_CHECK(total, "rows*5");
  UR_GRID_1D(blocks, total, 256);
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("niqe_fit", 60.0 * total, 80.0 * total, s);
  hipLaunchKernelGGL(niqe_fit_kernel, dim3(blocks), dim3(256), 0, s, moments, rho, scale, mean_ratio, features, alpha_index, total,
                     (double)block_pixels, ld, col_off);
  return ur::check_launch("ur_niqe_fit");
}

}  // extern "C"
