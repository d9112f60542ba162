// Full-reference image metrics (PSNR, SSIM) for gfx950: skimage semantics, fp64 moments, fixed-order reductions, no atomics.
#include "common.h"

#include <climits>

namespace {

constexpr int MT_TW = 64;      // output tile width: one lane per output column
constexpr int MT_TH = 16;      // output tile height
constexpr int MT_CH = 16;      // horizontal-moment rows held in LDS at once
constexpr int MT_WAVES = 4;    // 256 threads; wave g owns tile rows g, g+4, g+8, g+12

// Sum of one double per thread over the 256-thread block, in a fixed order (xor butterfly in each wave, then the four wave
// totals left to right): the same inputs give the same bits on every run.  Valid in thread 0.
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// Pass 1: one block per (output tile, image-channel plane).  The SSIM map is evaluated on the valid interior
// (H-win+1) x (W-win+1); the tile's horizontal win-tap sums of the five moments x, y, x^2, y^2, xy are built MT_CH input rows
// at a time in LDS (fp64, moment-major so a wave reads 64 consecutive doubles), and every output row adds the rows it covers
// into fp64 registers in ascending row order - the order, and so the bits, do not depend on MT_CH or on win.  The squared
// error for PSNR is summed over this tile's share of a disjoint partition of the FULL plane: tile (ty, tx) owns input rows
// [ty*TH, (ty+1)*TH) and columns [tx*TW, (tx+1)*TW), the last tile row / column also owns the win-1 border rows / columns.
__global__ __launch_bounds__(256) void image_metrics_tiles_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                  int H, int W, int win, int tiles_x, int tiles_y, double c1,
                                                                  double c2, double* __restrict__ ssim_part,
                                                                  double* __restrict__ sse_part) {
  __shared__ double mom[5][MT_CH][MT_TW];
  __shared__ double red[2][MT_WAVES];
  const int T = tiles_x * tiles_y;
  const int tile = blockIdx.x % T;
  const long long plane = blockIdx.x / T;
  const int ty = tile / tiles_x, tx = tile % tiles_x;
  const int OH = H - win + 1, OW = W - win + 1;
  const int y0 = ty * MT_TH, x0 = tx * MT_TW;
  const int orows = min(MT_TH, OH - y0), ocols = min(MT_TW, OW - x0);
  const int nrows = orows + win - 1;                         // input rows the tile's outputs read
  const int x = threadIdx.x & 63, g = threadIdx.x >> 6;
  const float* p = pred + plane * H * W;
  const float* t = target + plane * H * W;

  double acc[4][5];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int m = 0; m < 5; ++m) acc[i][m] = 0.0;

  for (int c0 = 0; c0 < nrows; c0 += MT_CH) {
    // horizontal pass: chunk row j = c0 + g + 4i, column x0 + x (in bounds: x0+x+win-1 <= W-1, y0+j <= H-1)
#pragma unroll
    for (int i = 0; i < MT_CH / MT_WAVES; ++i) {
      const int jj = g + MT_WAVES * i, j = c0 + jj;
      double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      if (x < ocols && j < nrows) {
        const long long off = (long long)(y0 + j) * W + x0 + x;
        for (int k = 0; k < win; ++k) {
          const double a = p[off + k], b = t[off + k];
          s[0] += a;
          s[1] += b;
          s[2] += a * a;
          s[3] += b * b;
          s[4] += a * b;
        }
      }
#pragma unroll
      for (int m = 0; m < 5; ++m) mom[m][jj][x] = s[m];
    }
    __syncthreads();
    // vertical pass: output row r = g + 4i adds input rows [r, r+win-1] of this chunk, ascending (wave-uniform bounds)
#pragma unroll
    for (int i = 0; i < MT_TH / MT_WAVES; ++i) {
      const int r = g + MT_WAVES * i;
      const int lo = max(r, c0), hi = min(r + win - 1, c0 + MT_CH - 1);
      for (int j = lo; j <= hi; ++j)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[i][m] += mom[m][j - c0][x];
    }
    __syncthreads();
  }

  const double inv_np = 1.0 / ((double)win * win);
  const double cov_norm = (double)win * win / ((double)win * win - 1.0);
  double ssum = 0.0;
#pragma unroll
  for (int i = 0; i < MT_TH / MT_WAVES; ++i) {
    const int r = g + MT_WAVES * i;
    if (r < orows && x < ocols) {
      const double ux = acc[i][0] * inv_np, uy = acc[i][1] * inv_np;
      const double vx = cov_norm * (acc[i][2] * inv_np - ux * ux);
      const double vy = cov_norm * (acc[i][3] * inv_np - uy * uy);
      const double vxy = cov_norm * (acc[i][4] * inv_np - ux * uy);
      ssum += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
    }
  }

  const int ry0 = y0, ry1 = ty == tiles_y - 1 ? H : y0 + MT_TH;
  const int rx0 = x0, rx1 = tx == tiles_x - 1 ? W : x0 + MT_TW;
  double se = 0.0;
  for (int yy = ry0 + g; yy < ry1; yy += MT_WAVES)
    for (int xx = rx0 + x; xx < rx1; xx += 64) {
      const double d = (double)p[(long long)yy * W + xx] - (double)t[(long long)yy * W + xx];
      se += d * d;
    }

  const double bs = block_sum(ssum, red[0]);
  const double be = block_sum(se, red[1]);
  if (threadIdx.x == 0) {
    ssim_part[blockIdx.x] = bs;
    sse_part[blockIdx.x] = be;
  }
}

// Pass 2: one block per image sums its C*T partials in a fixed order (strided per thread, then block_sum).
__global__ __launch_bounds__(256) void image_metrics_final_kernel(const double* __restrict__ ssim_part,
                                                                  const double* __restrict__ sse_part, int parts,
                                                                  double ssim_count, double px_count, double peak2,
                                                                  double* __restrict__ psnr, double* __restrict__ ssim) {
  __shared__ double red[2][MT_WAVES];
  const long long base = (long long)blockIdx.x * parts;
  double s = 0.0, e = 0.0;
  for (int i = threadIdx.x; i < parts; i += 256) {
    s += ssim_part[base + i];
    e += sse_part[base + i];
  }
  const double bs = block_sum(s, red[0]);
  const double be = block_sum(e, red[1]);
  if (threadIdx.x == 0) {
    ssim[blockIdx.x] = bs / ssim_count;
    psnr[blockIdx.x] = 10.0 * log10(peak2 / (be / px_count));      // mse == 0 -> +inf, as the CPU path
  }
}

// (64-bit: W + 63 and tx * ty do not fit an int for every W and H an int holds; bad_shape bounds the product afterwards)
inline long long tiles_of(int H, int W, int win, int* tx, int* ty) {
  *tx = (int)(((long long)W - win + MT_TW) / MT_TW);
  *ty = (int)(((long long)H - win + MT_TH) / MT_TH);
  return (long long)*tx * *ty;
}

// shape rules shared by the two entry points; "" when the shape is legal
const char* bad_shape(int N, int C, int H, int W, int win) {
  if (N < 1 || C < 1) return "N and C must be >= 1";
  if (win < 3 || win % 2 == 0) return "win must be odd and >= 3";
  if (H < win || W < win) return "H and W must be >= win";
  int tx, ty;
  // one 256-thread block per tile and plane; the launch's work-item count has to stay below 2^31
  const long long tiles = tiles_of(H, W, win, &tx, &ty);
  if (tiles > INT_MAX / 256 || (long long)N * C > INT_MAX / 256 || (long long)N * C * tiles > INT_MAX / 256) return "too many tiles: N*C*tiles must be below 2^23";
  return "";
}

}  // namespace

extern "C" {

long long ur_image_metrics_ws_size(int N, int C, int H, int W, int win) {
  const char* why = bad_shape(N, C, H, W, win);
  if (*why) return ur::fail(UR_E_INVALID, std::string("ur_image_metrics_ws_size: ") + why);
  int tx, ty;
  return 2LL * N * C * tiles_of(H, W, win, &tx, &ty) * (long long)sizeof(double);
}

int ur_image_metrics(const float* pred, const float* target, int N, int C, int H, int W, int win, double data_range,
                     double* psnr, double* ssim, void* ws, long long ws_bytes, ur_stream_t stream) {
  UR_REQUIRE(pred && target && psnr && ssim && ws, "null pointer");
  const char* why = bad_shape(N, C, H, W, win);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(data_range > 0.0, "data_range must be > 0");
  const long long need = ur_image_metrics_ws_size(N, C, H, W, win);
  UR_REQUIRE(ws_bytes >= need, "workspace too small: " + std::to_string(ws_bytes) + " < " + std::to_string(need) + " bytes");
  int tx, ty;
  const int T = (int)tiles_of(H, W, win, &tx, &ty);
  const int blocks = N * C * T;
  double* ssim_part = (double*)ws;
  double* sse_part = ssim_part + blocks;
  hipStream_t s = (hipStream_t)stream;
  const double px = (double)N * C * H * W;
  ur::ProfScope prof("image_metrics", px * (10.0 * win + 30.0), 8.0 * px, s);
  hipLaunchKernelGGL(image_metrics_tiles_kernel, dim3(blocks), dim3(256), 0, s, pred, target, H, W, win, tx, ty,
                     (0.01 * data_range) * (0.01 * data_range), (0.03 * data_range) * (0.03 * data_range), ssim_part, sse_part);
  int rc = ur::check_launch("ur_image_metrics (tiles)");
  if (rc) return rc;
  hipLaunchKernelGGL(image_metrics_final_kernel, dim3(N), dim3(256), 0, s, ssim_part, sse_part, C * T,
                     (double)C * (H - win + 1) * (W - win + 1), (double)C * H * W, data_range * data_range, psnr, ssim);
  return ur::check_launch("ur_image_metrics (final)");
}

}  // extern "C"
