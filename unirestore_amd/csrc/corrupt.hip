// ImageNet-C style corruptions of u8 images for gfx950 (the specification is the ur_corrupt_* comment in include/unirestore_hip.h).
// x u8 [N,H,W,3] contiguous HWC -> out of the same shape: u8 (out_kind 0) or the fp32 value before the floor, clamped to [0, 255]
// (out_kind 1).  fp32 arithmetic on the 0-255 scale; an image's randomness comes from its own key (philox.h), never from the batch.
// A handful of primitives, one thread per element (or pixel) each: these are bandwidth-bound image passes next to a 33 ms forward.
// No allocation, no synchronisation, no atomics, no order that depends on scheduling: the same inputs give the same bits.
#include "common.h"
#include "philox.h"

#include <climits>

namespace {

constexpr int CR_SPX = 16384;                      // pixels (map cells) per workgroup of a reduction's first stage
constexpr uint32_t DRAW_GAUSSIAN = 16, DRAW_SPECKLE = 17, DRAW_FLIP = 18, DRAW_SALT = 19, DRAW_SHOT = 20, DRAW_FOG = 21;

__device__ __forceinline__ void put(void* out, long long i, float v, int out_kind) {
  v = fminf(fmaxf(v, 0.f), 255.f);
  if (out_kind) ((float*)out)[i] = v;
  else ((uint8_t*)out)[i] = (uint8_t)v;            // truncation: floor of a value >= 0
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- keyed pointwise noise: one thread per Philox counter = four consecutive elements of one image ---------------------------
__global__ __launch_bounds__(256) void corrupt_noise_kernel(const uint8_t* __restrict__ x, const uint32_t* __restrict__ keys, void* out, int N,
                                                            int count, int mode, float c, const uint32_t* __restrict__ table, int out_kind) {
  const int nctr = (count + 3) >> 2;
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  if (t >= (long long)N * nctr) return;
  const int n = (int)(t / nctr), q = (int)(t % nctr);
  const uint32_t k0 = keys[2 * n], k1 = keys[2 * n + 1];
  const uint32_t draw = mode == 0 ? DRAW_GAUSSIAN : mode == 1 ? DRAW_SPECKLE : mode == 2 ? DRAW_FLIP : DRAW_SHOT;
  uint32_t w[4], w2[4] = {0u, 0u, 0u, 0u};
  philox4x32_10((uint32_t)q, draw, 0u, 0u, k0, k1, w);
  float f[4] = {0.f, 0.f, 0.f, 0.f};
  if (mode <= 1) {
    box_muller(w[0], w[1], &f[0], &f[1]);
    box_muller(w[2], w[3], &f[2], &f[3]);
  } else if (mode == 2) {
    philox4x32_10((uint32_t)q, DRAW_SALT, 0u, 0u, k0, k1, w2);
  }
  const long long base = (long long)n * count;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = 4 * q + j;
    if (e >= count) break;
    const uint8_t xb = x[base + e];
    const float xv = (float)xb;
    float v;
    if (mode == 0) {
      v = xv + c * f[j];
    } else if (mode == 1) {
      v = xv + xv * (c * f[j]);
    } else if (mode == 2) {
      v = word_to_uniform(w[j]) < c ? (word_to_uniform(w2[j]) < 0.5f ? 255.f : 0.f) : xv;
    } else {                                       // Poisson by table: the number of k with T[x][k] <= v24 (T is non-decreasing in k)
      const uint32_t v24 = w[j] >> 8;
      const uint32_t* row = table + (int)xb * 128;
      int lo = 0, hi = 128;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] <= v24) lo = mid + 1; else hi = mid;
      }
      v = (float)(min(lo, 127) * 255) / c;
    }
    put(out, base + e, v, out_kind);
  }
}

// ---- separable filter, replicate border: one pass along one axis, taps[k + r] on the sample at offset k, k ascending ---------------
template <typename TIn>
__global__ __launch_bounds__(256) void corrupt_sep_kernel(const TIn* __restrict__ in, const float* __restrict__ taps, int r, int vertical, void* out,
                                                          long long total, int H, int W, int final, int out_kind) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const int xc = (int)(i % (3 * W)), y = (int)((i / (3 * W)) % H), px = xc / 3, ch = xc - 3 * px;
  const TIn* img = in + (i / ((long long)3 * W * H)) * ((long long)3 * W * H);
  float acc = 0.f;
  for (int k = -r; k <= r; ++k) {
    const int yy = vertical ? clampi(y + k, 0, H - 1) : y, xx = vertical ? px : clampi(px + k, 0, W - 1);
    acc += taps[k + r] * (float)img[((long long)yy * W + xx) * 3 + ch];
  }
  if (final) put(out, i, acc, out_kind);
  else ((float*)out)[i] = acc;
}

// ---- tap list: out = sum over t (ascending) of w_t * x[b(y + ty_t)][b(x + tx_t)], b = replicate (0) or reflect-101 (1) -------------
__global__ __launch_bounds__(256) void corrupt_taps_kernel(const uint8_t* __restrict__ x, const int* __restrict__ taps, int n_taps, int per_image,
                                                           int border, void* out, long long total, int H, int W, int out_kind) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const int xc = (int)(i % (3 * W)), y = (int)((i / (3 * W)) % H), px = xc / 3, ch = xc - 3 * px;
  const long long n = i / ((long long)3 * W * H);
  const uint8_t* img = x + n * ((long long)3 * W * H);
  const int* tp = taps + (per_image ? n * 3LL * n_taps : 0);
  float acc = 0.f;
  for (int t = 0; t < n_taps; ++t) {
    int xx = px + tp[3 * t], yy = y + tp[3 * t + 1];
    if (border) {
      xx = xx < 0 ? -xx : xx >= W ? 2 * W - 2 - xx : xx;
      yy = yy < 0 ? -yy : yy >= H ? 2 * H - 2 - yy : yy;
    }
    xx = clampi(xx, 0, W - 1);                     // the border rule of mode 0; in mode 1 it only keeps a wild table inside the image
    yy = clampi(yy, 0, H - 1);
    acc += __int_as_float(tp[3 * t + 2]) * (float)img[((long long)yy * W + xx) * 3 + ch];
  }
  put(out, i, acc, out_kind);
}

// ---- zoom: (x + sum of K bilinear layers) / (K + 1); layer = (top, left, ch, cw, oh, ow): the crop and the size it is resampled to ----
__global__ __launch_bounds__(256) void corrupt_zoom_kernel(const uint8_t* __restrict__ x, const int* __restrict__ layers, int K, void* out,
                                                           long long total, int H, int W, int out_kind) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const int xc = (int)(i % (3 * W)), y = (int)((i / (3 * W)) % H), px = xc / 3, ch = xc - 3 * px;
  const uint8_t* img = x + (i / ((long long)3 * W * H)) * ((long long)3 * W * H) + ch;
  float acc = (float)x[i];
  for (int k = 0; k < K; ++k) {
    const int* L = layers + 6 * k;
    const int top = L[0], left = L[1], chh = L[2], cww = L[3], oh = max(L[4], 2), ow = max(L[5], 2);
    if (y >= oh || px >= ow) continue;             // the resampled crop does not reach this pixel: the layer adds nothing
    // position o * (in - 1) / (out - 1) in integers: the cell exactly, the fraction to one rounding
    const int ny = y * (chh - 1), iy = ny / (oh - 1), nx = px * (cww - 1), ix = nx / (ow - 1);
    const float fy = (float)(ny - iy * (oh - 1)) / (float)(oh - 1), fx = (float)(nx - ix * (ow - 1)) / (float)(ow - 1);
    const int y0 = clampi(top + iy, 0, H - 1), y1 = clampi(top + min(iy + 1, chh - 1), 0, H - 1);
    const int x0 = clampi(left + ix, 0, W - 1), x1 = clampi(left + min(ix + 1, cww - 1), 0, W - 1);
    const float p00 = img[((long long)y0 * W + x0) * 3], p01 = img[((long long)y0 * W + x1) * 3];
    const float p10 = img[((long long)y1 * W + x0) * 3], p11 = img[((long long)y1 * W + x1) * 3];
    const float a = p00 + fx * (p01 - p00), b = p10 + fx * (p11 - p10);      // pixel differences are exact
    acc += a + fy * (b - a);
  }
  put(out, i, acc / (float)(K + 1), out_kind);
}

// ---- integer statistics: per image the sum of every channel and the maximum over all of them, two stages ---------------------------
// stage 1: one block of CR_SPX pixels -> part[n][j][4] (sums of R, G, B <= 16384 * 255, maximum); integers, so any order is exact
__global__ __launch_bounds__(256) void corrupt_stats_kernel(const uint8_t* __restrict__ x, long long P, int parts, uint32_t* __restrict__ part) {
  __shared__ uint32_t red[4][4];
  const int n = blockIdx.x / parts, j = blockIdx.x % parts;
  const uint8_t* img = x + (long long)n * P * 3;
  const long long p0 = (long long)j * CR_SPX, p1 = min(P, p0 + CR_SPX);
  uint32_t acc[4] = {0u, 0u, 0u, 0u};
  for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t v = img[p * 3 + k];
      acc[k] += v;
      acc[3] = max(acc[3], v);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64);
      v = k < 3 ? v + u : max(v, u);
    }
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const uint32_t* r = red[threadIdx.x];
    part[(long long)blockIdx.x * 4 + threadIdx.x] = threadIdx.x < 3 ? r[0] + r[1] + r[2] + r[3] : max(max(r[0], r[1]), max(r[2], r[3]));
  }
}
// stage 2: one workgroup per image -> stats[n] = (mean R, mean G, mean B, maximum) in fp32; the means are the exact integer sums
// divided in fp64 and rounded once
__global__ __launch_bounds__(64) void corrupt_stats_finalize_kernel(const uint32_t* __restrict__ part, int parts, double P, float* __restrict__ stats) {
  if (threadIdx.x >= 4) return;
  const uint32_t* p = part + (long long)blockIdx.x * parts * 4 + threadIdx.x;
  unsigned long long s = 0;
  for (int j = 0; j < parts; ++j) s = threadIdx.x < 3 ? s + p[4LL * j] : max(s, (unsigned long long)p[4LL * j]);
  stats[blockIdx.x * 4 + threadIdx.x] = threadIdx.x < 3 ? (float)((double)s / P) : (float)s;
}

// ---- colour pointwise, one thread per pixel: contrast (0), brightness (1: V + a), saturate (2: S * a + b) through HSV ---------------
__global__ __launch_bounds__(256) void corrupt_color_kernel(const uint8_t* __restrict__ x, const float* __restrict__ stats, void* out, long long pixels,
                                                            long long P, int mode, float a, float b, int out_kind) {
  const long long p = blockIdx.x * 256LL + threadIdx.x;
  if (p >= pixels) return;
  const float r = x[3 * p], g = x[3 * p + 1], bl = x[3 * p + 2];
  float o0, o1, o2;
  if (mode == 0) {
    const float* m = stats + (p / P) * 4;
    o0 = (r - m[0]) * a + m[0];
    o1 = (g - m[1]) * a + m[1];
    o2 = (bl - m[2]) * a + m[2];
  } else {
    float v = fmaxf(r, fmaxf(g, bl));
    const float delta = v - fminf(r, fminf(g, bl));                       // exact: integers
    float s = delta == 0.f ? 0.f : delta / v, h6 = 0.f;
    if (delta != 0.f) {                             // ties go to blue, then green, then red; all of them give the same hue
      if (bl == v) h6 = 4.f + (r - g) / delta;
      else if (g == v) h6 = 2.f + (bl - r) / delta;
      else h6 = (g - bl) / delta;
      if (h6 < 0.f) h6 += 6.f;
    }
    if (mode == 1) v = fminf(fmaxf(v + a, 0.f), 255.f);
    else s = fminf(fmaxf(s * a + b, 0.f), 1.f);
    const float hi = floorf(h6), f = h6 - hi;
    const float pp = v * (1.f - s), qq = v * (1.f - f * s), tt = v * (1.f - (1.f - f) * s);
    const int sector = (int)hi % 6;
    o0 = sector == 0 || sector == 5 ? v : sector == 1 ? qq : sector == 4 ? tt : pp;
    o1 = sector == 1 || sector == 2 ? v : sector == 3 ? qq : sector == 0 ? tt : pp;
    o2 = sector == 3 || sector == 4 ? v : sector == 5 ? qq : sector == 2 ? tt : pp;
  }
  put(out, 3 * p, o0, out_kind);
  put(out, 3 * p + 1, o1, out_kind);
  put(out, 3 * p + 2, o2, out_kind);
}

// ---- pixelate by tables: box[k] = (first, count) of the source range that output index k averages, map = nearest source index -----
// mean of `cnt` bytes rounded half up, in integers
__device__ __forceinline__ uint32_t box_mean(uint32_t sum, int cnt) { return (2u * sum + (uint32_t)cnt) / (2u * (uint32_t)cnt); }
// pass 1 (horizontal box, rounded to u8): x [N,H,W,3] -> small [N,H,sw,3]
__global__ __launch_bounds__(256) void corrupt_pixelate_rows_kernel(const uint8_t* __restrict__ x, const int* __restrict__ hbox, uint8_t* __restrict__ small,
                                                                    long long total, int W, int sw) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const int xc = (int)(i % (3 * sw)), xx = xc / 3, ch = xc - 3 * xx;
  const long long row = i / (3 * sw);              // n * H + y
  const int lo = clampi(hbox[2 * xx], 0, W - 1), hi = clampi(hbox[2 * xx] + hbox[2 * xx + 1], lo + 1, W);
  uint32_t sum = 0;
  for (int k = lo; k < hi; ++k) sum += x[(row * W + k) * 3 + ch];
  small[i] = (uint8_t)box_mean(sum, hi - lo);
}
// pass 2 (vertical box, rounded to u8, and the nearest-neighbour enlargement): every output element gathers its own small pixel
__global__ __launch_bounds__(256) void corrupt_pixelate_apply_kernel(const uint8_t* __restrict__ small, const int* __restrict__ vbox,
                                                                     const int* __restrict__ ymap, const int* __restrict__ xmap, void* out, long long total,
                                                                     int H, int W, int sh, int sw, int out_kind) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const int xc = (int)(i % (3 * W)), y = (int)((i / (3 * W)) % H), px = xc / 3, ch = xc - 3 * px;
  const long long n = i / ((long long)3 * W * H);
  const int yy = clampi(ymap[y], 0, sh - 1), xx = clampi(xmap[px], 0, sw - 1);
  const int lo = clampi(vbox[2 * yy], 0, H - 1), hi = clampi(vbox[2 * yy] + vbox[2 * yy + 1], lo + 1, H);
  uint32_t sum = 0;
  for (int k = lo; k < hi; ++k) sum += small[((n * H + k) * sw + xx) * 3 + ch];
  put(out, i, (float)box_mean(sum, hi - lo), out_kind);
}

// ---- fog: a diamond-square map of M x M cells per image (wrap-around neighbours), its minimum / maximum, and the blend ------------
// the random term of cell (y, x): wibble * (wibble * (2u - 1)), u = the uniform of element y * M + x of draw 21 (2u - 1 is exact)
__device__ __forceinline__ float fog_term(uint32_t k0, uint32_t k1, int cell, float wibble) {
  uint32_t w[4];
  philox4x32_10((uint32_t)cell >> 2, DRAW_FOG, 0u, 0u, k0, k1, w);
  const int k = cell & 3;                          // (selects, not w[k]: a dynamic index would put w in scratch)
  const uint32_t word = k == 0 ? w[0] : k == 1 ? w[1] : k == 2 ? w[2] : w[3];
  return wibble * (wibble * (2.f * word_to_uniform(word) - 1.f));
}
__global__ __launch_bounds__(64) void fog_origin_kernel(float* __restrict__ map, int N, long long cells) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n < N) map[n * cells] = 0.f;
}
// squares: the centre of every step x step square = mean of its four corners + term; G = M / step squares per side
__global__ __launch_bounds__(256) void fog_squares_kernel(float* map, const uint32_t* __restrict__ keys, int N, int M, int step, float wibble) {
  const int G = M / step, half = step >> 1;
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  if (t >= (long long)N * G * G) return;
  const int j = (int)(t % G), i = (int)((t / G) % G), n = (int)(t / ((long long)G * G));
  float* m = map + (long long)n * M * M;
  const int y0 = i * step, y1 = ((i + 1) % G) * step, x0 = j * step, x1 = ((j + 1) % G) * step;
  const float sum = (m[y0 * M + x0] + m[y1 * M + x0]) + (m[y0 * M + x1] + m[y1 * M + x1]);
  const int cell = (y0 + half) * M + x0 + half;
  m[cell] = sum * 0.25f + fog_term(keys[2 * n], keys[2 * n + 1], cell, wibble);
}
// diamonds: the midpoints of every square's top and left edges = mean of the two centres and the two corners around them + term
__global__ __launch_bounds__(256) void fog_diamonds_kernel(float* map, const uint32_t* __restrict__ keys, int N, int M, int step, float wibble) {
  const int G = M / step, half = step >> 1;
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  if (t >= (long long)N * G * G) return;
  const int j = (int)(t % G), i = (int)((t / G) % G), n = (int)(t / ((long long)G * G));
  float* m = map + (long long)n * M * M;
  const uint32_t k0 = keys[2 * n], k1 = keys[2 * n + 1];
  const int y0 = i * step, x0 = j * step, yc = y0 + half, xc = x0 + half;
  const int yp = ((i + G - 1) % G) * step + half, xp = ((j + G - 1) % G) * step + half;      // the centres above / to the left
  const int y1 = ((i + 1) % G) * step, x1 = ((j + 1) % G) * step;                          // the corners below / to the right
  const float top = (m[yc * M + xc] + m[yp * M + xc]) + (m[y0 * M + x0] + m[y0 * M + x1]);
  const float lft = (m[yc * M + xc] + m[yc * M + xp]) + (m[y0 * M + x0] + m[y1 * M + x0]);
  m[y0 * M + xc] = top * 0.25f + fog_term(k0, k1, y0 * M + xc, wibble);
  m[yc * M + x0] = lft * 0.25f + fog_term(k0, k1, yc * M + x0, wibble);
}
// minimum / maximum of a map: blocks of CR_SPX cells -> part[n][j][2], then one thread per image -> mm[n][2] (order-free)
__global__ __launch_bounds__(256) void fog_minmax_kernel(const float* __restrict__ map, long long cells, int parts, float* __restrict__ part) {
  __shared__ float red[2][4];
  const int n = blockIdx.x / parts, j = blockIdx.x % parts;
  const float* m = map + (long long)n * cells;
  const long long p0 = (long long)j * CR_SPX, p1 = min(cells, p0 + CR_SPX);
  float lo = m[p0], hi = lo;
  for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
    lo = fminf(lo, m[p]);
    hi = fmaxf(hi, m[p]);
  }
  lo = -wave_max(-lo);
  hi = wave_max(hi);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2LL * blockIdx.x] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    part[2LL * blockIdx.x + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}
__global__ __launch_bounds__(64) void fog_minmax_finalize_kernel(const float* __restrict__ part, int parts, int N, float* __restrict__ mm) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  const float* p = part + 2LL * n * parts;
  float lo = p[0], hi = p[1];
  for (int j = 1; j < parts; ++j) {
    lo = fminf(lo, p[2 * j]);
    hi = fmaxf(hi, p[2 * j + 1]);
  }
  mm[2 * n] = lo;
  mm[2 * n + 1] = hi;
}
// out = (x + c * (map - min) / (max - min)) * (m / (m + c)), m = the image's own maximum, c on the 0-255 scale
__global__ __launch_bounds__(256) void fog_apply_kernel(const uint8_t* __restrict__ x, const float* __restrict__ map, const float* __restrict__ mm,
                                                        const float* __restrict__ stats, void* out, long long total, int H, int W, int M, float c,
                                                        int out_kind) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const int px = (int)((i / 3) % W), y = (int)((i / (3 * W)) % H);
  const long long n = i / ((long long)3 * W * H);
  const float lo = mm[2 * n], hi = mm[2 * n + 1], m = stats[4 * n + 3];
  const float f = (map[(n * M + y) * M + px] - lo) / (hi - lo);
  put(out, i, ((float)x[i] + c * f) * (m / (m + c)), out_kind);
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline unsigned blocks_of(long long threads) { return (unsigned)((threads + 255) / 256); }
inline int parts_of(long long cells) { return (int)((cells + CR_SPX - 1) / CR_SPX); }
inline int map_side(int H, int W) {
  int M = 32;
  while (M < H || M < W) M <<= 1;
  return M;
}
inline size_t stats_bytes(int N, int H, int W) { return (size_t)N * parts_of((long long)H * W) * 4 * sizeof(uint32_t) + (size_t)N * 4 * sizeof(float); }

// argument rules shared by the entry points; "" when legal
const char* bad_image(const void* x, const void* out, int N, int H, int W, int out_kind) {
  if (!x || !out) return "null pointer";
  if (N <= 0) return "N must be positive";
  if (H < 32 || W < 32) return "H and W must be >= 32";
  if ((long long)N * H * W * 3 > INT_MAX - 256) return "N * H * W * 3 must stay below 2^31";
  if (out_kind != 0 && out_kind != 1) return "out_kind must be 0 (u8) or 1 (fp32 before the floor)";
  if (out_kind == 1 && !aligned(out, 4)) return "an fp32 out must be 4-byte aligned";
  if (out == x) return "out must not be x";
  return "";
}
const char* bad_ws(const void* ws, size_t ws_bytes, size_t need) {
  if (!ws) return "null pointer";
  if (!aligned(ws, 8)) return "workspace must be 8-byte aligned";
  if (ws_bytes < need) return "workspace too small";
  return "";
}

// per-image channel means and maximum -> stats fp32 [N][4] at the end of the (part, stats) pair that starts at `ws`
float* launch_stats(const uint8_t* x, int N, int H, int W, void* ws, hipStream_t s) {
  const long long P = (long long)H * W;
  const int parts = parts_of(P);
  uint32_t* part = (uint32_t*)ws;
  float* stats = (float*)(part + (size_t)N * parts * 4);
  hipLaunchKernelGGL(corrupt_stats_kernel, dim3(N * parts), dim3(256), 0, s, x, P, parts, part);
  hipLaunchKernelGGL(corrupt_stats_finalize_kernel, dim3(N), dim3(64), 0, s, part, parts, (double)P, stats);
  return stats;
}

}  // namespace

extern "C" {

int ur_corrupt_noise(const uint8_t* x, const uint32_t* keys, void* out, int N, int H, int W, int mode, float c, const uint32_t* table,
                     int out_kind, ur_stream_t stream) {
  const char* why = bad_image(x, out, N, H, W, out_kind);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(keys, "null pointer");
  UR_REQUIRE(mode >= 0 && mode <= 3, "mode must be 0 (gaussian), 1 (speckle), 2 (impulse) or 3 (shot)");
  UR_REQUIRE(mode != 3 || (table && aligned(table, 4)), "mode 3 needs the 4-byte aligned Poisson table uint32 [256][128]");
  UR_REQUIRE(c > 0.f, "c must be positive");
  const int count = H * W * 3;
  hipStream_t s = (hipStream_t)stream;
  const double elems = (double)N * count;
  ur::ProfScope prof("corrupt_noise", elems * 40.0, elems * (out_kind ? 5.0 : 2.0), s);
  hipLaunchKernelGGL(corrupt_noise_kernel, dim3(blocks_of((long long)N * ((count + 3) >> 2))), dim3(256), 0, s, x, keys, out, N, count, mode, c,
                     table, out_kind);
  return ur::check_launch("ur_corrupt_noise");
}

size_t ur_corrupt_filter_sep_ws_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * H * W * 3 * sizeof(float);
}

int ur_corrupt_filter_sep(const uint8_t* x, const float* taps, int radius, void* out, int N, int H, int W, void* ws, size_t ws_bytes,
                          int out_kind, ur_stream_t stream) {
  const char* why = bad_image(x, out, N, H, W, out_kind);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(taps && aligned(taps, 4), "taps must be a 4-byte aligned fp32 table of 2 * radius + 1 entries");
  UR_REQUIRE(radius >= 0 && radius <= 255, "radius must be in [0, 255]");
  why = bad_ws(ws, ws_bytes, ur_corrupt_filter_sep_ws_bytes(N, H, W));
  UR_REQUIRE(!*why, why);
  const long long total = (long long)N * H * W * 3;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("corrupt_filter_sep", total * 4.0 * (2 * radius + 1), total * 10.0, s);
  // rows first (axis 0), then columns, as scipy.ndimage.gaussian_filter walks the axes
  hipLaunchKernelGGL(corrupt_sep_kernel<uint8_t>, dim3(blocks_of(total)), dim3(256), 0, s, x, taps, radius, 1, ws, total, H, W, 0, 1);
  int rc = ur::check_launch("ur_corrupt_filter_sep (vertical)");
  if (rc) return rc;
  hipLaunchKernelGGL(corrupt_sep_kernel<float>, dim3(blocks_of(total)), dim3(256), 0, s, (const float*)ws, taps, radius, 0, out, total, H, W, 1,
                     out_kind);
  return ur::check_launch("ur_corrupt_filter_sep (horizontal)");
}

int ur_corrupt_taps(const uint8_t* x, const int32_t* taps, int n_taps, int per_image, int border, void* out, int N, int H, int W,
                    int out_kind, ur_stream_t stream) {
  const char* why = bad_image(x, out, N, H, W, out_kind);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(taps && aligned(taps, 4), "taps must be a 4-byte aligned table of (tx, ty, weight bits) triples");
  UR_REQUIRE(n_taps >= 1 && n_taps <= 4096, "n_taps must be in [1, 4096]");
  UR_REQUIRE(per_image == 0 || per_image == 1, "per_image must be 0 (one list) or 1 (one list per image)");
  UR_REQUIRE(border == 0 || border == 1, "border must be 0 (replicate) or 1 (reflect-101)");
  const long long total = (long long)N * H * W * 3;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("corrupt_taps", total * 2.0 * n_taps, total * 2.0, s);
  hipLaunchKernelGGL(corrupt_taps_kernel, dim3(blocks_of(total)), dim3(256), 0, s, x, (const int*)taps, n_taps, per_image, border, out, total, H,
                     W, out_kind);
  return ur::check_launch("ur_corrupt_taps");
}

int ur_corrupt_zoom(const uint8_t* x, const int32_t* layers, int n_layers, void* out, int N, int H, int W, int out_kind, ur_stream_t stream) {
  const char* why = bad_image(x, out, N, H, W, out_kind);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(layers && aligned(layers, 4), "layers must be a 4-byte aligned int32 table [n_layers][6]");
  UR_REQUIRE(n_layers >= 1 && n_layers <= 64, "n_layers must be in [1, 64]");
  const long long total = (long long)N * H * W * 3;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("corrupt_zoom", total * 12.0 * n_layers, total * 2.0, s);
  hipLaunchKernelGGL(corrupt_zoom_kernel, dim3(blocks_of(total)), dim3(256), 0, s, x, (const int*)layers, n_layers, out, total, H, W, out_kind);
  return ur::check_launch("ur_corrupt_zoom");
}

size_t ur_corrupt_color_ws_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return stats_bytes(N, H, W);
}

int ur_corrupt_color(const uint8_t* x, void* out, int N, int H, int W, int mode, float a, float b, void* ws, size_t ws_bytes, int out_kind,
                     ur_stream_t stream) {
  const char* why = bad_image(x, out, N, H, W, out_kind);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (contrast), 1 (brightness) or 2 (saturate)");
  why = bad_ws(ws, ws_bytes, ur_corrupt_color_ws_bytes(N, H, W));
  UR_REQUIRE(!*why, why);
  const long long pixels = (long long)N * H * W;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("corrupt_color", pixels * 40.0, pixels * 9.0, s);
  const float* stats = nullptr;
  if (mode == 0) {
    stats = launch_stats(x, N, H, W, ws, s);
    int rc = ur::check_launch("ur_corrupt_color (statistics)");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(corrupt_color_kernel, dim3(blocks_of(pixels)), dim3(256), 0, s, x, stats, out, pixels, (long long)H * W, mode, a, b, out_kind);
  return ur::check_launch("ur_corrupt_color");
}

size_t ur_corrupt_pixelate_ws_bytes(int N, int H, int small_w) {
  if (N <= 0 || H <= 0 || small_w <= 0) return 0;
  return ((size_t)N * H * small_w * 3 + 7) & ~(size_t)7;
}

int ur_corrupt_pixelate(const uint8_t* x, void* out, int N, int H, int W, int small_h, int small_w, const int32_t* hbox, const int32_t* vbox,
                        const int32_t* ymap, const int32_t* xmap, void* ws, size_t ws_bytes, int out_kind, ur_stream_t stream) {
  const char* why = bad_image(x, out, N, H, W, out_kind);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(hbox && vbox && ymap && xmap, "null pointer");
  UR_REQUIRE(aligned(hbox, 4) && aligned(vbox, 4) && aligned(ymap, 4) && aligned(xmap, 4), "the tables must be 4-byte aligned int32");
  UR_REQUIRE(small_h >= 1 && small_h <= H && small_w >= 1 && small_w <= W, "small_h / small_w must be in [1, H] / [1, W]");
  why = bad_ws(ws, ws_bytes, ur_corrupt_pixelate_ws_bytes(N, H, small_w));
  UR_REQUIRE(!*why, why);
  const long long total = (long long)N * H * W * 3, rows = (long long)N * H * small_w * 3;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("corrupt_pixelate", total * 4.0, total * 3.0, s);
  hipLaunchKernelGGL(corrupt_pixelate_rows_kernel, dim3(blocks_of(rows)), dim3(256), 0, s, x, (const int*)hbox, (uint8_t*)ws, rows, W, small_w);
  int rc = ur::check_launch("ur_corrupt_pixelate (rows)");
  if (rc) return rc;
  hipLaunchKernelGGL(corrupt_pixelate_apply_kernel, dim3(blocks_of(total)), dim3(256), 0, s, (const uint8_t*)ws, (const int*)vbox,
                     (const int*)ymap, (const int*)xmap, out, total, H, W, small_h, small_w, out_kind);
  return ur::check_launch("ur_corrupt_pixelate (apply)");
}

size_t ur_corrupt_fog_ws_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || H > 32768 || W > 32768) return 0;
  const long long cells = (long long)map_side(H, W) * map_side(H, W);
  // the map, its (min, max) parts and result, then the image statistics
  return ((size_t)N * cells + (size_t)N * parts_of(cells) * 2 + (size_t)N * 2) * sizeof(float) + stats_bytes(N, H, W);
}

int ur_corrupt_fog(const uint8_t* x, const uint32_t* keys, void* out, int N, int H, int W, float c, double decay, void* ws, size_t ws_bytes,
                   int out_kind, ur_stream_t stream) {
  const char* why = bad_image(x, out, N, H, W, out_kind);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(keys, "null pointer");
  UR_REQUIRE(c > 0.f && decay > 1.0, "c must be positive and decay > 1");
  UR_REQUIRE(H <= 16384 && W <= 16384, "H and W must be <= 16384 (the map's cell index is an int)");
  why = bad_ws(ws, ws_bytes, ur_corrupt_fog_ws_bytes(N, H, W));
  UR_REQUIRE(!*why, why);
  const int M = map_side(H, W);
  const long long cells = (long long)M * M, total = (long long)N * H * W * 3;
  UR_REQUIRE((long long)N * cells <= INT_MAX - 256, "N * M * M must stay below 2^31 (M = the power of two >= max(H, W))");
  const int parts = parts_of(cells);
  float* map = (float*)ws;
  float* part = map + (size_t)N * cells;
  float* mm = part + (size_t)N * parts * 2;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("corrupt_fog", (double)N * cells * 60.0 + total * 6.0, (double)N * cells * 16.0 + total * 6.0, s);
  hipLaunchKernelGGL(fog_origin_kernel, dim3((N + 63) / 64), dim3(64), 0, s, map, N, cells);
  double wibble = 100.0;
  for (int step = M; step >= 2; step >>= 1, wibble /= decay) {
    const long long squares = (long long)N * (M / step) * (M / step);
    hipLaunchKernelGGL(fog_squares_kernel, dim3(blocks_of(squares)), dim3(256), 0, s, map, keys, N, M, step, (float)wibble);
    hipLaunchKernelGGL(fog_diamonds_kernel, dim3(blocks_of(squares)), dim3(256), 0, s, map, keys, N, M, step, (float)wibble);
  }
  int rc = ur::check_launch("ur_corrupt_fog (map)");
  if (rc) return rc;
  hipLaunchKernelGGL(fog_minmax_kernel, dim3(N * parts), dim3(256), 0, s, map, cells, parts, part);
  hipLaunchKernelGGL(fog_minmax_finalize_kernel, dim3((N + 63) / 64), dim3(64), 0, s, part, parts, N, mm);
  const float* stats = launch_stats(x, N, H, W, mm + (size_t)N * 2, s);
  rc = ur::check_launch("ur_corrupt_fog (reductions)");
  if (rc) return rc;
  hipLaunchKernelGGL(fog_apply_kernel, dim3(blocks_of(total)), dim3(256), 0, s, x, map, mm, stats, out, total, H, W, M, c, out_kind);
  return ur::check_launch("ur_corrupt_fog");
}

}  // extern "C"
