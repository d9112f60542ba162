// Glass blur, snow and elastic transform of u8 images for gfx950: the stages that work on float fields between the u8 ends (the
// specification is the ur_distort_* comment in include/unirestore_hip.h; the planner is unirestore_amd/distort.py).
// x u8 [N,H,W,3] contiguous HWC; the per-pixel fields are fp32 planes.  An image's randomness comes from its own key (philox.h):
//   draws 32..37  glass_blur: iteration i takes 32 + 2 i for dy and 33 + 2 i for dx (ur_distort_shuffle: `draw` and `draw + 1`)
//   draw  40      snow: the normal of every pixel of the layer
//   draws 48, 49  elastic_transform: the uniforms of the dy and of the dx field
// (16..21 belong to corrupt.hip, 0 and 1 to the forward's keyed noise.)  Element e = y * W + x of a per-pixel field takes word
// e & 3 of the counter (e >> 2, draw, 0, 0).  fp32 arithmetic; gather- and bandwidth-bound passes, one thread per cell or pixel.
// No allocation, no synchronisation, no atomics, no order that depends on scheduling: the same inputs give the same bits.
#include "common.h"
#include "philox.h"

#include <climits>

namespace {

constexpr uint32_t DRAW_SNOW = 40, DRAW_ELASTIC = 48;
constexpr int MAX_TAPS = 64;                       // ur_distort_snow keeps an image's tap list in LDS

__device__ __forceinline__ void put(void* out, long long i, float v, int out_kind) {
  v = fminf(fmaxf(v, 0.f), 255.f);
  if (out_kind) ((float*)out)[i] = v;
  else ((uint8_t*)out)[i] = (uint8_t)v;            // truncation: floor of a value >= 0
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
// half-sample-symmetric reflection (d c b a | a b c d | d c b a), periodic: any int -> [0, n)
__device__ __forceinline__ int reflect_sym(int i, int n) {
  const int period = 2 * n;
  int p = i % period;
  if (p < 0) p += period;
  return p < n ? p : period - 1 - p;
}
// (selects, not w[k]: a dynamic index would put w in scratch)
__device__ __forceinline__ uint32_t pick(const uint32_t* w, int k) { return k == 0 ? w[0] : k == 1 ? w[1] : k == 2 ? w[2] : w[3]; }
__device__ __forceinline__ uint32_t keyed_word(uint32_t k0, uint32_t k1, uint32_t draw, int e) {
  uint32_t w[4];
  philox4x32_10((uint32_t)e >> 2, draw, 0u, 0u, k0, k1, w);
  return pick(w, e & 3);
}
// the standard normal of element e: Box-Muller on the word pair that holds it (the even word's r cos, the odd word's r sin)
__device__ __forceinline__ float keyed_normal(uint32_t k0, uint32_t k1, uint32_t draw, int e) {
  uint32_t w[4];
  philox4x32_10((uint32_t)e >> 2, draw, 0u, 0u, k0, k1, w);
  const bool second = (e & 2) != 0;
  float even, odd;
  box_muller(second ? w[2] : w[0], second ? w[3] : w[1], &even, &odd);
  return (e & 1) ? odd : even;
}

// ---- glass: one iteration of the local shuffle, one thread per Philox counter = four consecutive pixels of one image -----------
__global__ __launch_bounds__(256) void distort_shuffle_kernel(const uint8_t* __restrict__ x, const uint32_t* __restrict__ keys, uint8_t* __restrict__ out,
                                                              int N, int H, int W, int delta, uint32_t draw) {
  const int P = H * W, nctr = (P + 3) >> 2;
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  if (t >= (long long)N * nctr) return;
  const int n = (int)(t / nctr), q = (int)(t % nctr);
  const uint32_t k0 = keys[2 * n], k1 = keys[2 * n + 1];
  uint32_t wy[4], wx[4];
  philox4x32_10((uint32_t)q, draw, 0u, 0u, k0, k1, wy);
  philox4x32_10((uint32_t)q, draw + 1u, 0u, 0u, k0, k1, wx);
  const uint8_t* img = x + (long long)n * P * 3;
  uint8_t* o = out + (long long)n * P * 3;
  const uint32_t span = 2u * (uint32_t)delta;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = 4 * q + j;
    if (e >= P) break;
    const int y = e / W, px = e - y * W;
    int sy = y, sx = px;
    if (y >= delta && y < H - delta && px >= delta && px < W - delta) {      // interior: the whole pixel at (y + dy, x + dx)
      sy = y + (int)(((unsigned long long)wy[j] * span) >> 32) - delta;
      sx = px + (int)(((unsigned long long)wx[j] * span) >> 32) - delta;
    }
    const long long s = ((long long)sy * W + sx) * 3, d = (long long)e * 3;
    o[d] = img[s];
    o[d + 1] = img[s + 1];
    o[d + 2] = img[s + 2];
  }
}

// ---- snow, steps 1-3: the keyed normal layer, cropped and bilinearly enlarged, thresholded, clamped to [0, 1] ----------------------
__global__ __launch_bounds__(256) void snow_layer_kernel(const uint32_t* __restrict__ keys, float* __restrict__ field, long long total, int W, int top,
                                                         int left, int ch, int cw, int oh, int ow, float loc, float scale, float thr) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % ow), oy = (int)((i / ow) % oh), n = (int)(i / ((long long)ow * oh));
  const uint32_t k0 = keys[2 * n], k1 = keys[2 * n + 1];
  // position o * (in - 1) / (out - 1) in integers, as ur_corrupt_zoom: the cell exactly, the fraction to one rounding
  const int ny = oy * (ch - 1), iy = ny / (oh - 1), nx = ox * (cw - 1), ix = nx / (ow - 1);
  const float fy = (float)(ny - iy * (oh - 1)) / (float)(oh - 1), fx = (float)(nx - ix * (ow - 1)) / (float)(ow - 1);
  const int y0 = top + iy, y1 = top + min(iy + 1, ch - 1), x0 = left + ix, x1 = left + min(ix + 1, cw - 1);
  const float p00 = loc + scale * keyed_normal(k0, k1, DRAW_SNOW, y0 * W + x0), p01 = loc + scale * keyed_normal(k0, k1, DRAW_SNOW, y0 * W + x1);
  const float p10 = loc + scale * keyed_normal(k0, k1, DRAW_SNOW, y1 * W + x0), p11 = loc + scale * keyed_normal(k0, k1, DRAW_SNOW, y1 * W + x1);
  const float a = p00 + fx * (p01 - p00), b = p10 + fx * (p11 - p10);
  const float v = a + fy * (b - a);
  field[i] = v < thr ? 0.f : fminf(fmaxf(v, 0.f), 1.f);
}

// ---- snow, steps 4-5: L = rint(255 * motion blur of the oh x ow field), kept for the top-left H x W; the image's taps in LDS ------
__global__ __launch_bounds__(256) void snow_blur_kernel(const float* __restrict__ field, const int* __restrict__ taps, int n_taps, uint8_t* __restrict__ L,
                                                        int H, int W, int oh, int ow) {
  __shared__ int tap[MAX_TAPS * 3];
  const int n = blockIdx.y;
  for (int k = threadIdx.x; k < 3 * n_taps; k += 256) tap[k] = taps[(long long)n * 3 * n_taps + k];
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int y = p / W, px = p - y * W;
  const float* f = field + (long long)n * oh * ow;
  float acc = 0.f;
  for (int t = 0; t < n_taps; ++t) {
    const int xx = clampi(px + tap[3 * t], 0, ow - 1), yy = clampi(y + tap[3 * t + 1], 0, oh - 1);      // replicate border of the field
    acc += __int_as_float(tap[3 * t + 2]) * f[(long long)yy * ow + xx];
  }
  L[(long long)n * H * W + p] = (uint8_t)fminf(fmaxf(rintf(255.f * acc), 0.f), 255.f);          // rintf: round half to even
}

// ---- snow, step 6 (a launch of its own: every L is written before its mirror image is read) ---------------------------------------
__global__ __launch_bounds__(256) void snow_apply_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ L, void* out, long long pixels, int P,
                                                         float keep, int out_kind) {
  const long long p = blockIdx.x * 256LL + threadIdx.x;
  if (p >= pixels) return;
  const int e = (int)(p % P);
  const uint8_t* Ln = L + (p - e);
  const float flakes = (float)((int)Ln[e] + (int)Ln[P - 1 - e]);            // (H-1-y)*W + (W-1-x) = P - 1 - e
  const float r = x[3 * p], g = x[3 * p + 1], b = x[3 * p + 2];
  const float grey = 0.299f * r + 0.587f * g + 0.114f * b;
  const float lift = 1.5f * grey + 127.5f, rest = 1.f - keep;
  put(out, 3 * p, (keep * r + rest * fmaxf(r, lift)) + flakes, out_kind);
  put(out, 3 * p + 1, (keep * g + rest * fmaxf(g, lift)) + flakes, out_kind);
  put(out, 3 * p + 2, (keep * b + rest * fmaxf(b, lift)) + flakes, out_kind);
}

// ---- elastic, step 1: the two uniform planes m * (2 u - 1), one thread per Philox counter ----------------------------------------
__global__ __launch_bounds__(256) void field_draw_kernel(const uint32_t* __restrict__ keys, float* __restrict__ f, int N, int P, float m) {
  const int nctr = (P + 3) >> 2;
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  if (t >= 2LL * N * nctr) return;
  const int plane = (int)(t / nctr), q = (int)(t % nctr), n = plane >> 1;
  uint32_t w[4];
  philox4x32_10((uint32_t)q, DRAW_ELASTIC + (uint32_t)(plane & 1), 0u, 0u, keys[2 * n], keys[2 * n + 1], w);
  float* o = f + (long long)plane * P;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (4 * q + j < P) o[4 * q + j] = m * (2.f * word_to_uniform(w[j]) - 1.f);
}
// ---- elastic, step 2: one pass of the separable Gaussian along one axis, reflect border, taps[k + r] on offset k, k ascending ----
__global__ __launch_bounds__(256) void field_sep_kernel(const float* __restrict__ in, const float* __restrict__ taps, int r, int vertical,
                                                        float* __restrict__ out, long long total, int H, int W, float gain) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const int px = (int)(i % W), y = (int)((i / W) % H);
  const float* plane = in + (i - ((long long)y * W + px));
  float acc = 0.f;
  for (int k = -r; k <= r; ++k) {
    const int yy = vertical ? reflect_sym(y + k, H) : y, xx = vertical ? px : reflect_sym(px + k, W);
    acc += taps[k + r] * plane[(long long)yy * W + xx];
  }
  out[i] = acc * gain;
}

// ---- elastic, step 3: the bilinear sample at (y + dy, x + dx), indices reflected half-sample-symmetrically; one thread per pixel --
__global__ __launch_bounds__(256) void warp_kernel(const uint8_t* __restrict__ x, const float* __restrict__ field, void* out, long long pixels, int H,
                                                   int W, int out_kind) {
  const long long p = blockIdx.x * 256LL + threadIdx.x;
  if (p >= pixels) return;
  const int P = H * W, e = (int)(p % P), y = e / W, px = e - y * W;
  const long long n = p / P;
  const float* fld = field + n * 2 * P;
  // (a wild field value, NaN included, still lands on a finite position: every index below stays inside the image)
  const float py = fminf(fmaxf((float)y + fld[e], -1.0e6f), 1.0e6f), qx = fminf(fmaxf((float)px + fld[P + e], -1.0e6f), 1.0e6f);
  const float fy0 = floorf(py), fx0 = floorf(qx), fy = py - fy0, fx = qx - fx0;
  const int y0 = reflect_sym((int)fy0, H), y1 = reflect_sym((int)fy0 + 1, H), x0 = reflect_sym((int)fx0, W), x1 = reflect_sym((int)fx0 + 1, W);
  const uint8_t* img = x + n * 3 * P;
  const uint8_t *q00 = img + ((long long)y0 * W + x0) * 3, *q01 = img + ((long long)y0 * W + x1) * 3;
  const uint8_t *q10 = img + ((long long)y1 * W + x0) * 3, *q11 = img + ((long long)y1 * W + x1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p00 = q00[c], p01 = q01[c], p10 = q10[c], p11 = q11[c];
    const float a = p00 + fx * (p01 - p00), b = p10 + fx * (p11 - p10);      // pixel differences are exact
    put(out, 3 * p + c, a + fy * (b - a), out_kind);
  }
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline unsigned blocks_of(long long threads) { return (unsigned)((threads + 255) / 256); }

// argument rules shared by the entry points; "" when legal
const char* bad_shape(int N, int H, int W) {
  if (N <= 0) return "N must be positive";
  if (H < 32 || W < 32) return "H and W must be >= 32";
  if ((long long)N * H * W * 3 > INT_MAX - 256) return "N * H * W * 3 must stay below 2^31";
  return "";
}
const char* bad_image(const void* x, const void* out, int N, int H, int W, int out_kind) {
  if (!x || !out) return "null pointer";
  const char* why = bad_shape(N, H, W);
  if (*why) return why;
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
const char* bad_enlarged(int N, int H, int W, int oh, int ow) {
  if (oh < H || ow < W) return "oh and ow must be >= H and W";
  if (oh > 32768 || ow > 32768) return "oh and ow must be <= 32768";
  if ((long long)N * oh * ow > INT_MAX - 256) return "N * oh * ow must stay below 2^31";
  return "";
}

}  // namespace

extern "C" {

int ur_distort_shuffle(const uint8_t* x, const uint32_t* keys, uint8_t* out, int N, int H, int W, int delta, uint32_t draw, ur_stream_t stream) {
  const char* why = bad_image(x, out, N, H, W, 0);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(keys, "null pointer");
  UR_REQUIRE(delta >= 1 && delta <= 4, "delta must be in [1, 4]");
  UR_REQUIRE(draw != 0xffffffffu, "draw + 1 must fit in 32 bits");
  const long long pixels = (long long)N * H * W, threads = (long long)N * ((H * W + 3) >> 2);
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("distort_shuffle", pixels * 60.0, pixels * 6.0, s);
  hipLaunchKernelGGL(distort_shuffle_kernel, dim3(blocks_of(threads)), dim3(256), 0, s, x, keys, out, N, H, W, delta, draw);
  return ur::check_launch("ur_distort_shuffle");
}

int ur_distort_snow_layer(const uint32_t* keys, float* field, int N, int H, int W, int top, int left, int ch, int cw, int oh, int ow, float loc,
                          float scale, float thr, ur_stream_t stream) {
  UR_REQUIRE(keys && field, "null pointer");
  const char* why = bad_shape(N, H, W);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(aligned(field, 4), "the field must be 4-byte aligned");
  UR_REQUIRE(top >= 0 && left >= 0 && ch >= 1 && cw >= 1 && top <= H - ch && left <= W - cw, "the crop (top, left, ch, cw) must lie inside H x W");
  why = bad_enlarged(N, H, W, oh, ow);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(scale > 0.f, "scale must be positive");
  const long long total = (long long)N * oh * ow;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("distort_snow_layer", total * 500.0, total * 4.0, s);
  hipLaunchKernelGGL(snow_layer_kernel, dim3(blocks_of(total)), dim3(256), 0, s, keys, field, total, W, top, left, ch, cw, oh, ow, loc, scale, thr);
  return ur::check_launch("ur_distort_snow_layer");
}

size_t ur_distort_snow_ws_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return ((size_t)N * H * W + 7) & ~(size_t)7;
}

int ur_distort_snow(const uint8_t* x, const float* field, const int32_t* taps, int n_taps, void* out, int N, int H, int W, int oh, int ow,
                    float keep, void* ws, size_t ws_bytes, int out_kind, ur_stream_t stream) {
  const char* why = bad_image(x, out, N, H, W, out_kind);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(field && aligned(field, 4), "the field must be a 4-byte aligned fp32 array [N][oh][ow]");
  UR_REQUIRE(taps && aligned(taps, 4), "taps must be a 4-byte aligned table [N][n_taps][3] of (tx, ty, weight bits) triples");
  UR_REQUIRE(n_taps >= 1 && n_taps <= MAX_TAPS, "n_taps must be in [1, 64]");
  why = bad_enlarged(N, H, W, oh, ow);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(keep >= 0.f && keep <= 1.f, "keep must be in [0, 1]");
  UR_REQUIRE(N <= 65535, "N must be <= 65535 (one grid row per image)");
  why = bad_ws(ws, ws_bytes, ur_distort_snow_ws_bytes(N, H, W));
  UR_REQUIRE(!*why, why);
  const long long pixels = (long long)N * H * W;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("distort_snow", pixels * (2.0 * n_taps + 20.0), pixels * (4.0 * n_taps + 8.0), s);
  hipLaunchKernelGGL(snow_blur_kernel, dim3(blocks_of((long long)H * W), N), dim3(256), 0, s, field, (const int*)taps, n_taps, (uint8_t*)ws, H, W, oh, ow);
  int rc = ur::check_launch("ur_distort_snow (blur)");
  if (rc) return rc;
  hipLaunchKernelGGL(snow_apply_kernel, dim3(blocks_of(pixels)), dim3(256), 0, s, x, (const uint8_t*)ws, out, pixels, H * W, keep, out_kind);
  return ur::check_launch("ur_distort_snow (apply)");
}

size_t ur_distort_field_ws_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * 2 * H * W * sizeof(float);
}

int ur_distort_field(const uint32_t* keys, const float* taps_y, int ry, const float* taps_x, int rx, float* field, int N, int H, int W, float m,
                     float alpha, void* ws, size_t ws_bytes, ur_stream_t stream) {
  UR_REQUIRE(keys && field, "null pointer");
  const char* why = bad_shape(N, H, W);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(aligned(field, 4), "the field must be 4-byte aligned");
  UR_REQUIRE(taps_y && taps_x && aligned(taps_y, 4) && aligned(taps_x, 4), "taps must be 4-byte aligned fp32 tables of 2 * radius + 1 entries");
  UR_REQUIRE(ry >= 0 && ry <= 255 && rx >= 0 && rx <= 255, "the radii must be in [0, 255]");
  UR_REQUIRE(m >= 0.f, "m must not be negative");
  why = bad_ws(ws, ws_bytes, ur_distort_field_ws_bytes(N, H, W));
  UR_REQUIRE(!*why, why);
  UR_REQUIRE((const void*)field != (const void*)ws, "the field must not be the workspace");
  const int P = H * W;
  const long long total = 2LL * N * P;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("distort_field", total * (2.0 * (ry + rx + 1) + 30.0), total * 20.0, s);
  // the draws into `field`, rows (axis 0) into ws, then columns back into `field`, as scipy.ndimage.gaussian_filter walks the axes
  hipLaunchKernelGGL(field_draw_kernel, dim3(blocks_of(2LL * N * ((P + 3) >> 2))), dim3(256), 0, s, keys, field, N, P, m);
  int rc = ur::check_launch("ur_distort_field (draw)");
  if (rc) return rc;
  hipLaunchKernelGGL(field_sep_kernel, dim3(blocks_of(total)), dim3(256), 0, s, (const float*)field, taps_y, ry, 1, (float*)ws, total, H, W, 1.f);
  rc = ur::check_launch("ur_distort_field (vertical)");
  if (rc) return rc;
  hipLaunchKernelGGL(field_sep_kernel, dim3(blocks_of(total)), dim3(256), 0, s, (const float*)ws, taps_x, rx, 0, field, total, H, W, alpha);
  return ur::check_launch("ur_distort_field (horizontal)");
}

int ur_distort_warp(const uint8_t* x, const float* field, void* out, int N, int H, int W, int out_kind, ur_stream_t stream) {
  const char* why = bad_image(x, out, N, H, W, out_kind);
  UR_REQUIRE(!*why, why);
  UR_REQUIRE(field && aligned(field, 4), "the field must be a 4-byte aligned fp32 array [N][2][H][W]");
  const long long pixels = (long long)N * H * W;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("distort_warp", pixels * 50.0, pixels * (out_kind ? 35.0 : 26.0), s);
  hipLaunchKernelGGL(warp_kernel, dim3(blocks_of(pixels)), dim3(256), 0, s, x, field, out, pixels, H, W, out_kind);
  return ur::check_launch("ur_distort_warp");
}

}  // extern "C"
