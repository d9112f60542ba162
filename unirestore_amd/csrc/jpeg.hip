// Baseline JPEG round trip of u8 images for gfx950: the bytes a JPEG of a given quality decodes to, without the entropy coder (the
// specification is the ur_jpeg_roundtrip comment in include/unirestore_hip.h).  x u8 [N,H,W,3] contiguous HWC -> out of the same
// shape.  int32 arithmetic throughout; three launches over u8 planes in the caller's workspace:
//   1. RGB -> YCbCr, edge padding to whole 8 x 8 blocks and (4:2:0) the 2 x 2 chroma reduction,
//   2. one 8 x 8 block per thread in registers: level shift, forward DCT, quantise, dequantise, inverse DCT, clamp, in place
//      (adjacent threads take adjacent blocks of a block row: each of a wave's eight row reads is one contiguous 512-byte run),
//   3. (4:2:0) fancy chroma upsampling, YCbCr -> RGB.
// No allocation, no synchronisation, no atomics; every workspace byte that is read was written by this call.
#include "common.h"

#include <climits>

namespace {

// libjpeg's "islow" constants: FIX(x) = round(x * 2^13)
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

// one quantisation table by value (kernel argument: the compiler reads it with scalar loads): q in natural order and
// rcp = ceil(2^32 / (8 q)), which turns the quantiser's division into one multiply-high (exactness: the header comment)
struct QuantTable {
  uint32_t rcp[64];
  uint16_t q[64];
};

__device__ __forceinline__ int descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// the forward pass over eight values (jfdctint.c); FIRST: pass 1 (a row), else pass 2 (a column)
template <bool FIRST>
__device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int N = FIRST ? 11 : 15;
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d0 = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);          // (* 4, * 8192: a left shift of a negative int
  d4 = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);          //  is not defined before C++20)
  const int e = (t12 + t13) * F_0_541;
  d2 = descale(e + t13 * F_0_765, N);
  d6 = descale(e - t12 * F_1_847, N);
  const int z5 = (t4 + t6 + t5 + t7) * F_1_175;
  const int z1 = -(t4 + t7) * F_0_899, z2 = -(t5 + t6) * F_2_562, z3 = -(t4 + t6) * F_1_961 + z5, z4 = -(t5 + t7) * F_0_390 + z5;
  d7 = descale(t4 * F_0_298 + z1 + z3, N);
  d5 = descale(t5 * F_2_053 + z2 + z4, N);
  d3 = descale(t6 * F_3_072 + z2 + z3, N);
  d1 = descale(t7 * F_1_501 + z1 + z4, N);
}

// the inverse pass over eight values (jidctint.c); FIRST: pass 1 (a column, D(., 11)), else pass 2 (a row, D(., 18))
template <bool FIRST>
__device__ __forceinline__ void idct8(int& c0, int& c1, int& c2, int& c3, int& c4, int& c5, int& c6, int& c7) {
  constexpr int N = FIRST ? 11 : 18;
  const int e = (c2 + c6) * F_0_541;
  const int e2 = e - c6 * F_1_847, e3 = e + c2 * F_0_765;
  const int e0 = (c0 + c4) * 8192, e1 = (c0 - c4) * 8192;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  const int z5 = (c7 + c3 + c5 + c1) * F_1_175;
  const int z1 = -(c7 + c1) * F_0_899, z2 = -(c5 + c3) * F_2_562, z3 = -(c7 + c3) * F_1_961 + z5, z4 = -(c5 + c1) * F_0_390 + z5;
  const int o0 = c7 * F_0_298 + z1 + z3, o1 = c5 * F_2_053 + z2 + z4, o2 = c3 * F_3_072 + z2 + z3, o3 = c1 * F_1_501 + z1 + z4;
  c0 = descale(t10 + o3, N);
  c7 = descale(t10 - o3, N);
  c1 = descale(t11 + o2, N);
  c6 = descale(t11 - o2, N);
  c2 = descale(t12 + o1, N);
  c5 = descale(t12 - o1, N);
  c3 = descale(t13 + o0, N);
  c4 = descale(t13 - o0, N);
}

__device__ __forceinline__ void to_ycc(const uint8_t* px, int& y, int& cb, int& cr) {
  const int r = px[0], g = px[1], b = px[2];
  y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// ---- 1a. 4:4:4: one thread per pixel of the padded planes [N][Hp][Wp]; a padding pixel copies the nearest pixel of the image -----
__global__ __launch_bounds__(256) void jpeg_planes444_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ yp, uint8_t* __restrict__ cbp,
                                                             uint8_t* __restrict__ crp, long long total, int H, int W, int Hp, int Wp) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const int px = (int)(i % Wp), py = (int)((i / Wp) % Hp);
  const long long n = i / ((long long)Wp * Hp);
  int y, cb, cr;
  to_ycc(x + ((n * H + min(py, H - 1)) * W + min(px, W - 1)) * 3, y, cb, cr);
  yp[i] = (uint8_t)y;
  cbp[i] = (uint8_t)cb;
  crp[i] = (uint8_t)cr;
}

// ---- 1b. 4:2:0: one thread per sample of the padded chroma planes [N][chb][cwb]: its 2 x 2 pixels give four bytes of the Y plane
// [N][Hp][Wp] (those inside it) and one reduced byte of Cb and of Cr.  A chroma row beyond ch copies reduced row ch - 1: it reduces
// the pixels of that row, not copies of the image's last row ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_planes420_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ yp, uint8_t* __restrict__ cbp,
                                                             uint8_t* __restrict__ crp, long long total, int H, int W, int Hp, int Wp, int ch,
                                                             int chb, int cwb) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const int cx = (int)(i % cwb), cy = (int)((i / cwb) % chb);
  const long long n = i / ((long long)cwb * chb);
  const uint8_t* img = x + n * H * W * 3;
  uint8_t* yimg = yp + n * Hp * Wp;
  int sb = 0, sr = 0;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int py = 2 * cy + dy, px = 2 * cx + dx;
      int y, cb, cr;
      to_ycc(img + ((long long)min(py, H - 1) * W + min(px, W - 1)) * 3, y, cb, cr);
      if (py < Hp && px < Wp) yimg[(long long)py * Wp + px] = (uint8_t)y;
      sb += cb;
      sr += cr;
    }
  }
  if (cy >= ch) {                                  // (at most 7 rows per image)
    sb = sr = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        int y, cb, cr;
        to_ycc(img + ((long long)min(2 * (ch - 1) + dy, H - 1) * W + min(2 * cx + dx, W - 1)) * 3, y, cb, cr);
        sb += cb;
        sr += cr;
      }
    }
  }
  const int bias = 1 + (cx & 1);
  cbp[i] = (uint8_t)((sb + bias) >> 2);
  crp[i] = (uint8_t)((sr + bias) >> 2);
}

// ---- 2. one 8 x 8 block per thread, in place in a plane [N][rows][cols] (multiples of 8, rows of 8-byte aligned blocks) ----------
__global__ __launch_bounds__(256) void jpeg_blocks_kernel(uint8_t* plane, long long blocks, int cols, const QuantTable qt) {
  const long long b = blockIdx.x * 256LL + threadIdx.x;
  if (b >= blocks) return;
  const int bw = cols >> 3;
  uint8_t* p = plane + (b / bw) * 8 * cols + (b % bw) * 8;          // (n * rows/8 + by) block rows of 8 * cols bytes each
  int v[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint2 w = *reinterpret_cast<const uint2*>(p + (long long)r * cols);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[8 * r + k] = (int)((w.x >> (8 * k)) & 255u) - 128;
      v[8 * r + 4 + k] = (int)((w.y >> (8 * k)) & 255u) - 128;
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) fdct8<true>(v[8 * r], v[8 * r + 1], v[8 * r + 2], v[8 * r + 3], v[8 * r + 4], v[8 * r + 5], v[8 * r + 6], v[8 * r + 7]);
#pragma unroll
  for (int c = 0; c < 8; ++c) fdct8<false>(v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c]);
#pragma unroll
  for (int k = 0; k < 64; ++k) {                   // sign(c) * ((|c| + 4q) / 8q) * q
    const int q = qt.q[k];
    const int m = (int)__umulhi((uint32_t)(abs(v[k]) + 4 * q), qt.rcp[k]) * q;
    v[k] = v[k] < 0 ? -m : m;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) idct8<true>(v[c], v[8 + c], v[16 + c], v[24 + c], v[32 + c], v[40 + c], v[48 + c], v[56 + c]);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    idct8<false>(v[8 * r], v[8 * r + 1], v[8 * r + 2], v[8 * r + 3], v[8 * r + 4], v[8 * r + 5], v[8 * r + 6], v[8 * r + 7]);
    uint2 w = make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      w.x |= (uint32_t)clamp255(v[8 * r + k] + 128) << (8 * k);
      w.y |= (uint32_t)clamp255(v[8 * r + 4 + k] + 128) << (8 * k);
    }
    *reinterpret_cast<uint2*>(p + (long long)r * cols) = w;
  }
}

// ---- 3. one thread per pixel: Y, the chroma (4:2:0: the fancy-upsampled value of its two rows and two columns), RGB --------------
// chroma planes [N][crows][ccols]; FANCY: the samples inside ch x cw, neighbours clamped to them
template <bool FANCY>
__global__ __launch_bounds__(256) void jpeg_decode_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ cbp,
                                                          const uint8_t* __restrict__ crp, uint8_t* __restrict__ out, long long pixels, int H, int W,
                                                          int Hp, int Wp, int ch, int cw, int crows, int ccols) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= pixels) return;
  const int px = (int)(i % W), py = (int)((i / W) % H);
  const long long n = i / ((long long)W * H);
  const int y = yp[(n * Hp + py) * Wp + px];
  const uint8_t* pb = cbp + n * crows * ccols;
  const uint8_t* pr = crp + n * crows * ccols;
  int cb, cr;
  if (FANCY) {
    const int cy = py >> 1, cx = px >> 1;
    const int ny = (py & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0), nx = (px & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
    const int o00 = cy * ccols + cx, o01 = cy * ccols + nx, o10 = ny * ccols + cx, o11 = ny * ccols + nx, round_ = (px & 1) ? 7 : 8;
    cb = (3 * (3 * pb[o00] + pb[o10]) + (3 * pb[o01] + pb[o11]) + round_) >> 4;
    cr = (3 * (3 * pr[o00] + pr[o10]) + (3 * pr[o01] + pr[o11]) + round_) >> 4;
  } else {
    cb = pb[py * ccols + px];
    cr = pr[py * ccols + px];
  }
  cb -= 128;
  cr -= 128;
  out[3 * i] = (uint8_t)clamp255(y + ((91881 * cr + 32768) >> 16));
  out[3 * i + 1] = (uint8_t)clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  out[3 * i + 2] = (uint8_t)clamp255(y + ((116130 * cb + 32768) >> 16));
}

inline unsigned blocks_of(long long threads) { return (unsigned)((threads + 255) / 256); }
inline int up8(int v) { return (v + 7) & ~7; }

// Annex K of the JPEG standard, natural order
const int LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24,  40,  57,  69,  56,
                      14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64,  81,  104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const int CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

QuantTable quant_table(const int* base, int quality) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  QuantTable t;
  for (int k = 0; k < 64; ++k) {
    const int q = std::min(std::max((base[k] * s + 50) / 100, 1), 255);
    t.q[k] = (uint16_t)q;
    t.rcp[k] = (uint32_t)(((1ull << 32) + 8ull * q - 1) / (8ull * q));
  }
  return t;
}

// the plane sizes of one image: Y rows x cols, chroma rows x cols (4:2:0: ch, cw = the samples inside them)
struct Layout {
  int Hp, Wp, ch, cw, crows, ccols;
};
inline Layout layout_of(int H, int W, int subsampling) {
  Layout l;
  l.Hp = up8(H);
  l.Wp = up8(W);
  l.ch = subsampling ? (H + 1) / 2 : H;
  l.cw = subsampling ? (W + 1) / 2 : W;
  l.crows = up8(l.ch);
  l.ccols = up8(l.cw);
  return l;
}

}  // namespace

extern "C" {

size_t ur_jpeg_roundtrip_ws_bytes(int N, int H, int W, int subsampling) {
  if (N <= 0 || H <= 0 || W <= 0 || (subsampling != 0 && subsampling != 2)) return 0;
  const Layout l = layout_of(H, W, subsampling);
  return (size_t)N * ((size_t)l.Hp * l.Wp + 2 * (size_t)l.crows * l.ccols);        // a multiple of 64
}

int ur_jpeg_roundtrip(const uint8_t* x, uint8_t* out, int N, int H, int W, int quality, int subsampling, void* ws, size_t ws_bytes,
                      ur_stream_t stream) {
  UR_REQUIRE(x && out && ws, "null pointer");
  UR_REQUIRE(N > 0, "N must be positive");
  UR_REQUIRE(H >= 16 && W >= 16, "H and W must be >= 16");
  UR_REQUIRE((long long)N * (H + 7) * (W + 7) * 3 <= INT_MAX - 256, "N * (H + 7) * (W + 7) * 3 must stay below 2^31");
  UR_REQUIRE(quality >= 1 && quality <= 100, "quality must be in [1, 100]");
  UR_REQUIRE(subsampling == 0 || subsampling == 2, "subsampling must be 0 (4:4:4) or 2 (4:2:0)");
  UR_REQUIRE(out != x, "out must not be x");
  UR_REQUIRE(((uintptr_t)ws & 7) == 0, "workspace must be 8-byte aligned");
  UR_REQUIRE(ws_bytes >= ur_jpeg_roundtrip_ws_bytes(N, H, W, subsampling), "workspace too small");
  const Layout l = layout_of(H, W, subsampling);
  const long long ysize = (long long)N * l.Hp * l.Wp, csize = (long long)N * l.crows * l.ccols, pixels = (long long)N * H * W;
  uint8_t* yp = (uint8_t*)ws;
  uint8_t* cbp = yp + ysize;
  uint8_t* crp = cbp + csize;
  const QuantTable ql = quant_table(LUMA, quality), qc = quant_table(CHROMA, quality);
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("jpeg_roundtrip", (double)(ysize + 2 * csize) * 30.0, (double)pixels * 6.0 + (double)(ysize + 2 * csize) * 4.0, s);
  if (subsampling)
    hipLaunchKernelGGL(jpeg_planes420_kernel, dim3(blocks_of(csize)), dim3(256), 0, s, x, yp, cbp, crp, csize, H, W, l.Hp, l.Wp, l.ch, l.crows, l.ccols);
  else
    hipLaunchKernelGGL(jpeg_planes444_kernel, dim3(blocks_of(ysize)), dim3(256), 0, s, x, yp, cbp, crp, ysize, H, W, l.Hp, l.Wp);
  int rc = ur::check_launch("ur_jpeg_roundtrip (planes)");
  if (rc) return rc;
  hipLaunchKernelGGL(jpeg_blocks_kernel, dim3(blocks_of(ysize / 64)), dim3(256), 0, s, yp, ysize / 64, l.Wp, ql);
  hipLaunchKernelGGL(jpeg_blocks_kernel, dim3(blocks_of(2 * csize / 64)), dim3(256), 0, s, cbp, 2 * csize / 64, l.ccols, qc);      // Cb, then Cr
  rc = ur::check_launch("ur_jpeg_roundtrip (blocks)");
  if (rc) return rc;
  if (subsampling)
    hipLaunchKernelGGL(jpeg_decode_kernel<true>, dim3(blocks_of(pixels)), dim3(256), 0, s, yp, cbp, crp, out, pixels, H, W, l.Hp, l.Wp, l.ch, l.cw,
                       l.crows, l.ccols);
  else
    hipLaunchKernelGGL(jpeg_decode_kernel<false>, dim3(blocks_of(pixels)), dim3(256), 0, s, yp, cbp, crp, out, pixels, H, W, l.Hp, l.Wp, l.ch, l.cw,
                       l.crows, l.ccols);
  return ur::check_launch("ur_jpeg_roundtrip");
}

}  // extern "C"
