// LPIPS (AlexNet, v0.1 linear layers) for gfx950, exact fp32: input scaling, an implicit-GEMM convolution on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: k-ordered fp32 fma chains, bit for bit), 3x3 / stride-2 max-pool, and the per-tap distance
// (unit-normalise over channels, weighted squared difference, fixed-order sums).  NHWC activations, no atomics, no split-K:
// the same inputs give the same bits on every run, eagerly and under graph replay.
#include "common.h"

#include <climits>

namespace {

// ------------------------------------------------------------------------------------------ geometry shared with the planner
constexpr int LP_MIN_HW = 31;       // the smallest input at which the fifth tap still has one pixel
constexpr int LP_TAPS = 5;
constexpr int LP_PIX = 64;          // pixels per block of the layer kernel (16 per wave)

inline int conv_out(int x, int k, int s, int p) { return (x + 2 * p - k) / s + 1; }
inline int pool_out(int x) { return (x - 3) / 2 + 1; }
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

// ------------------------------------------------------------------------------------------ convolution
// y[m][n] = act(sum_k A[m][k] * Wp[k][n] + bias[n] (+ res[m][n])):  m = (image, oh, ow), k = (kh, kw, cin), n = cout.
// Block = 128 (M) x 64 (N) outputs, K in tiles of 16; four waves, wave g owns rows 32g..32g+31 and both 32-column halves (two
// 32x32 accumulators, one A read per two MFMAs).  Both operands sit in LDS K-major ([k][m], [k][n]), which is exactly what the
// 32x32x2 operand map wants: lane l reads A[k0 + (l >> 5)][m = l & 31] - 32 consecutive floats per half wave, no bank conflict.
// The A tile is gathered straight from the NHWC activations (padding and the K tail become zeros in registers: no padded copy),
// W comes from the host's zero-padded [Kpad][Cout_pad] repack, so its loads need no bounds.  Two LDS buffers: the global loads
// of tile t+1 are in flight while tile t is multiplied, one barrier per tile.
constexpr int CV_BM = 128, CV_BN = 64, CV_BK = 16;
constexpr int CV_LDA = CV_BM + 4;      // row stride 132: the 16 k-rows a wave writes at once land in 16 different bank groups
constexpr int CV_LDB = CV_BN;
// One MFMA accumulator is a k-ordered fp32 fma chain, whose rounding error grows with its length (about 3e-7 of sum|a b| at
// K = 3456, conv4).  Every CV_FLUSH K tiles (256 products) the chain is added into a second register set and restarts from
// zero: the error stays at that of a 256-long chain plus K / 256 additions, below what a blocked CPU convolution has.
constexpr int CV_FLUSH = 16;

struct ConvArgs {
  const float* x;
  const float* w;
  const float* bias;
  const float* res;      // [M][Cout] added after the bias, or null (ur_conv2d_f32: always null)
  float* y;
  int H, W, Cin, Cout, KH, KW, stride, pad, OH, OW, K, nk, ldw, relu, M;
};

// VEC = 4: Cin % 4 == 0 and x 16-byte aligned - one 16-byte load covers four consecutive k (channels of one filter tap);
// VEC = 1: any Cin (conv1's 3): one k per thread and tile, eight rows.
template <int VEC>
__global__ __launch_bounds__(256) void conv2d_f32_kernel(ConvArgs p) {
  __shared__ float As[2][CV_BK][CV_LDA];
  __shared__ __attribute__((aligned(16))) float Bs[2][CV_BK][CV_LDB];
  constexpr int KG = CV_BK / VEC;        // k groups per tile
  constexpr int RPP = 256 / KG;          // rows one pass of the block covers
  constexpr int NR = CV_BM / RPP;        // rows per thread
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.x * CV_BM, n0 = blockIdx.y * CV_BN;
  const int kg = t % KG, r0 = t / KG;
  const int kb = t >> 4, nb = (t & 15) * 4;

  int ih0[NR], iw0[NR];
  long long base[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int m = m0 + r0 + i * RPP;
    if (m < p.M) {
      const int n = m / (p.OH * p.OW), rem = m - n * (p.OH * p.OW);
      const int oh = rem / p.OW, ow = rem - oh * p.OW;
      ih0[i] = oh * p.stride - p.pad;
      iw0[i] = ow * p.stride - p.pad;
      base[i] = (long long)n * p.H * p.W * p.Cin;
    } else {
      ih0[i] = iw0[i] = -(1 << 30);      // every tap fails the bounds test: the row is all zeros and is never stored
      base[i] = 0;
    }
  }

  float a[NR][VEC];
  float4 b;
  auto load_tile = [&](int kt) {
    const int k = kt * CV_BK + kg * VEC;
    const int tap = k / p.Cin, c = k - tap * p.Cin;
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const bool k_ok = k < p.K;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int ih = ih0[i] + kh, iw = iw0[i] + kw;
      const bool ok = k_ok && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      const float* src = p.x + base[i] + ((long long)ih * p.W + iw) * p.Cin + c;
      if constexpr (VEC == 4) {
        const float4 v = ok ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
        a[i][0] = v.x; a[i][1] = v.y; a[i][2] = v.z; a[i][3] = v.w;
      } else {
        a[i][0] = ok ? *src : 0.f;
      }
    }
    b = *reinterpret_cast<const float4*>(p.w + (long long)(kt * CV_BK + kb) * p.ldw + n0 + nb);
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
      for (int j = 0; j < VEC; ++j) As[buf][kg * VEC + j][r0 + i * RPP] = a[i][j];
    *reinterpret_cast<float4*>(&Bs[buf][kb][nb]) = b;
  };

  f32x16 acc[2], sum[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = sum[j][r] = 0.f;

  load_tile(0);
  store_tile(0);
  __syncthreads();
  const int half = lane >> 5, col = lane & 31;
  for (int kt = 0; kt < p.nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < p.nk) load_tile(kt + 1);
#pragma unroll
    for (int kk = 0; kk < CV_BK / 2; ++kk) {
      const float av = As[buf][2 * kk + half][wave * 32 + col];
      const float b0 = Bs[buf][2 * kk + half][col];
      const float b1 = Bs[buf][2 * kk + half][32 + col];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[1], 0, 0, 0);
    }
    if ((kt & (CV_FLUSH - 1)) == CV_FLUSH - 1) {      // blocked summation: the chain restarts every CV_FLUSH * CV_BK products
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sum[j][r] += acc[j][r];
          acc[j][r] = 0.f;
        }
    }
    if (kt + 1 < p.nk) store_tile(buf ^ 1);      // last read in iteration kt-1, which every wave left at the barrier below
    __syncthreads();
  }

  // C/D map of the 32x32 MFMAs: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + 32 * j + col;
    if (n >= p.Cout) continue;
    const float bv = p.bias[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (m < p.M) {
        float v = (sum[j][r] + acc[j][r]) + bv;
        if (p.res) v += p.res[(long long)m * p.Cout + n];
        p.y[(long long)m * p.Cout + n] = p.relu ? fmaxf(v, 0.f) : v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ max-pool 3x3 / 2, floor, no padding
__global__ __launch_bounds__(256) void maxpool2d_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int H,
                                                            int W, int C, int OH, int OW) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = i % C;
  int r = i / C;
  const int ow = r % OW;
  r /= OW;
  const int oh = r % OH, n = r / OH;
  const float* src = x + (((long long)n * H + 2 * oh) * W + 2 * ow) * C + c;
  float v = src[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) v = fmaxf(v, src[((long long)dy * W + dx) * C]);
  y[i] = v;
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

int ur_conv2d_f32_wpack_dims(int Cin, int Cout, int KH, int KW, int* kpad, int* cout_pad) {
  UR_REQUIRE(kpad && cout_pad, "null pointer");
  UR_REQUIRE(Cin >= 1 && Cout >= 1 && KH >= 1 && KW >= 1, "Cin, Cout, KH and KW must be >= 1");
  UR_REQUIRE((long long)Cin * KH * KW <= (1 << 24) && Cout <= (1 << 24), "filter too large");
  *kpad = (Cin * KH * KW + CV_BK - 1) / CV_BK * CV_BK;
  *cout_pad = (Cout + CV_BN - 1) / CV_BN * CV_BN;
  return 0;
}

int ur_conv2d_f32_res(const float* x, const float* w, const float* bias, const float* res, float* y, int N, int H, int W, int Cin, int Cout,
                      int KH, int KW, int stride, int pad, int relu, ur_stream_t stream) {
  UR_REQUIRE(x && w && bias && y, "null pointer");
  UR_REQUIRE(N >= 1 && H >= 1 && W >= 1, "N, H and W must be >= 1");
  UR_REQUIRE(Cin >= 1 && Cout >= 1 && KH >= 1 && KW >= 1, "Cin, Cout, KH and KW must be >= 1");
  UR_REQUIRE((long long)Cin * KH * KW <= (1 << 24) && Cout <= (1 << 24), "filter too large");
  UR_REQUIRE(stride >= 1 && pad >= 0, "stride must be >= 1 and pad >= 0");
  UR_REQUIRE(H + 2 * pad >= KH && W + 2 * pad >= KW, "the padded map is smaller than the filter");
  UR_REQUIRE(((uintptr_t)w & 15) == 0, "w must be 16-byte aligned");
  UR_REQUIRE(res != y || !res, "res and y must not be the same buffer");
  const int OH = conv_out(H, KH, stride, pad), OW = conv_out(W, KW, stride, pad);
  const long long M = (long long)N * OH * OW;
  UR_REQUIRE(M <= INT_MAX - CV_BM && (long long)N * H * W <= INT_MAX, "too many pixels: N*OH*OW must be below 2^31 - 128 and N*H*W below 2^31");
  ConvArgs p;
  p.x = x; p.w = w; p.bias = bias; p.res = res; p.y = y;
  p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad; p.OH = OH; p.OW = OW;
  p.K = Cin * KH * KW;
  p.nk = (p.K + CV_BK - 1) / CV_BK;
  p.ldw = (Cout + CV_BN - 1) / CV_BN * CV_BN;
  p.relu = relu != 0;
  p.M = (int)M;
  const dim3 grid((unsigned)((M + CV_BM - 1) / CV_BM), (unsigned)(p.ldw / CV_BN));
  UR_REQUIRE(grid.y <= 65535u, "Cout too large");
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("conv2d_f32", 2.0 * (double)M * Cout * p.K, 4.0 * ((double)N * H * W * Cin + (double)M * Cout * (res ? 2 : 1)), s);
  if (Cin % 4 == 0 && ((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL(conv2d_f32_kernel<4>, grid, dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(conv2d_f32_kernel<1>, grid, dim3(256), 0, s, p);
  return ur::check_launch("ur_conv2d_f32");
}

int ur_conv2d_f32(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                  int stride, int pad, int relu, ur_stream_t stream) {
  return ur_conv2d_f32_res(x, w, bias, nullptr, y, N, H, W, Cin, Cout, KH, KW, stride, pad, relu, stream);
}

int ur_maxpool2d_f32(const float* x, float* y, int N, int H, int W, int C, ur_stream_t stream) {
  UR_REQUIRE(x && y, "null pointer");
  UR_REQUIRE(N >= 1 && C >= 1, "N and C must be >= 1");
  UR_REQUIRE(H >= 3 && W >= 3, "H and W must be >= 3");
  const int OH = pool_out(H), OW = pool_out(W);
  UR_REQUIRE((long long)N * H * W * C <= INT_MAX, "too many elements: N*H*W*C must be below 2^31");
  const int total = N * OH * OW * C;                   // <= N*H*W*C / 9 (H, W >= 3): far inside the launch margin
  UR_GRID_1D(blocks, total, 256);
  hipLaunchKernelGGL(maxpool2d_f32_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, total, H, W, C, OH, OW);
  return ur::check_launch("ur_maxpool2d_f32");
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
