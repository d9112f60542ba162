// The fp32 NHWC layers of the scoring networks (LPIPS's AlexNet, the classifier's ResNet, the segmenters' RefineNet-LW and
// DeepLabV3+) for gfx950, exact fp32: an implicit-GEMM convolution on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: k-ordered fp32
// fma chains, bit for bit) with a dilation, bias, residual and ReLU in its epilogue and an output row stride, the three max-pools, the global average pool, the
// table-driven bilinear resize (align_corners=True or half-pixel, dense or into a channel slice), the broadcast of a pooled vector
// and a + b.  No atomics, no split-K; every sum runs in a fixed order, so the same inputs give the
// same bits on every run, eagerly and under graph replay, and an image's results do not depend on its place in the batch.
// What belongs to one metric alone (its preprocess, its distance or counts) is in lpips.hip, classify.hip and segment.hip.
//
// Non-finite inputs.  Every kernel here treats NaN, +inf and -inf as torch's operator of the same name does, so a non-finite pixel
// of a scored image reaches the score instead of being erased on the way: each output element is finite, +inf, -inf or NaN exactly
// where the fp64 restatement of the layer is (tests/nonfinite_cases.py; NaN payload bits are not part of the contract), the finite
// ones keep their bounds, and an image that holds no non-finite value gives the bits it gives in a clean batch - the "does not
// depend on its place in the batch" promise with a poisoned neighbour.  In particular the convolution's ReLU is maximum(v, 0)
// (NaN stays NaN, as torch.relu; fmaxf(NaN, 0) would be 0), the blocked sum carries a NaN or an infinity from
// every K tile, a pixel no filter tap reads (padding, stride, dilation) does not reach any output, and the max-pools take a NaN
// in any tap of a window as the window's maximum (torch.max_pool2d; fmaxf would drop it); a window of -inf gives -inf.
#include "common.h"
#include "f32_layers.h"

#include <climits>
#include <cmath>

namespace {

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
  float* y;              // row m starts at y + m * ldy: ldy > Cout writes a channel slice of a wider NHWC buffer
  int H, W, Cin, Cout, KH, KW, stride, pad, dil, OH, OW, K, nk, ldw, ldy, relu, M;
};

// VEC = 4: Cin % 4 == 0 and x 16-byte aligned - one 16-byte load covers four consecutive k (channels of one filter tap);
// VEC = 1: any Cin (conv1's 3): one k per thread and tile, eight rows.
// DIL: the taps are p.dil apart; false (dil = 1) keeps the two multiplies per tile out of the undilated networks' gather, which
// measured 1.4 % on the classifier and the RefineNet-LW segmenter with the multiply in it.
// ReLU that keeps NaN, as torch.relu: IEEE 754-2019 maximum(v, 0), one v_maximum3_f32 on gfx950 - where fmaxf (maxNum) returns
// the other operand for a NaN.  v < 0 ? 0 : v says the same in a compare and a select, which measured 0.7 - 1.0 % on every
// network's convolutions (profiles/nonfinite_timing.txt).  A -0.0 comes out as +0.0.
__device__ __forceinline__ float relu_keep_nan(float v) { return __builtin_elementwise_maximum(v, 0.f); }

template <int VEC, bool DIL>
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
      const int ih = ih0[i] + (DIL ? kh * p.dil : kh), iw = iw0[i] + (DIL ? kw * p.dil : kw);
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
        p.y[(long long)m * p.ldy + n] = p.relu ? relu_keep_nan(v) : v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ the max-pools' fold
// max(v, t) as torch.max_pool2d folds a window: a NaN tap wins and stays (fmaxf would drop it).
__device__ __forceinline__ float pool_max(float v, float t) { return (t > v || t != t) ? t : v; }

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
  float v = -INFINITY;                     // every tap is inside the map, so every output is a real input value
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) v = pool_max(v, src[((long long)dy * W + dx) * C]);
  y[i] = v;
}

// ------------------------------------------------------------------------------------------ max-pool 3x3 / 2, padding 1 (= -inf)
__global__ __launch_bounds__(256) void maxpool2d_pad_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int H,
                                                                int W, int C, int OH, int OW) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = i % C;
  int r = i / C;
  const int ow = r % OW;
  r /= OW;
  const int oh = r % OH, n = r / OH;
  float v = -INFINITY;                     // the centre tap is always inside the map, so every output is a real input value
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int ih = 2 * oh - 1 + dy, iw = 2 * ow - 1 + dx;
      if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) v = pool_max(v, x[(((long long)n * H + ih) * W + iw) * C + c]);
    }
  y[i] = v;
}

// ------------------------------------------------------------------------------------------ max-pool 5x5 / 1, padding 2 (= -inf)
template <int V>
__global__ __launch_bounds__(256) void maxpool5_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int H, int W, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;       // over N*H*W*(C/V)
  if (i >= total) return;
  const int cv = C / V;
  const int c = (i % cv) * V;
  int r = i / cv;
  const int ow = r % W;
  r /= W;
  const int oh = r % H, n = r / H;
  float v[V];                              // the centre tap is always inside the map, so every output is a real input value
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = -INFINITY;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int ih = oh + dy, iw = ow + dx;
      if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) {
        const float* src = x + (((long long)n * H + ih) * W + iw) * C + c;
        if constexpr (V == 4) {
          const float4 t = *(const float4*)src;
          v[0] = pool_max(v[0], t.x); v[1] = pool_max(v[1], t.y); v[2] = pool_max(v[2], t.z); v[3] = pool_max(v[3], t.w);
        } else {
          v[0] = pool_max(v[0], *src);
        }
      }
    }
  float* dst = y + (long long)i * V;
  if constexpr (V == 4) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
  else *dst = v[0];
}

// ------------------------------------------------------------------------------------------ global average pool
// x [N][P][C] -> y [N][C]: one thread per (image, channel), the P pixels in ascending order in an fp64 sum, rounded to fp32 once.
__global__ __launch_bounds__(256) void avgpool_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int P, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int n = i / C, c = i - n * C;
  const float* src = x + (long long)n * P * C + c;
  double s = 0.0;
  for (int p = 0; p < P; ++p) s += (double)src[(long long)p * C];
  y[i] = (float)(s / (double)P);
}

// ------------------------------------------------------------------------------------------ broadcast of a pooled vector
// v [N][C] -> y[(n * P + p) * ldy + c] for every pixel p: the bilinear resize of a 1 x 1 map, which is the value itself.
__global__ __launch_bounds__(256) void dlv3_broadcast_kernel(const float* __restrict__ v, float* __restrict__ y, int total, int P, int C,
                                                             int ldy) {
  const int i = blockIdx.x * 256 + threadIdx.x;       // over N*P*C
  if (i >= total) return;
  const int c = i % C;
  const int r = i / C;                                // = n * P + p
  const int n = r / P;
  y[(long long)r * ldy + c] = v[n * C + c];
}

// ------------------------------------------------------------------------------------------ bilinear resize by axis tables
// x [N][h][w][C] -> y[((n * H + oy) * W + ox) * ldy + c], with whatever tables it is given (align_corners=True or half-pixel).
// ldy == C is the dense [N][H][W][C]; ldy > C writes a channel slice of a wider NHWC buffer, so DeepLabV3+'s ASPP features land in
// channels 48..303 of the classifier's input with no concat copy.  V channels per thread (float4 when C, ldy % 4 == 0 and both
// pointers are 16-byte aligned).
template <int V>
__global__ __launch_bounds__(256) void upsample_bilinear_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int h, int w,
                                                                int C, int H, int W, int ldy, const int* __restrict__ iy,
                                                                const float* __restrict__ wy, const int* __restrict__ ix,
                                                                const float* __restrict__ wx) {
  const int i = blockIdx.x * 256 + threadIdx.x;       // over N*H*W*(C/V)
  if (i >= total) return;
  const int cv = C / V;
  const int c = (i % cv) * V;
  int r = i / cv;                                     // = (n * H + oy) * W + ox
  const int pix = r;
  const int ox = r % W;
  r /= W;
  const int oy = r % H, n = r / H;
  const int y0 = min(max(iy[oy], 0), h - 1), y1 = min(y0 + 1, h - 1);
  const int x0 = min(max(ix[ox], 0), w - 1), x1 = min(x0 + 1, w - 1);
  const float h0 = wy[2ll * oy], h1 = wy[2ll * oy + 1], w0 = wx[2ll * ox], w1 = wx[2ll * ox + 1];      // (an axis may have 2^30 outputs or more)
  const float* img = x + (long long)n * h * w * C + c;
  const float* p00 = img + ((long long)y0 * w + x0) * C;
  const float* p01 = img + ((long long)y0 * w + x1) * C;
  const float* p10 = img + ((long long)y1 * w + x0) * C;
  const float* p11 = img + ((long long)y1 * w + x1) * C;
  float* dst = y + (long long)pix * ldy + c;
  if constexpr (V == 4) {
    const float4 a = *(const float4*)p00, b = *(const float4*)p01, cc = *(const float4*)p10, d = *(const float4*)p11;
    float4 o;
    o.x = bilerp(a.x, b.x, cc.x, d.x, w0, w1, h0, h1);
    o.y = bilerp(a.y, b.y, cc.y, d.y, w0, w1, h0, h1);
    o.z = bilerp(a.z, b.z, cc.z, d.z, w0, w1, h0, h1);
    o.w = bilerp(a.w, b.w, cc.w, d.w, w0, w1, h0, h1);
    *(float4*)dst = o;
  } else {
    *dst = bilerp(*p00, *p01, *p10, *p11, w0, w1, h0, h1);
  }
}

// ------------------------------------------------------------------------------------------ a + b
// The chained residual pooling's `x = top + x` where `top` itself feeds the next pool (its last stage rides the convolution's
// residual input instead).  V floats per thread.
template <int V>
__global__ __launch_bounds__(256) void add_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;       // over n / V
  if (i >= total) return;
  if constexpr (V == 4) {
    const float4 p = ((const float4*)a)[i], q = ((const float4*)b)[i];
    ((float4*)y)[i] = make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w);
  } else {
    y[i] = a[i] + b[i];
  }
}

// ------------------------------------------------------------------------------------------ the convolution's one launcher
// `who` names the export in a refusal, `launch_name` in a launch error.  dil = 1 and ldy = Cout is the dense convolution.
#define CV_REQUIRE(cond, msg)                                                      \
  do {                                                                             \
    if (!(cond)) return ur::fail(UR_E_INVALID, std::string(who) + ": " + (msg));  \
  } while (0)

int conv2d_f32_launch(const char* who, const char* launch_name, const float* x, const float* w, const float* bias, const float* res, float* y,
                      int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, int ldy, int relu,
                      ur_stream_t stream) {
  CV_REQUIRE(x && w && bias && y, "null pointer");
  CV_REQUIRE(N >= 1 && H >= 1 && W >= 1, "N, H and W must be >= 1");
  CV_REQUIRE(Cin >= 1 && Cout >= 1 && KH >= 1 && KW >= 1, "Cin, Cout, KH and KW must be >= 1");
  CV_REQUIRE((long long)Cin * KH * KW <= (1 << 24) && Cout <= (1 << 24), "filter too large");
  CV_REQUIRE(stride >= 1 && pad >= 0, "stride must be >= 1 and pad >= 0");
  CV_REQUIRE(dil >= 1 && ldy >= Cout, "dil must be >= 1 and ldy >= Cout");
  const long long PH = (long long)H + 2ll * pad, PW = (long long)W + 2ll * pad;            // the padded map
  const long long EH = (long long)dil * (KH - 1) + 1, EW = (long long)dil * (KW - 1) + 1;  // the dilated filter's extent
  CV_REQUIRE(PH <= INT_MAX && PW <= INT_MAX && EH <= INT_MAX && EW <= INT_MAX,
             "H + 2 pad, W + 2 pad, dil * (KH - 1) + 1 and dil * (KW - 1) + 1 must fit an int");
  CV_REQUIRE(PH >= EH && PW >= EW, "the padded map is smaller than the filter");
  CV_REQUIRE(((uintptr_t)w & 15) == 0, "w must be 16-byte aligned");
  CV_REQUIRE(res != y || !res, "res and y must not be the same buffer");
  const int OH = conv_out(H, (int)EH, stride, pad), OW = conv_out(W, (int)EW, stride, pad);
  const long long M = (long long)N * OH * OW;
  CV_REQUIRE(M <= INT_MAX - CV_BM && (long long)N * H * W <= INT_MAX, "too many pixels: N*OH*OW must be below 2^31 - 128 and N*H*W below 2^31");
  ConvArgs p;
  p.x = x; p.w = w; p.bias = bias; p.res = res; p.y = y;
  p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad; p.dil = dil; p.OH = OH; p.OW = OW;
  p.K = Cin * KH * KW;
  p.nk = (p.K + CV_BK - 1) / CV_BK;
  p.ldw = (Cout + CV_BN - 1) / CV_BN * CV_BN;
  p.ldy = ldy;
  p.relu = relu != 0;
  p.M = (int)M;
  const dim3 grid((unsigned)((M + CV_BM - 1) / CV_BM), (unsigned)(p.ldw / CV_BN));
  CV_REQUIRE(grid.y <= 65535u, "Cout too large");
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("conv2d_f32", 2.0 * (double)M * Cout * p.K, 4.0 * ((double)N * H * W * Cin + (double)M * Cout * (res ? 2 : 1)), s);
  const bool vec = Cin % 4 == 0 && ((uintptr_t)x & 15) == 0;
  if (vec && dil == 1) hipLaunchKernelGGL((conv2d_f32_kernel<4, false>), grid, dim3(256), 0, s, p);
  else if (vec) hipLaunchKernelGGL((conv2d_f32_kernel<4, true>), grid, dim3(256), 0, s, p);
  else if (dil == 1) hipLaunchKernelGGL((conv2d_f32_kernel<1, false>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((conv2d_f32_kernel<1, true>), grid, dim3(256), 0, s, p);
  return ur::check_launch(launch_name);
}

// ------------------------------------------------------------------------------------------ the table-driven resize's one launcher
// ldy = C is the dense resize.
int upsample_bilinear_launch(const char* who, const float* x, float* y, int N, int h, int w, int C, int H, int W, int ldy, const int* idx_h,
                             const float* wt_h, const int* idx_w, const float* wt_w, ur_stream_t stream) {
  CV_REQUIRE(x && y && idx_h && wt_h && idx_w && wt_w, "null pointer");
  CV_REQUIRE(x != y, "x and y must not be the same buffer");
  CV_REQUIRE(N >= 1 && C >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "N, C, h, w, H and W must be >= 1");
  CV_REQUIRE(ldy >= C, "ldy must be >= C");
  CV_REQUIRE((long long)N * h * w * C < ur::GRID_1D_LIMIT && (long long)N * H * W * C < ur::GRID_1D_LIMIT,
             "too many elements: N*h*w*C and N*H*W*C must be below 2^31 - 256");
  const bool vec = C % 4 == 0 && ldy % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  const int total = N * H * W * (vec ? C / 4 : C);
  unsigned blocks = 0;
  if (int rc = ur::grid_1d(who, total, 256, &blocks)) return rc;
  const auto kernel = vec ? upsample_bilinear_kernel<4> : upsample_bilinear_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, total, h, w, C, H, W, ldy, idx_h, wt_h, idx_w, wt_w);
  return ur::check_launch(who);
}
#undef CV_REQUIRE

}  // namespace

extern "C" {

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
  return conv2d_f32_launch("ur_conv2d_f32_res", "ur_conv2d_f32", x, w, bias, res, y, N, H, W, Cin, Cout, KH, KW, stride, pad, 1, Cout, relu, stream);
}

int ur_dlv3_conv2d_f32(const float* x, const float* w, const float* bias, const float* res, float* y, int N, int H, int W, int Cin, int Cout,
                       int KH, int KW, int stride, int pad, int dil, int ldy, int relu, ur_stream_t stream) {
  return conv2d_f32_launch("ur_dlv3_conv2d_f32", "ur_dlv3_conv2d_f32", x, w, bias, res, y, N, H, W, Cin, Cout, KH, KW, stride, pad, dil, ldy, relu,
                           stream);
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

int ur_maxpool2d_pad_f32(const float* x, float* y, int N, int H, int W, int C, ur_stream_t stream) {
  UR_REQUIRE(x && y, "null pointer");
  UR_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1, "N, C, H and W must be >= 1");
  UR_REQUIRE((long long)N * H * W * C < ur::GRID_1D_LIMIT, "too many elements: N*H*W*C must be below 2^31 - 256");
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const int total = N * OH * OW * C;                   // = N*H*W*C on a 1 x 1 map
  UR_GRID_1D(blocks, total, 256);
  hipLaunchKernelGGL(maxpool2d_pad_f32_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, total, H, W, C, OH, OW);
  return ur::check_launch("ur_maxpool2d_pad_f32");
}

int ur_maxpool5_f32(const float* x, float* y, int N, int H, int W, int C, ur_stream_t stream) {
  UR_REQUIRE(x && y, "null pointer");
  UR_REQUIRE(x != y, "x and y must not be the same buffer");
  UR_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1, "N, C, H and W must be >= 1");
  UR_REQUIRE((long long)N * H * W * C < ur::GRID_1D_LIMIT, "too many elements: N*H*W*C must be below 2^31 - 256");
  hipStream_t s = (hipStream_t)stream;
  if (C % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
    const int total = N * H * W * (C / 4);
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(maxpool5_f32_kernel<4>, dim3(blocks), dim3(256), 0, s, x, y, total, H, W, C);
  } else {
    const int total = N * H * W * C;
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(maxpool5_f32_kernel<1>, dim3(blocks), dim3(256), 0, s, x, y, total, H, W, C);
  }
  return ur::check_launch("ur_maxpool5_f32");
}

int ur_avgpool_f32(const float* x, float* y, int N, int P, int C, ur_stream_t stream) {
  UR_REQUIRE(x && y, "null pointer");
  UR_REQUIRE(N >= 1 && P >= 1 && C >= 1, "N, P and C must be >= 1");
  UR_REQUIRE((long long)N * P * C < ur::GRID_1D_LIMIT, "too many elements: N*P*C must be below 2^31 - 256");
  const int total = N * C;                             // = N*P*C for P = 1
  UR_GRID_1D(blocks, total, 256);
  hipLaunchKernelGGL(avgpool_f32_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, total, P, C);
  return ur::check_launch("ur_avgpool_f32");
}

int ur_upsample_bilinear_ac_f32(const float* x, float* y, int N, int h, int w, int C, int H, int W, const int* idx_h, const float* wt_h,
                                const int* idx_w, const float* wt_w, ur_stream_t stream) {
  return upsample_bilinear_launch("ur_upsample_bilinear_ac_f32", x, y, N, h, w, C, H, W, C, idx_h, wt_h, idx_w, wt_w, stream);
}

int ur_dlv3_upsample_f32(const float* x, float* y, int N, int h, int w, int C, int H, int W, int ldy, const int* idx_h, const float* wt_h,
                         const int* idx_w, const float* wt_w, ur_stream_t stream) {
  return upsample_bilinear_launch("ur_dlv3_upsample_f32", x, y, N, h, w, C, H, W, ldy, idx_h, wt_h, idx_w, wt_w, stream);
}

int ur_dlv3_broadcast_f32(const float* v, float* y, int N, int P, int C, int ldy, ur_stream_t stream) {
  UR_REQUIRE(v && y, "null pointer");
  UR_REQUIRE(v != y, "v and y must not be the same buffer");
  UR_REQUIRE(N >= 1 && P >= 1 && C >= 1, "N, P and C must be >= 1");
  UR_REQUIRE(ldy >= C, "ldy must be >= C");
  UR_REQUIRE((long long)N * P * C < ur::GRID_1D_LIMIT, "too many elements: N*P*C must be below 2^31 - 256");
  const int total = N * P * C;
  UR_GRID_1D(blocks, total, 256);
  hipLaunchKernelGGL(dlv3_broadcast_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, v, y, total, P, C, ldy);
  return ur::check_launch("ur_dlv3_broadcast_f32");
}

int ur_add_f32(const float* a, const float* b, float* y, long long n, ur_stream_t stream) {
  UR_REQUIRE(a && b && y, "null pointer");
  UR_REQUIRE(n >= 1 && n < ur::GRID_1D_LIMIT, "n must be in [1, 2^31 - 256): inside [1, 2^31) with a whole last workgroup inside an int");
  UR_REQUIRE(y != a && y != b, "y must be neither a nor b");
  hipStream_t s = (hipStream_t)stream;
  if (n % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)y) & 15) == 0) {
    const int total = (int)(n / 4);
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(add_f32_kernel<4>, dim3(blocks), dim3(256), 0, s, a, b, y, total);
  } else {
    const int total = (int)n;
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(add_f32_kernel<1>, dim3(blocks), dim3(256), 0, s, a, b, y, total);
  }
  return ur::check_launch("ur_add_f32");
}

}  // extern "C"
