// VGG scoring of the cls output (torchvision's VGG configurations A, B, D and E, with or without BatchNorm) for gfx950, exact fp32 on
// NHWC maps.  The 3 x 3 convolutions are the convolution of f32_layers.hip; what the network adds is here: a Linear for a handful
// of rows against a very large matrix (classifier.0 is 25088 -> 4096: 411 MB of weights read once per batch), the 2 x 2 / stride 2
// max-pool and AdaptiveAvgPool2d((7, 7)).  No atomics; every sum runs in a fixed order, so the same inputs give the same bits on
// every run, eagerly and under graph replay, and an output row depends on its own input row alone - not on the number of rows, not
// on its place among them.
//
// The Linear, y[M][N] = act(x[M][K] . W^T + bias).  The weights are streamed: grid = (ceil(N / 128), S, ceil(M / 32)) workgroups of
// four waves, workgroup (t, s, r) multiplies rows 32 r .. 32 r + 31 with k in [512 s, 512 s + 512) for columns 128 t .. 128 t + 127,
// wave g of it for columns 128 t + 32 g .. + 31 on v_mfma_f32_32x32x2_f32.  THE SPLIT RULE: S = ceil(K / 512) - a function of K
// alone, as every tile boundary is a function of (K, N) alone; M only adds row tiles.  The weights are packed once on the host
// (ur_vgg_linear_wpack_dims) so that they go from HBM to the MFMA's B operand through nothing but registers:
//   wp as float4 [Npad / 32][Kpad / 8][64]: element j of lane l in (column tile c, k block b) = W[32 c + (l & 31)][8 b + 4 (l >> 5) + j],
//   zero where the column is >= N or k >= K; Kpad = K rounded up to 64, Npad = N rounded up to 32.
// A wave's loads are 1 KB each, contiguous over k: 64 KB per (wave, split).  The x tile is staged through LDS in steps of 64 k
// (two buffers, one barrier per step); rows >= M and k >= K are zeros made in registers, never read.  Within a split the k-ordered
// MFMA chain restarts every 256 products (the convolution's blocked sum), the partial sums go to ws[S][M][N] with plain vector
// stores, and a second launch adds the S partials of an element in ascending s in fp64, adds the bias, rounds to fp32 once and
// applies the ReLU (maximum(v, 0): NaN and +inf stay, -inf becomes 0).  A NaN or an infinity in one row of x reaches that row only.
#include "common.h"

#include <climits>
#include <cmath>

namespace {

// ------------------------------------------------------------------------------------------ the Linear
constexpr int VL_BM = 32;        // rows per workgroup: one MFMA tile
constexpr int VL_WN = 32;        // columns per wave
constexpr int VL_BN = 128;       // columns per workgroup
constexpr int VL_KS = 64;        // k per LDS step
constexpr int VL_KC = 512;       // k per split
constexpr int VL_KB = 8;         // k per float4 pair of the packed weights (two halves of four)
constexpr int VL_STEPS = VL_KC / VL_KS;
constexpr int VL_FLUSH = 256 / VL_KS;      // steps per MFMA chain
constexpr int VL_LDA = VL_BM + 1;          // float4 row stride of the staged x tile: the 16 k groups a row's loader threads write spread over banks
constexpr int VL_MAX_KN = 1 << 24;
constexpr int VL_MAX_M = 1 << 20;

struct LinArgs {
  const float* x;
  const float4* w;
  float* part;
  int M, K, N, nkb, nct, nsteps;      // nkb = Kpad / 8, nct = Npad / 32, nsteps = Kpad / 64
};

// VEC = 4: K % 4 == 0 and x 16-byte aligned - a float4 of a row is inside the row or beyond it; VEC = 1: any K, four bounded loads.
template <int VEC>
__global__ __launch_bounds__(256) void vgg_linear_kernel(LinArgs p) {
  __shared__ float4 As[2][(VL_KS / 4) * VL_LDA];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ct = blockIdx.x * (VL_BN / VL_WN) + wave;      // this wave's 32-column tile
  const bool active = ct < p.nct;                           // (wave-uniform) a wave beyond Npad only helps staging x
  const int s = blockIdx.y, m0 = blockIdx.z * VL_BM;
  const int st0 = s * VL_STEPS, st1 = min(st0 + VL_STEPS, p.nsteps);
  const int half = lane >> 5, col = lane & 31;

  // staging: 32 rows x 16 float4 per step, two per thread; consecutive threads read consecutive 16 bytes of a row
  float4 a[2];
  auto load_a = [&](int st) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = t + 256 * i;
      const int m = m0 + (idx >> 4), k = st * VL_KS + 4 * (idx & 15);
      const float* src = p.x + (long long)m * p.K + k;
      if constexpr (VEC == 4) {
        a[i] = (m < p.M && k < p.K) ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        const bool row = m < p.M;
        a[i].x = (row && k < p.K) ? src[0] : 0.f;
        a[i].y = (row && k + 1 < p.K) ? src[1] : 0.f;
        a[i].z = (row && k + 2 < p.K) ? src[2] : 0.f;
        a[i].w = (row && k + 3 < p.K) ? src[3] : 0.f;
      }
    }
  };
  auto store_a = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = t + 256 * i;
      As[buf][(idx & 15) * VL_LDA + (idx >> 4)] = a[i];
    }
  };
  constexpr int NB = VL_KS / VL_KB;      // weight float4 per lane and step
  float4 b[NB], bn[NB];
  const float4* wsrc = p.w + ((long long)(active ? ct : 0) * p.nkb) * 64 + lane;
  auto load_b = [&](int st, float4* dst) {
#pragma unroll
    for (int q = 0; q < NB; ++q) dst[q] = wsrc[(long long)(st * NB + q) * 64];
  };

  f32x16 acc, sum;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = sum[r] = 0.f;

  load_a(st0);
  if (active) load_b(st0, b);
  store_a(0);
  __syncthreads();
  for (int st = st0; st < st1; ++st) {
    const int buf = (st - st0) & 1;
    const bool more = st + 1 < st1;
    if (more) {
      load_a(st + 1);
      if (active) load_b(st + 1, bn);
    }
    if (active) {
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        const float4 av = As[buf][(2 * q + half) * VL_LDA + col];      // row `col`, k = 8 q + 4 half .. + 3 of this step
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b[q].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b[q].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b[q].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b[q].w, acc, 0, 0, 0);
      }
      if (((st - st0) & (VL_FLUSH - 1)) == VL_FLUSH - 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sum[r] += acc[r];
          acc[r] = 0.f;
        }
      }
    }
    if (more) store_a(buf ^ 1);      // last read in step st - 1, which every wave left at the barrier below
    if (more && active) {
#pragma unroll
      for (int q = 0; q < NB; ++q) b[q] = bn[q];
    }
    __syncthreads();
  }

  // C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  const int n = ct * VL_WN + col;
  if (!active || n >= p.N) return;
  float* dst = p.part + (long long)s * p.M * p.N + n;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (m < p.M) dst[(long long)m * p.N] = sum[r] + acc[r];
  }
}

__device__ __forceinline__ float vgg_relu_keep_nan(float v) { return __builtin_elementwise_maximum(v, 0.f); }

// y[i] = act(fp32(sum over s ascending of part[s][i] + bias[i % N])), the sum in fp64
__global__ __launch_bounds__(256) void vgg_linear_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                                float* __restrict__ y, int total, int N, int S, int relu) {
  const int i = blockIdx.x * 256 + threadIdx.x;       // over M*N
  if (i >= total) return;
  double v = 0.0;
  for (int s = 0; s < S; ++s) v += (double)part[(long long)s * total + i];
  const float r = (float)(v + (double)bias[i % N]);
  y[i] = relu ? vgg_relu_keep_nan(r) : r;
}

// ------------------------------------------------------------------------------------------ max-pool 2x2 / 2, floor, no padding
// max(v, t) as torch.max_pool2d folds a window: a NaN tap wins and stays (fmaxf would drop it).
__device__ __forceinline__ float vgg_pool_max(float v, float t) { return (t > v || t != t) ? t : v; }

template <int V>
__global__ __launch_bounds__(256) void vgg_maxpool2_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int H, int W, int C,
                                                           int OH, int OW) {
  const int i = blockIdx.x * 256 + threadIdx.x;       // over N*OH*OW*(C/V)
  if (i >= total) return;
  const int cv = C / V;
  const int c = (i % cv) * V;
  int r = i / cv;
  const int ow = r % OW;
  r /= OW;
  const int oh = r % OH, n = r / OH;
  const float* src = x + (((long long)n * H + 2 * oh) * W + 2 * ow) * C + c;
  float v[V];                              // every tap is inside the map, so every output is a real input value
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = -INFINITY;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const float* tap = src + ((long long)dy * W + dx) * C;
      if constexpr (V == 4) {
        const float4 q = *(const float4*)tap;
        v[0] = vgg_pool_max(v[0], q.x); v[1] = vgg_pool_max(v[1], q.y); v[2] = vgg_pool_max(v[2], q.z); v[3] = vgg_pool_max(v[3], q.w);
      } else {
        v[0] = vgg_pool_max(v[0], *tap);
      }
    }
  float* dst = y + (long long)i * V;
  if constexpr (V == 4) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
  else *dst = v[0];
}

// ------------------------------------------------------------------------------------------ adaptive average pool to 7 x 7
// One thread per output element: rows [floor(i H / 7), ceil((i + 1) H / 7)), the columns likewise, row-major in an fp64 sum,
// divided by the count and rounded to fp32 once.  A window of one value returns its bits.
constexpr int VP_OUT = 7;

__global__ __launch_bounds__(256) void vgg_avgpool7_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int H, int W, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;       // over N*7*7*C
  if (i >= total) return;
  const int c = i % C;
  int r = i / C;
  const int ow = r % VP_OUT;
  r /= VP_OUT;
  const int oh = r % VP_OUT, n = r / VP_OUT;
  const int h0 = (int)((long long)oh * H / VP_OUT), h1 = (int)(((long long)(oh + 1) * H + VP_OUT - 1) / VP_OUT);
  const int w0 = (int)((long long)ow * W / VP_OUT), w1 = (int)(((long long)(ow + 1) * W + VP_OUT - 1) / VP_OUT);
  const float* img = x + (long long)n * H * W * C + c;
  double s = 0.0;
  for (int ih = h0; ih < h1; ++ih)
    for (int iw = w0; iw < w1; ++iw) s += (double)img[((long long)ih * W + iw) * C];
  y[i] = (float)(s / (double)((h1 - h0) * (w1 - w0)));
}

bool vgg_overlaps(const void* a, double a_bytes, const void* b, double b_bytes) {
  const double a0 = (double)(uintptr_t)a, b0 = (double)(uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

extern "C" {

int ur_vgg_linear_wpack_dims(int K, int N, int* kpad, int* npad, int* splits) {
  UR_REQUIRE(kpad && npad && splits, "null pointer");
  UR_REQUIRE(K >= 1 && N >= 1 && K <= VL_MAX_KN && N <= VL_MAX_KN, "K and N must be in [1, 2^24]");
  *kpad = (K + VL_KS - 1) / VL_KS * VL_KS;
  *npad = (N + VL_WN - 1) / VL_WN * VL_WN;
  *splits = (K + VL_KC - 1) / VL_KC;
  return 0;
}

long long ur_vgg_linear_ws_bytes(int M, int K, int N) {
  if (M < 1 || K < 1 || N < 1 || M > VL_MAX_M || K > VL_MAX_KN || N > VL_MAX_KN || (long long)M * N >= ur::GRID_1D_LIMIT) return 0;
  return 4ll * ((K + VL_KC - 1) / VL_KC) * M * N;
}

int ur_vgg_linear_f32(const float* x, const float* wp, const float* bias, float* y, void* ws, long long ws_bytes, int M, int K, int N,
                      int relu, ur_stream_t stream) {
  UR_REQUIRE(x && wp && bias && y && ws, "null pointer");
  UR_REQUIRE(M >= 1 && M <= VL_MAX_M, "M must be in [1, 2^20]");
  UR_REQUIRE(K >= 1 && N >= 1 && K <= VL_MAX_KN && N <= VL_MAX_KN, "K and N must be in [1, 2^24]");
  UR_REQUIRE((long long)M * N < ur::GRID_1D_LIMIT, "too many outputs: M*N must be below 2^31 - 256");
  UR_REQUIRE(relu == 0 || relu == 1, "relu must be 0 or 1");
  const long long need = ur_vgg_linear_ws_bytes(M, K, N);
  UR_REQUIRE(ws_bytes >= need, "the workspace is smaller than ur_vgg_linear_ws_bytes(M, K, N)");
  UR_REQUIRE(((uintptr_t)wp & 15) == 0, "wp must be 16-byte aligned");
  UR_REQUIRE((((uintptr_t)x | (uintptr_t)bias | (uintptr_t)y | (uintptr_t)ws) & 3) == 0, "x, bias, y and ws must be 4-byte aligned");
  const double y_bytes = 4.0 * M * N;
  UR_REQUIRE(!vgg_overlaps(y, y_bytes, x, 4.0 * M * K) && !vgg_overlaps(y, y_bytes, ws, (double)need) &&
                 !vgg_overlaps(ws, (double)need, x, 4.0 * M * K),
             "y, ws and x must not overlap");
  LinArgs p;
  p.x = x; p.w = reinterpret_cast<const float4*>(wp); p.part = reinterpret_cast<float*>(ws);
  p.M = M; p.K = K; p.N = N;
  p.nsteps = (K + VL_KS - 1) / VL_KS;
  p.nkb = p.nsteps * (VL_KS / VL_KB);
  p.nct = (N + VL_WN - 1) / VL_WN;
  const int S = (K + VL_KC - 1) / VL_KC;
  const dim3 grid((unsigned)((N + VL_BN - 1) / VL_BN), (unsigned)S, (unsigned)((M + VL_BM - 1) / VL_BM));      // <= (2^17, 2^15, 2^15)
  hipStream_t s = (hipStream_t)stream;
  {
    ur::ProfScope prof("vgg_linear_f32", 2.0 * M * (double)N * K, 4.0 * ((double)grid.z * N * K + (double)M * K + 2.0 * S * M * N), s);
    if (K % 4 == 0 && ((uintptr_t)x & 15) == 0) hipLaunchKernelGGL(vgg_linear_kernel<4>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(vgg_linear_kernel<1>, grid, dim3(256), 0, s, p);
    if (int rc = ur::check_launch("ur_vgg_linear_f32")) return rc;
    const int total = M * N;
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(vgg_linear_reduce_kernel, dim3(blocks), dim3(256), 0, s, p.part, bias, y, total, N, S, relu);
  }
  return ur::check_launch("ur_vgg_linear_f32 (reduce)");
}

int ur_vgg_maxpool2_f32(const float* x, float* y, int N, int H, int W, int C, ur_stream_t stream) {
  UR_REQUIRE(x && y, "null pointer");
  UR_REQUIRE(x != y, "x and y must not be the same buffer");
  UR_REQUIRE(N >= 1 && C >= 1, "N and C must be >= 1");
  UR_REQUIRE(H >= 2 && W >= 2, "H and W must be >= 2");
  UR_REQUIRE((long long)N * H * W * C < ur::GRID_1D_LIMIT, "too many elements: N*H*W*C must be below 2^31 - 256");
  const int OH = H / 2, OW = W / 2;
  hipStream_t s = (hipStream_t)stream;
  if (C % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
    const int total = N * OH * OW * (C / 4);
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(vgg_maxpool2_kernel<4>, dim3(blocks), dim3(256), 0, s, x, y, total, H, W, C, OH, OW);
  } else {
    const int total = N * OH * OW * C;
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(vgg_maxpool2_kernel<1>, dim3(blocks), dim3(256), 0, s, x, y, total, H, W, C, OH, OW);
  }
  return ur::check_launch("ur_vgg_maxpool2_f32");
}

int ur_vgg_avgpool7_f32(const float* x, float* y, int N, int H, int W, int C, ur_stream_t stream) {
  UR_REQUIRE(x && y, "null pointer");
  UR_REQUIRE(x != y, "x and y must not be the same buffer");
  UR_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1, "N, C, H and W must be >= 1");
  UR_REQUIRE((long long)N * H * W * C < ur::GRID_1D_LIMIT && (long long)N * VP_OUT * VP_OUT * C < ur::GRID_1D_LIMIT,
             "too many elements: N*H*W*C and N*49*C must be below 2^31 - 256");
  const int total = N * VP_OUT * VP_OUT * C;
  UR_GRID_1D(blocks, total, 256);
  hipLaunchKernelGGL(vgg_avgpool7_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, total, H, W, C);
  return ur::check_launch("ur_vgg_avgpool7_f32");
}

}  // extern "C"
