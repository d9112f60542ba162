// The transformer layers of the ViT scorer (unirestore_amd/vit.py) for gfx950, exact fp32 in and out, token-major ([N][S][D], which
// is NHWC [N][1][S][D]): LayerNorm over the last axis, the exact-erf GELU, the class-token / positional-embedding assembly, and
// multi-head self-attention with both products on the fp32-input MFMA (v_mfma_f32_32x32x2_f32) and an exact softmax.  The Linears
// of the network are the convolution of f32_layers.hip, unchanged.  No atomics, no split sums; every sum runs in a fixed order, so
// the same inputs give the same bits on every run, eagerly and under graph replay, and an image's results do not depend on its
// place in the batch (a LayerNorm row, a GELU element, an attention (image, head) never reads another image).
//
// Limits, checked before any HIP call:
//   ur_layernorm_f32: rows, D >= 1, ldx >= D, rows below 2^31 - 256 (one wave per row, four rows per workgroup); 64-bit offsets.
//   ur_layernorm_res_f32 (y = res + LN(x), the post-norm residual of the Swin-V2 scorer): the same with ldx = D; y is not res.
//   ur_gelu_f32: n in [1, 2^31 - 256).
//   ur_vit_embed_f32: N, P, D >= 1, N * (P + 1) * D below 2^31 - 256.
//   ur_vit_attention_f32: d = 64, D = H * d, 1 <= S <= UR_VIT_S_MAX = 256 (K and V of one head stay in LDS: S rounded up to 32
//     rows of 65 + 64 floats, 129 KiB at 256), N * H <= 2^22, qkv 16-byte aligned.
//
// Non-finite inputs follow the rule of f32_layers.hip: each output is finite, +inf, -inf or NaN exactly where the fp64 restatement
// of the layer is (tests/vit_reference.py), and an image without a non-finite value keeps the bits it has in a clean batch.
//   LayerNorm: a row that holds a NaN or an infinity is all NaN (inf - inf in the centring), as F.layer_norm.
//   GELU: NaN -> NaN, +inf -> +inf, -inf -> NaN (0.5 * -inf * (1 + -1) = -inf * 0), the formula's own result.
//   Attention: a score row that holds a NaN or +inf is all NaN (exp(inf - inf)); a -inf score has weight 0; a NaN in V reaches every
//     query of its (image, head), since 0 * NaN = NaN inside the MFMA.  Keys added to fill the last 32-key tile take no part in the
//     maximum or the sum, and enter P V as 0 * 0.
#include "common.h"

#include <climits>
#include <cmath>

namespace {

// ------------------------------------------------------------------------------------------ LayerNorm
// One wave per row, V floats per lane and step.  The moments are fp64: the mean first, then the variance of the centred values
// (biased, as F.layer_norm) - never E[x^2] - mean^2, which loses every digit of a row with a large mean.  Each lane adds its
// elements in ascending order, the 64 partial sums meet in an xor butterfly (a + b = b + a: every lane ends with the same bits).
// A row of at most 4 * 64 * V floats stays in registers between the passes; a longer one is read again (it sits in the cache).
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int LN_KEEP = 4;      // vectors per lane held in registers

// RES: y = res + LN(x), the post-norm residual of a Swin-V2 block - LN(x) rounded to fp32 once as without RES, then one fp32 addition
// (res is dense [rows][D], not y).
template <int V, bool RES = false>
__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y, int rows, int D,
                                                            double eps, long long ldx, const float* __restrict__ res) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                       // whole waves leave: no barrier follows
  const float* src = x + (long long)row * ldx;
  float* dst = y + (long long)row * D;
  const int nv = D / V;                          // V = 4 only when D % 4 == 0
  const bool keep = nv <= LN_KEEP * 64;
  float held[LN_KEEP][V];
  auto load = [&](int i, float* v) {
    if constexpr (V == 4) {
      const float4 t = *reinterpret_cast<const float4*>(src + 4ll * i);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
      v[0] = src[i];
    }
  };
  double s = 0.0;
  if (keep) {
#pragma unroll
    for (int j = 0; j < LN_KEEP; ++j) {
      const int i = lane + 64 * j;
#pragma unroll
      for (int k = 0; k < V; ++k) held[j][k] = 0.f;
      if (i < nv) {
        load(i, held[j]);
#pragma unroll
        for (int k = 0; k < V; ++k) s += (double)held[j][k];
      }
    }
  } else {
    for (int i = lane; i < nv; i += 64) {
      float v[V];
      load(i, v);
#pragma unroll
      for (int k = 0; k < V; ++k) s += (double)v[k];
    }
  }
  const double mean = wave_sum_f64(s) / (double)D;
  double q = 0.0;
  if (keep) {
#pragma unroll
    for (int j = 0; j < LN_KEEP; ++j)
      if (lane + 64 * j < nv) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const double c = (double)held[j][k] - mean;
          q += c * c;
        }
      }
  } else {
    for (int i = lane; i < nv; i += 64) {
      float v[V];
      load(i, v);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const double c = (double)v[k] - mean;
        q += c * c;
      }
    }
  }
  const double rstd = 1.0 / sqrt(wave_sum_f64(q) / (double)D + eps);
  auto store = [&](int i, const float* v) {
    float o[V];
#pragma unroll
    for (int k = 0; k < V; ++k)
      o[k] = (float)(((double)v[k] - mean) * rstd * (double)gamma[(long long)i * V + k] + (double)beta[(long long)i * V + k]);
    if constexpr (RES) {
      const float* rp = res + (long long)row * D + (long long)i * V;
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = rp[k] + o[k];
    }
    if constexpr (V == 4) *reinterpret_cast<float4*>(dst + 4ll * i) = make_float4(o[0], o[1], o[2], o[3]);
    else dst[i] = o[0];
  };
  if (keep) {
#pragma unroll
    for (int j = 0; j < LN_KEEP; ++j)
      if (lane + 64 * j < nv) store(lane + 64 * j, held[j]);
  } else {
    for (int i = lane; i < nv; i += 64) {
      float v[V];
      load(i, v);
      store(i, v);
    }
  }
}

// ------------------------------------------------------------------------------------------ GELU
// 0.5 x (1 + erf(x / sqrt 2)) with libm's erff (no fast-math intrinsic): erf(+-inf) = +-1, so +inf stays +inf and -inf gives
// -inf * 0 = NaN, as the formula does in fp64.
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

template <int V>
__global__ __launch_bounds__(256) void gelu_f32_kernel(const float* x, float* y, int total) {      // (x may be y: no __restrict__)
  const int i = blockIdx.x * 256 + threadIdx.x;       // over n / V
  if (i >= total) return;
  if constexpr (V == 4) {
    const float4 t = reinterpret_cast<const float4*>(x)[i];
    reinterpret_cast<float4*>(y)[i] = make_float4(gelu_erf(t.x), gelu_erf(t.y), gelu_erf(t.z), gelu_erf(t.w));
  } else {
    y[i] = gelu_erf(x[i]);
  }
}

// ------------------------------------------------------------------------------------------ class token + positional embedding
// y[n][0] = class_token + pos[0]; y[n][1 + p] = patches[n][p] + pos[1 + p]: one addition per element.
template <int V>
__global__ __launch_bounds__(256) void vit_embed_kernel(const float* __restrict__ patches, const float* __restrict__ cls,
                                                        const float* __restrict__ pos, float* __restrict__ y, int total, int P, int D) {
  const int i = blockIdx.x * 256 + threadIdx.x;       // over N * (P + 1) * (D / V)
  if (i >= total) return;
  const int dv = D / V;
  const int c = (i % dv) * V;
  const int r = i / dv;                               // = n * (P + 1) + s
  const int n = r / (P + 1), s = r - n * (P + 1);
  const float* a = s == 0 ? cls + c : patches + ((long long)n * P + (s - 1)) * D + c;
  const float* b = pos + (long long)s * D + c;
  float* dst = y + (long long)r * D + c;
  if constexpr (V == 4) {
    const float4 p = *reinterpret_cast<const float4*>(a), q = *reinterpret_cast<const float4*>(b);
    *reinterpret_cast<float4*>(dst) = make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w);
  } else {
    *dst = *a + *b;
  }
}

// ------------------------------------------------------------------------------------------ attention
// One workgroup per (image, head, group of four 32-query tiles); wave g owns query tile 4 * blockIdx.y + g.  K and V of the head
// sit in LDS, S rounded up to NKT tiles of 32 keys with zeros in the added rows: K rows 65 floats apart (the A operand reads one
// column of 32 rows: 32 different banks), V rows 64 apart (the B operand reads 32 consecutive floats of one row).
//   scores^T tile kt = K_kt Q^T (A = K: lane l gives K[key = l & 31][k = 2 kk + (l >> 5)]; B = Q^T: lane l gives
//     Q[query = l & 31][k] / 8, held in 32 registers; 1 / sqrt(64) is a power of two, so scaling q first is exact).  The C map
//     then leaves lane l with 16 scores per tile of ONE query, l & 31: keys (r & 3) + 8 (r >> 2) + 4 (l >> 5); lane l ^ 32 has the
//     other 16, so a query's whole score row lives in one lane pair - the softmax needs one exchange for the maximum and one for
//     the sum, and nothing online.
//   O = P V (A = P: lane l gives P[query = l & 31][key]: register j of tile kt IS that operand for the key named above - P never
//     leaves its registers; B = V: lane l gives V[that same key][dt * 32 + (l & 31)]).  The keys are thus summed in the fixed
//     order kt, j, half; the C map gives lane l column dt * 32 + (l & 31) of 16 queries: 128-byte rows on the way out.
// Softmax of a row: m = max over the S real keys (fmaxf: a NaN score does not hide the others, it comes back through
// expf(NaN - m)), e = expf(score - m) with libm's expf, sum = lane's 16 NKT values in register order + the partner's, p = e / sum
// with an IEEE division.
constexpr int VA_D = 64, VA_LDK = 65, VA_LDV = 64, VA_S_MAX = UR_VIT_S_MAX;
static_assert(VA_S_MAX == 8 * 32, "the launcher instantiates 1..8 key tiles");

template <int NKT>
__global__ __launch_bounds__(256) void vit_attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, int S, int H) {
  extern __shared__ __attribute__((aligned(16))) float va_lds[];
  float* Ks = va_lds;                                // [NKT * 32][VA_LDK]
  float* Vs = va_lds + NKT * 32 * VA_LDK;            // [NKT * 32][VA_LDV]; NKT * 32 * 65 * 4 bytes is a multiple of 16
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = blockIdx.x / H, h = blockIdx.x - n * H;
  const int D = H * VA_D;
  const long long ld = 3ll * D;
  const float* base = qkv + (long long)n * S * ld + h * VA_D;

  {                                                  // K, V -> LDS: thread t takes 4 floats of row t / 16 + 16 i
    const int c4 = (t & 15) * 4;
#pragma unroll 4
    for (int r = t >> 4; r < NKT * 32; r += 16) {
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (r < S) {
        kv = *reinterpret_cast<const float4*>(base + r * ld + D + c4);
        vv = *reinterpret_cast<const float4*>(base + r * ld + 2 * D + c4);
      }
      float* kd = Ks + r * VA_LDK + c4;
      kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
      *reinterpret_cast<float4*>(Vs + r * VA_LDV + c4) = vv;
    }
  }
  __syncthreads();
  const int q0 = (blockIdx.y * 4 + wave) * 32;
  if (q0 >= S) return;                               // a wave without queries: the only barrier is behind it

  const int col = lane & 31, half = lane >> 5;
  float qr[32];
  {
    const int q = q0 + col;
    const float* qp = base + (long long)q * ld + half;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) qr[kk] = q < S ? qp[2 * kk] * 0.125f : 0.f;
  }
  f32x16 sc[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[kt][r] = 0.f;
#pragma unroll
  for (int kk = 0; kk < 32; ++kk)
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
      sc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[(kt * 32 + col) * VA_LDK + 2 * kk + half], qr[kk], sc[kt], 0, 0, 0);

  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (key < S) m = fmaxf(m, sc[kt][r]);
    }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const float e = key < S ? expf(sc[kt][r] - m) : 0.f;
      sc[kt][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 32, 64);
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      sc[kt][r] = key < S ? sc[kt][r] / sum : 0.f;   // (a NaN sum must not reach the added keys: 0 / NaN)
    }

  f32x16 o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float* vrow = Vs + (kt * 32 + (j & 3) + 8 * (j >> 2) + 4 * half) * VA_LDV + col;
      o[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[kt][j], vrow[0], o[0], 0, 0, 0);
      o[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[kt][j], vrow[32], o[1], 0, 0, 0);
    }

  float* ob = out + (long long)n * S * D + h * VA_D + col;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int q = q0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (q < S) {
      ob[(long long)q * D] = o[0][r];
      ob[(long long)q * D + 32] = o[1][r];
    }
  }
}

template <int NKT>
int vit_attention_launch(const float* qkv, float* out, int N, int S, int H, hipStream_t s) {
  constexpr int lds = NKT * 32 * (VA_LDK + VA_LDV) * 4;
  if constexpr (lds > 64 * 1024) {
    static ur::DeviceOnce attr_once;      // the attribute is per device
    if (auto once_guard = attr_once.first())
      hipFuncSetAttribute(reinterpret_cast<const void*>(&vit_attention_kernel<NKT>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  }
  const dim3 grid((unsigned)(N * H), (unsigned)((S + 127) / 128));
  ur::ProfScope prof("vit_attention_f32", 4.0 * N * H * (double)S * S * VA_D, 16.0 * N * S * H * VA_D, s);
  hipLaunchKernelGGL(vit_attention_kernel<NKT>, grid, dim3(256), lds, s, qkv, out, S, H);
  return ur::check_launch("ur_vit_attention_f32");
}

}  // namespace

extern "C" {

int ur_vit_attention_s_max(void) { return VA_S_MAX; }

int ur_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int rows, int D, double eps, long long ldx,
                     ur_stream_t stream) {
  UR_REQUIRE(x && gamma && beta && y, "null pointer");
  UR_REQUIRE(x != y, "x and y must not be the same buffer");
  UR_REQUIRE(rows >= 1 && D >= 1, "rows and D must be >= 1");
  UR_REQUIRE(ldx >= D, "ldx must be >= D");
  UR_REQUIRE(eps >= 0.0 && eps == eps, "eps must be >= 0");
  UR_REQUIRE((long long)rows < ur::GRID_1D_LIMIT, "too many rows: rows must be below 2^31 - 256");
  UR_GRID_1D(blocks, rows, 4);
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("layernorm_f32", 8.0 * rows * (double)D, 8.0 * rows * (double)D, s);
  const bool vec = D % 4 == 0 && ldx % 4 == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0;
  if (vec) hipLaunchKernelGGL(layernorm_f32_kernel<4>, dim3(blocks), dim3(256), 0, s, x, gamma, beta, y, rows, D, eps, ldx, nullptr);
  else hipLaunchKernelGGL(layernorm_f32_kernel<1>, dim3(blocks), dim3(256), 0, s, x, gamma, beta, y, rows, D, eps, ldx, nullptr);
  return ur::check_launch("ur_layernorm_f32");
}

int ur_layernorm_res_f32(const float* x, const float* res, const float* gamma, const float* beta, float* y, int rows, int D, double eps,
                         ur_stream_t stream) {
  UR_REQUIRE(x && res && gamma && beta && y, "null pointer");
  UR_REQUIRE(x != y && res != y, "y must not be the same buffer as x or res");
  UR_REQUIRE(rows >= 1 && D >= 1, "rows and D must be >= 1");
  UR_REQUIRE(eps >= 0.0 && eps == eps, "eps must be >= 0");
  UR_REQUIRE((long long)rows < ur::GRID_1D_LIMIT, "too many rows: rows must be below 2^31 - 256");
  UR_GRID_1D(blocks, rows, 4);
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("layernorm_res_f32", 9.0 * rows * (double)D, 12.0 * rows * (double)D, s);
  const long long ldx = D;
  const bool vec = D % 4 == 0 && (((uintptr_t)x | (uintptr_t)res | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0;
  if (vec) hipLaunchKernelGGL((layernorm_f32_kernel<4, true>), dim3(blocks), dim3(256), 0, s, x, gamma, beta, y, rows, D, eps, ldx, res);
  else hipLaunchKernelGGL((layernorm_f32_kernel<1, true>), dim3(blocks), dim3(256), 0, s, x, gamma, beta, y, rows, D, eps, ldx, res);
  return ur::check_launch("ur_layernorm_res_f32");
}

int ur_gelu_f32(const float* x, float* y, long long n, ur_stream_t stream) {
  UR_REQUIRE(x && y, "null pointer");
  UR_REQUIRE(n >= 1 && n < ur::GRID_1D_LIMIT, "n must be in [1, 2^31 - 256)");
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("gelu_f32", 20.0 * (double)n, 8.0 * (double)n, s);
  if (n % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
    const int total = (int)(n / 4);
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(gelu_f32_kernel<4>, dim3(blocks), dim3(256), 0, s, x, y, total);
  } else {
    const int total = (int)n;
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(gelu_f32_kernel<1>, dim3(blocks), dim3(256), 0, s, x, y, total);
  }
  return ur::check_launch("ur_gelu_f32");
}

int ur_vit_embed_f32(const float* patches, const float* class_token, const float* pos, float* y, int N, int P, int D, ur_stream_t stream) {
  UR_REQUIRE(patches && class_token && pos && y, "null pointer");
  UR_REQUIRE(y != patches, "y and patches must not be the same buffer");
  UR_REQUIRE(N >= 1 && P >= 1 && D >= 1, "N, P and D must be >= 1");
  UR_REQUIRE((long long)N * ((long long)P + 1) * D < ur::GRID_1D_LIMIT, "too many elements: N*(P+1)*D must be below 2^31 - 256");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = D % 4 == 0 && (((uintptr_t)patches | (uintptr_t)class_token | (uintptr_t)pos | (uintptr_t)y) & 15) == 0;
  const int total = N * (P + 1) * (vec ? D / 4 : D);
  UR_GRID_1D(blocks, total, 256);
  ur::ProfScope prof("vit_embed_f32", (double)N * (P + 1) * D, 12.0 * N * (P + 1) * D, s);
  if (vec) hipLaunchKernelGGL(vit_embed_kernel<4>, dim3(blocks), dim3(256), 0, s, patches, class_token, pos, y, total, P, D);
  else hipLaunchKernelGGL(vit_embed_kernel<1>, dim3(blocks), dim3(256), 0, s, patches, class_token, pos, y, total, P, D);
  return ur::check_launch("ur_vit_embed_f32");
}

int ur_vit_attention_f32(const float* qkv, float* out, int N, int S, int H, int d, int D, ur_stream_t stream) {
  UR_REQUIRE(qkv && out, "null pointer");
  UR_REQUIRE(qkv != out, "qkv and out must not be the same buffer");
  UR_REQUIRE(d == VA_D, "the head dimension d must be 64");
  UR_REQUIRE(N >= 1 && H >= 1, "N and H must be >= 1");
  UR_REQUIRE((long long)N * H <= (1 << 22), "too many heads: N*H must be at most 2^22");
  UR_REQUIRE(D == H * d, "D must be H * d");
  UR_REQUIRE(S >= 1 && S <= VA_S_MAX, "S must be in [1, 256] (UR_VIT_S_MAX): K and V of a head stay in LDS");
  UR_REQUIRE(((uintptr_t)qkv & 15) == 0, "qkv must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  switch ((S + 31) / 32) {
    case 1: return vit_attention_launch<1>(qkv, out, N, S, H, s);
    case 2: return vit_attention_launch<2>(qkv, out, N, S, H, s);
    case 3: return vit_attention_launch<3>(qkv, out, N, S, H, s);
    case 4: return vit_attention_launch<4>(qkv, out, N, S, H, s);
    case 5: return vit_attention_launch<5>(qkv, out, N, S, H, s);
    case 6: return vit_attention_launch<6>(qkv, out, N, S, H, s);
    case 7: return vit_attention_launch<7>(qkv, out, N, S, H, s);
    default: return vit_attention_launch<8>(qkv, out, N, S, H, s);
  }
}

}  // extern "C"
