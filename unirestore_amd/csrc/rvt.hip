// The two layers the RVT scorer (unirestore_amd/rvt.py) needs beyond csrc/vit.hip and the convolution of f32_layers.hip, for gfx950,
// exact fp32 in and out: multi-head self-attention with head dimension 32 or 64 and an optional per-(head, query, key) gate on the
// scaled scores (RVT's position-aware attention scaling: the scores times sigmoid(att_mask) before the softmax), and the depthwise
// 3 x 3 convolution with a channel multiplier, stride 1 or 2, and the exact-erf GELU in its epilogue.  No atomics, no split sums;
// every sum runs in a fixed order, so the same inputs give the same bits on every run, eagerly and under graph replay, and an
// image's results do not depend on its place in the batch.
//
// Limits, checked before any HIP call (64-bit arithmetic):
//   ur_rvt_attention_f32: d = 32 or 64, 1 <= S <= UR_VIT_S_MAX = 256 (K and V of one head stay in LDS: S rounded up to 32 rows of
//     d + 1 + d floats, 129 KiB at d = 64 and 65 KiB at d = 32), N, H >= 1, N * H <= 2^22, qkv 16-byte aligned, gate (when given)
//     4-byte aligned, out neither qkv nor gate.
//   ur_dwconv3x3_f32: N, H, W, C, mult >= 1, stride 1 or 2, N * H * W * C and N * OH * OW * C * mult below 2^31 - 256 (one thread
//     per output or per four, 64-bit offsets), every pointer 4-byte aligned, y none of x, w, bias.
//
// Non-finite inputs follow the rule of vit.hip.  Attention: a score row that holds a NaN or +inf is all NaN (exp(inf - inf)); a -inf
// score has weight 0; a NaN in V reaches every query of its (image, head); a gate of exactly 0 against an infinite score is NaN
// (0 * inf), as in torch, and a NaN gate is a NaN score.  Depthwise convolution: a padded tap is skipped, not multiplied by 0, so a
// non-finite input reaches exactly the outputs whose 3 x 3 window holds it (of its own channel's outputs); the GELU maps NaN -> NaN,
// +inf -> +inf, -inf -> NaN as ur_gelu_f32 does.
#include "common.h"

#include <climits>
#include <cmath>

namespace {

// ------------------------------------------------------------------------------------------ attention
// vit_attention_kernel (vit.hip: the operand and C layouts of v_mfma_f32_32x32x2_f32 are documented there) with the head dimension
// and the gate as template parameters.  One workgroup per (image, head, group of four 32-query tiles); wave g owns query tile
// 4 * blockIdx.y + g.  K and V of the head sit in LDS, S rounded up to NKT tiles of 32 keys with zeros in the added rows: K rows
// D + 1 floats apart (the A operand reads one column of 32 rows: 32 different banks), V rows D apart.
//   scores^T tile kt = K_kt Q^T leaves lane l with 16 scores per tile of ONE query, l & 31, for keys kt * 32 + (r & 3) + 8 (r >> 2)
//     + 4 (l >> 5); lane l ^ 32 has the other 16.  D = 64: q is multiplied by 1/8 on the way into its registers (a power of two:
//     exact, and the same bits as ur_vit_attention_f32).  D = 32: the finished dot product is multiplied by fp32(32^-0.5) once.
//   GATE: the scaled score is multiplied by gate[h][query][key], read straight from global memory in that C-map order: register
//     group r >> 2 of tile kt is four consecutive keys, one float4 (GATE = 2: S % 4 == 0 and gate 16-byte aligned, so a group lies
//     wholly below S or wholly beyond it) or four scalars (GATE = 1).  Queries and keys beyond S read nothing.  The gate is not
//     staged through LDS: [H][S][S] is 1.8 MB at 12 heads and 196 tokens and stays in L2 across the batch.
//   Softmax and P V exactly as in vit_attention_kernel: maximum over the S real keys with fmaxf, libm expf, the lane's 16 NKT values
//     summed in register order + the partner's, IEEE division; the probabilities never leave their registers on the way into P V.
constexpr int RA_S_MAX = UR_VIT_S_MAX;
static_assert(RA_S_MAX == 8 * 32, "the launcher instantiates 1..8 key tiles");
constexpr float RA_SCALE_32 = 0.17677669529663688110f;      // 32^-0.5 rounded to fp32

template <int D, int NKT, int GATE>
__global__ __launch_bounds__(256) void rvt_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ gate,
                                                            float* __restrict__ out, int S, int H) {
#pragma clang fp contract(off)                       // scale, gate and score - m stay three roundings: no fma across them
  static_assert(D == 32 || D == 64, "head dimension");
  constexpr int LDK = D + 1, LDV = D, TPR = D / 4;   // threads per K / V row of the copy
  extern __shared__ __attribute__((aligned(16))) float ra_lds[];
  float* Ks = ra_lds;                                // [NKT * 32][LDK]
  float* Vs = ra_lds + NKT * 32 * LDK;               // [NKT * 32][LDV]; NKT * 32 * LDK * 4 bytes is a multiple of 16
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = blockIdx.x / H, h = blockIdx.x - n * H;
  const int Dm = H * D;
  const long long ld = 3ll * Dm;
  const float* base = qkv + (long long)n * S * ld + h * D;

  {                                                  // K, V -> LDS: thread t takes 4 floats of row t / TPR + (256 / TPR) i
    const int c4 = (t % TPR) * 4;
#pragma unroll 4
    for (int r = t / TPR; r < NKT * 32; r += 256 / TPR) {
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (r < S) {
        kv = *reinterpret_cast<const float4*>(base + r * ld + Dm + c4);
        vv = *reinterpret_cast<const float4*>(base + r * ld + 2 * Dm + c4);
      }
      float* kd = Ks + r * LDK + c4;
      kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
      *reinterpret_cast<float4*>(Vs + r * LDV + c4) = vv;
    }
  }
  __syncthreads();
  const int q0 = (blockIdx.y * 4 + wave) * 32;
  if (q0 >= S) return;                               // a wave without queries: the only barrier is behind it

  const int col = lane & 31, half = lane >> 5;
  const int q = q0 + col;
  float qr[D / 2];
  {
    const float* qp = base + (long long)q * ld + half;
#pragma unroll
    for (int kk = 0; kk < D / 2; ++kk) {
      const float v = q < S ? qp[2 * kk] : 0.f;
      qr[kk] = D == 64 ? v * 0.125f : v;
    }
  }
  f32x16 sc[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[kt][r] = 0.f;
#pragma unroll
  for (int kk = 0; kk < D / 2; ++kk)
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
      sc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[(kt * 32 + col) * LDK + 2 * kk + half], qr[kk], sc[kt], 0, 0, 0);

  if constexpr (D == 32) {
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[kt][r] = sc[kt][r] * RA_SCALE_32;
  }
  if constexpr (GATE != 0) {
    if (q < S) {
      const float* grow = gate + ((long long)h * S + q) * S + 4 * half;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int key = kt * 32 + 8 * g;           // + 4 half + (0..3): the four keys of register group g
          if constexpr (GATE == 2) {
            if (key + 4 * half < S) {                // S % 4 == 0: the whole group is real
              const float4 gv = *reinterpret_cast<const float4*>(grow + key);
              sc[kt][4 * g + 0] = sc[kt][4 * g + 0] * gv.x;
              sc[kt][4 * g + 1] = sc[kt][4 * g + 1] * gv.y;
              sc[kt][4 * g + 2] = sc[kt][4 * g + 2] * gv.z;
              sc[kt][4 * g + 3] = sc[kt][4 * g + 3] * gv.w;
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (key + 4 * half + e < S) sc[kt][4 * g + e] = sc[kt][4 * g + e] * grow[key + e];
          }
        }
    }
  }

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

  f32x16 o[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float* vrow = Vs + (kt * 32 + (j & 3) + 8 * (j >> 2) + 4 * half) * LDV + col;
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[kt][j], vrow[32 * dt], o[dt], 0, 0, 0);
    }

  float* ob = out + (long long)n * S * Dm + h * D + col;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qo = q0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (qo < S) {
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) ob[(long long)qo * Dm + 32 * dt] = o[dt][r];
    }
  }
}

template <int D, int NKT, int GATE>
int rvt_attention_launch(const float* qkv, const float* gate, float* out, int N, int S, int H, hipStream_t s) {
  constexpr int lds = NKT * 32 * (D + 1 + D) * 4;
  if constexpr (lds > 64 * 1024) {
    static ur::DeviceOnce attr_once;      // the attribute is per device
    if (auto once_guard = attr_once.first())
      hipFuncSetAttribute(reinterpret_cast<const void*>(&rvt_attention_kernel<D, NKT, GATE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          lds);
  }
  const dim3 grid((unsigned)(N * H), (unsigned)((S + 127) / 128));
  ur::ProfScope prof(GATE ? "rvt_attention_gated_f32" : "rvt_attention_f32", 4.0 * N * H * (double)S * S * D,
                     16.0 * N * S * H * D + (GATE ? 4.0 * H * (double)S * S : 0.0), s);
  hipLaunchKernelGGL((rvt_attention_kernel<D, NKT, GATE>), grid, dim3(256), lds, s, qkv, gate, out, S, H);
  return ur::check_launch("ur_rvt_attention_f32");
}

template <int D, int GATE>
int rvt_attention_tiles(const float* qkv, const float* gate, float* out, int N, int S, int H, hipStream_t s) {
  switch ((S + 31) / 32) {
    case 1: return rvt_attention_launch<D, 1, GATE>(qkv, gate, out, N, S, H, s);
    case 2: return rvt_attention_launch<D, 2, GATE>(qkv, gate, out, N, S, H, s);
    case 3: return rvt_attention_launch<D, 3, GATE>(qkv, gate, out, N, S, H, s);
    case 4: return rvt_attention_launch<D, 4, GATE>(qkv, gate, out, N, S, H, s);
    case 5: return rvt_attention_launch<D, 5, GATE>(qkv, gate, out, N, S, H, s);
    case 6: return rvt_attention_launch<D, 6, GATE>(qkv, gate, out, N, S, H, s);
    case 7: return rvt_attention_launch<D, 7, GATE>(qkv, gate, out, N, S, H, s);
    default: return rvt_attention_launch<D, 8, GATE>(qkv, gate, out, N, S, H, s);
  }
}

template <int D>
int rvt_attention_gate(const float* qkv, const float* gate, float* out, int N, int S, int H, hipStream_t s) {
  if (!gate) return rvt_attention_tiles<D, 0>(qkv, gate, out, N, S, H, s);
  if (S % 4 == 0 && ((uintptr_t)gate & 15) == 0) return rvt_attention_tiles<D, 2>(qkv, gate, out, N, S, H, s);
  return rvt_attention_tiles<D, 1>(qkv, gate, out, N, S, H, s);
}

// ------------------------------------------------------------------------------------------ depthwise 3 x 3 convolution
// NHWC, pad 1, stride 1 or 2; output channel o reads input channel o / mult (groups = C, Cout = C * mult).  w is tap-major
// [9][C * mult], so the channels of one pixel are contiguous in x, w, bias and y alike.  One thread per output (V = 1) or per four
// channels of one output pixel (V = 4: mult == 1, C % 4 == 0, 16-byte aligned pointers).  The taps inside the map are accumulated
// from 0 in row-major tap order with fmaf; a tap in the padding is skipped.  Then + bias, then the GELU of ur_gelu_f32 when ACT.
__device__ __forceinline__ float rvt_gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

template <int V, bool ACT>
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y, int total, int H, int W,
                                                        int C, int OH, int OW, int mult, int stride) {
  const int i = blockIdx.x * 256 + threadIdx.x;      // over N * OH * OW * (CO / V)
  if (i >= total) return;
  const int CO = C * mult;
  const int cv = CO / V;
  const int o = (i % cv) * V;
  int p = i / cv;
  const int ox = p % OW;
  p /= OW;
  const int oy = p % OH;
  const int n = p / OH;
  const int c = V == 4 ? o : o / mult;
  const int iy0 = oy * stride - 1, ix0 = ox * stride - 1;
  float acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = iy0 + ky;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ix0 + kx;
      if (ix < 0 || ix >= W) continue;
      const float* xp = x + (((long long)n * H + iy) * W + ix) * C + c;
      const float* wp = w + (long long)(ky * 3 + kx) * CO + o;
      if constexpr (V == 4) {
        const float4 xv = *reinterpret_cast<const float4*>(xp), wv = *reinterpret_cast<const float4*>(wp);
        acc[0] = fmaf(xv.x, wv.x, acc[0]);
        acc[1] = fmaf(xv.y, wv.y, acc[1]);
        acc[2] = fmaf(xv.z, wv.z, acc[2]);
        acc[3] = fmaf(xv.w, wv.w, acc[3]);
      } else {
        acc[0] = fmaf(*xp, *wp, acc[0]);
      }
    }
  }
  float r[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    r[k] = acc[k] + bias[o + k];
    if constexpr (ACT) r[k] = rvt_gelu_erf(r[k]);
  }
  float* yp = y + (long long)i * V;
  if constexpr (V == 4) *reinterpret_cast<float4*>(yp) = make_float4(r[0], r[1], r[2], r[3]);
  else *yp = r[0];
}

bool overlaps(const void* a, double a_bytes, const void* b, double b_bytes) {
  const double a0 = (double)(uintptr_t)a, b0 = (double)(uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

extern "C" {

int ur_rvt_attention_f32(const float* qkv, const float* gate, float* out, int N, int S, int H, int d, ur_stream_t stream) {
  UR_REQUIRE(qkv && out, "null pointer (only gate may be null: no gate)");
  UR_REQUIRE(d == 32 || d == 64, "the head dimension d must be 32 or 64");
  UR_REQUIRE(N >= 1 && H >= 1, "N and H must be >= 1");
  UR_REQUIRE((long long)N * H <= (1 << 22), "too many heads: N*H must be at most 2^22");
  UR_REQUIRE(S >= 1 && S <= RA_S_MAX, "S must be in [1, 256] (UR_VIT_S_MAX): K and V of a head stay in LDS");
  UR_REQUIRE(((uintptr_t)qkv & 15) == 0, "qkv must be 16-byte aligned");
  UR_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)gate & 3) == 0, "out and gate must be 4-byte aligned");
  const double out_bytes = 4.0 * N * S * H * d;
  UR_REQUIRE(!overlaps(out, out_bytes, qkv, 3.0 * out_bytes), "out must not overlap qkv");
  UR_REQUIRE(!gate || !overlaps(out, out_bytes, gate, 4.0 * H * S * S), "out must not overlap gate");
  hipStream_t s = (hipStream_t)stream;
  return d == 64 ? rvt_attention_gate<64>(qkv, gate, out, N, S, H, s) : rvt_attention_gate<32>(qkv, gate, out, N, S, H, s);
}

int ur_dwconv3x3_f32(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, int mult, int stride, int act,
                     ur_stream_t stream) {
  UR_REQUIRE(x && w && bias && y, "null pointer");
  UR_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 1, "N, H, W and C must be >= 1");
  UR_REQUIRE(mult >= 1, "mult must be >= 1");
  UR_REQUIRE(stride == 1 || stride == 2, "stride must be 1 or 2");
  UR_REQUIRE(act == 0 || act == 1, "act must be 0 (none) or 1 (GELU)");
  const long long OH = ((long long)H - 1) / stride + 1, OW = ((long long)W - 1) / stride + 1, CO = (long long)C * mult;
  const double in_elems = (double)N * H * W * C, out_elems = (double)N * OH * OW * (double)CO;
  UR_REQUIRE(in_elems < (double)ur::GRID_1D_LIMIT && out_elems < (double)ur::GRID_1D_LIMIT,
             "too many elements: N*H*W*C and N*OH*OW*C*mult must be below 2^31 - 256");
  UR_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)y) & 3) == 0, "x, w, bias and y must be 4-byte aligned");
  UR_REQUIRE(!overlaps(y, 4.0 * out_elems, x, 4.0 * in_elems) && !overlaps(y, 4.0 * out_elems, w, 36.0 * CO) &&
                 !overlaps(y, 4.0 * out_elems, bias, 4.0 * CO),
             "y must not overlap x, w or bias");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = mult == 1 && CO % 4 == 0 && (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)y) & 15) == 0;
  const int total = (int)((long long)out_elems / (vec ? 4 : 1));
  UR_GRID_1D(blocks, total, 256);
  ur::ProfScope prof("dwconv3x3_f32", 18.0 * out_elems, 4.0 * (in_elems + out_elems), s);
  const int oh = (int)OH, ow = (int)OW;
  if (vec) {
    if (act) hipLaunchKernelGGL((dwconv3x3_kernel<4, true>), dim3(blocks), dim3(256), 0, s, x, w, bias, y, total, H, W, C, oh, ow, mult, stride);
    else hipLaunchKernelGGL((dwconv3x3_kernel<4, false>), dim3(blocks), dim3(256), 0, s, x, w, bias, y, total, H, W, C, oh, ow, mult, stride);
  } else {
    if (act) hipLaunchKernelGGL((dwconv3x3_kernel<1, true>), dim3(blocks), dim3(256), 0, s, x, w, bias, y, total, H, W, C, oh, ow, mult, stride);
    else hipLaunchKernelGGL((dwconv3x3_kernel<1, false>), dim3(blocks), dim3(256), 0, s, x, w, bias, y, total, H, W, C, oh, ow, mult, stride);
  }
  return ur::check_launch("ur_dwconv3x3_f32");
}

}  // extern "C"
