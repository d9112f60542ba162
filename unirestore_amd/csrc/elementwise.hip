// HBM-bound stencil / reduction / elementwise kernels + tiny fp32 vector math for gfx950.
#include "common.h"

namespace {

// ---- depthwise 3x3 (pad 1) + bias (+ SimpleGate): one thread = 8 channels of one output pixel ------
template <bool F16>
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, uint16_t* __restrict__ y, int N,
                                                        int H, int W, int C, int gate) {
  const int Cout = gate ? C / 2 : C;
  const int CV = Cout >> 3;
  const long long total = (long long)N * H * W * CV;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int v = (int)(i % CV);
    long long pix = i / CV;
    const int ow = (int)(pix % W);
    const int oh = (int)((pix / W) % H);
    const int n = (int)(pix / ((long long)W * H));
    float acc[2][8];
    const int halves = gate ? 2 : 1;
    for (int hf = 0; hf < halves; ++hf) {
      const int c0 = v * 8 + hf * Cout;
      float4 b0 = *reinterpret_cast<const float4*>(bias + c0), b1 = *reinterpret_cast<const float4*>(bias + c0 + 4);
      float* a = acc[hf];
      a[0] = b0.x; a[1] = b0.y; a[2] = b0.z; a[3] = b0.w; a[4] = b1.x; a[5] = b1.y; a[6] = b1.z; a[7] = b1.w;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int ih = oh + dy - 1;
        if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int iw = ow + dx - 1;
          if ((unsigned)iw >= (unsigned)W) continue;
          uint4 raw = *reinterpret_cast<const uint4*>(x + (((long long)n * H + ih) * W + iw) * C + c0);
          float f[8];
          unpack8t<F16>(raw, f);
          const float* wp = w + (dy * 3 + dx) * C + c0;
          float4 w0 = *reinterpret_cast<const float4*>(wp), w1 = *reinterpret_cast<const float4*>(wp + 4);
          a[0] += f[0] * w0.x; a[1] += f[1] * w0.y; a[2] += f[2] * w0.z; a[3] += f[3] * w0.w;
          a[4] += f[4] * w1.x; a[5] += f[5] * w1.y; a[6] += f[6] * w1.z; a[7] += f[7] * w1.w;
        }
      }
    }
    if (gate) {
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[0][e] *= acc[1][e];
    }
    *reinterpret_cast<uint4*>(y + pix * Cout + v * 8) = pack8t<F16>(acc[0]);
  }
}

// Strip form (round 5): one thread = 8 channels of FOUR consecutive output pixels of a row.  The 3 x 6 input window is loaded once
// (18 16-byte loads per channel half instead of 36) and the nine weights of the thread's channels sit in registers; per output pixel the
// taps are added in the same (dy, dx) order as in the one-pixel kernel above, so the results are bit-identical.  Needs W % 4 == 0.
template <bool F16>
__global__ __launch_bounds__(256) void dwconv3x3_strip_kernel(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, uint16_t* __restrict__ y, int N,
                                                              int H, int W, int C, int gate) {
  constexpr int S = 4;
  const int Cout = gate ? C / 2 : C;
  const int CV = Cout >> 3, WS = W / S;
  const long long total = (long long)N * H * WS * CV;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int v = (int)(i % CV);
    long long r = i / CV;
    const int ow0 = (int)(r % WS) * S;
    r /= WS;
    const int oh = (int)(r % H), n = (int)(r / H);
    float acc[2][S][8];
    const int halves = gate ? 2 : 1;
    for (int hf = 0; hf < halves; ++hf) {
      const int c0 = v * 8 + hf * Cout;
      const float4 b0 = *reinterpret_cast<const float4*>(bias + c0), b1 = *reinterpret_cast<const float4*>(bias + c0 + 4);
#pragma unroll
      for (int sx = 0; sx < S; ++sx) {
        float* a = acc[hf][sx];
        a[0] = b0.x; a[1] = b0.y; a[2] = b0.z; a[3] = b0.w; a[4] = b1.x; a[5] = b1.y; a[6] = b1.z; a[7] = b1.w;
      }
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int ih = oh + dy - 1;
        if ((unsigned)ih >= (unsigned)H) continue;
        uint4 raw[S + 2];
#pragma unroll
        for (int j = 0; j < S + 2; ++j) {
          const int iw = ow0 + j - 1;
          raw[j] = (unsigned)iw < (unsigned)W ? *reinterpret_cast<const uint4*>(x + (((long long)n * H + ih) * W + iw) * C + c0) : make_uint4(0, 0, 0, 0);
        }
        float wk[3][8];
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const float* wp = w + (dy * 3 + dx) * C + c0;
          const float4 w0 = *reinterpret_cast<const float4*>(wp), w1 = *reinterpret_cast<const float4*>(wp + 4);
          wk[dx][0] = w0.x; wk[dx][1] = w0.y; wk[dx][2] = w0.z; wk[dx][3] = w0.w; wk[dx][4] = w1.x; wk[dx][5] = w1.y; wk[dx][6] = w1.z; wk[dx][7] = w1.w;
        }
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
          for (int sx = 0; sx < S; ++sx) {
            const int iw = ow0 + sx + dx - 1;
            if ((unsigned)iw >= (unsigned)W) continue;          // (zero padding: the tap is skipped, as in the one-pixel kernel)
            float f[8];
            unpack8t<F16>(raw[sx + dx], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[hf][sx][e] += f[e] * wk[dx][e];
          }
      }
    }
#pragma unroll
    for (int sx = 0; sx < S; ++sx) {
      if (gate) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[0][sx][e] *= acc[1][sx][e];
      }
      *reinterpret_cast<uint4*>(y + ((((long long)n * H + oh) * W + ow0 + sx) * Cout) + v * 8) = pack8t<F16>(acc[0][sx]);
    }
  }
}

template <bool F16>
__global__ __launch_bounds__(256) void scale_channels_kernel(const uint16_t* __restrict__ x, const float* __restrict__ s,
                                                             const uint16_t* __restrict__ res, uint16_t* __restrict__ y,
                                                             long long HWCV, int CV, long long totalv) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < totalv; i += (long long)gridDim.x * 256) {
    const int v = (int)(i % CV);
    const long long n = i / HWCV;
    uint4 raw = *reinterpret_cast<const uint4*>(x + i * 8);
    float f[8];
    unpack8t<F16>(raw, f);
    const float* sp = s + (n * CV + v) * 8;
    float4 s0 = *reinterpret_cast<const float4*>(sp), s1 = *reinterpret_cast<const float4*>(sp + 4);
    f[0] *= s0.x; f[1] *= s0.y; f[2] *= s0.z; f[3] *= s0.w; f[4] *= s1.x; f[5] *= s1.y; f[6] *= s1.z; f[7] *= s1.w;
    if (res) {
      float r[8];
      unpack8t<F16>(*reinterpret_cast<const uint4*>(res + i * 8), r);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += r[e];
    }
    *reinterpret_cast<uint4*>(y + i * 8) = pack8t<F16>(f);
  }
}

// Multi-task fan-out of scale_channels_kernel: x [B,HW,C] is shared by K tasks, y [K*B,HW,C] is task-major (task k's image b is row
// k*B+b).  One thread loads its 16-byte vector of x ONCE and writes the K scaled results (plain vector stores): (1 + K) tensors of HBM
// traffic instead of 2K.  The product is the one of scale_channels_kernel (fp32 multiply, pack8t), so slice k equals
// ur_scale_channels(x, s[k*B:(k+1)*B]) bit for bit.  s == nullptr: K bit copies of x.
constexpr int FANOUT_MAX_K = 8;
template <bool F16>
__global__ __launch_bounds__(256) void scale_channels_fanout_kernel(const uint16_t* __restrict__ x, const float* __restrict__ s,
                                                                    uint16_t* __restrict__ y, long long HWCV, int CV, long long totalv,
                                                                    int B, int K) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < totalv; i += (long long)gridDim.x * 256) {
    const uint4 raw = *reinterpret_cast<const uint4*>(x + i * 8);
    if (!s) {
#pragma unroll
      for (int k = 0; k < FANOUT_MAX_K; ++k)
        if (k < K) *reinterpret_cast<uint4*>(y + (k * totalv + i) * 8) = raw;
      continue;
    }
    const int v = (int)(i % CV);
    const long long b = i / HWCV;
    float f[8];
    unpack8t<F16>(raw, f);
#pragma unroll
    for (int k = 0; k < FANOUT_MAX_K; ++k) {
      if (k < K) {
        const float* sp = s + (((long long)k * B + b) * CV + v) * 8;
        const float4 s0 = *reinterpret_cast<const float4*>(sp), s1 = *reinterpret_cast<const float4*>(sp + 4);
        float g[8];
        g[0] = f[0] * s0.x; g[1] = f[1] * s0.y; g[2] = f[2] * s0.z; g[3] = f[3] * s0.w;
        g[4] = f[4] * s1.x; g[5] = f[5] * s1.y; g[6] = f[6] * s1.z; g[7] = f[7] * s1.w;
        *reinterpret_cast<uint4*>(y + (k * totalv + i) * 8) = pack8t<F16>(g);
      }
    }
  }
}

template <bool F16>
__global__ __launch_bounds__(256) void axpy_channels_kernel(const uint16_t* __restrict__ a, const uint16_t* __restrict__ b,
                                                            const float* __restrict__ s, uint16_t* __restrict__ y, int CV,
                                                            long long totalv) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < totalv; i += (long long)gridDim.x * 256) {
    const int v = (int)(i % CV);
    float fa[8], fb[8];
    unpack8t<F16>(*reinterpret_cast<const uint4*>(a + i * 8), fa);
    unpack8t<F16>(*reinterpret_cast<const uint4*>(b + i * 8), fb);
    const float* sp = s + v * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) fa[e] += fb[e] * sp[e];
    *reinterpret_cast<uint4*>(y + i * 8) = pack8t<F16>(fa);
  }
}

// SPADE modulation: y = n * (1 + gamma) + beta (+ residual), gamma | beta from one fused conv output [rows][2C]
template <bool F16>
__global__ __launch_bounds__(256) void spade_modulate_kernel(const uint16_t* __restrict__ n, const uint16_t* __restrict__ gb, int ldgb,
                                                             const uint16_t* __restrict__ res, uint16_t* __restrict__ y, int CV,
                                                             long long totalv) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < totalv; i += (long long)gridDim.x * 256) {
    const long long r = i / CV;
    const int v = (int)(i - r * CV);
    float fn[8], fg[8], fb[8], fr[8];
    unpack8t<F16>(*reinterpret_cast<const uint4*>(n + i * 8), fn);
    unpack8t<F16>(*reinterpret_cast<const uint4*>(gb + r * ldgb + v * 8), fg);
    unpack8t<F16>(*reinterpret_cast<const uint4*>(gb + r * ldgb + (CV + v) * 8), fb);
    if (res) unpack8t<F16>(*reinterpret_cast<const uint4*>(res + i * 8), fr);
#pragma unroll
    for (int e = 0; e < 8; ++e) fn[e] = fmaf(fn[e], 1.f + fg[e], fb[e]) + (res ? fr[e] : 0.f);
    *reinterpret_cast<uint4*>(y + i * 8) = pack8t<F16>(fn);
  }
}

// ---- tiny fp32 linear: one wave per output column, all M rows (M small) ------------------------------
__global__ __launch_bounds__(256) void linear_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y, int M, int N,
                                                         int K, int groups, int act) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int Ng = N / groups, Kg = K / groups, g = n / Ng;
  const float* wr = w + (long long)n * Kg;
  for (int m0 = 0; m0 < M; m0 += 8) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // four k per lane and iteration with all 36 loads issued before the first use (one load per dependent step made this
    // kernel K / 64 serialised memory round trips: 24 us for a 512-wide gate MLP); same per-lane summation order
    for (int k0 = lane; k0 < Kg; k0 += 256) {
      float wv[4], xv[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + 64 * u;
        const bool kin = k < Kg;
        wv[u] = kin ? wr[k] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[u][j] = (kin && m0 + j < M) ? x[(long long)(m0 + j) * K + g * Kg + k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (k0 + 64 * u < Kg && m0 + j < M) acc[j] += wv[u] * xv[u][j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = wave_sum(acc[j]);
      if (lane == 0 && m0 + j < M) y[(long long)(m0 + j) * N + n] = apply_act(v + (bias ? bias[n] : 0.f), act);
    }
  }
}

// ---- TFA prompt update: softmax_D(filter), softmax_D(info), tanh(content); upd = f*cond + i*c ---------
__global__ __launch_bounds__(256) void tfa_prompt_kernel(const float* __restrict__ pooled, const float* __restrict__ cond,
                                                         float* __restrict__ upd, int T, int D) {
  __shared__ float red[16];
  const int bt = blockIdx.x, b = bt / T, tt = bt - b * T, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const float* pf = pooled + ((long long)b * 3 + 0) * T * D + (long long)tt * D;
  const float* pi = pooled + ((long long)b * 3 + 1) * T * D + (long long)tt * D;
  const float* pc = pooled + ((long long)b * 3 + 2) * T * D + (long long)tt * D;
  float mf = -INFINITY, mi = -INFINITY;
  for (int d = t; d < D; d += 256) { mf = fmaxf(mf, pf[d]); mi = fmaxf(mi, pi[d]); }
  mf = wave_max(mf); mi = wave_max(mi);
  if (lane == 0) { red[w] = mf; red[4 + w] = mi; }
  __syncthreads();
  mf = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  mi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  float lf = 0.f, li = 0.f;
  for (int d = t; d < D; d += 256) { lf += expf(pf[d] - mf); li += expf(pi[d] - mi); }
  lf = wave_sum(lf); li = wave_sum(li);
  if (lane == 0) { red[8 + w] = lf; red[12 + w] = li; }
  __syncthreads();
  lf = red[8] + red[9] + red[10] + red[11];
  li = red[12] + red[13] + red[14] + red[15];
  for (int d = t; d < D; d += 256) {
    const float f = expf(pf[d] - mf) / lf, iv = expf(pi[d] - mi) / li, c = tanhf(pc[d]);
    upd[(long long)bt * D + d] = f * cond[(long long)bt * D + d] + iv * c;
  }
}

// Multi-task fan-out of tfa_prompt_kernel: block n*T+tt of K*B*T; `pooled` row n % B (shared by the tasks), `cond` row n / B of a
// [K][T][D] prompt table (cond_per_row = 0) or row n (cond_per_row = 1).  The arithmetic and its order are tfa_prompt_kernel's.
__global__ __launch_bounds__(256) void tfa_prompt_fanout_kernel(const float* __restrict__ pooled, const float* __restrict__ cond,
                                                                float* __restrict__ upd, int B, int T, int D, int cond_per_row) {
  __shared__ float red[16];
  const int bt = blockIdx.x, n = bt / T, tt = bt - n * T, b = n % B, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const float* pf = pooled + ((long long)b * 3 + 0) * T * D + (long long)tt * D;
  const float* pi = pooled + ((long long)b * 3 + 1) * T * D + (long long)tt * D;
  const float* pc = pooled + ((long long)b * 3 + 2) * T * D + (long long)tt * D;
  const float* cd = cond + ((long long)(cond_per_row ? n : n / B) * T + tt) * D;
  float mf = -INFINITY, mi = -INFINITY;
  for (int d = t; d < D; d += 256) { mf = fmaxf(mf, pf[d]); mi = fmaxf(mi, pi[d]); }
  mf = wave_max(mf); mi = wave_max(mi);
  if (lane == 0) { red[w] = mf; red[4 + w] = mi; }
  __syncthreads();
  mf = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  mi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  float lf = 0.f, li = 0.f;
  for (int d = t; d < D; d += 256) { lf += expf(pf[d] - mf); li += expf(pi[d] - mi); }
  lf = wave_sum(lf); li = wave_sum(li);
  if (lane == 0) { red[8 + w] = lf; red[12 + w] = li; }
  __syncthreads();
  lf = red[8] + red[9] + red[10] + red[11];
  li = red[12] + red[13] + red[14] + red[15];
  for (int d = t; d < D; d += 256) {
    const float f = expf(pf[d] - mf) / lf, iv = expf(pi[d] - mi) / li, c = tanhf(pc[d]);
    upd[(long long)bt * D + d] = f * cd[d] + iv * c;
  }
}

__global__ void vec_mul_group_kernel(const float* a, const float* b, float* out, int N, int C, int G) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C;
  out[i] = a[i] * b[n * G + c / (C / G)];
}

// ---- layout / boundary kernels --------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ x, uint16_t* __restrict__ y, int C,
                                                           long long HW, int Cpad, float mul, float add, long long total) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long n = i / HW, p = i - n * HW;
    const float* xi = x + n * C * HW + p;
    uint16_t* yo = y + i * Cpad;
    for (int c = 0; c < Cpad; ++c) yo[c] = c < C ? f2h16<F16>(xi[(long long)c * HW] * mul + add) : (uint16_t)0;
  }
}

template <bool F16>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const void* __restrict__ x, int is_f32, float* __restrict__ out,
                                                           int C, long long HW, int ld, float mul, float add,
                                                           long long total) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long n = i / HW, p = i - n * HW;
    for (int c = 0; c < C; ++c) {
      float v = is_f32 ? reinterpret_cast<const float*>(x)[i * ld + c] : Act<F16>::one(reinterpret_cast<const uint16_t*>(x)[i * ld + c]);
      out[(n * C + c) * HW + p] = v * mul + add;
    }
  }
}

// ---- image boundary: bicubic resize (PyTorch semantics: A = -0.75, align_corners=False, antialias=False, source
// index NOT clamped for cubic, tap indices clamped to the image) fused with reflect pad / crop and the layout pass ----
__device__ __forceinline__ void cubic_taps(int dst, float scale, int in_size, int idx[4], float wt[4]) {
  const float real = scale * (dst + 0.5f) - 0.5f;          // upsample_bicubic2d: area_pixel_compute_source_index(cubic=true)
  const float fl = floorf(real);
  const float t = fminf(fmaxf(real - fl, 0.f), 1.f);
  const int i0 = (int)fl;
  const float A = -0.75f;
  const float x1 = t, x2 = 1.f - t;
  wt[0] = ((A * (x1 + 1.f) - 5.f * A) * (x1 + 1.f) + 8.f * A) * (x1 + 1.f) - 4.f * A;
  wt[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
  wt[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
  wt[3] = ((A * (x2 + 1.f) - 5.f * A) * (x2 + 1.f) + 8.f * A) * (x2 + 1.f) - 4.f * A;
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = max(min(i0 + j - 1, in_size - 1), 0);
}

// The tap / accumulate arithmetic of the two boundary directions, shared by the fp32-tensor kernels and the ragged 8-bit ones
// (image_u8_ingest_kernel / image_u8_egress_kernel) so that both compile from the same expressions: an image gives the same bits
// whichever kernel it goes through.  `at(a, b)` returns the source sample at tap row a, tap column b.
__device__ __forceinline__ int reflect_index(int o, int size) { return o < size ? o : 2 * (size - 1) - o; }   // F.pad(mode="reflect")

// sum_a wy[a] * (sum_b wx[b] * at(a, b)), written out with explicit fused multiply-adds and contraction off: which products of
// such a sum the compiler fuses depends on the code around it (its vectoriser pairs lanes differently in each kernel), and a
// differently fused product is a different fp32 result.  The pattern is the one image_resize_pad_kernel has always compiled to.
template <class At>
__device__ __forceinline__ float bicubic_in(const float wy[4], const float wx[4], At at) {
#pragma clang fp contract(off)
  float row[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float head = __builtin_fmaf(wx[2], at(a, 2), __builtin_fmaf(wx[0], at(a, 0), wx[1] * at(a, 1)));
    row[a] = a < 3 ? head + wx[3] * at(a, 3) : __builtin_fmaf(wx[3], at(a, 3), head);
  }
  return __builtin_fmaf(wy[3], row[3], __builtin_fmaf(wy[2], row[2], __builtin_fmaf(wy[1], row[1], __builtin_fmaf(wy[0], row[0], 0.f))));
}

template <class At>
__device__ __forceinline__ float bicubic_out(const float wy[4], const float wx[4], int taps, float mul, float add, At at) {
  float v = 0.f;
  for (int a = 0; a < taps; ++a) {
    float rowv = 0.f;
    for (int b = 0; b < taps; ++b) rowv += wx[b] * (at(a, b) * mul + add);
    v += wy[a] * rowv;
  }
  return v;
}

// torch.round = half-to-even = rintf; the code value 0..255 as a float
__device__ __forceinline__ float quantize_code(float v) { return fminf(fmaxf(rintf(v * 255.f), 0.f), 255.f); }
__device__ __forceinline__ bool finite_sample(float v) { return fabsf(v) <= 3.0e38f; }

// img [N,C,H,W] fp32 -> (bicubic to RH x RW) -> reflect pad right/bottom -> v*mul+add -> y bf16 [N,RH+PH,RW+PW,Cpad]
template <bool F16>
__global__ __launch_bounds__(256) void image_resize_pad_kernel(const float* __restrict__ img, uint16_t* __restrict__ y, int C,
                                                               int H, int W, int RH, int RW, int PH, int PW, int Cpad,
                                                               float mul, float add, long long total) {
  const int OH = RH + PH, OW = RW + PW;
  const bool resize = RH != H || RW != W;
  const float sh = (float)H / RH, sw = (float)W / RW;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ox = (int)(i % OW);
    const long long r = i / OW;
    const int oy = (int)(r % OH), n = (int)(r / OH);
    const int ry = reflect_index(oy, RH), rx = reflect_index(ox, RW);
    const float* base = img + (long long)n * C * H * W;
    uint16_t* yo = y + i * Cpad;
    if (!resize) {
      for (int c = 0; c < Cpad; ++c) yo[c] = c < C ? f2h16<F16>(base[((long long)c * H + ry) * W + rx] * mul + add) : (uint16_t)0;
      continue;
    }
    int iy[4], ix[4];
    float wy[4], wx[4];
    cubic_taps(ry, sh, H, iy, wy);
    cubic_taps(rx, sw, W, ix, wx);
    for (int c = 0; c < Cpad; ++c) {
      float v = 0.f;
      if (c < C) {
        const float* pc = base + (long long)c * H * W;
        v = bicubic_in(wy, wx, [&](int a, int b) { return pc[(long long)iy[a] * W + ix[b]]; });
      }
      yo[c] = c < C ? f2h16<F16>(v * mul + add) : (uint16_t)0;
    }
  }
}

// x NHWC (bf16 | fp32) [N,XH,XW,ld] -> v*mul+add -> crop [0:CH, 0:CW] -> bicubic to OH x OW -> optional
// mul(255).round().clamp(0,255).div(255) -> out fp32 [N,C,OH,OW]
template <bool F16>
__global__ __launch_bounds__(256) void image_unpad_resize_kernel(const void* __restrict__ x, int is_f32, float* __restrict__ out,
                                                                 int C, int XH, int XW, int ld, int CH, int CW, int OH, int OW,
                                                                 float mul, float add, int quantize, long long total) {
  const bool resize = OH != CH || OW != CW;
  const float sh = (float)CH / OH, sw = (float)CW / OW;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ox = (int)(i % OW);
    const long long r = i / OW;
    const int oy = (int)(r % OH), n = (int)(r / OH);
    int iy[4] = {oy, 0, 0, 0}, ix[4] = {ox, 0, 0, 0};
    float wy[4] = {1.f, 0.f, 0.f, 0.f}, wx[4] = {1.f, 0.f, 0.f, 0.f};
    if (resize) { cubic_taps(oy, sh, CH, iy, wy); cubic_taps(ox, sw, CW, ix, wx); }
    const long long nb = (long long)n * XH * XW;
    for (int c = 0; c < C; ++c) {
      float v = bicubic_out(wy, wx, resize ? 4 : 1, mul, add, [&](int a, int b) {
        const long long e = (nb + (long long)iy[a] * XW + ix[b]) * ld + c;
        return is_f32 ? reinterpret_cast<const float*>(x)[e] : Act<F16>::one(reinterpret_cast<const uint16_t*>(x)[e]);
      });
      // A non-finite value stays non-finite (torch.clamp propagates NaN; fmaxf would turn it into a black pixel and hide an
      // fp16 overflow from DiffUIE.forward's finite check): NaN and +-inf both leave as NaN.
      if (quantize) v = finite_sample(v) ? quantize_code(v) / 255.f : __builtin_nanf("");
      out[(((long long)n * C + c) * OH + oy) * OW + ox] = v;
    }
  }
}

// ---- ragged 8-bit batch: slot n of `src` / `dst` holds one dense uint8 HWC [H_n, W_n, 3] image at n * slot_bytes;
// geom int32 [N,4] = (H_n, W_n, RH_n, RW_n) in DEVICE memory, so that one captured launch serves any images that fit the canvas.
// A row of geom that does not fit the canvas is never followed: ingest writes zeros, egress writes nothing but flag 2.
__device__ __forceinline__ bool ragged_geom_ok(int H, int W, int RH, int RW, int CH, int CW) {
  return H > 0 && W > 0 && H <= RH && W <= RW && RH <= CH && RW <= CW && CH - RH < RH && CW - RW < RW;
}

// u8 / 255 (a true division, = torch's u8.float() / 255) -> what image_resize_pad_kernel does -> y 16-bit [N,CH,CW,Cpad]
template <bool F16>
__global__ __launch_bounds__(256) void image_u8_ingest_kernel(const uint8_t* __restrict__ src, long long slot_bytes,
                                                              const int* __restrict__ geom, uint16_t* __restrict__ y, int CH, int CW,
                                                              int Cpad, float mul, float add, long long total) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ox = (int)(i % CW);
    const long long r = i / CW;
    const int oy = (int)(r % CH), n = (int)(r / CH);
    const int H = geom[4 * n], W = geom[4 * n + 1], RH = geom[4 * n + 2], RW = geom[4 * n + 3];
    uint16_t* yo = y + i * Cpad;
    if (!ragged_geom_ok(H, W, RH, RW, CH, CW)) {
      for (int c = 0; c < Cpad; ++c) yo[c] = 0;
      continue;
    }
    const bool resize = RH != H || RW != W;
    const float sh = (float)H / RH, sw = (float)W / RW;
    const int ry = reflect_index(oy, RH), rx = reflect_index(ox, RW);
    const uint8_t* base = src + n * slot_bytes;
    if (!resize) {
      const uint8_t* px = base + ((long long)ry * W + rx) * 3;
      for (int c = 0; c < Cpad; ++c) yo[c] = c < 3 ? f2h16<F16>((float)px[c] / 255.f * mul + add) : (uint16_t)0;
      continue;
    }
    int iy[4], ix[4];
    float wy[4], wx[4];
    cubic_taps(ry, sh, H, iy, wy);
    cubic_taps(rx, sw, W, ix, wx);
    for (int c = 0; c < Cpad; ++c) {
      float v = 0.f;
      if (c < 3) v = bicubic_in(wy, wx, [&](int a, int b) { return (float)base[((long long)iy[a] * W + ix[b]) * 3 + c] / 255.f; });
      yo[c] = c < 3 ? f2h16<F16>(v * mul + add) : (uint16_t)0;
    }
  }
}

// what image_unpad_resize_kernel does with quantize -> the code value as uint8 HWC into slot n.  One thread per CANVAS pixel
// (the launch cannot know H_n x W_n); threads outside the image leave.  A non-finite sample stores code 0 and sets nonfinite[n].
template <bool F16>
__global__ __launch_bounds__(256) void image_u8_egress_kernel(const void* __restrict__ x, int is_f32, uint8_t* __restrict__ dst,
                                                              long long slot_bytes, const int* __restrict__ geom,
                                                              int* __restrict__ nonfinite, int C, int XH, int XW, int ld, float mul,
                                                              float add, long long total) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ox = (int)(i % XW);
    const long long r = i / XW;
    const int oy = (int)(r % XH), n = (int)(r / XH);
    const int OH = geom[4 * n], OW = geom[4 * n + 1], CH = geom[4 * n + 2], CW = geom[4 * n + 3];
    if (!ragged_geom_ok(OH, OW, CH, CW, XH, XW)) {
      if (oy == 0 && ox == 0) nonfinite[n] = 2;
      continue;
    }
    if (oy >= OH || ox >= OW) continue;
    const bool resize = OH != CH || OW != CW;
    const float sh = (float)CH / OH, sw = (float)CW / OW;
    int iy[4] = {oy, 0, 0, 0}, ix[4] = {ox, 0, 0, 0};
    float wy[4] = {1.f, 0.f, 0.f, 0.f}, wx[4] = {1.f, 0.f, 0.f, 0.f};
    if (resize) { cubic_taps(oy, sh, CH, iy, wy); cubic_taps(ox, sw, CW, ix, wx); }
    const long long nb = (long long)n * XH * XW;
    uint8_t* px = dst + n * slot_bytes + ((long long)oy * OW + ox) * C;
    for (int c = 0; c < C; ++c) {
      const float v = bicubic_out(wy, wx, resize ? 4 : 1, mul, add, [&](int a, int b) {
        const long long e = (nb + (long long)iy[a] * XW + ix[b]) * ld + c;
        return is_f32 ? reinterpret_cast<const float*>(x)[e] : Act<F16>::one(reinterpret_cast<const uint16_t*>(x)[e]);
      });
      const bool ok = finite_sample(v);
      if (!ok) nonfinite[n] = 1;
      px[c] = ok ? (uint8_t)quantize_code(v) : (uint8_t)0;
    }
  }
}

template <bool F16>
__global__ __launch_bounds__(256) void vae_sample_kernel(const float* __restrict__ mom, int ld, const float* __restrict__ noise,
                                                         float* __restrict__ z, uint16_t* __restrict__ zb, long long HW,
                                                         int Clat, int Cpad, float scale, long long total) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long n = i / HW, p = i - n * HW;
    for (int c = 0; c < Cpad; ++c) {
      float v = 0.f;
      if (c < Clat) {
        const float mean = mom[i * ld + c];
        const float lv = fminf(fmaxf(mom[i * ld + Clat + c], -30.f), 20.f);
        v = (mean + expf(0.5f * lv) * noise[(n * Clat + c) * HW + p]) * scale;
      }
      z[i * Cpad + c] = v;
      zb[i * Cpad + c] = f2h16<F16>(v);
    }
  }
}

template <bool F16>
__global__ __launch_bounds__(256) void add_noise_kernel(const float* __restrict__ z0, const float* __restrict__ noise,
                                                        float* __restrict__ zt, uint16_t* __restrict__ zb, long long HW,
                                                        int Clat, int Cpad, float sa, float sb, long long total) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long n = i / HW, p = i - n * HW;
    for (int c = 0; c < Cpad; ++c) {
      const float v = c < Clat ? sa * z0[i * Cpad + c] + sb * noise[(n * Clat + c) * HW + p] : 0.f;
      zt[i * Cpad + c] = v;
      zb[i * Cpad + c] = f2h16<F16>(v);
    }
  }
}

template <bool F16>
__global__ __launch_bounds__(256) void ddim_step_kernel(float* __restrict__ zt, const float* __restrict__ eps, int ld_eps,
                                                        uint16_t* __restrict__ zb, int Clat, int Cpad, float cx, float ce,
                                                        long long total) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    for (int c = 0; c < Cpad; ++c) {
      const float v = c < Clat ? cx * zt[i * Cpad + c] + ce * eps[i * ld_eps + c] : 0.f;
      zt[i * Cpad + c] = v;
      zb[i * Cpad + c] = f2h16<F16>(v);
    }
  }
}

template <bool F16>
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ x, int ld, uint16_t* __restrict__ y, int C,
                                                          int Cpad, float mul, long long total) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
    for (int c = 0; c < Cpad; ++c) y[i * Cpad + c] = c < C ? f2h16<F16>(x[i * ld + c] * mul) : (uint16_t)0;
}

// ---- tiled latent sampling (unirestore_amd/tiling.py): tile gather + blended DDIM step ---------------------------------
// origins: device int [T][2] = (y0, x0); a tile that would not lie inside the latent on all four sides is skipped by both
// kernels (gather writes zeros for it; blend neither reads its eps nor writes its slots).
__device__ __forceinline__ bool tile_inside(int y0, int x0, int th, int tw, int LH, int LW) {
  return y0 >= 0 && x0 >= 0 && y0 + th <= LH && x0 + tw <= LW;
}

template <bool F16>
__global__ __launch_bounds__(256) void latent_tiles_gather_kernel(const float* __restrict__ z, uint16_t* __restrict__ tiles,
                                                                  int LH, int LW, int Cpad, int T, int th, int tw,
                                                                  const int* __restrict__ origins, long long total) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {   // i = tile-batch pixel
    const int x = (int)(i % tw);
    const long long r = i / tw;
    const int y = (int)(r % th);
    const long long nk = r / th;
    const int k = (int)(nk % T), n = (int)(nk / T);
    const int y0 = origins[2 * k], x0 = origins[2 * k + 1];
    const bool ok = tile_inside(y0, x0, th, tw, LH, LW);
    const float* src = z + (((long long)n * LH + (y0 + y)) * LW + (x0 + x)) * Cpad;
    for (int c = 0; c < Cpad; ++c) tiles[i * Cpad + c] = ok ? f2h16<F16>(src[c]) : (uint16_t)0;
  }
}

// Output-stationary over full-latent pixels: eps(p) = sum_k wn_k(p) eps_k(p) over the covering tiles in ascending k (fp32),
// zt' = cx*zt + ce*eps, then zt' to the fp32 latent and its 16-bit copy to every covering tile slot (each slot has exactly
// one writer: no atomics, bit-reproducible).
template <bool F16>
__global__ __launch_bounds__(256) void latent_tiles_blend_ddim_kernel(float* __restrict__ zt, const float* __restrict__ eps,
                                                                      int ld_eps, uint16_t* __restrict__ tiles,
                                                                      const float* __restrict__ wn, int LH, int LW, int Clat,
                                                                      int Cpad, int T, int th, int tw,
                                                                      const int* __restrict__ origins, float cx, float ce,
                                                                      long long total) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {   // i = latent pixel
    const int x = (int)(i % LW);
    const long long r = i / LW;
    const int y = (int)(r % LH);
    const long long n = r / LH;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < T; ++k) {
      const int ty = y - origins[2 * k], tx = x - origins[2 * k + 1];
      if (ty < 0 || tx < 0 || ty >= th || tx >= tw || !tile_inside(origins[2 * k], origins[2 * k + 1], th, tw, LH, LW)) continue;
      const long long q = ((long long)k * th + ty) * tw + tx;
      const float w = wn[q];
      const float* e = eps + ((n * T) * th * tw + q) * ld_eps;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < Clat) acc[c] += w * e[c];
    }
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = c < Clat ? cx * zt[i * Cpad + c] + ce * acc[c] : 0.f;
    for (int c = 0; c < Cpad; ++c) zt[i * Cpad + c] = c < 8 ? v[c] : 0.f;
    for (int k = 0; k < T; ++k) {
      const int ty = y - origins[2 * k], tx = x - origins[2 * k + 1];
      if (ty < 0 || tx < 0 || ty >= th || tx >= tw || !tile_inside(origins[2 * k], origins[2 * k + 1], th, tw, LH, LW)) continue;
      uint16_t* d = tiles + ((n * T + k) * th * tw + (long long)ty * tw + tx) * Cpad;
      for (int c = 0; c < Cpad; ++c) d[c] = c < 8 ? f2h16<F16>(v[c]) : (uint16_t)0;
    }
  }
}

inline int nblocks(long long total) { return (int)std::min<long long>((total + 255) / 256, 8192); }

}  // namespace

extern "C" {

int ur_dwconv3x3_nhwc(const void* x, const float* w9c, const float* bias, void* y, int N, int H, int W, int C, int gate,
                      int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(x && w9c && bias && y, "null pointer");
  UR_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "N, H, W, C must be positive");
  UR_REQUIRE(C % (gate ? 16 : 8) == 0, "C must be a multiple of 8 (16 with gate)");
  hipStream_t s = (hipStream_t)stream;
  const double elems = (double)N * H * W * C;
  ur::ProfScope prof("dwconv3x3", 18.0 * elems, 2.0 * elems * (gate ? 1.5 : 2.0), s);
  const long long total = (long long)N * H * W * ((gate ? C / 2 : C) / 8);
  if (W % 4 == 0) {
    UR_DT_SWITCH(dtype, hipLaunchKernelGGL(dwconv3x3_strip_kernel<F16>, dim3(nblocks(total / 4)), dim3(256), 0, s, (const uint16_t*)x, w9c, bias, (uint16_t*)y,
                       N, H, W, C, gate));
    return ur::check_launch("ur_dwconv3x3_nhwc");
  }
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(dwconv3x3_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, s, (const uint16_t*)x, w9c, bias, (uint16_t*)y, N,
                     H, W, C, gate));
  return ur::check_launch("ur_dwconv3x3_nhwc");
}

int ur_scale_channels(const void* x, const float* sc, const void* residual, void* y, int N, int HW, int C,
                      int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(x && sc && y && N > 0 && HW > 0 && C > 0 && C % 8 == 0, "bad args");
  hipStream_t s = (hipStream_t)stream;
  const long long totalv = (long long)N * HW * (C / 8);
  ur::ProfScope prof("elementwise", 0.0, (residual ? 6.0 : 4.0) * totalv * 8.0, s);
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(scale_channels_kernel<F16>, dim3(nblocks(totalv)), dim3(256), 0, s, (const uint16_t*)x, sc,
                     (const uint16_t*)residual, (uint16_t*)y, (long long)HW * (C / 8), C / 8, totalv));
  return ur::check_launch("ur_scale_channels");
}

int ur_scale_channels_fanout(const void* x, const float* sc, void* y, int B, int K, int HW, int C, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(x && y && B > 0 && HW > 0 && C > 0 && C % 8 == 0, "bad args");
  UR_REQUIRE(K >= 1 && K <= FANOUT_MAX_K, "ur_scale_channels_fanout: 1 <= K <= 8");
  hipStream_t s = (hipStream_t)stream;
  const long long totalv = (long long)B * HW * (C / 8);
  ur::ProfScope prof("elementwise", 0.0, 2.0 * (1.0 + K) * totalv * 8.0, s);
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(scale_channels_fanout_kernel<F16>, dim3(nblocks(totalv)), dim3(256), 0, s, (const uint16_t*)x, sc,
                     (uint16_t*)y, (long long)HW * (C / 8), C / 8, totalv, B, K));
  return ur::check_launch("ur_scale_channels_fanout");
}

int ur_axpy_channels(const void* a, const void* b, const float* sc, void* y, long long rows, int C, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(a && b && sc && y && rows > 0 && C > 0 && C % 8 == 0, "bad args");
  hipStream_t s = (hipStream_t)stream;
  const long long totalv = rows * (C / 8);
  ur::ProfScope prof("elementwise", 0.0, 6.0 * totalv * 8.0, s);
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(axpy_channels_kernel<F16>, dim3(nblocks(totalv)), dim3(256), 0, s, (const uint16_t*)a, (const uint16_t*)b, sc,
                     (uint16_t*)y, C / 8, totalv));
  return ur::check_launch("ur_axpy_channels");
}

int ur_spade_modulate(const void* n, const void* gb, int ldgb, const void* residual, void* y, long long rows, int C,
                      int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(n && gb && y && C > 0 && C % 8 == 0 && ldgb % 8 == 0 && ldgb >= 2 * C && rows > 0, "bad args");
  hipStream_t s = (hipStream_t)stream;
  const long long totalv = rows * (C / 8);
  ur::ProfScope prof("elementwise", 0.0, (residual ? 10.0 : 8.0) * totalv * 8.0, s);
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(spade_modulate_kernel<F16>, dim3(nblocks(totalv)), dim3(256), 0, s, (const uint16_t*)n, (const uint16_t*)gb, ldgb,
                     (const uint16_t*)residual, (uint16_t*)y, C / 8, totalv));
  return ur::check_launch("ur_spade_modulate");
}

int ur_linear_f32(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int groups, int act,
                  ur_stream_t stream) {
  UR_REQUIRE(x && w && y && M > 0 && N > 0 && K > 0 && groups > 0 && N % groups == 0 && K % groups == 0, "bad args");
  UR_GRID_1D(blocks, N, 4);                            // four output columns (one per wave) per block
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("linear_f32", 2.0 * M * (double)N * K / groups, 4.0 * N * (double)K / groups, s);
  hipLaunchKernelGGL(linear_f32_kernel, dim3(blocks), dim3(256), 0, s, x, w, bias, y, M, N, K, groups, act);
  return ur::check_launch("ur_linear_f32");
}

int ur_tfa_prompt_update(const float* pooled, const float* cond, float* upd, int B, int T, int D, ur_stream_t stream) {
  UR_REQUIRE(pooled && cond && upd && B > 0 && T > 0 && D > 0, "bad args");
  hipLaunchKernelGGL(tfa_prompt_kernel, dim3(B * T), dim3(256), 0, (hipStream_t)stream, pooled, cond, upd, T, D);
  return ur::check_launch("ur_tfa_prompt_update");
}

int ur_tfa_prompt_update_fanout(const float* pooled, const float* cond, float* upd, int B, int K, int T, int D, int cond_per_row,
                                ur_stream_t stream) {
  UR_REQUIRE(pooled && cond && upd && B > 0 && K > 0 && T > 0 && D > 0 && (long long)B * K * T < (1ll << 31), "bad args");
  hipLaunchKernelGGL(tfa_prompt_fanout_kernel, dim3(B * K * T), dim3(256), 0, (hipStream_t)stream, pooled, cond, upd, B, T, D,
                     (int)(cond_per_row != 0));
  return ur::check_launch("ur_tfa_prompt_update_fanout");
}

int ur_vec_mul_group(const float* a, const float* b, float* out, int N, int C, int G, ur_stream_t stream) {
  UR_REQUIRE(a && b && out && N > 0 && C > 0 && G > 0, "null pointer / N, C, G must be positive");      // G > 0 before C % G
  UR_REQUIRE(C % G == 0 && (long long)N * C < (1ll << 31) - 256, "G must divide C and N * C must fit an int");
  UR_GRID_1D(blocks, (long long)N * C, 256);
  hipLaunchKernelGGL(vec_mul_group_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, b, out, N, C, G);
  return ur::check_launch("ur_vec_mul_group");
}

int ur_nchw_f32_to_nhwc(const float* x, void* y, int N, int C, int H, int W, int Cpad, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(x && y, "null pointer");
  UR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && Cpad >= C, "N, C, H, W must be positive and Cpad >= C");
  const long long total = (long long)N * H * W;
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(nchw_to_nhwc_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, (hipStream_t)stream, x, (uint16_t*)y, C,
                     (long long)H * W, Cpad, 1.f, 0.f, total));
  return ur::check_launch("ur_nchw_f32_to_nhwc");
}

int ur_image_to_nhwc(const float* img, void* y, int N, int C, int H, int W, int Cpad, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(img && y, "null pointer");
  UR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && Cpad >= C, "N, C, H, W must be positive and Cpad >= C");
  const long long total = (long long)N * H * W;
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(nchw_to_nhwc_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, (hipStream_t)stream, img, (uint16_t*)y, C,
                     (long long)H * W, Cpad, 2.f, -1.f, total));
  return ur::check_launch("ur_image_to_nhwc");
}

int ur_nhwc_to_nchw_f32(const void* x, int x_is_f32, float* out, int N, int C, int H, int W, int ld, float mul, float add,
                        int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(x && out, "null pointer");
  UR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && ld >= C, "N, C, H, W must be positive and ld >= C");
  const long long total = (long long)N * H * W;
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(nhwc_to_nchw_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, (hipStream_t)stream, x, x_is_f32, out, C,
                     (long long)H * W, ld, mul, add, total));
  return ur::check_launch("ur_nhwc_to_nchw_f32");
}

int ur_image_resize_pad_nhwc(const float* img, void* y, int N, int C, int H, int W, int RH, int RW, int PH, int PW, int Cpad,
                             float mul, float add, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(img && y, "null pointer");
  UR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && RH > 0 && RW > 0 && Cpad >= C, "N, C, H, W, RH, RW must be positive and Cpad >= C");
  UR_REQUIRE(PH >= 0 && PW >= 0 && PH < RH && PW < RW, "reflect padding must be smaller than the image");
  const long long total = (long long)N * (RH + PH) * (RW + PW);
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(image_resize_pad_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, (hipStream_t)stream, img, (uint16_t*)y, C, H, W,
                     RH, RW, PH, PW, Cpad, mul, add, total));
  return ur::check_launch("ur_image_resize_pad_nhwc");
}

int ur_image_unpad_resize_nchw(const void* x, int x_is_f32, float* out, int N, int C, int XH, int XW, int ld, int CH, int CW,
                               int OH, int OW, float mul, float add, int quantize, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(x && out, "null pointer");
  UR_REQUIRE(N > 0 && C > 0 && OH > 0 && OW > 0 && ld >= C, "N, C, OH, OW must be positive and ld >= C");
  UR_REQUIRE(CH > 0 && CW > 0 && CH <= XH && CW <= XW, "crop window must lie inside the input");
  const long long total = (long long)N * OH * OW;
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(image_unpad_resize_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, (hipStream_t)stream, x, x_is_f32, out, C, XH, XW,
                     ld, CH, CW, OH, OW, mul, add, quantize, total));
  return ur::check_launch("ur_image_unpad_resize_nchw");
}

int ur_image_u8_ingest(const uint8_t* src, long long slot_bytes, const int* geom, void* y, int N, int CH, int CW, int Cpad, float mul,
                       float add, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(src && geom && y, "null pointer");
  UR_REQUIRE(N > 0 && CH > 0 && CW > 0 && Cpad >= 3, "N, CH, CW must be positive and Cpad >= 3");
  UR_REQUIRE(slot_bytes >= 3LL * CH * CW, "slot_bytes must hold a canvas-sized image (CH * CW * 3)");
  const long long total = (long long)N * CH * CW;
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(image_u8_ingest_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, (hipStream_t)stream, src, slot_bytes, geom,
                     (uint16_t*)y, CH, CW, Cpad, mul, add, total));
  return ur::check_launch("ur_image_u8_ingest");
}

int ur_image_u8_egress(const void* x, int x_is_f32, uint8_t* dst, long long slot_bytes, const int* geom, int* nonfinite, int N, int C,
                       int XH, int XW, int ld, float mul, float add, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(x && dst && geom && nonfinite, "null pointer");
  UR_REQUIRE(N > 0 && XH > 0 && XW > 0 && C > 0 && ld >= C, "N, C, XH, XW must be positive and ld >= C");
  UR_REQUIRE(slot_bytes >= (long long)C * XH * XW, "slot_bytes must hold a canvas-sized image (XH * XW * C)");
  const long long total = (long long)N * XH * XW;
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(image_u8_egress_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, (hipStream_t)stream, x, x_is_f32, dst,
                     slot_bytes, geom, nonfinite, C, XH, XW, ld, mul, add, total));
  return ur::check_launch("ur_image_u8_egress");
}

int ur_vae_sample(const float* moments, int ld, const float* noise_nchw, float* z_nhwc, void* z_16, int N, int HW,
                  int Clat, int Cpad, float scale, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(moments && noise_nchw && z_nhwc && z_16, "null pointer");
  UR_REQUIRE(N > 0 && HW > 0 && Clat > 0, "N, HW, Clat must be positive");
  UR_REQUIRE(ld >= 2 * Clat && Cpad >= Clat, "channels: ld >= 2 * Clat, Cpad >= Clat");
  const long long total = (long long)N * HW;
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(vae_sample_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, (hipStream_t)stream, moments, ld, noise_nchw,
                     z_nhwc, (uint16_t*)z_16, (long long)HW, Clat, Cpad, scale, total));
  return ur::check_launch("ur_vae_sample");
}

int ur_add_noise(const float* z0, const float* noise_nchw, float* zt, void* zt_16, int N, int HW, int Clat, int Cpad,
                 float sa, float sb, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(z0 && noise_nchw && zt && zt_16, "null pointer");
  UR_REQUIRE(N > 0 && HW > 0 && Clat > 0 && Cpad >= Clat, "N, HW, Clat must be positive and Cpad >= Clat");
  const long long total = (long long)N * HW;
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(add_noise_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, (hipStream_t)stream, z0, noise_nchw, zt,
                     (uint16_t*)zt_16, (long long)HW, Clat, Cpad, sa, sb, total));
  return ur::check_launch("ur_add_noise");
}

int ur_ddim_step(float* zt, const float* eps, int ld_eps, void* zt_16, long long M, int Clat, int Cpad, float c_x,
                 float c_e, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(zt && eps && zt_16, "null pointer");
  UR_REQUIRE(M > 0 && Clat > 0, "M, Clat must be positive");
  UR_REQUIRE(Cpad >= Clat && ld_eps >= Clat, "channels: Cpad >= Clat, ld_eps >= Clat");
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(ddim_step_kernel<F16>, dim3(nblocks(M)), dim3(256), 0, (hipStream_t)stream, zt, eps, ld_eps,
                     (uint16_t*)zt_16, Clat, Cpad, c_x, c_e, M));
  return ur::check_launch("ur_ddim_step");
}

int ur_latent_tiles_gather(const float* z, void* tiles_16, int N, int LH, int LW, int Cpad, int T, int th, int tw,
                           const int* origins, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(z && tiles_16 && origins, "null pointer");
  UR_REQUIRE(N > 0 && LH > 0 && LW > 0 && Cpad > 0 && T > 0 && th > 0 && tw > 0 && th <= LH && tw <= LW, "bad shape");
  const long long total = (long long)N * T * th * tw;
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(latent_tiles_gather_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, (hipStream_t)stream, z,
                     (uint16_t*)tiles_16, LH, LW, Cpad, T, th, tw, origins, total));
  return ur::check_launch("ur_latent_tiles_gather");
}

int ur_latent_tiles_blend_ddim(float* zt, const float* eps_tiles, int ld_eps, void* zt_tiles_16, const float* wn, int N, int LH,
                               int LW, int Clat, int Cpad, int T, int th, int tw, const int* origins, float c_x, float c_e,
                               int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(zt && eps_tiles && zt_tiles_16 && wn && origins, "null pointer");
  UR_REQUIRE(N > 0 && LH > 0 && LW > 0 && T > 0 && th > 0 && tw > 0 && th <= LH && tw <= LW, "bad shape");
  UR_REQUIRE(Clat > 0 && Clat <= 8 && Cpad >= Clat && ld_eps >= Clat, "channels: Clat <= 8, Cpad >= Clat, ld_eps >= Clat");
  const long long total = (long long)N * LH * LW;
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(latent_tiles_blend_ddim_kernel<F16>, dim3(nblocks(total)), dim3(256), 0, (hipStream_t)stream,
                     zt, eps_tiles, ld_eps, (uint16_t*)zt_tiles_16, wn, LH, LW, Clat, Cpad, T, th, tw, origins, c_x, c_e, total));
  return ur::check_launch("ur_latent_tiles_blend_ddim");
}

int ur_f32_to_bf16_scaled(const float* x, int ld, void* y, long long M, int C, int Cpad, float mul, int dtype, ur_stream_t stream) {
  UR_REQUIRE_DT(dtype);
  UR_REQUIRE(x && y, "null pointer");
  UR_REQUIRE(M > 0 && C > 0 && ld >= C && Cpad >= C, "M, C must be positive, ld >= C and Cpad >= C");
  UR_DT_SWITCH(dtype, hipLaunchKernelGGL(f32_to_bf16_kernel<F16>, dim3(nblocks(M)), dim3(256), 0, (hipStream_t)stream, x, ld, (uint16_t*)y, C, Cpad,
                     mul, M));
  return ur::check_launch("ur_f32_to_bf16_scaled");
}

}  // extern "C"
