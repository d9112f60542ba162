// Shifted-window cosine attention of the Swin-V2 scorer (unirestore_amd/swin.py) for gfx950, exact fp32 in and out, on the natural
// NHWC map: qkv [N][H][W][3C] (q | k | v, head h in columns 32 h .. 32 h + 31 of each) -> out [N][H][W][C].  One kernel does what
// torchvision's shifted_window_attention does in eight passes between its two Linears: the zero padding of the map to multiples of
// 8, the cyclic shift, the cut into 8 x 8 windows, the cosine scores with the per-head temperature, the relative-position bias, the
// region mask, the softmax, P V, the reverse of the windows, the shift back and the crop.  No padded, rolled or partitioned tensor
// exists in memory: every window slot finds its source by index arithmetic, and only real tokens are written, to their own (i, j).
//
//   pH, pW = H, W rounded up to multiples of 8; per axis the shift is 0 when the padded axis is one window (8 >= p), else `shift`.
//   Slot s = 8 wy + wx of window (winY, winX) holds the rolled position (8 winY + wy, 8 winX + wx), which is the padded position
//   ((8 winY + wy + shift_y) mod pH, (8 winX + wx + shift_x) mod pW) - torch.roll by (-shift_y, -shift_x).  A padded position
//   below (H, W) is a real token; any other is a PAD token: the qkv Linear of a zero row is its bias, so the kernel reads
//   qkv_bias [3C] in its place (the caller zeroes the k third, as torchvision does: a pad token's k is then 0, its normalised k 0,
//   and it stays a key of its window with score bias + mask - pad tokens are NOT masked, as in torchvision).
//   score[i][j] = (q_i / max(|q_i|, 1e-12)) . (k_j / max(|k_j|, 1e-12)) * scale[h] + bias[h][i][j] - 100 [region_i != region_j],
//   the mask only when a shift is in force.  Per axis the region of rolled coordinate r is 0 for r < p - 8, 1 for p - 8 <= r <
//   p - shift, 2 beyond, and 0 everywhere on an axis whose shift is 0: only the last window of a shifted axis has two regions.
//
// One workgroup of two waves per (image, window, head); wave g owns queries 32 g .. 32 g + 31.  The 64 normalised keys sit in LDS
// 33 floats apart (the A operand reads one column of 32 rows: 32 banks), the 64 values 32 apart (the B operand reads 32
// consecutive floats of one row).  Operand and C layout of v_mfma_f32_32x32x2_f32 as documented above vit_attention_kernel
// (vit.hip): scores^T tile kt = K_kt Q^T leaves lane l with 16 scores per tile of ONE query, l & 31, for keys kt * 32 + (r & 3) +
// 8 (r >> 2) + 4 (l >> 5); lane l ^ 32 has the other 16, so a query's score row of 64 lives in one lane pair and the probabilities
// never leave their registers on the way into P V.  q is normalised and multiplied by scale[h] in registers before the product.
// Softmax: row maximum (fmaxf: a NaN score comes back through expf(NaN - m)), libm expf, the lane's 32 values summed in register
// order + the partner's, IEEE division.  No atomics, every sum in a fixed order; nothing depends on the place in the batch.
//
// Non-finite inputs: a score row that holds a NaN or +inf is all NaN (exp(inf - inf)); a NaN or an infinity in a q or k row
// makes the row's norm NaN or inf and the normalised row NaN; a NaN in V reaches every query of its (window, head).  The other
// images keep their bits.
//
// Limits, checked before any HIP call: N, H, W, heads >= 1, shift 0 or 4, N * H * W below 2^31, N * windows * heads below
// 2^31 - 256 (one workgroup each), qkv, qkv_bias and bias 16-byte aligned, out not qkv.
#include "common.h"

#include <climits>
#include <cmath>

namespace {

constexpr int SW_WIN = 8, SW_T = SW_WIN * SW_WIN, SW_D = 32, SW_LDK = 33, SW_LDV = 32;

// region of window slot s on one axis pair: 3 * idy + idx, from whether the window is the last of a shifted axis
__device__ __forceinline__ int sw_region(int s, bool last_y, bool last_x, int shift) {
  const int idy = last_y ? 1 + ((s >> 3) >= SW_WIN - shift) : 0;
  const int idx = last_x ? 1 + ((s & 7) >= SW_WIN - shift) : 0;
  return 3 * idy + idx;
}

__global__ __launch_bounds__(128) void swin_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ qkv_bias,
                                                             const float* __restrict__ scale, const float* __restrict__ bias,
                                                             float* __restrict__ out, int H, int W, int heads, int shift) {
  __shared__ __attribute__((aligned(16))) float Ks[SW_T * SW_LDK];
  __shared__ __attribute__((aligned(16))) float Vs[SW_T * SW_LDV];
  __shared__ int tok[SW_T];                          // slot -> token index n * H * W + y * W + x, or -1 for a pad token
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nwx = (W + SW_WIN - 1) / SW_WIN, nwy = (H + SW_WIN - 1) / SW_WIN;
  const int pH = nwy * SW_WIN, pW = nwx * SW_WIN;
  const int sy = nwy > 1 ? shift : 0, sx = nwx > 1 ? shift : 0;
  int b = blockIdx.x;
  const int h = b % heads;
  b /= heads;
  const int win = b % (nwx * nwy), n = b / (nwx * nwy);
  const int winy = win / nwx, winx = win - winy * nwx;
  const int C = heads * SW_D;
  const long long ld = 3ll * C;

  if (t < SW_T) {
    int y = winy * SW_WIN + (t >> 3) + sy, x = winx * SW_WIN + (t & 7) + sx;
    y -= y >= pH ? pH : 0;
    x -= x >= pW ? pW : 0;
    tok[t] = (y < H && x < W) ? (n * H + y) * W + x : -1;
  }
  __syncthreads();

  {                                                  // k / max(|k|, 1e-12) and v -> LDS: eight lanes per row, 16 rows per pass
    const int c4 = (t & 7) * 4;
#pragma unroll
    for (int r = t >> 3; r < SW_T; r += 16) {
      const int tk = tok[r];
      const float* src = (tk >= 0 ? qkv + tk * ld : qkv_bias) + h * SW_D + c4;
      const float4 kv = *reinterpret_cast<const float4*>(src + C);
      const float4 vv = *reinterpret_cast<const float4*>(src + 2 * C);
      float ss = kv.x * kv.x;
      ss = fmaf(kv.y, kv.y, ss);
      ss = fmaf(kv.z, kv.z, ss);
      ss = fmaf(kv.w, kv.w, ss);
      ss += __shfl_xor(ss, 1, 64);                   // (a + b = b + a: the eight lanes of a row end with the same bits)
      ss += __shfl_xor(ss, 2, 64);
      ss += __shfl_xor(ss, 4, 64);
      const float nrm = fmaxf(sqrtf(ss), 1e-12f);
      float* kd = Ks + r * SW_LDK + c4;
      kd[0] = kv.x / nrm; kd[1] = kv.y / nrm; kd[2] = kv.z / nrm; kd[3] = kv.w / nrm;
      *reinterpret_cast<float4*>(Vs + r * SW_LDV + c4) = vv;
    }
  }

  const int col = lane & 31, half = lane >> 5;
  const int qs = wave * 32 + col;                    // this lane's query slot
  float qr[16];
  {
    const int tk = tok[qs];
    const float* qp = (tk >= 0 ? qkv + tk * ld : qkv_bias) + h * SW_D + half;
    float ss = 0.f;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      qr[kk] = qp[2 * kk];
      ss = fmaf(qr[kk], qr[kk], ss);
    }
    ss += __shfl_xor(ss, 32, 64);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
    const float sc_h = scale[h];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) qr[kk] = qr[kk] / nrm * sc_h;
  }
  __syncthreads();

  f32x16 sc[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[kt][r] = 0.f;
#pragma unroll
  for (int kk = 0; kk < 16; ++kk)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
      sc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[(kt * 32 + col) * SW_LDK + 2 * kk + half], qr[kk], sc[kt], 0, 0, 0);

  const bool masked = (sy | sx) != 0;
  const bool last_y = sy != 0 && winy == nwy - 1, last_x = sx != 0 && winx == nwx - 1;
  const int qreg = sw_region(qs, last_y, last_x, shift);
  const float* brow = bias + ((long long)h * SW_T + qs) * SW_T + 4 * half;
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 bv = *reinterpret_cast<const float4*>(brow + kt * 32 + 8 * g);
      const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        const int key = kt * 32 + 8 * g + 4 * half + e;
        float s = sc[kt][r] + bb[e];
        if (masked && sw_region(key, last_y, last_x, shift) != qreg) s += -100.0f;
        sc[kt][r] = s;
        m = fmaxf(m, s);
      }
    }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = expf(sc[kt][r] - m);
      sc[kt][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 32, 64);
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[kt][r] = sc[kt][r] / sum;

  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int j = 0; j < 16; ++j)
      o = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[kt][j], Vs[(kt * 32 + (j & 3) + 8 * (j >> 2) + 4 * half) * SW_LDV + col], o, 0, 0, 0);

  float* ob = out + h * SW_D + col;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int tk = tok[wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
    if (tk >= 0) ob[(long long)tk * C] = o[r];       // a pad token has no place in the map
  }
}

}  // namespace

extern "C" {

int ur_swin_attention_f32(const float* qkv, const float* qkv_bias, const float* scale, const float* bias, float* out, int N, int H,
                          int W, int heads, int shift, ur_stream_t stream) {
  UR_REQUIRE(qkv && qkv_bias && scale && bias && out, "null pointer");
  UR_REQUIRE(qkv != out, "qkv and out must not be the same buffer");
  UR_REQUIRE(N >= 1 && H >= 1 && W >= 1 && heads >= 1, "N, H, W and heads must be >= 1");
  UR_REQUIRE(shift == 0 || shift == 4, "shift must be 0 or 4 (half the 8 x 8 window)");
  UR_REQUIRE((long long)N * H * W <= INT_MAX, "too many tokens: N*H*W must be below 2^31");
  const long long windows = (((long long)H + SW_WIN - 1) / SW_WIN) * (((long long)W + SW_WIN - 1) / SW_WIN);
  UR_REQUIRE((double)N * (double)windows * (double)heads < (double)ur::GRID_1D_LIMIT,
             "too many windows: N*windows*heads must be below 2^31 - 256");
  UR_REQUIRE((((uintptr_t)qkv | (uintptr_t)qkv_bias | (uintptr_t)bias) & 15) == 0, "qkv, qkv_bias and bias must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long long units = (long long)N * windows * heads;
  ur::ProfScope prof("swin_attention_f32", 4.0 * (double)units * SW_T * SW_T * SW_D, 16.0 * (double)N * H * W * heads * SW_D, s);
  hipLaunchKernelGGL(swin_attention_kernel, dim3((unsigned)units), dim3(128), 0, s, qkv, qkv_bias, scale, bias, out, H, W, heads, shift);
  return ur::check_launch("ur_swin_attention_f32");
}

}  // extern "C"
