// DeepLabV3+'s own kernels for gfx950, exact fp32: one scale of the evaluator's test-time augmentation fused with the ImageNet
// Normalize (bilinear align_corners=True resize, (v - mean) / std, NCHW in, NHWC out), the broadcast of ASPP's pooled branch into
// its slice of the concat buffer, and the two-stage multi-scale average + argmax that ends the metric.  The dilated convolution
// (ur_dlv3_conv2d_f32) is the shared kernel of f32_layers.hip; the half-pixel resize of the head is that file's table-driven
// up-sample with another table.  No atomics; every sum runs in a fixed order, so the same inputs give the same bits on every
// run, eagerly and under graph replay, and an image's results do not depend on its place in the batch.
#include "common.h"
#include "f32_layers.h"

#include <climits>
#include <cmath>

namespace {

// (v - mean) / std with two roundings and a true division, as torchvision's Normalize computes sub_(mean).div_(std).
__device__ __forceinline__ float normalize(float v, float mean, float std) {
#pragma clang fp contract(off)
  const float t = v - mean;
  return __fdiv_rn(t, std);
}

// ------------------------------------------------------------------------------------------ TTA scale + Normalize
// x [N][3][H][W] in [0,1] -> y [N][OH][OW][3], channel c of y = (resized channel c - mean_c) / std_c.
__global__ __launch_bounds__(256) void dlv3_prep_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int H, int W, int OH,
                                                        int OW, const int* __restrict__ iy, const float* __restrict__ wy,
                                                        const int* __restrict__ ix, const float* __restrict__ wx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = i % OW;
  const int r = i / OW;
  const int oy = r % OH, n = r / OH;
  const int y0 = min(max(iy[oy], 0), H - 1), y1 = min(y0 + 1, H - 1);
  const int x0 = min(max(ix[ox], 0), W - 1), x1 = min(x0 + 1, W - 1);
  const float h0 = wy[2ll * oy], h1 = wy[2ll * oy + 1], w0 = wx[2ll * ox], w1 = wx[2ll * ox + 1];
  const float mean[3] = {0.485f, 0.456f, 0.406f}, std[3] = {0.229f, 0.224f, 0.225f};      // R, G, B
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* src = x + ((long long)n * 3 + c) * H * W;
    const float v = bilerp(src[y0 * W + x0], src[y0 * W + x1], src[y1 * W + x0], src[y1 * W + x1], w0, w1, h0, h1);
    y[(long long)i * 3 + c] = normalize(v, mean[c], std[c]);
  }
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

// ------------------------------------------------------------------------------------------ bilinear resize into a channel slice
// x [N][h][w][C] -> y[((n * H + oy) * W + ox) * ldy + c]: f32_layers.hip's table-driven sample (any table: the head's is the
// half-pixel one) with an output row stride, so the ASPP features land in channels 48..303 of the classifier's input with no
// concat copy.  V channels per thread (float4 when C, ldy % 4 == 0 and both pointers are 16-byte aligned).
template <int V>
__global__ __launch_bounds__(256) void dlv3_upsample_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int h, int w, int C,
                                                            int H, int W, int ldy, const int* __restrict__ iy, const float* __restrict__ wy,
                                                            const int* __restrict__ ix, const float* __restrict__ wx) {
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
  const float h0 = wy[2ll * oy], h1 = wy[2ll * oy + 1], w0 = wx[2ll * ox], w1 = wx[2ll * ox + 1];
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

// ------------------------------------------------------------------------------------------ two-stage multi-scale average + argmax
// One thread per output pixel.  Scale k's classifier map q_k [N][hq][wq][C] is first resized to the scale's network input (hs, ws)
// with half-pixel centres (L_k, the model's own align_corners=False resize), and L_k to the output (H, W) with align_corners=True
// (U_k, the evaluator's).  Neither L_k nor U_k is stored: the output pixel's align_corners=True sample touches L_k at rows Y0, Y1
// and columns X0, X1, and each of those four values is the half-pixel sample of q_k at rows (Y -> y0, y1) and columns
// (X -> x0, x1).  Both samples are `bilerp` in fp32, in its operand order; the scales are averaged as ((a + b) + c) / NM and the
// best class kept as in seg_tta_argmax_kernel: a larger value, or the first NaN; ties stay with the lowest class.
// Every index read from a table is clamped to its axis.  All per-scale state is indexed with unrolled constants: registers only.
struct Tta2Args {
  const float* q[3];
  int hq[3], wq[3], hs[3], ws[3];
  long long oh[3], ow[3];        // where scale k's rows start in the half-pixel tables: sum of hs (ws) of the scales before it
  const int *aiy, *aix;          // align_corners=True, L_k -> output: [NM][H], [NM][W]
  const float *awy, *awx;        // [NM][H][2], [NM][W][2]
  const int *hiy, *hix;          // half-pixel, q_k -> L_k: [sum hs], [sum ws]
  const float *hwy, *hwx;        // [sum hs][2], [sum ws][2]
  unsigned char* pred;
  float* avg;                    // [N][H][W][C] or null
  int total, H, W, C;
};

template <int NM>
__global__ __launch_bounds__(256) void dlv3_tta_argmax_kernel(const Tta2Args p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int ox = i % p.W;
  const int r = i / p.W;
  const int oy = r % p.H, n = r / p.H;
  const float* img[NM];
  int ro[NM][2][2], co[NM][2][2];                                      // element offsets of q rows / columns: [scale][L tap][q tap]
  float ry[NM][2][2], cx[NM][2][2];                                    // their half-pixel weights
  float H0[NM], H1[NM], W0[NM], W1[NM];                                // the align_corners=True weights of the L taps
#pragma unroll
  for (int k = 0; k < NM; ++k) {
    const int hq = p.hq[k], wq = p.wq[k], hs = p.hs[k], ws = p.ws[k];
    const long long ty = (long long)k * p.H + oy, tx = (long long)k * p.W + ox;
    const int Y0 = min(max(p.aiy[ty], 0), hs - 1), Y1 = min(Y0 + 1, hs - 1);
    const int X0 = min(max(p.aix[tx], 0), ws - 1), X1 = min(X0 + 1, ws - 1);
    H0[k] = p.awy[2 * ty]; H1[k] = p.awy[2 * ty + 1];
    W0[k] = p.awx[2 * tx]; W1[k] = p.awx[2 * tx + 1];
    img[k] = p.q[k] + (long long)n * hq * wq * p.C;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const long long sy = p.oh[k] + (a ? Y1 : Y0), sx = p.ow[k] + (a ? X1 : X0);
      const int y0 = min(max(p.hiy[sy], 0), hq - 1), y1 = min(y0 + 1, hq - 1);
      const int x0 = min(max(p.hix[sx], 0), wq - 1), x1 = min(x0 + 1, wq - 1);
      ro[k][a][0] = y0 * wq * p.C; ro[k][a][1] = y1 * wq * p.C;         // < N*hq*wq*C <= INT_MAX
      co[k][a][0] = x0 * p.C;      co[k][a][1] = x1 * p.C;
      ry[k][a][0] = p.hwy[2 * sy]; ry[k][a][1] = p.hwy[2 * sy + 1];
      cx[k][a][0] = p.hwx[2 * sx]; cx[k][a][1] = p.hwx[2 * sx + 1];
    }
  }
  float bv = 0.f;
  int bi = 0;
  float* avg = p.avg ? p.avg + (long long)i * p.C : nullptr;
  for (int c = 0; c < p.C; ++c) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      const float* q = img[k] + c;
      float L[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          L[a][b] = bilerp(q[ro[k][a][0] + co[k][b][0]], q[ro[k][a][0] + co[k][b][1]], q[ro[k][a][1] + co[k][b][0]],
                           q[ro[k][a][1] + co[k][b][1]], cx[k][b][0], cx[k][b][1], ry[k][a][0], ry[k][a][1]);
      const float v = bilerp(L[0][0], L[0][1], L[1][0], L[1][1], W0[k], W1[k], H0[k], H1[k]);
      s = k == 0 ? v : __fadd_rn(s, v);
    }
    s = __fdiv_rn(s, (float)NM);
    if (avg) avg[c] = s;
    const bool sn = s != s, bn = bv != bv;
    if (c == 0 || (!bn && (sn || s > bv))) {
      bv = s;
      bi = c;
    }
  }
  p.pred[i] = (unsigned char)bi;
}

}  // namespace

extern "C" {

int ur_dlv3_prep(const float* x, float* y, int N, int C, int H, int W, int OH, int OW, const int* idx_h, const float* wt_h, const int* idx_w,
                 const float* wt_w, ur_stream_t stream) {
  UR_REQUIRE(x && y && idx_h && wt_h && idx_w && wt_w, "null pointer");
  UR_REQUIRE(N >= 1 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1, "N, H, W, OH and OW must be >= 1");
  UR_REQUIRE(C == 3, "C must be 3 (RGB)");
  UR_REQUIRE((long long)N * 3 * H * W <= INT_MAX && (long long)N * 3 * OH * OW <= INT_MAX, "too many pixels: N*3*H*W and N*3*OH*OW must be below 2^31");
  const int total = N * OH * OW;                       // <= INT_MAX / 3 by the check above: far inside the launch margin
  UR_GRID_1D(blocks, total, 256);
  hipLaunchKernelGGL(dlv3_prep_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, total, H, W, OH, OW, idx_h, wt_h, idx_w,
                     wt_w);
  return ur::check_launch("ur_dlv3_prep");
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

int ur_dlv3_upsample_f32(const float* x, float* y, int N, int h, int w, int C, int H, int W, int ldy, const int* idx_h, const float* wt_h,
                         const int* idx_w, const float* wt_w, ur_stream_t stream) {
  UR_REQUIRE(x && y && idx_h && wt_h && idx_w && wt_w, "null pointer");
  UR_REQUIRE(x != y, "x and y must not be the same buffer");
  UR_REQUIRE(N >= 1 && C >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "N, C, h, w, H and W must be >= 1");
  UR_REQUIRE(ldy >= C, "ldy must be >= C");
  UR_REQUIRE((long long)N * h * w * C < ur::GRID_1D_LIMIT && (long long)N * H * W * C < ur::GRID_1D_LIMIT,
             "too many elements: N*h*w*C and N*H*W*C must be below 2^31 - 256");
  hipStream_t s = (hipStream_t)stream;
  if (C % 4 == 0 && ldy % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
    const int total = N * H * W * (C / 4);
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(dlv3_upsample_kernel<4>, dim3(blocks), dim3(256), 0, s, x, y, total, h, w, C, H, W, ldy, idx_h, wt_h, idx_w, wt_w);
  } else {
    const int total = N * H * W * C;
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(dlv3_upsample_kernel<1>, dim3(blocks), dim3(256), 0, s, x, y, total, h, w, C, H, W, ldy, idx_h, wt_h, idx_w, wt_w);
  }
  return ur::check_launch("ur_dlv3_upsample_f32");
}

int ur_dlv3_tta_argmax(const float* q0, const float* q1, const float* q2, int nmaps, int N, int C, int hq0, int wq0, int hs0, int ws0, int hq1,
                       int wq1, int hs1, int ws1, int hq2, int wq2, int hs2, int ws2, int H, int W, const int* ac_idx_h, const float* ac_wt_h, const int* ac_idx_w, const float* ac_wt_w, const int* hp_idx_h,
                       const float* hp_wt_h, const int* hp_idx_w, const float* hp_wt_w, unsigned char* pred, float* avg, ur_stream_t stream) {
  UR_REQUIRE(nmaps >= 1 && nmaps <= 3, "nmaps must be 1, 2 or 3");
  UR_REQUIRE(q0 && (nmaps < 2 || q1) && (nmaps < 3 || q2) && ac_idx_h && ac_wt_h && ac_idx_w && ac_wt_w && hp_idx_h && hp_wt_h &&
                 hp_idx_w && hp_wt_w && pred,
             "null pointer");
  UR_REQUIRE(N >= 1 && H >= 1 && W >= 1, "N, H and W must be >= 1");
  UR_REQUIRE(C >= 1 && C <= 255, "C must be in [1, 255]: the prediction is one byte");
  Tta2Args p = {};
  const float* maps[3] = {q0, q1, q2};
  const int dims[12] = {hq0, wq0, hs0, ws0, hq1, wq1, hs1, ws1, hq2, wq2, hs2, ws2};
  long long oh = 0, ow = 0;
  for (int k = 0; k < nmaps; ++k) {
    const int hq = dims[4 * k], wq = dims[4 * k + 1], hs = dims[4 * k + 2], ws = dims[4 * k + 3];
    UR_REQUIRE(hq >= 1 && wq >= 1 && hs >= 1 && ws >= 1, "every map's hq, wq, hs and ws must be >= 1");
    UR_REQUIRE((long long)N * hq * wq * C <= INT_MAX, "too many elements: N*hq*wq*C of every map must be below 2^31");
    UR_REQUIRE((const void*)maps[k] != (const void*)avg, "a map and avg must not be the same buffer");
    p.q[k] = maps[k]; p.hq[k] = hq; p.wq[k] = wq; p.hs[k] = hs; p.ws[k] = ws; p.oh[k] = oh; p.ow[k] = ow;
    oh += hs; ow += ws;
  }
  UR_REQUIRE((long long)N * H * W < ur::GRID_1D_LIMIT && (!avg || (long long)N * H * W * C < ur::GRID_1D_LIMIT),
             "too many pixels: N*H*W (N*H*W*C with avg) must be below 2^31 - 256");
  p.aiy = ac_idx_h; p.awy = ac_wt_h; p.aix = ac_idx_w; p.awx = ac_wt_w;
  p.hiy = hp_idx_h; p.hwy = hp_wt_h; p.hix = hp_idx_w; p.hwx = hp_wt_w;
  p.pred = pred; p.avg = avg;
  p.total = N * H * W; p.H = H; p.W = W; p.C = C;
  UR_GRID_1D(blocks, p.total, 256);
  const dim3 grid(blocks);
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("dlv3_tta_argmax", 45.0 * nmaps * (double)p.total * C, (double)p.total, s);
  if (nmaps == 1) hipLaunchKernelGGL(dlv3_tta_argmax_kernel<1>, grid, dim3(256), 0, s, p);
  else if (nmaps == 2) hipLaunchKernelGGL(dlv3_tta_argmax_kernel<2>, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(dlv3_tta_argmax_kernel<3>, grid, dim3(256), 0, s, p);
  return ur::check_launch("ur_dlv3_tta_argmax");
}

}  // extern "C"
