// The segmenter's own kernels for gfx950, exact fp32: one scale of the evaluator's test-time augmentation fused with
// RefineNet-LW's preprocess (bilinear align_corners=True resize, v * 255 - mean, RGB -> BGR, NCHW in, NHWC out), the multi-scale
// average + argmax that ends the metric, and the confusion matrix of the mIoU.  The convolutions, the head's bilinear up-sample,
// 5x5 max-pool and a + b are in f32_layers.hip; the bilinear sample and its axis tables are f32_layers.h's.  No atomics; every
// sum runs in a fixed order, so the same inputs give the same bits on every run, eagerly and under graph replay, and an image's
// results do not depend on its place in the batch.
#include "common.h"
#include "f32_layers.h"

#include <climits>
#include <cmath>

namespace {

// v * 255 - mean with two roundings, as torch computes x * 255 - mean: never contracted into one fma.
__device__ __forceinline__ float scale255_minus(float v, float mean) {
#pragma clang fp contract(off)
  const float t = v * 255.f;
  return t - mean;
}

// ------------------------------------------------------------------------------------------ TTA scale + preprocess
// x [N][3][H][W] in [0,1] -> y [N][OH][OW][3], channel k of y = 255 * resized channel 2 - k, minus that channel's mean.
__global__ __launch_bounds__(256) void seg_prep_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int H, int W, int OH,
                                                       int OW, const int* __restrict__ iy, const float* __restrict__ wy,
                                                       const int* __restrict__ ix, const float* __restrict__ wx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = i % OW;
  const int r = i / OW;
  const int oy = r % OH, n = r / OH;
  const int y0 = min(max(iy[oy], 0), H - 1), y1 = min(y0 + 1, H - 1);
  const int x0 = min(max(ix[ox], 0), W - 1), x1 = min(x0 + 1, W - 1);
  const float h0 = wy[2ll * oy], h1 = wy[2ll * oy + 1], w0 = wx[2ll * ox], w1 = wx[2ll * ox + 1];      // (an axis may have 2^30 outputs or more)
  const float mean[3] = {123.68f, 116.779f, 103.939f};                 // R, G, B
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* src = x + ((long long)n * 3 + c) * H * W;
    const float v = bilerp(src[y0 * W + x0], src[y0 * W + x1], src[y1 * W + x0], src[y1 * W + x1], w0, w1, h0, h1);
    y[(long long)i * 3 + (2 - c)] = scale255_minus(v, mean[c]);
  }
}

// ------------------------------------------------------------------------------------------ multi-scale average + argmax
// One thread per output pixel.  For every class, in ascending order: sample each of the NM maps bilinearly, average them as
// ((a + b) + c) / NM and keep the running best - a larger value, or a NaN when no NaN was seen yet; an equal value never replaces
// an earlier class (torch.argmax: ties to the lowest index, NaN is the maximum, the first one wins).  The four tap offsets and
// weights of every map stay in registers; a wave's 64 neighbouring pixels read a few neighbouring source pixels, whose C
// consecutive floats they walk together, so the maps are served from L1 / L2 and the only HBM traffic is the byte written.
struct TtaArgs {
  const float* m[3];
  int h[3], w[3];
  const int *iy, *ix;            // [NM][H], [NM][W]
  const float *wy, *wx;          // [NM][H][2], [NM][W][2]
  unsigned char* pred;
  float* avg;                    // [N][H][W][C] or null
  int total, H, W, C;
};

template <int NM>
__global__ __launch_bounds__(256) void seg_tta_argmax_kernel(const TtaArgs p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int ox = i % p.W;
  const int r = i / p.W;
  const int oy = r % p.H, n = r / p.H;
  const float* t00[NM];
  int d01[NM], d10[NM], d11[NM];                                       // offsets of the other three taps from the first
  float w0[NM], w1[NM], h0[NM], h1[NM];
#pragma unroll
  for (int k = 0; k < NM; ++k) {
    const int h = p.h[k], w = p.w[k];
    const long long ty = (long long)k * p.H + oy, tx = (long long)k * p.W + ox;      // table rows: 64-bit, k * H may pass 2^31
    const int y0 = min(max(p.iy[ty], 0), h - 1), y1 = min(y0 + 1, h - 1);
    const int x0 = min(max(p.ix[tx], 0), w - 1), x1 = min(x0 + 1, w - 1);
    t00[k] = p.m[k] + (((long long)n * h + y0) * w + x0) * p.C;
    d01[k] = (x1 - x0) * p.C;
    d10[k] = (y1 - y0) * w * p.C;
    d11[k] = d10[k] + d01[k];
    h0[k] = p.wy[2 * ty]; h1[k] = p.wy[2 * ty + 1];
    w0[k] = p.wx[2 * tx]; w1[k] = p.wx[2 * tx + 1];
  }
  float bv = 0.f;
  int bi = 0;
  float* avg = p.avg ? p.avg + (long long)i * p.C : nullptr;
  for (int c = 0; c < p.C; ++c) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      const float* q = t00[k] + c;
      const float v = bilerp(q[0], q[d01[k]], q[d10[k]], q[d11[k]], w0[k], w1[k], h0[k], h1[k]);
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

// ------------------------------------------------------------------------------------------ confusion matrix
// conf[t][p] over the pixels with 0 <= t < C, t != ignore_index and p < C.  No atomics: a block turns a chunk of SC_CHUNK pixels
// into 16-bit keys t * C + p in LDS (0xFFFF: not counted), then thread j counts the keys equal to j (and to j + 256, ... in
// further passes) by reading every key - LDS broadcasts, 8 keys per read.  part [blocks][C*C] int32 are the blocks' counts; the
// finish adds them in block order into int64.
constexpr int SC_CHUNK = 4096;
constexpr int SC_MAX_BLOCKS = 1024;

template <typename T>
__global__ __launch_bounds__(256) void seg_confusion_part_kernel(const unsigned char* __restrict__ pred, const T* __restrict__ target, long long P,
                                                                 int C, int ignore_index, int* __restrict__ part) {
  __shared__ uint4 keys4[SC_CHUNK / 8];
  unsigned short* keys = (unsigned short*)keys4;
  const int bins = C * C;
  const long long chunks = (P + SC_CHUNK - 1) / SC_CHUNK;
  for (int base = 0; base < bins; base += 256) {
    const unsigned mine = base + threadIdx.x;           // < 65536; a bin beyond C*C matches no key but 0xFFFF, which C <= 255 excludes
    int count = 0;
    for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
      __syncthreads();
      for (int j = threadIdx.x; j < SC_CHUNK; j += 256) {
        const long long q = ch * SC_CHUNK + j;
        unsigned short key = 0xFFFF;
        if (q < P) {
          const long long t = (long long)target[q];
          const int pr = pred[q];
          if (t >= 0 && t < C && t != ignore_index && pr < C) key = (unsigned short)(t * C + pr);
        }
        keys[j] = key;
      }
      __syncthreads();
      if (mine < (unsigned)bins) {
        const unsigned m2 = mine | (mine << 16);
#pragma unroll 4
        for (int j = 0; j < SC_CHUNK / 8; ++j) {
          const uint4 k = keys4[j];
          const unsigned a = k.x ^ m2, b = k.y ^ m2, c = k.z ^ m2, d = k.w ^ m2;
          count += ((a & 0xFFFFu) == 0) + ((a >> 16) == 0) + ((b & 0xFFFFu) == 0) + ((b >> 16) == 0) + ((c & 0xFFFFu) == 0) + ((c >> 16) == 0) +
                   ((d & 0xFFFFu) == 0) + ((d >> 16) == 0);
        }
      }
    }
    if (mine < (unsigned)bins) part[(long long)blockIdx.x * bins + mine] = count;
  }
}

__global__ __launch_bounds__(256) void seg_confusion_finish_kernel(const int* __restrict__ part, int blocks, int bins, long long* __restrict__ conf) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= bins) return;
  long long s = 0;
  for (int k = 0; k < blocks; ++k) s += part[(long long)k * bins + b];
  conf[b] = s;
}

int confusion_blocks(long long P) {
  const long long chunks = (P + SC_CHUNK - 1) / SC_CHUNK;
  return (int)(chunks < SC_MAX_BLOCKS ? chunks : SC_MAX_BLOCKS);
}

}  // namespace

extern "C" {

int ur_seg_prep(const float* x, float* y, int N, int C, int H, int W, int OH, int OW, const int* idx_h, const float* wt_h, const int* idx_w,
                const float* wt_w, ur_stream_t stream) {
  UR_REQUIRE(x && y && idx_h && wt_h && idx_w && wt_w, "null pointer");
  UR_REQUIRE(N >= 1 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1, "N, H, W, OH and OW must be >= 1");
  UR_REQUIRE(C == 3, "C must be 3 (RGB)");
  UR_REQUIRE((long long)N * 3 * H * W <= INT_MAX && (long long)N * 3 * OH * OW <= INT_MAX, "too many pixels: N*3*H*W and N*3*OH*OW must be below 2^31");
  const int total = N * OH * OW;                       // <= INT_MAX / 3 by the check above: far inside the launch margin
  UR_GRID_1D(blocks, total, 256);
  hipLaunchKernelGGL(seg_prep_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, total, H, W, OH, OW, idx_h, wt_h, idx_w,
                     wt_w);
  return ur::check_launch("ur_seg_prep");
}

int ur_seg_tta_argmax(const float* m0, const float* m1, const float* m2, int nmaps, int N, int C, int h0, int w0, int h1, int w1, int h2, int w2,
                      int H, int W, const int* idx_h, const float* wt_h, const int* idx_w, const float* wt_w, unsigned char* pred, float* avg,
                      ur_stream_t stream) {
  UR_REQUIRE(nmaps >= 1 && nmaps <= 3, "nmaps must be 1, 2 or 3");
  UR_REQUIRE(m0 && (nmaps < 2 || m1) && (nmaps < 3 || m2) && idx_h && wt_h && idx_w && wt_w && pred, "null pointer");
  UR_REQUIRE(N >= 1 && H >= 1 && W >= 1, "N, H and W must be >= 1");
  UR_REQUIRE(C >= 1 && C <= 255, "C must be in [1, 255]: the prediction is one byte");
  TtaArgs p = {};
  const float* maps[3] = {m0, m1, m2};
  const int hs[3] = {h0, h1, h2}, ws[3] = {w0, w1, w2};
  for (int k = 0; k < nmaps; ++k) {
    UR_REQUIRE(hs[k] >= 1 && ws[k] >= 1, "every map's h and w must be >= 1");
    UR_REQUIRE((long long)N * hs[k] * ws[k] * C <= INT_MAX, "too many elements: N*h*w*C of every map must be below 2^31");
    UR_REQUIRE((const void*)maps[k] != (const void*)avg, "a map and avg must not be the same buffer");
    p.m[k] = maps[k]; p.h[k] = hs[k]; p.w[k] = ws[k];
  }
  UR_REQUIRE((long long)N * H * W < ur::GRID_1D_LIMIT && (!avg || (long long)N * H * W * C < ur::GRID_1D_LIMIT),
             "too many pixels: N*H*W (N*H*W*C with avg) must be below 2^31 - 256");
  p.iy = idx_h; p.wy = wt_h; p.ix = idx_w; p.wx = wt_w; p.pred = pred; p.avg = avg;
  p.total = N * H * W; p.H = H; p.W = W; p.C = C;
  UR_GRID_1D(blocks, p.total, 256);
  const dim3 grid(blocks);
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof("seg_tta_argmax", 9.0 * nmaps * (double)p.total * C, (double)p.total, s);
  if (nmaps == 1) hipLaunchKernelGGL(seg_tta_argmax_kernel<1>, grid, dim3(256), 0, s, p);
  else if (nmaps == 2) hipLaunchKernelGGL(seg_tta_argmax_kernel<2>, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(seg_tta_argmax_kernel<3>, grid, dim3(256), 0, s, p);
  return ur::check_launch("ur_seg_tta_argmax");
}

long long ur_seg_confusion_ws_bytes(long long P, int C) {
  if (P < 1 || C < 1 || C > 255) return 0;
  return (long long)confusion_blocks(P) * C * C * (long long)sizeof(int);
}

int ur_seg_confusion(const unsigned char* pred, const void* target, int target_i64, long long P, int C, int ignore_index, void* ws,
                     long long ws_bytes, long long* conf, ur_stream_t stream) {
  UR_REQUIRE(pred && target && ws && conf, "null pointer");
  UR_REQUIRE(P >= 1 && P <= INT_MAX, "P must be in [1, 2^31)");
  UR_REQUIRE(C >= 1 && C <= 255, "C must be in [1, 255]");
  UR_REQUIRE(target_i64 == 0 || target_i64 == 1, "target_i64 must be 0 (uint8) or 1 (int64)");
  UR_REQUIRE(ws_bytes >= ur_seg_confusion_ws_bytes(P, C), "workspace too small: see ur_seg_confusion_ws_bytes");
  UR_REQUIRE(((uintptr_t)ws & 3) == 0, "ws must be 4-byte aligned");
  const int blocks = confusion_blocks(P), bins = C * C;
  UR_GRID_1D(finish_blocks, bins, 256);                // bins <= 255 * 255
  hipStream_t s = (hipStream_t)stream;
  if (target_i64)
    hipLaunchKernelGGL(seg_confusion_part_kernel<long long>, dim3(blocks), dim3(256), 0, s, pred, (const long long*)target, P, C, ignore_index,
                       (int*)ws);
  else
    hipLaunchKernelGGL(seg_confusion_part_kernel<unsigned char>, dim3(blocks), dim3(256), 0, s, pred, (const unsigned char*)target, P, C, ignore_index,
                       (int*)ws);
  hipLaunchKernelGGL(seg_confusion_finish_kernel, dim3(finish_blocks), dim3(256), 0, s, (const int*)ws, blocks, bins, conf);
  return ur::check_launch("ur_seg_confusion");
}

}  // extern "C"
