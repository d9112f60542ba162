// The segmenters' own kernels for gfx950, exact fp32, for both networks the seg task is scored with - RefineNet-LW and
// DeepLabV3+: one scale of the evaluator's test-time augmentation fused with the network's preprocess (bilinear
// align_corners=True resize, NCHW in, NHWC out; then v * 255 - mean, RGB -> BGR for RefineNet-LW, the ImageNet (v - mean) / std
// for DeepLabV3+), the multi-scale average + argmax that ends the metric (one-stage for RefineNet-LW, whose logits the evaluator
// resizes once; two-stage for DeepLabV3+, whose own half-pixel resize comes first), and the confusion matrix of the mIoU.  The
// convolutions (dilated and into a channel slice for DeepLabV3+), the heads' bilinear resizes, the pools, the broadcast and a + b
// are in f32_layers.hip; the bilinear sample and its axis tables are f32_layers.h's.  No atomics; every sum runs in a fixed
// order, so the same inputs give the same bits on every run, eagerly and under graph replay, and an image's results do not
// depend on its place in the batch.
#include "common.h"
#include "f32_layers.h"

#include <climits>
#include <cmath>

namespace {

// A refusal from a launcher or a check that two entry points share: `who` names the export.
#define SEG_REQUIRE(cond, msg)                                                     \
  do {                                                                             \
    if (!(cond)) return ur::fail(UR_E_INVALID, std::string(who) + ": " + (msg));  \
  } while (0)

// ------------------------------------------------------------------------------------------ TTA scale + preprocess
// What a network does to the resized value v of source channel c (0, 1, 2 = R, G, B): the value, and in *oc the output channel.
// RefineNet-LW: v * 255 - mean with two roundings, as torch computes x * 255 - mean (never contracted into one fma), into
// channel 2 - c (BGR).
struct RflwPreprocess {
  __device__ __forceinline__ float operator()(float v, int c, int* oc) const {
#pragma clang fp contract(off)
    const float mean[3] = {123.68f, 116.779f, 103.939f};
    const float t = v * 255.f;
    *oc = 2 - c;
    return t - mean[c];
  }
};

// DeepLabV3+: (v - mean) / std with two roundings and a true division, as torchvision's Normalize computes sub_(mean).div_(std),
// into channel c.
struct Dlv3Preprocess {
  __device__ __forceinline__ float operator()(float v, int c, int* oc) const {
#pragma clang fp contract(off)
    const float mean[3] = {0.485f, 0.456f, 0.406f}, std[3] = {0.229f, 0.224f, 0.225f};
    const float t = v - mean[c];
    *oc = c;
    return __fdiv_rn(t, std[c]);
  }
};

// x [N][3][H][W] in [0,1] -> y [N][OH][OW][3]: every channel resized with the axis tables, then through the network's functor.
template <class Preprocess>
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
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* src = x + ((long long)n * 3 + c) * H * W;
    const float v = bilerp(src[y0 * W + x0], src[y0 * W + x1], src[y1 * W + x0], src[y1 * W + x1], w0, w1, h0, h1);
    int oc;
    const float o = Preprocess()(v, c, &oc);
    y[(long long)i * 3 + oc] = o;
  }
}

template <class Preprocess>
int prep_launch(const char* who, const float* x, float* y, int N, int C, int H, int W, int OH, int OW, const int* idx_h, const float* wt_h,
                const int* idx_w, const float* wt_w, ur_stream_t stream) {
  SEG_REQUIRE(x && y && idx_h && wt_h && idx_w && wt_w, "null pointer");
  SEG_REQUIRE(N >= 1 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1, "N, H, W, OH and OW must be >= 1");
  SEG_REQUIRE(C == 3, "C must be 3 (RGB)");
  SEG_REQUIRE((long long)N * 3 * H * W <= INT_MAX && (long long)N * 3 * OH * OW <= INT_MAX, "too many pixels: N*3*H*W and N*3*OH*OW must be below 2^31");
  const int total = N * OH * OW;                       // <= INT_MAX / 3 by the check above: far inside the launch margin
  unsigned blocks = 0;
  if (int rc = ur::grid_1d(who, total, 256, &blocks)) return rc;
  hipLaunchKernelGGL(seg_prep_kernel<Preprocess>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, total, H, W, OH, OW, idx_h, wt_h,
                     idx_w, wt_w);
  return ur::check_launch(who);
}

// ------------------------------------------------------------------------------------------ multi-scale average + argmax
// One thread per output pixel.  For every class, in ascending order: sample each of the NM maps bilinearly, average them as
// ((a + b) + c) / NM and keep the running best - a larger value, or a NaN when no NaN was seen yet; an equal value never replaces
// an earlier class (torch.argmax: ties to the lowest index, NaN is the maximum, the first one wins).  The four tap offsets and
// weights of every map stay in registers; a wave's 64 neighbouring pixels read a few neighbouring source pixels, whose C
// consecutive floats they walk together, so the maps are served from L1 / L2 and the only HBM traffic is the byte written.
// DeepLabV3+'s two-stage kernel below ends in the same step; the two share it and the pixel decode, and stay two kernels: the
// one-stage one is 3 - 4 times faster.

// Output pixel i of [N][H][W] -> its column, row and image.
__device__ __forceinline__ void tta_pixel(int i, int H, int W, int* ox, int* oy, int* n) {
  *ox = i % W;
  const int r = i / W;
  *oy = r % H;
  *n = r / H;
}

// Class c of one pixel, v[k] its value in scale k: the average ((v0 + v1) + v2) / NM, stored when avg is given, and the running
// best (bv, bi).
template <int NM>
__device__ __forceinline__ void tta_class(const float (&v)[NM], int c, float* avg, float* bv, int* bi) {
  float s = v[0];
#pragma unroll
  for (int k = 1; k < NM; ++k) s = __fadd_rn(s, v[k]);
  s = __fdiv_rn(s, (float)NM);
  if (avg) avg[c] = s;
  const bool sn = s != s, bn = *bv != *bv;
  if (c == 0 || (!bn && (sn || s > *bv))) {
    *bv = s;
    *bi = c;
  }
}

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
  int ox, oy, n;
  tta_pixel(i, p.H, p.W, &ox, &oy, &n);
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
    float v[NM];
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      const float* q = t00[k] + c;
      v[k] = bilerp(q[0], q[d01[k]], q[d10[k]], q[d11[k]], w0[k], w1[k], h0[k], h1[k]);
    }
    tta_class<NM>(v, c, avg, &bv, &bi);
  }
  p.pred[i] = (unsigned char)bi;
}

// ------------------------------------------------------------------------------------------ two-stage multi-scale average + argmax
// One thread per output pixel.  Scale k's classifier map q_k [N][hq][wq][C] is first resized to the scale's network input (hs, ws)
// with half-pixel centres (L_k, the model's own align_corners=False resize), and L_k to the output (H, W) with align_corners=True
// (U_k, the evaluator's).  Neither L_k nor U_k is stored: the output pixel's align_corners=True sample touches L_k at rows Y0, Y1
// and columns X0, X1, and each of those four values is the half-pixel sample of q_k at rows (Y -> y0, y1) and columns
// (X -> x0, x1).  Both samples are `bilerp` in fp32, in its operand order; the scales are averaged and the best class kept by
// `tta_class`, as in seg_tta_argmax_kernel.
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
  int ox, oy, n;
  tta_pixel(i, p.H, p.W, &ox, &oy, &n);
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
    float v[NM];
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
      v[k] = bilerp(L[0][0], L[0][1], L[1][0], L[1][1], W0[k], W1[k], H0[k], H1[k]);
    }
    tta_class<NM>(v, c, avg, &bv, &bi);
  }
  p.pred[i] = (unsigned char)bi;
}

// What both argmax entry points refuse, in one order.  tables: no table pointer is null.  mh, mw: every map's own height and
// width, `area` their names in the message; dims_ok[k]: all of map k's sizes are >= 1, `dims` their names.
int tta_check(const char* who, int nmaps, const float* const* maps, bool tables, const unsigned char* pred, const float* avg, int N, int C,
              int H, int W, const int* mh, const int* mw, const char* area, const bool* dims_ok, const char* dims) {
  SEG_REQUIRE(nmaps >= 1 && nmaps <= 3, "nmaps must be 1, 2 or 3");
  SEG_REQUIRE(maps[0] && (nmaps < 2 || maps[1]) && (nmaps < 3 || maps[2]) && tables && pred, "null pointer");
  SEG_REQUIRE(N >= 1 && H >= 1 && W >= 1, "N, H and W must be >= 1");
  SEG_REQUIRE(C >= 1 && C <= 255, "C must be in [1, 255]: the prediction is one byte");
  for (int k = 0; k < nmaps; ++k) {
    SEG_REQUIRE(dims_ok[k], std::string("every map's ") + dims + " must be >= 1");
    SEG_REQUIRE((long long)N * mh[k] * mw[k] * C <= INT_MAX, std::string("too many elements: N*") + area + "*C of every map must be below 2^31");
    SEG_REQUIRE((const void*)maps[k] != (const void*)avg, "a map and avg must not be the same buffer");
  }
  SEG_REQUIRE((long long)N * H * W < ur::GRID_1D_LIMIT && (!avg || (long long)N * H * W * C < ur::GRID_1D_LIMIT),
              "too many pixels: N*H*W (N*H*W*C with avg) must be below 2^31 - 256");
  return 0;
}

// The launch both entry points end in: kernels[nmaps - 1] over p.total pixels; flop: the profile's count per map, pixel and class.
template <class Args>
int tta_launch(const char* who, const char* prof_name, double flop, void (*const (&kernels)[3])(Args), int nmaps, const Args& p,
               ur_stream_t stream) {
  unsigned blocks = 0;
  if (int rc = ur::grid_1d(who, p.total, 256, &blocks)) return rc;
  hipStream_t s = (hipStream_t)stream;
  ur::ProfScope prof(prof_name, flop * nmaps * (double)p.total * p.C, (double)p.total, s);
  hipLaunchKernelGGL(kernels[nmaps - 1], dim3(blocks), dim3(256), 0, s, p);
  return ur::check_launch(who);
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

#undef SEG_REQUIRE

}  // namespace

extern "C" {

int ur_seg_prep(const float* x, float* y, int N, int C, int H, int W, int OH, int OW, const int* idx_h, const float* wt_h, const int* idx_w,
                const float* wt_w, ur_stream_t stream) {
  return prep_launch<RflwPreprocess>("ur_seg_prep", x, y, N, C, H, W, OH, OW, idx_h, wt_h, idx_w, wt_w, stream);
}

int ur_dlv3_prep(const float* x, float* y, int N, int C, int H, int W, int OH, int OW, const int* idx_h, const float* wt_h, const int* idx_w,
                 const float* wt_w, ur_stream_t stream) {
  return prep_launch<Dlv3Preprocess>("ur_dlv3_prep", x, y, N, C, H, W, OH, OW, idx_h, wt_h, idx_w, wt_w, stream);
}

int ur_seg_tta_argmax(const float* m0, const float* m1, const float* m2, int nmaps, int N, int C, int h0, int w0, int h1, int w1, int h2, int w2,
                      int H, int W, const int* idx_h, const float* wt_h, const int* idx_w, const float* wt_w, unsigned char* pred, float* avg,
                      ur_stream_t stream) {
  const float* maps[3] = {m0, m1, m2};
  const int hs[3] = {h0, h1, h2}, ws[3] = {w0, w1, w2};
  const bool ok[3] = {h0 >= 1 && w0 >= 1, h1 >= 1 && w1 >= 1, h2 >= 1 && w2 >= 1};
  if (int rc = tta_check("ur_seg_tta_argmax", nmaps, maps, idx_h && wt_h && idx_w && wt_w, pred, avg, N, C, H, W, hs, ws, "h*w", ok, "h and w"))
    return rc;
  TtaArgs p = {};
  for (int k = 0; k < nmaps; ++k) {
    p.m[k] = maps[k]; p.h[k] = hs[k]; p.w[k] = ws[k];
  }
  p.iy = idx_h; p.wy = wt_h; p.ix = idx_w; p.wx = wt_w; p.pred = pred; p.avg = avg;
  p.total = N * H * W; p.H = H; p.W = W; p.C = C;
  void (*const kernels[3])(TtaArgs) = {seg_tta_argmax_kernel<1>, seg_tta_argmax_kernel<2>, seg_tta_argmax_kernel<3>};
  return tta_launch("ur_seg_tta_argmax", "seg_tta_argmax", 9.0, kernels, nmaps, p, stream);
}

int ur_dlv3_tta_argmax(const float* q0, const float* q1, const float* q2, int nmaps, int N, int C, int hq0, int wq0, int hs0, int ws0, int hq1,
                       int wq1, int hs1, int ws1, int hq2, int wq2, int hs2, int ws2, int H, int W, const int* ac_idx_h, const float* ac_wt_h, const int* ac_idx_w, const float* ac_wt_w, const int* hp_idx_h,
                       const float* hp_wt_h, const int* hp_idx_w, const float* hp_wt_w, unsigned char* pred, float* avg, ur_stream_t stream) {
  const float* maps[3] = {q0, q1, q2};
  const int hq[3] = {hq0, hq1, hq2}, wq[3] = {wq0, wq1, wq2}, hs[3] = {hs0, hs1, hs2}, ws[3] = {ws0, ws1, ws2};
  bool ok[3];
  for (int k = 0; k < 3; ++k) ok[k] = hq[k] >= 1 && wq[k] >= 1 && hs[k] >= 1 && ws[k] >= 1;
  const bool tables = ac_idx_h && ac_wt_h && ac_idx_w && ac_wt_w && hp_idx_h && hp_wt_h && hp_idx_w && hp_wt_w;
  if (int rc = tta_check("ur_dlv3_tta_argmax", nmaps, maps, tables, pred, avg, N, C, H, W, hq, wq, "hq*wq", ok, "hq, wq, hs and ws")) return rc;
  Tta2Args p = {};
  long long oh = 0, ow = 0;
  for (int k = 0; k < nmaps; ++k) {
    p.q[k] = maps[k]; p.hq[k] = hq[k]; p.wq[k] = wq[k]; p.hs[k] = hs[k]; p.ws[k] = ws[k]; p.oh[k] = oh; p.ow[k] = ow;
    oh += hs[k]; ow += ws[k];
  }
  p.aiy = ac_idx_h; p.awy = ac_wt_h; p.aix = ac_idx_w; p.awx = ac_wt_w;
  p.hiy = hp_idx_h; p.hwy = hp_wt_h; p.hix = hp_idx_w; p.hwx = hp_wt_w;
  p.pred = pred; p.avg = avg;
  p.total = N * H * W; p.H = H; p.W = W; p.C = C;
  void (*const kernels[3])(Tta2Args) = {dlv3_tta_argmax_kernel<1>, dlv3_tta_argmax_kernel<2>, dlv3_tta_argmax_kernel<3>};
  return tta_launch("ur_dlv3_tta_argmax", "dlv3_tta_argmax", 45.0, kernels, nmaps, p, stream);
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
