// RetinaNet scoring of the det output (torchvision's retinanet_resnet50_fpn_v2 in eval mode) for gfx950, exact fp32 on NHWC maps.
// The trunk and every convolution are f32_layers.hip's; what a detector adds is here: the preprocess into a zero-padded canvas, the
// FPN's `lateral + nearest(top)`, the head's GroupNorm + ReLU, and the part that is no dense layer - a thresholded top-k over the
// millions of class logits of a level (ur_det_select), the box decode (ur_det_decode) and class-aware greedy NMS (ur_det_nms).
// No global atomics (the histograms of the radix select count integers with LDS atomics inside one workgroup and are summed over
// the workgroups in a fixed order - integer sums, so the order could not matter anyway); every floating-point sum runs in a fixed
// order; nothing allocates or synchronises: the same inputs give the same bits, eagerly and under graph replay, and an image's
// result depends on that image alone.
//
// ur_det_select, per image, over L = HWA * K logits: key(v) = the order-preserving 32-bit image of v (-0 counts as +0, a NaN is
// key 0 and never a candidate); a candidate has key > key(lt).  (1) four passes of an 8-bit radix select find the k-th largest
// candidate key T: every workgroup histograms the digit of its 4096 logits whose higher digits match the prefix found so far, one
// workgroup per image adds the histograms up and walks the bins from the top.  With count <= k the cut is key(lt) itself: every
// candidate is taken.  (2) A count pass gives every workgroup its number of keys > T and == T; (3) the compaction writes the keys
// > T in index order and the first `k - above` keys == T in index order (its offsets are the sums of the counts of the workgroups
// in front of it); (4) one workgroup per image sorts the <= 1024 (key, index) pairs in LDS, (key descending, index ascending),
// and writes score = sigmoid(logit), anchor = index / K, label = index % K and the count.  Nothing is ever cut by a buffer size.
#include "common.h"

#include <climits>
#include <cmath>
#include <cstring>

namespace {

typedef unsigned long long u64;

constexpr int DS_EPB = 4096;           // logits per workgroup of the select passes: 16 tiles of 256
constexpr int DS_KMAX = 1024;          // most candidates kept per image and level: one LDS sort
constexpr int DN_MMAX = 8192;          // most candidates of an image in the NMS
constexpr int DN_T = 1024;             // threads of the NMS workgroup

__device__ __forceinline__ unsigned det_key(float v) {
  if (v != v) return 0u;
  if (v == 0.f) v = 0.f;               // -0 -> +0: equal values, equal keys
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float det_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ bool det_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and the infinities

// descending bitonic sort of a[0 .. P), P a power of two, by all `nt` threads of the workgroup (a in LDS or in global memory)
__device__ void det_bitonic_desc(u64* a, int P, int tid, int nt) {
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < (P >> 1); i += nt) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const u64 x = a[lo], y = a[hi];
        if ((x < y) == desc) {
          a[lo] = y;
          a[hi] = x;
        }
      }
    }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------ preprocess
// x NCHW [N,3,H,W] in [0,1] -> canvas NHWC [N,HP,WP,3]: (v - mean_c) / std_c, then the half-pixel bilinear resize to RH x RW (the
// tables of f32net.hp_table), zeros beyond.  One thread per canvas element.
__global__ __launch_bounds__(256) void det_prep_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int H, int W, int RH, int RW,
                                                       int HP, int WP, const int* __restrict__ iy, const float* __restrict__ wy,
                                                       const int* __restrict__ ix, const float* __restrict__ wx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = i % 3;
  int r = i / 3;
  const int ow = r % WP;
  r /= WP;
  const int oh = r % HP, n = r / HP;
  float v = 0.f;
  if (oh < RH && ow < RW) {
    const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f, sd = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
    const int y0 = iy[oh], y1 = min(y0 + 1, H - 1), x0 = ix[ow], x1 = min(x0 + 1, W - 1);
    const float* p = x + ((long long)n * 3 + c) * H * W;
    const float a = (p[(long long)y0 * W + x0] - mean) / sd, b = (p[(long long)y0 * W + x1] - mean) / sd;
    const float d = (p[(long long)y1 * W + x0] - mean) / sd, e = (p[(long long)y1 * W + x1] - mean) / sd;
    v = wy[2 * oh] * (wx[2 * ow] * a + wx[2 * ow + 1] * b) + wy[2 * oh + 1] * (wx[2 * ow] * d + wx[2 * ow + 1] * e);
  }
  y[i] = v;
}

// ------------------------------------------------------------------------------------------ FPN: a + nearest(b)
template <int V>
__global__ __launch_bounds__(256) void det_nearest_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y,
                                                              int total, int OH, int OW, int C, int h, int w, const int* __restrict__ iy,
                                                              const int* __restrict__ ix) {
  const int i = blockIdx.x * 256 + threadIdx.x;       // over N*OH*OW*(C/V)
  if (i >= total) return;
  const int cv = C / V;
  const int c = (i % cv) * V;
  int r = i / cv;
  const int ow = r % OW;
  r /= OW;
  const int oh = r % OH, n = r / OH;
  const float* src = b + (((long long)n * h + iy[oh]) * w + ix[ow]) * C + c;
  const long long o = (long long)i * V;
  if constexpr (V == 4) {
    const float4 p = *(const float4*)(a + o), q = *(const float4*)src;
    *(float4*)(y + o) = make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w);
  } else {
    y[o] = a[o] + *src;
  }
}

// ------------------------------------------------------------------------------------------ GroupNorm (+ ReLU)
// One workgroup per (image, group): the mean, then the biased variance of the centred values, both in fp64 - every thread adds its
// elements in ascending order, the 256 partial sums are added in a fixed tree - then (x - mean) * rstd * gamma + beta in fp64,
// rounded to fp32 once.  Scalar loads throughout: any 4-byte aligned pointer.
__device__ __forceinline__ double det_block_sum(double v, double* red, int t) {
  __syncthreads();                         // the previous use of red is over
  red[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void det_groupnorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y, int HW, int C, int G,
                                                            double eps, int relu) {
  __shared__ double red[256];
  const int t = threadIdx.x, g = blockIdx.x % G, n = blockIdx.x / G;
  const int cg = C / G;
  const long long cnt = (long long)HW * cg;
  const float* src = x + (long long)n * HW * C + g * cg;
  float* dst = y + (long long)n * HW * C + g * cg;
  double s = 0.0;
  for (long long e = t; e < cnt; e += 256) s += (double)src[(e / cg) * C + (e % cg)];
  const double mean = det_block_sum(s, red, t) / (double)cnt;
  s = 0.0;
  for (long long e = t; e < cnt; e += 256) {
    const double d = (double)src[(e / cg) * C + (e % cg)] - mean;
    s += d * d;
  }
  const double rstd = 1.0 / sqrt(det_block_sum(s, red, t) / (double)cnt + eps);
  for (long long e = t; e < cnt; e += 256) {
    const int c = (int)(e % cg);
    const long long o = (e / cg) * C + c;
    const float v = (float)(((double)src[o] - mean) * rstd * (double)gamma[g * cg + c] + (double)beta[g * cg + c]);
    dst[o] = relu ? __builtin_elementwise_maximum(v, 0.f) : v;      // maximum: a NaN stays
  }
}

// ------------------------------------------------------------------------------------------ select
struct SelState {                 // per image, in the workspace
  unsigned prefix;                // the digits of T found so far, in their places
  unsigned above;                 // candidates known to lie above the prefix's group
  unsigned need;                  // the rank wanted inside the group (>= 1)
  unsigned all;                   // 1: count <= k, every candidate is taken (T = key(lt), need = 0)
  unsigned total;                 // candidates of the image
  unsigned pad[3];
};

struct SelArgs {
  const float* logits;            // [N][L]
  const float* reg;               // [N][R] or null
  long long L, R;
  int B, K, k;
  unsigned klt;
  unsigned* hist;                 // [N][B][256]
  unsigned* cnt;                  // [N][B][2]
  unsigned* bad;                  // [N][B]
  SelState* st;                   // [N]
  u64* cand;                      // [N][DS_KMAX]
};

// pass = 0..3 from the top digit.  Pass 0 also looks for non-finite logits and regressions in the workgroup's share.
__global__ __launch_bounds__(256) void det_hist_kernel(SelArgs p, int pass) {
  __shared__ unsigned h[256];
  __shared__ unsigned flag;
  const int t = threadIdx.x, b = blockIdx.x, n = blockIdx.y;
  unsigned* out = p.hist + ((long long)n * p.B + b) * 256;
  const SelState st = p.st[n];
  if (pass > 0 && st.all) return;          // (uniform) nothing to refine
  h[t] = 0;
  if (t == 0) flag = 0;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
  const float* src = p.logits + (long long)n * p.L;
  const long long e0 = (long long)b * DS_EPB, e1 = min(e0 + DS_EPB, p.L);
  bool bad = false;
  for (long long e = e0 + t; e < e1; e += 256) {
    const float v = src[e];
    const unsigned key = det_key(v);
    if (pass == 0) bad = bad || !det_finite(v);
    if (key > p.klt && (key & himask) == (st.prefix & himask)) atomicAdd(&h[(key >> shift) & 255u], 1u);
  }
  if (pass == 0 && p.reg) {
    const long long per = (p.R + p.B - 1) / p.B;
    const long long r0 = (long long)b * per, r1 = min(r0 + per, p.R);
    const float* rs = p.reg + (long long)n * p.R;
    for (long long e = r0 + t; e < r1; e += 256) bad = bad || !det_finite(rs[e]);
  }
  if (pass == 0 && bad) flag = 1;           // (a benign race: every writer stores 1)
  __syncthreads();
  out[t] = h[t];
  if (pass == 0 && t == 0) p.bad[(long long)n * p.B + b] = flag;
}

// one workgroup per image: add the workgroups' histograms (bin t by thread t, workgroups ascending) and pick the digit
__global__ __launch_bounds__(256) void det_pick_kernel(SelArgs p, int pass) {
  __shared__ unsigned h[256];
  const int t = threadIdx.x, n = blockIdx.x;
  SelState st = p.st[n];
  if (pass > 0 && st.all) return;
  const unsigned* src = p.hist + (long long)n * p.B * 256 + t;
  unsigned s = 0;
  for (int b = 0; b < p.B; ++b) s += src[(long long)b * 256];
  h[t] = s;
  __syncthreads();
  if (t != 0) return;
  if (pass == 0) {
    unsigned total = 0;
    for (int d = 0; d < 256; ++d) total += h[d];
    st.prefix = 0; st.above = 0; st.need = (unsigned)p.k; st.total = total;
    st.all = total <= (unsigned)p.k;
    if (st.all) {
      st.prefix = p.klt; st.above = total; st.need = 0;
      p.st[n] = st;
      return;
    }
  }
  unsigned cum = 0;
  int d = 255;
  for (; d > 0; --d) {
    if (cum + h[d] >= st.need) break;
    cum += h[d];
  }
  st.prefix |= (unsigned)d << (24 - 8 * pass);
  st.above += cum;
  st.need -= cum;
  p.st[n] = st;
}

__global__ __launch_bounds__(256) void det_count_kernel(SelArgs p) {
  __shared__ unsigned c[2];
  const int t = threadIdx.x, b = blockIdx.x, n = blockIdx.y;
  if (t < 2) c[t] = 0;
  __syncthreads();
  const unsigned T = p.st[n].prefix;
  const float* src = p.logits + (long long)n * p.L;
  const long long e0 = (long long)b * DS_EPB, e1 = min(e0 + DS_EPB, p.L);
  unsigned gt = 0, eq = 0;
  for (long long e = e0 + t; e < e1; e += 256) {
    const unsigned key = det_key(src[e]);
    gt += key > T;
    eq += key == T;
  }
  if (gt) atomicAdd(&c[0], gt);
  if (eq) atomicAdd(&c[1], eq);
  __syncthreads();
  if (t < 2) p.cnt[((long long)n * p.B + b) * 2 + t] = c[t];
}

// the keys > T, and the first `need` keys == T, in index order -> cand[n][0 .. above + need)
__global__ __launch_bounds__(256) void det_compact_kernel(SelArgs p) {
  __shared__ unsigned base[2];
  __shared__ unsigned wsum[4][2];
  const int t = threadIdx.x, b = blockIdx.x, n = blockIdx.y, lane = t & 63, wave = t >> 6;
  const SelState st = p.st[n];
  const unsigned* cnt = p.cnt + (long long)n * p.B * 2;
  if (cnt[2 * b] == 0 && (st.need == 0 || cnt[2 * b + 1] == 0)) return;       // (uniform) nothing of this workgroup is taken
  if (t < 2) base[t] = 0;
  __syncthreads();
  unsigned g = 0, q = 0;
  for (int j = t; j < b; j += 256) {
    g += cnt[2 * j];
    q += cnt[2 * j + 1];
  }
  if (g) atomicAdd(&base[0], g);
  if (q) atomicAdd(&base[1], q);
  __syncthreads();
  unsigned pos_gt = base[0], pos_eq = base[1];
  const unsigned T = st.prefix;
  const float* src = p.logits + (long long)n * p.L;
  u64* dst = p.cand + (long long)n * DS_KMAX;
  const long long e0 = (long long)b * DS_EPB, e1 = min(e0 + DS_EPB, p.L);
  for (long long t0 = e0; t0 < e1; t0 += 256) {
    const long long e = t0 + t;
    const unsigned key = e < e1 ? det_key(src[e]) : 0u;
    const bool is_gt = e < e1 && key > T, is_eq = e < e1 && key == T && st.need > 0;
    const u64 mg = __ballot(is_gt), me = __ballot(is_eq);
    const u64 below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    if (lane == 0) {
      wsum[wave][0] = (unsigned)__popcll(mg);
      wsum[wave][1] = (unsigned)__popcll(me);
    }
    __syncthreads();
    unsigned og = pos_gt + (unsigned)__popcll(mg & below), oe = pos_eq + (unsigned)__popcll(me & below);
    unsigned tg = 0, te = 0;
    for (int w2 = 0; w2 < 4; ++w2) {
      if (w2 < wave) {
        og += wsum[w2][0];
        oe += wsum[w2][1];
      }
      tg += wsum[w2][0];
      te += wsum[w2][1];
    }
    const u64 item = ((u64)key << 32) | (u64)(0xffffffffu - (unsigned)e);
    if (is_gt && og < (unsigned)p.k) dst[og] = item;
    if (is_eq && oe < st.need && st.above + oe < (unsigned)p.k) dst[st.above + oe] = item;
    pos_gt += tg;
    pos_eq += te;
    __syncthreads();                       // wsum is rewritten by the next tile
  }
}

// one workgroup per image: sort, write the candidates, their count and the image's non-finite flag
__global__ __launch_bounds__(256) void det_sort_kernel(SelArgs p, float* __restrict__ scores, int* __restrict__ anchors, int* __restrict__ labels,
                                                       int* __restrict__ index, int ld, int* __restrict__ counts, int* __restrict__ nonfinite) {
  __shared__ u64 a[DS_KMAX];
  __shared__ unsigned flag;
  const int t = threadIdx.x, n = blockIdx.x;
  const SelState st = p.st[n];
  const int m = (int)min(st.above + st.need, (unsigned)p.k);
  if (t == 0) flag = 0;
  const u64* src = p.cand + (long long)n * DS_KMAX;
  for (int i = t; i < DS_KMAX; i += 256) a[i] = i < m ? src[i] : 0ull;
  det_bitonic_desc(a, DS_KMAX, t, 256);
  bool bad = false;
  for (int b = t; b < p.B; b += 256) bad = bad || p.bad[(long long)n * p.B + b] != 0;
  if (bad) flag = 1;
  for (int i = t; i < p.k; i += 256) {
    const long long o = (long long)n * ld + i;
    if (i < m) {
      const unsigned idx = 0xffffffffu - (unsigned)(a[i] & 0xffffffffull);
      const double v = (double)det_unkey((unsigned)(a[i] >> 32));
      scores[o] = (float)(1.0 / (1.0 + exp(-v)));
      anchors[o] = (int)(idx / (unsigned)p.K);
      labels[o] = (int)(idx % (unsigned)p.K);
      if (index) index[o] = (int)idx;
    } else {
      scores[o] = 0.f;
      anchors[o] = 0;
      labels[o] = 0;
      if (index) index[o] = 0;
    }
  }
  __syncthreads();
  if (t == 0) {
    counts[n] = m;
    nonfinite[n] = (int)flag;
  }
}

// ------------------------------------------------------------------------------------------ decode
struct DecArgs {
  const float* reg;               // [N][HWA][4]
  const int* anchors;             // [N] rows of ld
  const int* counts;              // [N]
  const float* base;              // [A][4]
  float* raw;                     // [N] rows of ld * 4, or null
  float* clipped;
  float* scaled;
  long long HWA;
  int N, k, ld, A, WF, stride_h, stride_w;
  float img_h, img_w, ratio_h, ratio_w, clamp;
};

__global__ __launch_bounds__(256) void det_decode_kernel(DecArgs p) {
  const int i = blockIdx.x * 256 + threadIdx.x;       // over N * k
  if (i >= p.N * p.k) return;
  const int n = i / p.k, j = i % p.k;
  const long long o = ((long long)n * p.ld + j) * 4;
  float4 raw = make_float4(0.f, 0.f, 0.f, 0.f), cl = raw, sc = raw;
  if (j < p.counts[n]) {
    const int an = p.anchors[(long long)n * p.ld + j];
    const int a = an % p.A, cell = an / p.A;
    const float sx = (float)((cell % p.WF) * p.stride_w), sy = (float)((cell / p.WF) * p.stride_h);
    const float x1 = p.base[4 * a] + sx, y1 = p.base[4 * a + 1] + sy, x2 = p.base[4 * a + 2] + sx, y2 = p.base[4 * a + 3] + sy;
    const float* r = p.reg + ((long long)n * p.HWA + an) * 4;
    const float w = x2 - x1, h = y2 - y1, cx = x1 + 0.5f * w, cy = y1 + 0.5f * h;
    const float dw = fminf(r[2], p.clamp), dh = fminf(r[3], p.clamp);          // (fminf drops a NaN; the image is flagged by the select)
    const float pcx = r[0] * w + cx, pcy = r[1] * h + cy, pw = expf(dw) * w, ph = expf(dh) * h;
    const float hw = 0.5f * pw, hh = 0.5f * ph;
    raw = make_float4(pcx - hw, pcy - hh, pcx + hw, pcy + hh);
    cl = make_float4(fminf(fmaxf(raw.x, 0.f), p.img_w), fminf(fmaxf(raw.y, 0.f), p.img_h), fminf(fmaxf(raw.z, 0.f), p.img_w),
                     fminf(fmaxf(raw.w, 0.f), p.img_h));
    sc = make_float4(cl.x * p.ratio_w, cl.y * p.ratio_h, cl.z * p.ratio_w, cl.w * p.ratio_h);
  }
  if (p.raw) *(float4*)(p.raw + o) = raw;
  *(float4*)(p.clipped + o) = cl;
  *(float4*)(p.scaled + o) = sc;
}

// ------------------------------------------------------------------------------------------ NMS
struct NmsArgs {
  const float* boxes;             // [N][M][4], what the IoUs are taken of
  const float* out_boxes;         // [N][M][4], what is written for a kept box
  const float* scores;            // [N][M]
  const int* labels;              // [N][M]
  const int* counts;              // [levels][N]: position p is a candidate when p % seg < counts[p / seg][n]
  const int* flags;               // [levels][N] or null: any set -> the image has no detections and its nonfinite flag is set
  u64* ws;                        // [N][P]
  float* y_boxes;                 // [N][D][4]
  float* y_scores;                // [N][D]
  long long* y_labels;            // [N][D]
  int* y_keep;                    // [N][D]: the kept positions
  int* y_count;                   // [N]
  int* y_nonfinite;               // [N]
  int N, M, P, seg, levels, D;
  float thresh;
};

__global__ __launch_bounds__(DN_T) void det_nms_kernel(NmsArgs p) {
#pragma clang fp contract(off)             // the IoU is formed operation by operation, as torchvision's nms forms it: no fused multiply-add
  __shared__ unsigned char sup[DN_MMAX];
  __shared__ int wmin[DN_T / 64];
  __shared__ int s_cur;
  const int t = threadIdx.x, n = blockIdx.x, lane = t & 63, wave = t >> 6;
  u64* a = p.ws + (long long)n * p.P;
  const float* sc = p.scores + (long long)n * p.M;
  const int* lb = p.labels + (long long)n * p.M;
  const float4* bx = (const float4*)p.boxes + (long long)n * p.M;
  const float4* obx = (const float4*)p.out_boxes + (long long)n * p.M;
  bool bad = false;
  int V = 0;
  for (int l = 0; l < p.levels; ++l) {
    V += min(max(p.counts[(long long)l * p.N + n], 0), max(min(p.seg, p.M - l * p.seg), 0));
    if (p.flags) bad = bad || p.flags[(long long)l * p.N + n] != 0;
  }
  for (int i = t; i < p.P; i += DN_T) {
    u64 item = 0ull;
    if (i < p.M && (i % p.seg) < p.counts[(long long)(i / p.seg) * p.N + n]) {
      const unsigned key = det_key(sc[i]);
      item = ((u64)key << 32) | (u64)(0xffffffffu - (unsigned)i);
    }
    a[i] = item;
    if (i < DN_MMAX) sup[i] = 0;
  }
  det_bitonic_desc(a, p.P, t, DN_T);
  if (bad) V = 0;
  // greedy: `cur` walks the sorted list; a kept box marks what it suppresses behind it, then the first unmarked one is next
  int kept = 0, cur = 0;
  while (cur < V && kept < p.D) {
    const int pc = (int)(0xffffffffu - (unsigned)(a[cur] & 0xffffffffull));
    const float4 bc = bx[pc];
    const int lc = lb[pc];
    if (t == 0) {
      const long long o = (long long)n * p.D + kept;
      *((float4*)p.y_boxes + o) = obx[pc];
      p.y_scores[o] = sc[pc];
      p.y_labels[o] = (long long)lc;
      p.y_keep[o] = pc;
    }
    ++kept;
    const float area_c = (bc.z - bc.x) * (bc.w - bc.y);
    int next = V;
    for (int j = cur + 1 + t; j < V; j += DN_T) {
      if (sup[j]) continue;
      const int pj = (int)(0xffffffffu - (unsigned)(a[j] & 0xffffffffull));
      if (lb[pj] == lc) {
        const float4 bj = bx[pj];
        const float iw = fmaxf(fminf(bc.z, bj.z) - fmaxf(bc.x, bj.x), 0.f), ih = fmaxf(fminf(bc.w, bj.w) - fmaxf(bc.y, bj.y), 0.f);
        const float inter = iw * ih, area_j = (bj.z - bj.x) * (bj.w - bj.y);
        if (inter / (area_c + area_j - inter) > p.thresh) {
          sup[j] = 1;
          continue;
        }
      }
      next = min(next, j);                 // the thread goes on: every surviving position behind the kept box is compared with it
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) next = min(next, __shfl_xor(next, o, 64));
    if (lane == 0) wmin[wave] = next;
    __syncthreads();
    if (t == 0) {
      int m = wmin[0];
      for (int w2 = 1; w2 < DN_T / 64; ++w2) m = min(m, wmin[w2]);
      s_cur = m;
    }
    __syncthreads();
    cur = s_cur;
    __syncthreads();                       // s_cur and wmin are rewritten by the next round
  }
  for (int i = kept + t; i < p.D; i += DN_T) {
    const long long o = (long long)n * p.D + i;
    *((float4*)p.y_boxes + o) = make_float4(0.f, 0.f, 0.f, 0.f);
    p.y_scores[o] = 0.f;
    p.y_labels[o] = 0;
    p.y_keep[o] = -1;
  }
  if (t == 0) {
    p.y_count[n] = kept;
    p.y_nonfinite[n] = bad ? 1 : 0;
  }
}

int det_pow2(int m) {
  int p = 2;
  while (p < m) p <<= 1;
  return p;
}

long long det_align16(long long v) { return (v + 15) / 16 * 16; }

}  // namespace

extern "C" {

int ur_det_prep(const float* x, float* y, int N, int H, int W, int RH, int RW, int HP, int WP, const int32_t* iy, const float* wy,
                const int32_t* ix, const float* wx, ur_stream_t stream) {
  UR_REQUIRE(x && y && iy && wy && ix && wx, "null pointer");
  UR_REQUIRE(x != y, "x and y must not be the same buffer");
  UR_REQUIRE(N >= 1 && H >= 1 && W >= 1, "N, H and W must be >= 1");
  UR_REQUIRE(RH >= 1 && RW >= 1 && HP >= RH && WP >= RW, "the canvas must hold the resized image: 1 <= RH <= HP, 1 <= RW <= WP");
  UR_REQUIRE((long long)N * 3 * H * W < ur::GRID_1D_LIMIT && (long long)N * 3 * HP * WP < ur::GRID_1D_LIMIT,
             "too many elements: N*3*H*W and N*3*HP*WP must be below 2^31 - 256");
  const int total = N * 3 * HP * WP;
  UR_GRID_1D(blocks, total, 256);
  hipLaunchKernelGGL(det_prep_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, total, H, W, RH, RW, HP, WP, iy, wy, ix, wx);
  return ur::check_launch("ur_det_prep");
}

int ur_upsample_nearest_add_f32(const float* a, const float* b, float* y, int N, int OH, int OW, int C, int h, int w, const int32_t* iy,
                                const int32_t* ix, ur_stream_t stream) {
  UR_REQUIRE(a && b && y && iy && ix, "null pointer");
  UR_REQUIRE(b != y && a != y, "y must be a buffer of its own");
  UR_REQUIRE(N >= 1 && OH >= 1 && OW >= 1 && C >= 1 && h >= 1 && w >= 1, "every size must be >= 1");
  UR_REQUIRE((long long)N * OH * OW * C < ur::GRID_1D_LIMIT && (long long)N * h * w * C < ur::GRID_1D_LIMIT,
             "too many elements: N*OH*OW*C and N*h*w*C must be below 2^31 - 256");
  hipStream_t s = (hipStream_t)stream;
  if (C % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)y) & 15) == 0) {
    const int total = N * OH * OW * (C / 4);
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(det_nearest_add_kernel<4>, dim3(blocks), dim3(256), 0, s, a, b, y, total, OH, OW, C, h, w, iy, ix);
  } else {
    const int total = N * OH * OW * C;
    UR_GRID_1D(blocks, total, 256);
    hipLaunchKernelGGL(det_nearest_add_kernel<1>, dim3(blocks), dim3(256), 0, s, a, b, y, total, OH, OW, C, h, w, iy, ix);
  }
  return ur::check_launch("ur_upsample_nearest_add_f32");
}

int ur_groupnorm_relu_f32(const float* x, const float* gamma, const float* beta, float* y, int N, int HW, int C, int G, double eps, int relu,
                          ur_stream_t stream) {
  UR_REQUIRE(x && gamma && beta && y, "null pointer");
  UR_REQUIRE(N >= 1 && HW >= 1 && C >= 1 && G >= 1, "N, HW, C and G must be >= 1");
  UR_REQUIRE(C % G == 0, "C must be a multiple of G");
  UR_REQUIRE(x != y, "x and y must not be the same buffer");
  UR_REQUIRE(eps > 0.0, "eps must be positive");
  UR_REQUIRE(relu == 0 || relu == 1, "relu must be 0 or 1");
  UR_REQUIRE((long long)N * HW * C < ur::GRID_1D_LIMIT && (long long)N * G < ur::GRID_1D_LIMIT,
             "too many elements: N*HW*C must be below 2^31 - 256");
  UR_REQUIRE((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 3) == 0, "the pointers must be 4-byte aligned");
  hipLaunchKernelGGL(det_groupnorm_kernel, dim3((unsigned)(N * G)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, HW, C, G, eps, relu);
  return ur::check_launch("ur_groupnorm_relu_f32");
}

int ur_det_select_kmax(void) { return DS_KMAX; }

long long ur_det_select_ws_bytes(int N, long long L) {
  if (N < 1 || L < 1 || L >= ur::GRID_1D_LIMIT) return 0;
  const long long B = (L + DS_EPB - 1) / DS_EPB;
  if (N * B >= ur::GRID_1D_LIMIT) return 0;
  return det_align16(4ll * N * B * 256) + det_align16(8ll * N * B) + det_align16(4ll * N * B) + det_align16((long long)sizeof(SelState) * N) +
         8ll * N * DS_KMAX;
}

int ur_det_select(const float* logits, const float* reg, int N, long long HWA, int K, float lt, int k, float* scores, int32_t* anchors,
                  int32_t* labels, int32_t* index, int ld, int32_t* counts, int32_t* nonfinite, void* ws, long long ws_bytes, ur_stream_t stream) {
  UR_REQUIRE(logits && scores && anchors && labels && counts && nonfinite && ws, "null pointer");
  UR_REQUIRE(N >= 1 && N <= 65535 && HWA >= 1 && K >= 1, "N must be in [1, 65535], HWA and K >= 1");
  UR_REQUIRE(k >= 1 && k <= DS_KMAX, "k must be in [1, 1024]");
  UR_REQUIRE(ld >= k, "ld must be >= k");
  UR_REQUIRE(lt == lt, "lt must not be NaN");
  UR_REQUIRE(HWA < ur::GRID_1D_LIMIT / K, "too many logits: HWA*K must be below 2^31 - 256");
  const long long L = HWA * K;
  const long long need = ur_det_select_ws_bytes(N, L);
  UR_REQUIRE(need > 0, "too many logits: N * ceil(HWA*K / 4096) must be below 2^31 - 256");
  UR_REQUIRE(ws_bytes >= need, "the workspace is smaller than ur_det_select_ws_bytes(N, HWA*K)");
  UR_REQUIRE(((uintptr_t)ws & 15) == 0, "ws must be 16-byte aligned");
  UR_REQUIRE((((uintptr_t)logits | (uintptr_t)reg | (uintptr_t)scores | (uintptr_t)anchors | (uintptr_t)labels | (uintptr_t)index |
               (uintptr_t)counts | (uintptr_t)nonfinite) & 3) == 0, "the pointers must be 4-byte aligned");
  const long long B = (L + DS_EPB - 1) / DS_EPB;
  SelArgs p;
  p.logits = logits; p.reg = reg; p.L = L; p.R = HWA * 4; p.B = (int)B; p.K = K; p.k = k;
  {
    float z = lt == 0.f ? 0.f : lt;
    unsigned u;
    memcpy(&u, &z, 4);
    p.klt = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  char* w = reinterpret_cast<char*>(ws);
  p.hist = reinterpret_cast<unsigned*>(w); w += det_align16(4ll * N * B * 256);
  p.cnt = reinterpret_cast<unsigned*>(w); w += det_align16(8ll * N * B);
  p.bad = reinterpret_cast<unsigned*>(w); w += det_align16(4ll * N * B);
  p.st = reinterpret_cast<SelState*>(w); w += det_align16((long long)sizeof(SelState) * N);
  p.cand = reinterpret_cast<u64*>(w);
  hipStream_t s = (hipStream_t)stream;
  ur::zero_async(p.st, (size_t)det_align16((long long)sizeof(SelState) * N), s);
  const dim3 grid((unsigned)B, (unsigned)N);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(det_hist_kernel, grid, dim3(256), 0, s, p, pass);
    hipLaunchKernelGGL(det_pick_kernel, dim3((unsigned)N), dim3(256), 0, s, p, pass);
  }
  hipLaunchKernelGGL(det_count_kernel, grid, dim3(256), 0, s, p);
  hipLaunchKernelGGL(det_compact_kernel, grid, dim3(256), 0, s, p);
  hipLaunchKernelGGL(det_sort_kernel, dim3((unsigned)N), dim3(256), 0, s, p, scores, anchors, labels, index, ld, counts, nonfinite);
  return ur::check_launch("ur_det_select");
}

int ur_det_decode(const float* reg, const int32_t* anchors, const int32_t* counts, const float* base, float* raw, float* clipped,
                  float* scaled, int N, long long HWA, int k, int ld, int A, int WF, int stride_h, int stride_w, float img_h, float img_w,
                  float ratio_h, float ratio_w, ur_stream_t stream) {
  UR_REQUIRE(reg && anchors && counts && base && clipped && scaled, "null pointer");
  UR_REQUIRE(N >= 1 && HWA >= 1 && k >= 1 && ld >= k && A >= 1 && WF >= 1, "N, HWA, k, A and WF must be >= 1 and ld >= k");
  UR_REQUIRE(HWA % ((long long)A * WF) == 0, "HWA must be a multiple of A * WF");
  UR_REQUIRE(stride_h >= 1 && stride_w >= 1, "the strides must be >= 1");
  UR_REQUIRE(HWA / A / WF * (long long)stride_h < (1 << 24) && (long long)WF * stride_w < (1 << 24), "the canvas must be below 2^24 pixels a side");
  UR_REQUIRE((long long)N * ld < ur::GRID_1D_LIMIT / 4, "too many candidates: N*ld*4 must be below 2^31 - 256");
  UR_REQUIRE((((uintptr_t)raw | (uintptr_t)clipped | (uintptr_t)scaled) & 15) == 0, "raw, clipped and scaled must be 16-byte aligned");
  DecArgs p;
  p.reg = reg; p.anchors = anchors; p.counts = counts; p.base = base; p.raw = raw; p.clipped = clipped; p.scaled = scaled;
  p.HWA = HWA; p.N = N; p.k = k; p.ld = ld; p.A = A; p.WF = WF; p.stride_h = stride_h; p.stride_w = stride_w;
  p.img_h = img_h; p.img_w = img_w; p.ratio_h = ratio_h; p.ratio_w = ratio_w;
  p.clamp = (float)std::log(1000.0 / 16.0);
  UR_GRID_1D(blocks, (long long)N * k, 256);
  hipLaunchKernelGGL(det_decode_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
  return ur::check_launch("ur_det_decode");
}

int ur_det_nms_mmax(void) { return DN_MMAX; }

long long ur_det_nms_ws_bytes(int N, int M) {
  if (N < 1 || M < 0 || M > DN_MMAX) return 0;
  return 8ll * N * det_pow2(M);
}

int ur_det_nms(const float* boxes, const float* out_boxes, const float* scores, const int32_t* labels, const int32_t* counts,
               const int32_t* flags, int N, int M, int seg, int levels, float thresh, int D, float* y_boxes, float* y_scores,
               long long* y_labels, int32_t* y_keep, int32_t* y_count, int32_t* y_nonfinite, void* ws, long long ws_bytes, ur_stream_t stream) {
  UR_REQUIRE(counts && y_boxes && y_scores && y_labels && y_keep && y_count && y_nonfinite && ws, "null pointer");
  UR_REQUIRE(N >= 1 && M >= 0 && M <= DN_MMAX, "N must be >= 1 and M in [0, 8192]");
  UR_REQUIRE(M == 0 || (boxes && out_boxes && scores && labels), "null pointer");
  UR_REQUIRE(seg >= 1 && levels >= 1 && (long long)seg * levels >= M, "seg and levels must be >= 1 and seg * levels >= M");
  UR_REQUIRE(D >= 1 && (long long)N * D < ur::GRID_1D_LIMIT / 4, "D must be >= 1 and N*D*4 below 2^31 - 256");
  UR_REQUIRE(thresh == thresh, "thresh must not be NaN");
  UR_REQUIRE(ws_bytes >= ur_det_nms_ws_bytes(N, M), "the workspace is smaller than ur_det_nms_ws_bytes(N, M)");
  UR_REQUIRE((((uintptr_t)boxes | (uintptr_t)out_boxes | (uintptr_t)y_boxes) & 15) == 0, "boxes, out_boxes and y_boxes must be 16-byte aligned");
  UR_REQUIRE((((uintptr_t)ws | (uintptr_t)y_labels) & 7) == 0, "ws and y_labels must be 8-byte aligned");
  NmsArgs p;
  p.boxes = boxes; p.out_boxes = out_boxes; p.scores = scores; p.labels = labels; p.counts = counts; p.flags = flags;
  p.ws = reinterpret_cast<u64*>(ws); p.y_boxes = y_boxes; p.y_scores = y_scores; p.y_labels = y_labels; p.y_keep = y_keep;
  p.y_count = y_count; p.y_nonfinite = y_nonfinite;
  p.N = N; p.M = M; p.P = det_pow2(M); p.seg = seg; p.levels = levels; p.D = D; p.thresh = thresh;
  hipLaunchKernelGGL(det_nms_kernel, dim3((unsigned)N), dim3(DN_T), 0, (hipStream_t)stream, p);
  return ur::check_launch("ur_det_nms");
}

}  // extern "C"
