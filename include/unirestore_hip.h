/*
 * unirestore_hip.h — C ABI of libunirestore_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for UniRestore's diffusion-prior restoration hot path
 * (DiffUIE.forward, /root/reference/src/modules/diffuie/unifie.py:107-169).  The reference has no
 * native layer: every entry point below replaces an ATen/cuDNN/cuBLAS op that the reference reaches
 * through torch.nn / diffusers.  The "replaces" notes cite the reference call sites.
 *
 * Conventions
 *   - every pointer is a DEVICE address unless marked "host"; activations are NHWC 16-bit (raw uint16 bit
 *     patterns of bf16 or fp16, chosen per call by a UR_DT_* `dtype`), statistics / tables / tiny vectors are fp32;
 *   - no kernel uses atomics: two runs (or two hipGraph replays) on the same inputs are bit-identical;
 *   - the library never allocates: workspaces are passed in by the caller;
 *   - every call is asynchronous on `stream` (a hipStream_t) and safe under hipGraph capture;
 *   - return value: 0 = UR_OK, negative = UR_E_*; ur_last_error() gives the message (thread-local).
 */
#ifndef UNIRESTORE_HIP_H
#define UNIRESTORE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ur_stream_t; /* hipStream_t */

enum { UR_OK = 0, UR_E_INVALID = -1, UR_E_UNSUPPORTED = -2, UR_E_LAUNCH = -3, UR_E_WORKSPACE = -4 };

/* 16-bit storage / matrix-core operand type of activations and weights (accumulation, statistics, softmax, the DDIM state
 * and every tiny vector are fp32 in both).  UR_DT_BF16: precision: bf16-mixed of the reference (configs/val.yaml:12);
 * UR_DT_F16: IEEE half - same bytes and MFMA rate, 8x smaller rounding error per stored tensor; a value beyond +-65504
 * overflows to +-inf (IEEE; rounds 2-4 clamped) and turns into NaN in the next normalisation / softmax, so an fp16 range
 * problem shows up in the output instead of as a silently clipped activation - fall back to UR_DT_BF16 for such weights
 * (BASELINE.json configs[4], "fp16"). */
enum { UR_DT_BF16 = 0, UR_DT_F16 = 1 };

/* epilogue activations */
enum {
  UR_ACT_NONE = 0,
  UR_ACT_SILU = 1,
  UR_ACT_GELU = 2,  /* exact erf GELU (nn.GELU default) */
  UR_ACT_GEGLU = 3, /* out[j] = a[j] * gelu(g[j]); weight rows pre-interleaved in blocks of 32 (a|g) */
  UR_ACT_GATE = 4,  /* NAFNet SimpleGate: out[j] = a[j] * g[j]; same interleave */
  UR_ACT_TANH = 5,
  UR_ACT_RELU = 6   /* SPADE's mlp_shared (spade.py:47-49) */
};

int ur_version(void);
const char* ur_last_error(void);

/* ---- implicit-GEMM convolution / linear (bf16 MFMA, fp32 accumulate) -------------------------
 * y[n,oh,ow,co] = epilogue( sum_{kh,kw,ci} x[n, ih, iw, ci] * w[co,kh,kw,ci] )
 * Replaces: nn.Conv2d 3x3/1x1 (ResnetBlock2D conv1/conv2/conv_shortcut, conv_in/out, Downsample2D,
 *   Upsample2D.conv — base_model.py:94-209, controller.py:193-220, autoencoder.py:11-72), nn.Linear
 *   (Transformer2DModel / BasicTransformerBlock / Attention projections), CSCEAdapter 1x1 convs
 *   (scedit.py:28-38), NAFBlock/AdaNAFV2 1x1 + grouped convs (nafnet_arch.py:32-95, cfrm.py:18-36),
 *   TaskFeatureAdapter convs (taskeditor.py:20-52), torch.cat on the UNet up path (base_model.py:189,197;
 *   "virtual concat": x2), F.interpolate(nearest, 2x) in Upsample2D (upsample2x).
 * Epilogue order: acc (+bias[co]) -> act -> (*out_scale) -> (+residual) -> store.
 * Batched / grouped form: blockIdx.y = b in [0,nbatch): every base pointer advances by its bs_* stride.
 * Size limits (checked in 64-bit arithmetic before any HIP call; a shape outside returns UR_E_INVALID naming ur_conv2d_nhwc):
 *   - x, x2: N*H*W*max(ldx, ldx2) must be below 2^31 elements (32-bit element offsets).  The LDS-DMA kernels read the sources
 *     through raw buffer descriptors whose byte offsets from 0xffffff00 up mean "read zero" (padding, ragged rows); the shapes
 *     they take end below that byte (whole 8 x 32 patches or 8 x 8 / 16 x 16 images: a multiple of 512 elements), the pure-GEMM
 *     LDS-DMA launchers (g1_*, gemm_256x*) are chosen only while M*ldx + K < 2^31 - 256, and every other shape runs on kernels
 *     that read through 64-bit pointers.
 *   - w: Cout*ldw must be below 2^31 - 256 elements (the same descriptors: the last weight rows must start below that byte).
 *   - output rows M = N*OH*OW must be below 2^31 - 512 (int row indices; a tile may start up to 256 rows short of M).  Defensive:
 *     with OH, OW derived from H, W the bound on x already implies it.
 *   - the tile grid of the planned launcher (ur_conv2d_plan_launch; row tiles of 64 to 256 rows x column tiles of 32 to 320
 *     columns) must be below 2^23 workgroups: a grid of 2^32 threads or more wraps silently, and workgroups have up to 512 threads.
 *   - y, yt, residual, bias rows (bias_img_stride), gn_part, gn_ab, row_stats, ln_stats and the split-K planes of the workspace are
 *     addressed with 64-bit offsets: no element limit of their own (M*ldy may exceed 2^31; tests/large_cases.py runs it).
 *   ur_gemm_bias_act: 0 < M < 2^31, then the same limits; ur_groupconv3x3_nhwc: the same limits with ldx = Cg*groups.
 */
typedef struct ur_conv_desc {
  const void* x;        /* bf16 [N,H,W,ldx]; first C1 input channels */
  const void* x2;       /* bf16 [N,H,W,ldx2] or NULL; next C2 input channels (virtual concat) */
  const void* w;        /* bf16 [Cout][KH*KW*(C1+C2)] row stride ldw */
  const float* bias;    /* fp32 [Cout] or NULL */
  const void* residual; /* bf16 [M, ldr] or NULL (M = N*OH*OW) */
  void* y;              /* 16-bit (or fp32 if out_f32) [M, ldy]; may be NULL if only gn_part is wanted */
  void* yt;             /* bf16 transposed output for columns >= n_split: [M/t_rows][Cout-n_split][t_ld] or NULL
                           (nbatch == 1 only: yt has no batch stride) */
  float* gn_part;       /* fp32 [N][P][nbatch*Cout_out][2] = partial (sum, sum of squares) of the 16-bit outputs per image,
                           row chunk and channel, plain stores (P = ur_conv_plan.gn_parts): statistics for the GroupNorm /
                           InstanceNorm / AdaptiveAvgPool2d(1) that consumes y (ur_groupnorm_finalize), or NULL.  With
                           ur_conv_plan.gn_fused the epilogue writes them and y may be NULL (pooled output only:
                           taskeditor.py:35); otherwise one extra pass over y does.  Needs Cout_out % 8 == 0 (the statistics run
                           on vectors of 8 channels), whichever source writes them: UR_E_INVALID otherwise.  The extra pass of
                           a batched launch (nbatch > 1) needs the batches side by side in y's rows (bs_y == Cout_out) */
  const float* gn_ab;   /* fp32 [N][2][C1+C2] per-(image, input channel) affine (a | b) from ur_groupnorm_finalize, or NULL:
                           the conv reads act(a*x + b) instead of x (GroupNorm apply [+ SiLU] of ResnetBlock2D fused into the
                           conv's loader; zero padding stays zero).  Only where ur_conv_plan.prologue_ok */
  int gn_silu;          /* 1: SiLU after the gn_ab affine */
  float* row_stats;     /* fp32 [parts][M][2] = per-row (sum, sum of squares) of this GEMM's output, one partial plane per N
                           tile (plain stores; parts = ur_conv_plan.row_stat_parts from ur_conv2d_plan): the LayerNorm statistics of the
                           GEMM that consumes y (BasicTransformerBlock norm1-3) or NULL.  With yt the sums cover only y's
                           columns below n_split: the transposed columns are not part of them */
  const float* ln_stats;  /* fp32 [ln_parts][M][2] row sums of x (a producer's row_stats): this GEMM computes W.LayerNorm(x) as
                             rstd*(acc - mean*ln_colsum[n]) + bias[n] with w = W*gamma, bias = W.beta + b prefolded; or NULL */
  const float* ln_colsum; /* fp32 [Cout]: sum_k of the (bf16) folded weight row */
  float ln_eps;
  int ln_dim;             /* normalised width (= K) */
  int ln_parts;           /* number of partial planes in ln_stats */
  float* workspace;     /* fp32 split-K scratch or NULL */
  size_t workspace_bytes;
  int N, H, W;          /* input dims (before upsample2x) */
  int C1, ldx, C2, ldx2;
  int Cout, ldw, ldy, ldr;
  int KH, KW, stride, pad_t, pad_l;
  int OH, OW;
  int upsample2x;       /* 1: x is read through a nearest-neighbour 2x upsample */
  int act;              /* UR_ACT_* */
  int out_f32;
  int n_split, t_rows, t_ld;
  float out_scale;      /* applied after act; 1.0 for none */
  int nbatch;           /* >= 1 */
  long long bs_x, bs_x2, bs_w, bs_bias, bs_y, bs_r; /* element strides per batch index */
  int k_chunk_major;    /* 1: weight K index runs (64-channel chunk, tap, channel) instead of (tap, channel): the taps of
                           one chunk are consecutive K tiles, so re-reads of a pixel hit L2 (needs C1, C1+C2 % 64 == 0) */
  long long bias_img_stride; /* 0: one bias row; else bias row of image n = m/(OH*OW) is bias + n*stride
                                (per-sample time embeddings, unifie.py:91-105).  Not with pair activations, ln_stats, yt
                                or row_stats */
  int dtype;            /* UR_DT_BF16 | UR_DT_F16: type of x, x2, w, residual, y (unless out_f32), yt */
  const void* w_frag;   /* optional second packing of the SAME weights for the weight-streaming kernel of the 8 x 8 maps (3x3, stride 1,
                           Cout % 128 == 0, (C1+C2) % 256 == 0), or NULL: MFMA-fragment-major
                           [Cout/128][(C1+C2)/64][tap 9][k-step 4][row block 4][lane 64][8], lane = (cout % 32) + 32 * ((cin % 16) / 8),
                           element = cin % 8 - one coalesced 1-KiB load per 32 x 16 weight fragment (csrc/conv_wstream.hip) */
  const void* w_up4;    /* optional folded weights of an upsampling 3x3 conv, honoured only with upsample2x (ignored otherwise), or
                           NULL: a nearest-2x upsample followed by the 3x3 conv (pad 1) is, for the output pixels of parity (py, px), a 2x2
                           conv over the source image, W4[py][px][co][a][b][ci] = sum of the taps (ky, kx) that fall on source pixel
                           (y - 1 + py + a, x - 1 + px + b): py = 0: {ky 0} -> a 0, {ky 1, 2} -> a 1; py = 1: {ky 0, 1} -> a 0, {ky 2} -> a 1;
                           the columns likewise.  Summed in fp32 from the fp32 weights, rounded once to the 16-bit type, laid out
                           [phase = 2 py + px][Cout][(C1)/64][tap = 2 a + b][64].  One launch then runs the four phases on the 8 x 32
                           halo kernels at 4/9 of the MACs (H % 8 == 0, W % 32 == 0, C1 % 64 == 0, C2 == 0, stride 1, pad 1,
                           k_chunk_major, nbatch == 1, 16-bit y, no gn_ab / row_stats / ln_stats / yt; ur_conv_plan.up4 says whether it will; a
                           batched / grouped launch, nbatch > 1, never reads w_up4: it has no batch stride);
                           every other launch, and every launch with w_up4 == NULL, runs as without it.  The result is not
                           bit-identical to the 9-tap launch: the tap sums are rounded once, where that launch rounds each tap and
                           adds the products in fp32.  gn_part then has 4 x patches partials per image */
} ur_conv_desc;
/* ur_conv_desc grows by trailing fields (w_frag: ur_version 101, w_up4: 102).  Zero-initialise the whole descriptor (ur_conv_desc d = {0};
 * or memset) before filling it, and rebuild callers against this header: a field left uninitialised, or a descriptor laid out by an older
 * header, hands the library a wild pointer. */

int ur_conv2d_nhwc(const ur_conv_desc* d, ur_stream_t stream);

/* host-only query (no launch): what the launch of `d` will do.  Fill d exactly as for the real call (non-NULL dummies
 * are fine for row_stats / gn_part / gn_ab when only the plan is wanted). */
typedef struct ur_conv_plan {
  int row_stat_parts; /* partial planes the launch writes into d->row_stats */
  int gn_parts;       /* partials per image (P) the launch writes into d->gn_part */
  int gn_fused;       /* 1: written by the conv epilogue itself (y may be NULL); 0: by an extra pass over y */
  int prologue_ok;    /* 1: d->gn_ab is honoured inside this launch; 0: apply the GroupNorm separately */
  int up4;            /* 1: the launch runs the folded kernel on d->w_up4 (four 2x2 phase convs); 0: w_up4 is not read */
} ur_conv_plan;
int ur_conv2d_plan(const ur_conv_desc* d, ur_conv_plan* plan);

/* host-only query (no launch, no HIP call): which launcher runs `d` and how it splits the work, by the same workspace rule as
 * the launch (d->workspace / d->workspace_bytes).  Fill d as for ur_conv2d_plan.  A grouped conv that runs one launch per group
 * (group_loop) reports the launch of one group.  It refuses, with the launch's own error, what the launch refuses and
 * ur_conv2d_plan only reports: gn_ab without prologue_ok, y == NULL without a fused gn_part, row_stats / ln_stats without a
 * staged 16-bit output of one batch. */
typedef struct ur_conv_launch_info {
  int launcher;       /* index of the launcher: ur_conv_launcher_name(launcher) */
  int splitk;         /* K splits (1: no split, no reduce pass) */
  int nk_per_split;   /* 64-deep K tiles per split */
  int reduce;         /* reduce pass after the splits: -1 none, 0 plain, 1 row-wise (LayerNorm statistics), 2 GroupNorm partials */
  int reduce_ri;      /* reduce 2: 16 * reduce_ri output rows per block (4, 2 or 1); else 0 */
  int gn_pass;        /* 1: the GroupNorm partials come from an extra pass over y (ur_conv_plan.gn_fused == 0); the launch then
                         needs a dense y (ldy == nbatch * Cout_out) and refuses any other before it runs anything */
  int group_loop;     /* 1: one halo launch per group on its channel slice */
} ur_conv_launch_info;
int ur_conv2d_plan_launch(const ur_conv_desc* d, ur_conv_launch_info* info);
int ur_conv_launcher_count(void);
const char* ur_conv_launcher_name(int i); /* static string, or NULL outside [0, ur_conv_launcher_count()) */

/* Linear / 1x1 convolution with the epilogues of SURVEY.md 8(b): y[m, n] = act(x[m, :] . w[n, :] + bias[n]) (+ residual);
 * act in UR_ACT_* (GEGLU / GATE: w rows pre-interleaved, N = 2 * output columns).  Thin wrapper over ur_conv2d_nhwc. */
int ur_gemm_bias_act(const void* x, const void* w, const float* bias, const void* residual, void* y, long long M, int N, int K,
                     int ldx, int ldw, int ldy, int ldr, int act, float* workspace, size_t workspace_bytes, int dtype,
                     ur_stream_t stream);
/* grouped 3x3 convolution (pad 1, stride 1) + activation: AdaNAFV2.group_conv (cfrm.py:20-21), the three TFA gate branches
 * (taskeditor.py:30-52).  x [N,H,W,G*Cg], w [G*Cog][9*Cg], y [N,H,W,G*Cog].  Thin wrapper over ur_conv2d_nhwc (nbatch = G). */
int ur_groupconv3x3_nhwc(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int Cg, int Cog,
                         int groups, int act, float* workspace, size_t workspace_bytes, int dtype, ur_stream_t stream);

/* ---- normalisation (HBM-bound) ----------------------------------------------------------------
 * GroupNorm over NHWC (+ optional SiLU) in three steps, all without atomics:
 *   1. statistics: fp32 partial planes part[N][P][C][2] (sum, sum of squares per image, pixel chunk, channel) - written by the
 *      PRODUCER's epilogue (ur_conv_desc.gn_part) or by ur_groupnorm_stats;
 *   2. ur_groupnorm_finalize: partials of one or two (virtually concatenated) sources -> fp32 ab[N][2][C] with
 *      y = a*x + b == GroupNorm(x); fp64 sums in a fixed order;
 *   3. ur_groupnorm_apply_act (or ur_conv_desc.gn_ab: applied inside the consuming convolution).
 * G == C with gamma = beta = NULL gives InstanceNorm2d; mean_out gives AdaptiveAvgPool2d(1).
 * Arguments are checked on the host before any arithmetic on them and before any launch: a null required pointer, a non-positive
 * N / HW / rows / C / C1 / G (C2 when x2 / part2 is given), C % 8 != 0, C % G != 0 or an unknown dtype returns UR_E_INVALID
 * (the size queries return UR_E_INVALID / the bytes of one partial).
 * Size limits: images run along the grid's y dimension, so N <= 65535 for ur_groupnorm_stats / ur_instnorm_stats /
 *   ur_groupnorm_finalize / ur_groupnorm_apply_act / ur_groupnorm_nhwc / ur_avgpool_hw (UR_E_INVALID beyond); N*HW*C itself has no
 *   limit (64-bit offsets; run past 2^31 elements in tests/large_cases.py).  ur_layernorm_rows and ur_softmax_rows_f32: rows is
 *   a long long without a limit of its own (more rows than one grid holds - 2^28 and 2^24 - run as several launches), and
 *   neither have rows*C / rows*ldp.
 * Replaces: nn.GroupNorm(32,C)+SiLU in every ResnetBlock2D / conv_norm_out, Transformer2D / Attention
 *   pre-norms, AdaNAFV2.group_norm (cfrm.py:19), nn.InstanceNorm2d (taskeditor.py:31,40,49), nn.AdaptiveAvgPool2d(1).
 */
int ur_groupnorm_stats_parts(int N, int HW, int C);   /* host: P of the plane ur_groupnorm_stats writes */
size_t ur_groupnorm_ws_bytes(int N, int HW, int C);   /* bytes of that plane */
size_t ur_groupnorm_ab_bytes(int N, int C);           /* bytes of an ab table */
int ur_groupnorm_stats(const void* x, float* part, int N, int HW, int C, int dtype, ur_stream_t stream);
int ur_instnorm_stats(const void* x, float* part, int N, int HW, int C, int dtype, ur_stream_t stream); /* same pass */
/* part2/parts2/C2 (optional): second source, virtually concatenated after part1's C1 channels (UNet up path: GroupNorm over
 * torch.cat([sample, skip]), base_model.py:189,197).  ab and/or mean_out ([N][G] group means) may be NULL. */
int ur_groupnorm_finalize(const float* part1, int parts1, int C1, const float* part2, int parts2, int C2, const float* gamma,
                          const float* beta, int N, int HW, int G, float eps, float* ab, float* mean_out, ur_stream_t stream);
/* y[N,HW,C1+C2] = act(a*x + b) over x [N,HW,C1] (| x2 [N,HW,C2]) */
int ur_groupnorm_apply_act(const void* x, const void* x2, void* y, const float* ab, int N, int HW, int C1, int C2, int silu,
                           int dtype, ur_stream_t stream);
/* the three chained.  pre1 / pre2 (optional): producer-side partial planes of x / x2 with parts1 / parts2 partials per image;
 * ws: ur_groupnorm_ws_bytes(N,HW,C1) [+ (N,HW,C2)] bytes of scratch, needed only for sources without producer partials */
int ur_groupnorm_nhwc(const void* x, const void* x2, void* y, const float* gamma, const float* beta, int N, int HW,
                      int C1, int C2, int G, float eps, int silu, float* ws, float* ab, const float* pre1, int parts1,
                      const float* pre2, int parts2, int dtype, ur_stream_t stream);
/* LayerNorm over the last dim of [rows, C] (nn.LayerNorm in BasicTransformerBlock; timm LayerNorm2d
 * in NAFBlock, nafnet_arch.py:97-98, which is LayerNorm-over-C in NHWC).  0 < C <= 2048, C % 8 == 0; gamma / beta may be NULL. */
int ur_layernorm_rows(const void* x, void* y, const float* gamma, const float* beta, long long rows, int C,
                      float eps, int dtype, ur_stream_t stream);
/* softmax over rows of an fp32 [rows, cols] matrix -> 16-bit (upcast_softmax): p [rows][ldp], ldp >= cols, columns [cols, ldp) are
 * written as zeros. */
int ur_softmax_rows_f32(const float* s, void* p, long long rows, int cols, int ldp, int dtype, ur_stream_t stream);

/* ---- attention (flash-style, bf16 MFMA, fp32 softmax) ------------------------------------------
 * o[b,t,h*D+d] = softmax_k(q.k * scale) v.  q:[B][Tq][ldq], k:[B][Tk][ldk] (head h at column h*D),
 * vt:[B][H*D][ldvt] (V transposed: row = channel, column = key index), o:[B][Tq][ldo].  D in {64,128,512}
 * (512: the single 512-wide head of the VAE mid-block attention, split over keys for q.k and over channels for p.v
 *  inside one workgroup - no Tq x Tk matrix is materialised at any D).
 * Scale convention for D == 64: the kernels work in the exp2 domain on scores multiplied by scale * log2(e).  Callers that
 *   want full accuracy fold that factor into the QUERY PROJECTION's fp32 weights before their one rounding to 16 bits and pass
 *   scale = ln 2 (scale * log2(e) == 1: q is used as it is) - unirestore_amd/modules/nn.py does.  Any other scale is honoured,
 *   but the ping-pong kernel then multiplies the 16-bit q by the factor and rounds it to 16 bits a second time (bf16: one more
 *   2^-9 relative rounding per q element; on scores of a few hundred that moves single softmax weights by ~5 %).
 * Replaces: F.scaled_dot_product_attention via diffusers AttnProcessor2_0 (UNet self/cross attention,
 *   Controller AttnDownBlock2D / UNetMidBlock2D attention) and the VAE mid-block AttentionBlock
 *   (/root/reference/src/modules/diffuie/autoencoder.py:37-45 calls it through vae.encoder/decoder.mid_block).
 */
int ur_attention_fwd(const void* q, const void* k, const void* vt, void* o, int B, int H, int Tq, int Tk,
                     int D, int ldq, int ldk, int ldvt, int ldo, long long bs_q, long long bs_k,
                     long long bs_vt, long long bs_o, float scale, int dtype, ur_stream_t stream);
/* The same with a scratch buffer.  The d = 64 self-attention kernel runs one 256-query workgroup per CU; when the launch is
 * whole rounds of the 256 CUs plus at most half a round (B = 8, 5 heads, T = 4096: 640 workgroups), the query tiles of that
 * remainder are split in two key halves that fill the last round, and a second small kernel merges the halves from `ws`
 * (un-normalised fp32 rows + running maximum + row sum).  ur_attention_workspace_bytes() is what the split needs (0: none);
 * ws == NULL or a smaller buffer just runs unsplit.  The library never allocates: the caller owns ws (16-byte aligned). */
size_t ur_attention_workspace_bytes(int B, int H, int Tq, int Tk, int D);
int ur_attention_fwd_ws(const void* q, const void* k, const void* vt, void* o, int B, int H, int Tq, int Tk,
                        int D, int ldq, int ldk, int ldvt, int ldo, long long bs_q, long long bs_k, long long bs_vt,
                        long long bs_o, float scale, void* ws, size_t ws_bytes, int dtype, ur_stream_t stream);
/* What ur_attention_fwd_ws would launch for these arguments: host only, no HIP call, nothing is read or written through the
 * pointers (placeholders will do - their values matter only for the ping-pong kernel's alignment rule: q, k, vt 16-byte and o
 * 8-byte aligned).  Same argument checks and return codes as the launch, which decides through the same function; honours
 * UR_ATTN_NOPP (read once per process).  Kernels, by index: the 128-query kernel at d = 64 and at d = 128, the d = 512 kernel, the
 * 256-query ping-pong kernel (d = 64, Tq and Tk multiples of 256, taken when its grid fills whole rounds of the CUs well enough). */
typedef struct ur_attention_plan {
  int kernel;      /* index for ur_attention_kernel_name(): 128-query d64, 128-query d128, d512, ping-pong */
  int workgroups;  /* grid of the main launch */
  int n_full;      /* ping-pong: whole (batch-head, query tile) work items; else 0 */
  int n_split;     /* ping-pong: trailing tiles split in two key halves (0: none, no combine launch) */
} ur_attention_plan;
int ur_attention_plan_launch(const void* q, const void* k, const void* vt, void* o, int B, int H, int Tq, int Tk,
                             int D, int ldq, int ldk, int ldvt, int ldo, long long bs_q, long long bs_k, long long bs_vt,
                             long long bs_o, void* ws, size_t ws_bytes, ur_attention_plan* plan);
int ur_attention_kernel_count(void);
const char* ur_attention_kernel_name(int i); /* static string, or NULL outside [0, ur_attention_kernel_count()) */

/* ---- token-stationary fused chains (csrc/tchain.hip) ----------------------------------------------
 * A wave keeps 32 tokens in registers through a whole chain of token-wise layers; the weights arrive as a pre-packed
 * stream of ur_chain_tile_bytes()-byte tiles that are the LDS image of each layer (unirestore_amd/chain.py packs them:
 * [row][128 B] blocks, XOR-swizzled slots, swap23-permuted output rows, LayerNorm folded, fp32 vectors in the tile tail).
 * Shapes: C == 320 (UNet level 0) and T % 128 == 0; anything else returns UR_E_UNSUPPORTED / UR_E_INVALID and the caller
 * uses the per-layer entry points above. */
size_t ur_chain_tile_bytes(void);
/* y[t,:] = x[t,:] + W2 . GEGLU(W1 . LayerNorm(x[t,:]) + b1) + b2: diffusers FeedForward(activation_fn="geglu") + norm3 + residual of
 * BasicTransformerBlock (reached through /root/reference/src/modules/diffuie/base_model.py:137-160,184-198).  The 4C-wide
 * hidden tensor never exists in memory.  stream_w: 3 * hidden/64 tiles. */
int ur_ff_geglu_fused(const void* x, const void* stream_w, size_t stream_bytes, void* y, long long T, int C, int hidden, int ldx,
                      int ldy, float ln_eps, int dtype, ur_stream_t stream);

/* h0 = proj_in(GroupNorm(x)) (gn_ab: the per-image affine [N][2][C] from ur_groupnorm_finalize, applied to the fragments in
 * registers) and q | k | v = to_q / to_k / to_v(LayerNorm1(h0)) of the block's self-attention: Transformer2DModel.norm + proj_in,
 * BasicTransformerBlock.norm1 + attn1 projections (base_model.py:137-160 via diffusers).  h0, q, k: [T][C]; vt: [N][C][tokens_per_image]
 * (V transposed, the layout ur_attention_fwd reads).  stream_w: 20 tiles. */
int ur_transformer_head_fused(const void* x, const float* gn_ab, const void* stream_w, size_t stream_bytes, void* h0, void* q, void* k,
                              void* vt, long long T, int tokens_per_image, int C, float ln_eps, int dtype, ur_stream_t stream);
/* Everything behind the self-attention: h1 = h0 + to_out(o1); cross-attention over the CONSTANT context (its K / V are baked into
 * the stream; tk <= 80 keys, heads x 64) with LayerNorm2 folded into to_q; h2 = h1 + to_out(o2); h3 = h2 + FF(LayerNorm3(h2));
 * y = xres + proj_out(h3).  gn_part (optional): fp32 [N][tokens_per_image/128][C][2] partial (sum, sum of squares) of y for the
 * GroupNorm of the next ResnetBlock2D (ur_groupnorm_finalize with parts = tokens_per_image/128).  stream_w: 25 + 3*hidden/64 tiles. */
int ur_transformer_tail_fused(const void* o1, const void* h0, const void* xres, const void* stream_w, size_t stream_bytes, void* y,
                              float* gn_part, long long T, int tokens_per_image, int C, int hidden, int heads, int tk, float ln_eps,
                              float attn_scale, int dtype, ur_stream_t stream);

/* SC-Tuner adapter (CSCEAdapter, /root/reference/src/modules/diffuie/scedit.py:24-38) in one launch: s = x + proj(cond),
 * y = tuner.2(GELU(tuner.0(s))) + s for a 320-channel UNet skip x [T][320] and the 256-channel Controller feature cond [T][256];
 * gn_part (optional) as in ur_transformer_tail_fused (the edited skip feeds a GroupNorm on the up path).  stream_w: 14 tiles. */
int ur_csce_fused(const void* x, const void* cond, const void* stream_w, size_t stream_bytes, void* y, float* gn_part, long long T,
                  int tokens_per_image, int C, int Ccond, int dtype, ur_stream_t stream);

/* ---- HBM-bound stencils / reductions / elementwise ---------------------------------------------*/
/* Every entry point of this block returns UR_E_INVALID for a null required pointer, an empty tensor (non-positive N, H, W, HW,
 * rows, M, B, T, D, C or G), C % 8 != 0 (16-bit tensors) or an unknown dtype - checked on the host before anything is launched.
 * Size limits: ur_dwconv3x3_nhwc, ur_scale_channels, ur_scale_channels_fanout, ur_axpy_channels and ur_spade_modulate index with
 * 64-bit grid-stride loops over at most 8192 workgroups: each dimension must fit its int / long long argument, their products
 * (N*H*W*C, K*B*HW*C, rows*C, rows*ldgb) have no limit (run past 2^31 elements in tests/large_cases.py). */
/* depthwise 3x3 (pad 1) + bias, optional SimpleGate (out channels C/2): nafnet_arch.py:41-49,22-25 */
int ur_dwconv3x3_nhwc(const void* x, const float* w9c, const float* bias, void* y, int N, int H, int W, int C,
                      int gate, int dtype, ur_stream_t stream);
/* mean over HW -> fp32 [N][C] (nn.AdaptiveAvgPool2d(1)): statistics pass + finalize; ws = ur_groupnorm_ws_bytes(N,HW,C) bytes */
int ur_avgpool_hw(const void* x, float* out, int N, int HW, int C, float* ws, int dtype, ur_stream_t stream);
/* y = x * s[n][c] (+ residual) : channel attention scaling (nafnet_arch.py:116, cfrm.py:46-48, taskeditor.py:95) */
int ur_scale_channels(const void* x, const float* s, const void* residual, void* y, int N, int HW, int C,
                      int dtype, ur_stream_t stream);
/* y = a + b * s[c] (per-channel learnable residual scale beta/gamma, nafnet_arch.py:121,130) */
int ur_axpy_channels(const void* a, const void* b, const float* s, void* y, long long rows, int C, int dtype, ur_stream_t stream);
/* SPADE modulation (spade.py:69): y = n * (1 + gamma) + beta (+ residual); gamma | beta = gb[:, 0:C] | gb[:, C:2C] (row stride ldgb) */
int ur_spade_modulate(const void* n, const void* gb, int ldgb, const void* residual, void* y, long long rows, int C,
                      int dtype, ur_stream_t stream);
/* tiny fp32 linear: y[m, g*Ng+n] = act(bias + sum_k x[m, g*Kg+k] * w[g*Ng+n, k]) (time MLPs, SCA, gates) */
int ur_linear_f32(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int groups,
                  int act, ur_stream_t stream);
/* TFA prompt update (taskeditor.py:80-91): pooled [B][3][T*D] (filter, info, content), cond [B][T][D] -> upd */
int ur_tfa_prompt_update(const float* pooled, const float* cond, float* upd, int B, int T, int D, ur_stream_t stream);
/* Multi-task fan-out of ur_scale_channels (DiffUIE.forward_tasks): x [B,HW,C] is shared by K tasks, s fp32 [K*B][C] holds one scale
   row per (task, image), y [K*B,HW,C] is task-major: y[k*B+b] = x[b] * s[k*B+b], rounded exactly as ur_scale_channels rounds it.
   s == NULL replicates x K times (bit copies).  Each 16-byte vector of x is read once and written K times: (1 + K) tensors of
   traffic instead of the 2K of K ur_scale_channels calls.  1 <= K <= 8.  No allocation, no synchronisation, no atomics. */
int ur_scale_channels_fanout(const void* x, const float* s, void* y, int B, int K, int HW, int C, int dtype, ur_stream_t stream);
/* Multi-task fan-out of ur_tfa_prompt_update: upd [K*B][T][D], row n = k*B+b reads pooled row n % B (pooled [B][3][T*D] is shared
   by the tasks) and cond row n / B of a [K][T][D] prompt table (cond_per_row = 0) or row n of a [K*B][T][D] tensor
   (cond_per_row = 1).  Same reduction order as ur_tfa_prompt_update: a row equals what that gives for the same inputs, bit for bit. */
int ur_tfa_prompt_update_fanout(const float* pooled, const float* cond, float* upd, int B, int K, int T, int D, int cond_per_row,
                                ur_stream_t stream);
/* out[n][c] = a[n][c] * b[n][c / (C/G)]  (combine intra/inter group attention, cfrm.py:46-48) */
/* G must divide C; N * C must fit an int */
int ur_vec_mul_group(const float* a, const float* b, float* out, int N, int C, int G, ur_stream_t stream);

/* ---- latent / image boundary --------------------------------------------------------------------*/
/* Every entry point of this block returns UR_E_INVALID for a null required pointer, an empty tensor (non-positive N, C, H, W, HW, M,
 * T, th, tw, RH, RW, OH, OW, Clat), Cpad < C or < Clat, ld < C, ld < 2 * Clat (ur_vae_sample), ld_eps < Clat, Clat > 8 (blend), a reflect
 * padding not smaller than the resized image, a crop window outside the input, a tile larger than the latent, slot_bytes smaller
 * than a canvas-sized image or an unknown dtype - checked on the host before any arithmetic on the arguments and before anything is
 * launched. */
/* Size limits: every kernel of this block runs a 64-bit grid-stride loop over pixels (at most 8192 workgroups) and forms every
 * offset in 64 bits.  Each dimension must fit its int / long long argument; the products N*H*W, N*C*H*W, N*XH*XW*ld, N*C*OH*OW, M*ld,
 * M*Cpad and N*slot_bytes have no limit (tests/large_cases.py runs ur_nhwc_to_nchw_f32, ur_nchw_f32_to_nhwc, ur_f32_to_bf16_scaled,
 * ur_image_unpad_resize_nchw and ur_image_u8_egress with an fp32 side past 2^32 bytes). */
/* images NCHW fp32 in [0,1] -> NHWC 16-bit (x*2-1), channels padded with zeros to Cpad (autoencoder.py:149) */
int ur_image_to_nhwc(const float* img, void* y, int N, int C, int H, int W, int Cpad, int dtype, ur_stream_t stream);
/* NHWC fp32/16-bit [N,H,W,ld] first C channels -> NCHW fp32, out = x*mul+add (autoencoder.py:175) */
int ur_nhwc_to_nchw_f32(const void* x, int x_is_f32, float* out, int N, int C, int H, int W, int ld, float mul,
                        float add, int dtype, ur_stream_t stream);
/* NCHW fp32 -> NHWC 16-bit with channel padding (module-level API plumbing) */
int ur_nchw_f32_to_nhwc(const float* x, void* y, int N, int C, int H, int W, int Cpad, int dtype, ur_stream_t stream);
/* DiffUIE.forward pre-processing (reference unifie.py:124-134) fused with the encoder's x*2-1 (autoencoder.py:152 -> vae.encode)
 * and the NHWC layout pass: img fp32 [N,C,H,W] -> F.interpolate(bicubic, align_corners=False, antialias=False) to RH x RW
 * (skipped when equal) -> F.pad(reflect) right/bottom by PW/PH -> v*mul+add -> y 16-bit [N,RH+PH,RW+PW,Cpad]. */
int ur_image_resize_pad_nhwc(const float* img, void* y, int N, int C, int H, int W, int RH, int RW, int PH, int PW, int Cpad,
                             float mul, float add, int dtype, ur_stream_t stream);
/* DiffUIE.forward post-processing (unifie.py:164-168) and the evaluator's 8-bit quantisation (eval_image_restoration.py:71):
 * x NHWC (16-bit | fp32) [N,XH,XW,ld] -> v*mul+add -> crop [0:CH,0:CW] -> bicubic to OH x OW -> optional
 * mul(255).round().clamp(0,255).div(255) -> out fp32 [N,C,OH,OW]. */
int ur_image_unpad_resize_nchw(const void* x, int x_is_f32, float* out, int N, int C, int XH, int XW, int ld, int CH, int CW,
                               int OH, int OW, float mul, float add, int quantize, int dtype, ur_stream_t stream);
/* Ragged 8-bit batch: N slots of one device buffer, slot n = one dense uint8 HWC [H_n, W_n, C] image at byte offset
 * n * slot_bytes (slot_bytes >= CH * CW * C for the batch's canvas CH x CW; an image is never larger than its canvas), and a
 * DEVICE table geom int32 [N][4] = (H_n, W_n, RH_n, RW_n): the image is resized to RH_n x RW_n and reflect-padded right / bottom
 * to the canvas.  The geometry is read by the kernel, not passed as arguments, so one captured launch serves any images that
 * fit the canvas.  A table row that does not fit (H > RH, RH > CH, padding >= RH, ...) is never followed.
 * ingest: per image float(v) / 255.f (a true division), then exactly ur_image_resize_pad_nhwc (C = 3) -> y 16-bit [N,CH,CW,Cpad];
 *         an image gives the same bits through either entry point.  A bad table row gives a zero image. */
int ur_image_u8_ingest(const uint8_t* src, long long slot_bytes, const int* geom, void* y, int N, int CH, int CW, int Cpad, float mul,
                       float add, int dtype, ur_stream_t stream);
/* egress: per image exactly ur_image_unpad_resize_nchw(..., quantize = 1) - v*mul+add, crop [0:RH_n, 0:RW_n], bicubic to
 *         H_n x W_n, rint(v*255) clamped to 0..255 - stored as the uint8 code value, HWC, into slot n of dst.  x NHWC (16-bit | fp32)
 *         [N,XH,XW,ld], the canvas is XH x XW.  nonfinite int32 [N], zeroed by the caller before the launch: a non-finite sample
 *         stores code 0 and sets nonfinite[n] = 1; a bad table row writes no pixel and sets nonfinite[n] = 2.
 * Arguments are checked before any HIP call (UR_E_INVALID).  No allocation, no synchronisation, no atomics. */
int ur_image_u8_egress(const void* x, int x_is_f32, uint8_t* dst, long long slot_bytes, const int* geom, int* nonfinite, int N, int C,
                       int XH, int XW, int ld, float mul, float add, int dtype, ur_stream_t stream);
/* z = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * scale; moments NHWC fp32 [M, ld] (mean | logvar) */
int ur_vae_sample(const float* moments, int ld, const float* noise_nchw, float* z_nhwc, void* z_16, int N,
                  int HW, int Clat, int Cpad, float scale, int dtype, ur_stream_t stream);
/* zt = sa * z0 + sb * noise (DDPMScheduler.add_noise, unifie.py:88); fp32 NHWC state + 16-bit copy */
int ur_add_noise(const float* z0, const float* noise_nchw, float* zt, void* zt_16, int N, int HW, int Clat,
                 int Cpad, float sa, float sb, int dtype, ur_stream_t stream);
/* DDIM update (unifie.py:150): zt <- c_x*zt + c_e*eps, eps fp32 NHWC [M, ld_eps]; refreshes the 16-bit copy */
int ur_ddim_step(float* zt, const float* eps, int ld_eps, void* zt_16, long long M, int Clat, int Cpad,
                 float c_x, float c_e, int dtype, ur_stream_t stream);
/* Tiled latent sampling (unirestore_amd/tiling.py).  Latents fp32 NHWC [N,LH,LW,Cpad]; tile batch [N*T,th,tw,.] with image n's
 * tile k at index n*T+k; origins device int [T][2] = (y0, x0), every tile inside the latent (others are skipped: a tile is valid when
 * y0 >= 0, x0 >= 0, y0 + th <= LH and x0 + tw <= LW, by one test shared by both kernels).
 * gather: tiles_16 <- 16-bit copy of each tile's window of z; the slots of a skipped tile are written as zeros. */
int ur_latent_tiles_gather(const float* z, void* tiles_16, int N, int LH, int LW, int Cpad, int T, int th, int tw,
                           const int* origins, int dtype, ur_stream_t stream);
/* Blended DDIM step, output-stationary per latent pixel p: eps(p) = sum_k wn[k](p) * eps_tiles_k(p) over the covering tiles in
 * ascending k (fp32), zt <- c_x*zt + c_e*eps, and the 16-bit zt into every covering tile slot of zt_tiles_16.  eps_tiles fp32
 * [N*T,th,tw,ld_eps], wn fp32 [T,th,tw] (normalised weights), Clat <= 8.  A skipped tile's eps and weights are not read and its slots
 * are not written; a pixel that no valid tile covers gets c_x*zt. */
int ur_latent_tiles_blend_ddim(float* zt, const float* eps_tiles, int ld_eps, void* zt_tiles_16, const float* wn, int N, int LH,
                               int LW, int Clat, int Cpad, int T, int th, int tw, const int* origins, float c_x, float c_e,
                               int dtype, ur_stream_t stream);
/* y_16[M][Cpad] = x_f32[M][ld] * mul (latents / scaling_factor before post_quant_conv) */
int ur_f32_to_bf16_scaled(const float* x, int ld, void* y, long long M, int C, int Cpad, float mul, int dtype, ur_stream_t stream);

/* ---- counter-based noise keyed per image (the forward's two draws when seeds are given) -------------------------------------
 * out[n][e] for image n (key row n), draw `draw` (0 = the VAE posterior draw, 1 = the t=999 draw) and element e of the image's
 * `count` elements (for a [C,H,W] latent in NCHW order e = (c*H + y)*W + x):
 *   Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85;
 *   key = (keys[n][0], keys[n][1]) = (seed_n & 0xffffffff, seed_n >> 32) of the image's unsigned 64-bit seed;
 *   counter = (e >> 2, draw, 0, 0); element e takes output word e & 3.
 *   kind 1: out uint32 = that word.
 *   kind 0: out fp32 = a standard normal by Box-Muller on the word pairs (0,1) and (2,3): u = ((word >> 9) + 0.5) * 2^-23 (exact in
 *           fp32, inside [2^-24, 1 - 2^-24], so the logarithm never sees 0), r = sqrt(-2 ln u_a), theta = 2 pi u_b, the even word
 *           gives r cos(theta), the odd word r sin(theta); fp32 arithmetic with the precise logf / sqrtf / sincosf, never the fast
 *           intrinsics.  |value| <= sqrt(48 ln 2) ~ 5.77; within 1e-5 of the same formula in fp64.
 * keys: DEVICE uint32 [N][2], read by the kernel (never baked into its arguments: one captured graph serves every seed).  One thread
 * per counter, a 16-byte store where the address allows it, 4-byte stores for the count % 4 tail and an `out` off 16 bytes (out must
 * be 4-byte aligned).  One launch; no allocation, no synchronisation, no atomics.  UR_E_INVALID before any launch for a null
 * pointer, N <= 0, count <= 0, count > 2^34 or an unknown kind. */
int ur_keyed_noise(const uint32_t* keys, uint32_t draw, void* out, int N, long long count, int kind, ur_stream_t stream);

/* ---- full-reference image metrics (evaluator side; the GPU counterpart of runner.psnr_per_image / runner.ssim) ----------
 * Full-reference metrics per image (skimage semantics, fp64 accumulation, fixed-order reductions): pred / target fp32 NCHW
 * [N,C,H,W] contiguous; psnr / ssim fp64 [N]; ws fp64 workspace of ur_image_metrics_ws_size(...) bytes.
 *   psnr[n] = 10 log10(data_range^2 / mean over C*H*W of (pred - target)^2)   (+inf for identical images)
 *   ssim[n] = mean over channels and the valid (H-win+1) x (W-win+1) interior of the SSIM map: uniform win x win window
 *             (win odd, >= 3; skimage's default is 7), K1 = 0.01, K2 = 0.03, sample covariance (win^2 / (win^2 - 1)).
 * Arguments are checked before any HIP call (UR_E_INVALID).  ur_image_metrics_ws_size returns UR_E_INVALID for a bad shape.
 * Size limits: N*C*tiles must be below 2^23 (tiles = ceil((W-win+1)/64) * ceil((H-win+1)/16): one 256-thread workgroup per tile and
 *   plane).  The planes are addressed with 64-bit offsets: N*C*H*W has no limit of its own (run past 2^32 bytes in
 *   tests/scoring_large_cases.py). */
int ur_image_metrics(const float* pred, const float* target, int N, int C, int H, int W, int win, double data_range,
                     double* psnr, double* ssim, void* ws, long long ws_bytes, ur_stream_t stream);
long long ur_image_metrics_ws_size(int N, int C, int H, int W, int win);

/* ---- LPIPS (AlexNet features, v0.1 linear layers), exact fp32 (evaluator side) ----------------------------------------------
 * The perceptual distance of the reference's LPIPS(net_type="alex", normalize=True): both images go through AlexNet's five
 * convolutions as ONE batch of 2N (predictions first), every ReLU output is a tap; per tap and pixel the features are
 * unit-normalised over channels (f / (sqrt(sum f^2) + 1e-10)), the squared difference is weighted per channel, averaged over
 * the pixels, and the five taps are added.  All kernels are fp32 on NHWC activations (the convolution on the fp32-input MFMA,
 * a k-ordered fma chain), use no atomics and sum in a fixed order: the same inputs give the same bits, eagerly and in a graph.
 * Every function checks its arguments before any HIP call (UR_E_INVALID).
 *
 * ur_lpips_prep: x fp32 NCHW [N,3,H,W] in [0,1] -> y fp32 NHWC [N,H,W,3] = ((2x - 1) - shift_c) / scale_c, shift = (-.030, -.088,
 *   -.188), scale = (.458, .448, .450).  C must be 3, H and W >= 31 (the smallest input whose fifth tap has a pixel).
 * ur_conv2d_f32: y[N,OH,OW,Cout] = act(conv(x[N,H,W,Cin], w) + bias), OH = (H + 2 pad - KH) / stride + 1, zero padding, relu 0 / 1.
 *   w is the host's repack [Kpad][Cout_pad] of the OIHW filter: row k = (kh * KW + kw) * Cin + cin, column cout, zero-filled up to
 *   the sizes ur_conv2d_f32_wpack_dims gives (K to a multiple of 16, Cout to a multiple of 64), 16-byte aligned.  The
 *   activations are read as they are: padding, the K tail and the M tail cost no copy.  bias fp32 [Cout].
 *   Non-finite inputs (this convolution under all three of its names, and the three max-pools): every output element is finite,
 *   +inf, -inf or NaN exactly where the fp64 computation of the same layer in torch is (F.conv2d + bias + res, torch.relu;
 *   F.max_pool2d) - NaN payload bits apart - and an image that holds no non-finite value gets the bits it gets in a clean batch.
 *   relu = 1 is IEEE 754-2019 maximum(v, 0): NaN stays NaN, +inf stays, -inf becomes 0 (and -0.0 becomes +0.0).  A NaN or an
 *   infinity in any of the K products or in res reaches the output; an input element that no filter tap reads (padding, stride,
 *   dilation) reaches none.
 * ur_maxpool2d_f32: 3x3 window, stride 2, no padding, floor mode: x [N,H,W,C] -> y [N,(H-3)/2+1,(W-3)/2+1,C].  A NaN in any tap
 *   of a window is that window's maximum, as in torch.max_pool2d; a window of -inf gives -inf; a row or column the floor drops
 *   is not read.
 * ur_lpips_layer: feat [2N][P][C] (one tap; images 0..N-1 predictions, N..2N-1 targets), lin fp32 [C] ->
 *   part fp64 [N][ur_lpips_layer_parts(P)]: partial sums over pixels of sum_c lin_c (u_c^pred - u_c^tgt)^2.
 * ur_lpips_finish: ws holds the five taps' partials one after the other (tap t of an H x W input has ur_lpips_tap_hw pixels, its
 *   block starts where tap t-1's N * parts doubles end; ur_lpips_ws_size bytes in all) -> out fp64 [N] = sum over taps, in tap
 *   order, of (sum of the tap's partials in ascending order) / pixels.
 * Size limits (64-bit arithmetic, before any HIP call; run from the accepted side in tests/scoring_large_cases.py):
 *   ur_lpips_prep, ur_lpips_ws_size, ur_lpips_finish: N*H*W must be below 2^28.
 *   ur_conv2d_f32 / ur_conv2d_f32_res: N*OH*OW must be below 2^31 - 128 (int row indices; the last 128-row tile stays inside an int)
 *     and N*H*W below 2^31; Cin*KH*KW and Cout at most 2^24.  x, y and res are addressed with 64-bit offsets: N*H*W*Cin and
 *     N*OH*OW*Cout have no limit of their own.
 *   ur_maxpool2d_f32: N*H*W*C must be below 2^31 (the launch is over the at most N*H*W*C / 9 outputs).
 *   ur_lpips_layer: N in [1, 65535], ceil(P / 64) at most 2^23 - 1; feat is addressed with 64-bit offsets (2N*P*C has no limit). */
int ur_lpips_prep(const float* x, float* y, int N, int C, int H, int W, ur_stream_t stream);
int ur_conv2d_f32_wpack_dims(int Cin, int Cout, int KH, int KW, int* kpad, int* cout_pad);
int ur_conv2d_f32(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                  int stride, int pad, int relu, ur_stream_t stream);
int ur_maxpool2d_f32(const float* x, float* y, int N, int H, int W, int C, ur_stream_t stream);
int ur_lpips_tap_hw(int H, int W, int tap, int* oh, int* ow);
long long ur_lpips_layer_parts(long long P);
int ur_lpips_layer(const float* feat, const float* lin, int N, int P, int C, double* part, long long part_bytes, ur_stream_t stream);
long long ur_lpips_ws_size(int N, int H, int W);
int ur_lpips_finish(const void* ws, long long ws_bytes, int N, int H, int W, double* out, ur_stream_t stream);

/* ---- classifier scoring of the cls output (ResNet top-1 accuracy; exact fp32, NHWC, no atomics, fixed-order sums) ---------
 * The network's convolutions, its FC layer included (a 1x1 convolution on a 1x1 map), are ur_conv2d_f32_res.
 *
 * ur_conv2d_f32_res: ur_conv2d_f32 with y = act(conv(x, w) + bias + res); res fp32 [N,OH,OW,Cout], not y, or NULL - with NULL it
 *   is ur_conv2d_f32, bit for bit (ur_conv2d_f32 calls it so).
 * ur_classify_preprocess: x fp32 NCHW [N,3,H,W] in [0,1] -> y fp32 NHWC [N,224,224,3]: separable resize, the W axis first (into
 *   tmp, fp32 [N,3,H,224]), then the H axis, then (v - mean_c) / std_c with the ImageNet mean (.485, .456, .406) and std (.229,
 *   .224, .225).  Each axis has a table on the device: first[224] (first input index of an output index), count[224] (its taps,
 *   <= taps) and wt[224][taps] (fp32 weights, taps of one output consecutive, summed in ascending order).  The host builds them
 *   (torch's antialiased bilinear rule in fp64, rounded to fp32); indices read from a table are clamped to the axis.  taps <= 64.
 * ur_maxpool2d_pad_f32: 3x3 window, stride 2, padding 1 (-inf, not 0): x [N,H,W,C] -> y [N,(H-1)/2+1,(W-1)/2+1,C].  NaN and -inf as
 *   in ur_maxpool2d_f32.
 * ur_avgpool_f32: x [N,P,C] -> y [N,C], the mean over the P pixels: ascending order in fp64, rounded to fp32 once.
 * ur_top1_counts: logits fp32 [N,C], labels int64 [N] (the CALLER checks 0 <= label < C) -> pred int64 [N], the argmax with ties
 *   to the lowest index and NaN as the maximum (torch.argmax), and counts int64 [3][C] of THIS batch: tp_c (pred = label = c),
 *   targets_c (label = c), predicted_c (pred = c).  Written, not accumulated.
 * Size limits (64-bit arithmetic, before any HIP call).  One thread per element or per output, int indices, 256-thread workgroups:
 *   a launch's count must be below 2^31 - 256 so that the whole last workgroup stays inside an int (csrc/launch_size.h), and the
 *   element counts that can become a launch count carry that bound:
 *   ur_classify_preprocess: N*3*H*max(W, 224) and N*3*224*224 must be below 2^31 - 256.
 *   ur_maxpool2d_pad_f32: N*H*W*C must be below 2^31 - 256 (a 1 x 1 map has as many outputs as inputs).
 *   ur_avgpool_f32: N*P*C must be below 2^31 - 256.          ur_top1_counts: N*C must be below 2^31 - 256. */
int ur_conv2d_f32_res(const float* x, const float* w, const float* bias, const float* res, float* y, int N, int H, int W, int Cin, int Cout,
                      int KH, int KW, int stride, int pad, int relu, ur_stream_t stream);
int ur_classify_preprocess(const float* x, float* tmp, float* y, int N, int C, int H, int W, const int* first_w, const int* count_w,
                           const float* wt_w, int taps_w, const int* first_h, const int* count_h, const float* wt_h, int taps_h,
                           ur_stream_t stream);
int ur_maxpool2d_pad_f32(const float* x, float* y, int N, int H, int W, int C, ur_stream_t stream);
int ur_avgpool_f32(const float* x, float* y, int N, int P, int C, ur_stream_t stream);
int ur_top1_counts(const float* logits, const long long* labels, int N, int C, long long* pred, long long* counts, ur_stream_t stream);

/* ---- segmenter scoring of the seg output (RefineNet-LW mIoU; exact fp32, NHWC, no atomics, fixed-order sums) ----------------
 * The network's convolutions are ur_conv2d_f32_res; its residual input carries the head's `x + up(y)` and `top + x` sums.
 *
 * An align_corners=True axis table (host-built in fp64): idx[n_out] = the first source index of an output index, wt[n_out][2] =
 *   the fp32 weights of sources idx and idx + 1.  Indices read from a table are clamped to the axis.  A pixel is
 *   h0 * (w0 * x00 + w1 * x01) + h1 * (w0 * x10 + w1 * x11), so weights (1, 0) copy a source whose neighbours (right, below) are
 *   finite bit for bit - but for a -0.0, which a non-negative neighbour turns into +0.0; a NaN or infinite neighbour makes the
 *   result NaN (0 x inf), as in torch's own resize.
 * ur_seg_prep: x fp32 NCHW [N,3,H,W] in [0,1] -> y fp32 NHWC [N,OH,OW,3]: the bilinear resize, then v * 255 - mean_c with the
 *   mean (123.68, 116.779, 103.939) of R, G, B, written in B, G, R order.
 * ur_upsample_bilinear_ac_f32: x [N,h,w,C] -> y [N,H,W,C], any C.
 * ur_maxpool5_f32: 5x5 window, stride 1, padding 2 (-inf): x [N,H,W,C] -> y of the same shape.  NaN and -inf as in
 *   ur_maxpool2d_f32, on the float4 path (C % 4 == 0) and the scalar one.
 * ur_add_f32: y[i] = a[i] + b[i] over n fp32 values; y is neither a nor b.
 * ur_seg_tta_argmax: nmaps (1..3) logit maps m_k fp32 [N,h_k,w_k,C], 1 <= C <= 255 (unused maps NULL, sizes ignored) -> pred
 *   uint8 [N,H,W]: per pixel and class every map is sampled bilinearly, the samples averaged as ((a + b) + c) / nmaps, and the
 *   best class kept - ties to the lowest index, NaN as the maximum (torch.argmax).  The tables hold the maps' axes one after the
 *   other: idx_h [nmaps][H], wt_h [nmaps][H][2], idx_w [nmaps][W], wt_w [nmaps][W][2].  avg: NULL, or fp32 [N,H,W,C] that
 *   receives the averaged logits (for tests; without it no full-resolution logit tensor exists anywhere).
 * ur_seg_confusion: pred uint8 [P], target uint8 [P] (target_i64 = 0) or int64 [P] (1) -> conf int64 [C][C], conf[t][p] = the
 *   pixels with target t and prediction p, over the pixels with 0 <= t < C, t != ignore_index and p < C.  Written, not
 *   accumulated.  ws: ur_seg_confusion_ws_bytes(P, C) bytes (0 for invalid arguments) of per-block counts.
 * Size limits (64-bit arithmetic, before any HIP call; the launch rule of the classifier section):
 *   ur_seg_prep: N*3*H*W and N*3*OH*OW must be below 2^31 (the launch is over the N*OH*OW outputs).
 *   ur_upsample_bilinear_ac_f32: N*h*w*C and N*H*W*C must be below 2^31 - 256.     ur_maxpool5_f32: N*H*W*C must be below 2^31 - 256.
 *   ur_add_f32: n in [1, 2^31 - 256).
 *   ur_seg_tta_argmax: N*H*W (N*H*W*C with avg) must be below 2^31 - 256, N*h*w*C of every map below 2^31.
 *   ur_seg_confusion: P in [1, 2^31) (64-bit pixel indices, at most 1024 workgroups that stride over the 4096-pixel chunks). */
int ur_seg_prep(const float* x, float* y, int N, int C, int H, int W, int OH, int OW, const int* idx_h, const float* wt_h, const int* idx_w,
                const float* wt_w, ur_stream_t stream);
int ur_upsample_bilinear_ac_f32(const float* x, float* y, int N, int h, int w, int C, int H, int W, const int* idx_h, const float* wt_h,
                                const int* idx_w, const float* wt_w, ur_stream_t stream);
int ur_maxpool5_f32(const float* x, float* y, int N, int H, int W, int C, ur_stream_t stream);
int ur_add_f32(const float* a, const float* b, float* y, long long n, ur_stream_t stream);
int ur_seg_tta_argmax(const float* m0, const float* m1, const float* m2, int nmaps, int N, int C, int h0, int w0, int h1, int w1, int h2, int w2,
                      int H, int W, const int* idx_h, const float* wt_h, const int* idx_w, const float* wt_w, unsigned char* pred, float* avg,
                      ur_stream_t stream);
long long ur_seg_confusion_ws_bytes(long long P, int C);
int ur_seg_confusion(const unsigned char* pred, const void* target, int target_i64, long long P, int C, int ignore_index, void* ws,
                     long long ws_bytes, long long* conf, ur_stream_t stream);

/* ---- DeepLabV3+ scoring of the seg output (ResNet-50 / 101, output stride 16; exact fp32, NHWC, no atomics) ------------------
 * The backbone's undilated convolutions are ur_conv2d_f32_res, the pooled branch's mean ur_avgpool_f32, the head's half-pixel
 * resize ur_upsample_bilinear_ac_f32 with a half-pixel table, the confusion matrix ur_seg_confusion.
 *
 * A half-pixel (align_corners=False) axis table has the layout of the align_corners=True one: idx[n_out], wt[n_out][2], with the
 *   source coordinate max(0, (o + 0.5) * n_in / n_out - 0.5); idx + 1 is clamped to the axis by the kernels.
 * ur_dlv3_conv2d_f32: ur_conv2d_f32_res (the same kernel: with dil = 1 and ldy = Cout the same bits) with a dilation dil >= 1 -
 *   tap (kh, kw) of output (oh, ow) reads input (oh stride - pad + kh dil, ow stride - pad + kw dil),
 *   OH = (H + 2 pad - dil (KH - 1) - 1) / stride + 1 - and an output row stride ldy >= Cout: pixel m's Cout values go to
 *   y + m * ldy, so with y offset by a channel count a launch fills a channel slice of a wider NHWC buffer (ASPP's five branches
 *   in one 1280-channel tensor) and touches nothing else of it.  res keeps its own dense [N*OH*OW][Cout] layout.
 * ur_dlv3_prep: x fp32 NCHW [N,3,H,W] in [0,1] -> y fp32 NHWC [N,OH,OW,3]: the align_corners=True bilinear resize (tables as for
 *   ur_seg_prep; the identity at the input's own size), then (v - mean_c) / std_c with the ImageNet mean (.485, .456, .406) and
 *   std (.229, .224, .225), channels in R, G, B order.
 * ur_dlv3_broadcast_f32: v fp32 [N][C] -> y[(n * P + p) * ldy + c] = v[n][c] for every pixel p < P: the resize of a 1 x 1 map.
 * ur_dlv3_upsample_f32: ur_upsample_bilinear_ac_f32 (the same table-driven sample; the head passes half-pixel tables) with an
 *   output row stride ldy >= C: x [N,h,w,C] -> y[((n H + oy) W + ox) * ldy + c], a channel slice of a wider NHWC buffer.
 * ur_dlv3_tta_argmax: nmaps (1..3) classifier maps q_k fp32 [N,hq_k,wq_k,C], 1 <= C <= 255 (unused maps NULL, sizes ignored) ->
 *   pred uint8 [N,H,W].  Per output pixel and class, map k is sampled in two stages, neither of which is stored: the
 *   align_corners=True sample of L_k at (H, W) <- (hs_k, ws_k), whose four values are each the half-pixel sample of q_k at
 *   (hs_k, ws_k) <- (hq_k, wq_k); both in fp32 as h0 * (w0 * x00 + w1 * x01) + h1 * (w0 * x10 + w1 * x11).  The samples are
 *   averaged as ((a + b) + c) / nmaps and the best class kept - ties to the lowest index, NaN as the maximum (torch.argmax).
 *   ac_* hold the align_corners=True tables of the maps one after the other: idx [nmaps][H] / [nmaps][W], wt [..][2]; hp_* the
 *   half-pixel ones: idx [hs_0 + hs_1 + ..] / [ws_0 + ws_1 + ..], wt [..][2].  avg: NULL, or fp32 [N,H,W,C] that receives the
 *   averaged logits (for tests).
 * Size limits (64-bit arithmetic, before any HIP call; the launch rule of the classifier section):
 *   ur_dlv3_conv2d_f32: those of ur_conv2d_f32_res - N*OH*OW below 2^31 - 128, N*H*W below 2^31, Cin*KH*KW and Cout at most 2^24,
 *     64-bit offsets into x, y and res - and ldy >= Cout, dil >= 1, and H + 2 pad, W + 2 pad, dil (KH - 1) + 1 and
 *     dil (KW - 1) + 1 each inside an int, the padded map no smaller than the dilated filter.
 *   ur_dlv3_prep: N*3*H*W and N*3*OH*OW must be below 2^31.     ur_dlv3_broadcast_f32: N*P*C must be below 2^31 - 256, ldy >= C.
 *   ur_dlv3_upsample_f32: N*h*w*C and N*H*W*C must be below 2^31 - 256, ldy >= C.
 *   ur_dlv3_tta_argmax: N*H*W (N*H*W*C with avg) must be below 2^31 - 256, N*hq*wq*C of every map below 2^31; hs, ws >= 1.
 *   Runs at these limits on 2-4 GiB tensors are not part of tests/scoring_large_cases.py yet. */
int ur_dlv3_conv2d_f32(const float* x, const float* w, const float* bias, const float* res, float* y, int N, int H, int W, int Cin, int Cout,
                       int KH, int KW, int stride, int pad, int dil, int ldy, int relu, ur_stream_t stream);
int ur_dlv3_prep(const float* x, float* y, int N, int C, int H, int W, int OH, int OW, const int* idx_h, const float* wt_h, const int* idx_w,
                 const float* wt_w, ur_stream_t stream);
int ur_dlv3_broadcast_f32(const float* v, float* y, int N, int P, int C, int ldy, ur_stream_t stream);
int ur_dlv3_upsample_f32(const float* x, float* y, int N, int h, int w, int C, int H, int W, int ldy, const int* idx_h, const float* wt_h,
                         const int* idx_w, const float* wt_w, ur_stream_t stream);
int ur_dlv3_tta_argmax(const float* q0, const float* q1, const float* q2, int nmaps, int N, int C, int hq0, int wq0, int hs0, int ws0, int hq1,
                       int wq1, int hs1, int ws1, int hq2, int wq2, int hs2, int ws2, int H, int W, const int* ac_idx_h,
                       const float* ac_wt_h, const int* ac_idx_w, const float* ac_wt_w, const int* hp_idx_h, const float* hp_wt_h,
                       const int* hp_idx_w, const float* hp_wt_w, unsigned char* pred, float* avg, ur_stream_t stream);

/* ---- ViT scoring of the cls output (torchvision's VisionTransformer; exact fp32, token-major, no atomics, fixed-order sums) ---
 * The network's Linears (patch embedding, in_proj, out_proj, fc1, fc2, head) are the convolution above on tokens [N,1,S,D]; the
 * residual sums ride its res input.  What is new here is csrc/vit.hip.  The same inputs give the same bits, eagerly and under
 * graph replay; an image's results do not depend on its place in the batch.
 *
 * The layer-norm entry point: row r of x starts at x + r * ldx (ldx >= D: ldx = S * D normalises the class-token rows of [N,S,D]
 *   alone), y is dense [rows][D], not x.  y = (x - mean) / sqrt(var + eps) * gamma + beta per row, with the mean first and then
 *   the biased variance of the centred values, both in fp64, rounded to fp32 once.  Any D >= 1; float4 accesses when D and ldx are
 *   multiples of 4 and the four pointers 16-byte aligned.  A row that holds a NaN or an infinity is all NaN, as F.layer_norm.
 * The GELU entry point: y = 0.5 x (1 + erf(x / sqrt 2)) with libm's erff over n values; y may be x.  NaN -> NaN, +inf -> +inf,
 *   -inf -> NaN (the formula's own result).
 * The embedding entry point: patches [N,P,D], class_token [D], pos [P+1,D] -> y [N,P+1,D]: token 0 = class_token + pos[0], token
 *   1 + p = patch p + pos[1 + p].
 * The attention entry point: qkv [N,S,3D] as nn.MultiheadAttention's in_proj writes it (q | k | v, head h in columns h d .. h d +
 *   d - 1 of each) -> out [N,S,D] = softmax(q k^T / sqrt d) v per (image, head), heads concatenated.  Both products run on
 *   v_mfma_f32_32x32x2_f32 with K and V of the head in LDS; the softmax is exact (row maximum, libm expf, fixed-order sum, IEEE
 *   division).  A score row with a NaN or +inf is all NaN, a -inf score has weight 0, a NaN in V reaches every query of its
 *   (image, head).  The size limit of S is what the s_max entry point returns: UR_VIT_S_MAX.
 * Limits (64-bit arithmetic, before any HIP call): layer norm: rows below 2^31 - 256, ldx >= D, eps >= 0.  GELU: n in
 *   [1, 2^31 - 256).  Embedding: N*(P+1)*D below 2^31 - 256.  Attention: d = 64, D = H * d, 1 <= S <= UR_VIT_S_MAX, N*H <= 2^22,
 *   qkv 16-byte aligned, out not qkv. */
#define UR_VIT_S_MAX 256
int ur_vit_attention_s_max(void);
int ur_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int rows, int D, double eps, long long ldx,
                     ur_stream_t stream);
int ur_gelu_f32(const float* x, float* y, long long n, ur_stream_t stream);
int ur_vit_embed_f32(const float* patches, const float* class_token, const float* pos, float* y, int N, int P, int D, ur_stream_t stream);
int ur_vit_attention_f32(const float* qkv, float* out, int N, int S, int H, int d, int D, ur_stream_t stream);

/* ---- Swin-V2 scoring of the cls output (torchvision's SwinTransformer with SwinTransformerBlockV2 / PatchMergingV2; exact fp32,
 * NHWC tokens [N,H,W,C], no atomics, fixed-order sums) ---------------------------------------------------------------------------
 * The network's Linears (patch embedding 4x4 / 4, qkv, proj, mlp.0, mlp.3, the patch-merging reduction as a 2x2 / 2 convolution,
 * head) are the convolution above; LayerNorm and GELU are the ViT block's.  What is new is csrc/swin.hip and the residual layer norm.
 *
 * The residual layer-norm entry point: y = res + LN(x) over dense [rows][D]: the layer-norm entry point's fp64 moments and single
 *   rounding to fp32, then one fp32 addition - the post-norm residual x + norm(f(x)) of a V2 block in one pass.  y is neither x
 *   nor res.  A row of x that holds a NaN or an infinity is all NaN; a non-finite res element stays in its place.
 * The window-attention entry point: qkv [N,H,W,3C] (q | k | v, head h in columns 32 h .. 32 h + 31 of each; C = 32 heads), qkv_bias
 *   [3C], scale [heads], bias [heads,64,64] -> out [N,H,W,C], all fp32.  Attention inside 8 x 8 windows of the map, zero-padded on
 *   the bottom and right to multiples of 8 and rolled by (-shift, -shift) (per axis the shift is 0 when the padded axis is one
 *   window): score = normalize(q) . normalize(k) * scale[h] + bias[h][i][j] - 100 where the two tokens' regions differ (only when
 *   a shift is in force), normalize(v) = v / max(|v|, 1e-12); softmax over the window's 64 slots; P V; each real token's result
 *   goes back to its own (i, j).  A padded token takes its q, k, v from qkv_bias (the Linear of a zero row) and is NOT masked, as
 *   in torchvision; the caller zeroes the k third of qkv_bias as torchvision's forward does.  No padded, rolled or partitioned
 *   tensor is ever written.  Both products run on v_mfma_f32_32x32x2_f32 with the window's K and V in LDS; the softmax is exact
 *   (row maximum, libm expf, fixed-order sum, IEEE division).  A score row with a NaN or +inf is all NaN, a NaN in V reaches every
 *   query of its (window, head); other images keep their bits.
 * Limits (64-bit arithmetic, before any HIP call): residual layer norm: rows below 2^31 - 256, eps >= 0.  Window attention: N, H,
 *   W, heads >= 1, shift 0 or 4, N*H*W below 2^31, N * ceil(H/8) * ceil(W/8) * heads below 2^31 - 256 (one workgroup per (image,
 *   window, head)), qkv, qkv_bias and bias 16-byte aligned, out not qkv. */
int ur_layernorm_res_f32(const float* x, const float* res, const float* gamma, const float* beta, float* y, int rows, int D, double eps,
                         ur_stream_t stream);
int ur_swin_attention_f32(const float* qkv, const float* qkv_bias, const float* scale, const float* bias, float* out, int N, int H,
                          int W, int heads, int shift, ur_stream_t stream);

/* ---- RVT scoring of the cls output (the reference's own PoolingTransformer, src/modules/rvt/robust_models.py; exact fp32, NHWC
 * tokens [N,H,W,C] = [N,S,C], no atomics, fixed-order sums) ---------------------------------------------------------------------
 * The network's Linears and 1 x 1 convolutions (the two stem convolutions, qkv, proj, fc1, fc2, head) are the convolution above
 * with every BatchNorm folded in; LayerNorm, GELU, the padded max-pool and the mean over the map exist.  What is new is csrc/rvt.hip.
 *
 * The attention entry point: qkv [N,S,3 H d] (q | k | v, head h in columns h d .. h d + d - 1 of each), gate [H,S,S] or NULL ->
 *   out [N,S,H d], all fp32.  score[i][j] = ((q_i . k_j) * d^-0.5) * gate[h][i][j] (without a gate: the scaled dot product), then
 *   an exact softmax over the S keys and P V, per (image, head) - RVT's position-aware attention scaling with gate =
 *   sigmoid(att_mask).  d = 64: q is scaled by 1/8 before the product (exact); d = 32: the finished dot product is multiplied by
 *   fp32(32^-0.5); the gate is one more fp32 multiplication.  With gate NULL and d = 64 the result equals the ViT attention entry
 *   point's bit for bit.  Both products run on v_mfma_f32_32x32x2_f32 with K and V of the head in LDS (rows d + 1 and d floats
 *   apart); the gate is read from global memory, as float4 when S % 4 == 0 and gate is 16-byte aligned.  Non-finite values as the
 *   ViT entry point; a gate of exactly 0 against an infinite score is NaN, as in torch.
 * The depthwise entry point: x NHWC [N,H,W,C], w [9][C mult] (tap-major: w[3 ky + kx][o] is the OIHW filter's [o][0][ky][kx]),
 *   bias [C mult] -> y [N,OH,OW,C mult], OH = (H - 1) / stride + 1 (3 x 3, pad 1).  Output channel o reads input channel o / mult
 *   (groups = C).  y = act(sum over the taps inside the map, in row-major tap order with fmaf from 0, + bias); act 0: none, 1: the
 *   GELU entry point's function (the same bits as act 0 followed by it).  A tap in the padding is skipped, so a non-finite input
 *   reaches only the outputs whose window holds it.  float4 accesses when mult == 1, C % 4 == 0 and the four pointers are 16-byte
 *   aligned.
 * Limits (64-bit arithmetic, before any HIP call): attention: d 32 or 64, 1 <= S <= UR_VIT_S_MAX, N, H >= 1, N*H <= 2^22, qkv
 *   16-byte aligned, out and gate 4-byte aligned, out overlapping neither qkv nor gate.  Depthwise: N, H, W, C, mult >= 1, stride 1
 *   or 2, act 0 or 1, N*H*W*C and N*OH*OW*C*mult below 2^31 - 256, pointers 4-byte aligned, y overlapping none of x, w, bias. */
int ur_rvt_attention_f32(const float* qkv, const float* gate, float* out, int N, int S, int H, int d, ur_stream_t stream);
int ur_dwconv3x3_f32(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, int mult, int stride, int act,
                     ur_stream_t stream);

/* ---- VGG scoring of the cls output (torchvision's VGG 11 / 13 / 16 / 19, with or without BatchNorm; exact fp32, NHWC, no atomics,
 * fixed-order sums) ------------------------------------------------------------------------------------------------------------
 * The 3 x 3 convolutions are the convolution above with the BatchNorm folded in.  What is new is csrc/vgg.hip.
 *
 * The Linear: y[M][N] = act(x[M][K] . W^T + bias), relu 0 or 1 (maximum(v, 0): NaN and +inf stay, -inf becomes 0), for a few rows
 *   against a large matrix.  The weights are streamed once per 32 rows: K is split into S = ceil(K / 512) parts over the grid
 *   (ceil(N / 128) x S x ceil(M / 32) workgroups; S and every tile boundary depend on K and N alone, never on M), each part is a
 *   k-ordered chain on v_mfma_f32_32x32x2_f32 restarted every 256 products, the fp32 partial sums go to ws[S][M][N] with plain
 *   stores, and a second launch adds them in ascending s in fp64, adds the bias, rounds to fp32 once and applies the ReLU.  An output
 *   row depends on its own input row alone: it has the same bits alone, in any batch and at any position, and a NaN or an infinity
 *   in one row of x reaches that row only.  Rows >= M, columns >= N and k >= K are zeros made in registers, never read.
 *   wp is the kernel's own layout, made once on the host: float4 [npad / 32][kpad / 8][64], element j of lane l in (column tile c,
 *   k block b) = W[32 c + (l & 31)][8 b + 4 (l >> 5) + j] of the [N][K] matrix, zero for a column >= N or k >= K;
 *   ur_vgg_linear_wpack_dims gives kpad (K rounded up to 64), npad (N rounded up to 32) and S.  ws: ur_vgg_linear_ws_bytes(M, K, N)
 *   = 4 S M N bytes (0 for sizes outside the limits).
 * The max-pool: 2 x 2 / stride 2, no padding, floor mode: [N,H,W,C] -> [N,H/2,W/2,C]; an odd last row or column is not read; a NaN
 *   tap is the window's maximum and a window of -inf gives -inf, as the max-pools above.  float4 accesses when C % 4 == 0 and both
 *   pointers are 16-byte aligned.
 * The adaptive average pool: [N,H,W,C] -> [N,7,7,C], output (i, j) is the mean of rows [floor(i H / 7), ceil((i + 1) H / 7)) and the
 *   columns likewise (F.adaptive_avg_pool2d), summed row-major in fp64, divided by the count, rounded to fp32 once.  On a 7 x 7 map
 *   it returns the input's bits; smaller maps replicate values.
 * Limits (64-bit arithmetic, before any HIP call): Linear: 1 <= M <= 2^20, 1 <= K, N <= 2^24, M*N below 2^31 - 256, wp 16-byte and
 *   x, bias, y, ws 4-byte aligned, ws_bytes >= ur_vgg_linear_ws_bytes, y, ws and x not overlapping.  Max-pool: N, C >= 1, H, W >= 2,
 *   N*H*W*C below 2^31 - 256, y not x.  Average pool: N, C, H, W >= 1, N*H*W*C and N*49*C below 2^31 - 256, y not x. */
int ur_vgg_linear_wpack_dims(int K, int N, int* kpad, int* npad, int* splits);
long long ur_vgg_linear_ws_bytes(int M, int K, int N);
int ur_vgg_linear_f32(const float* x, const float* wp, const float* bias, float* y, void* ws, long long ws_bytes, int M, int K, int N,
                      int relu, ur_stream_t stream);
int ur_vgg_maxpool2_f32(const float* x, float* y, int N, int H, int W, int C, ur_stream_t stream);
int ur_vgg_avgpool7_f32(const float* x, float* y, int N, int H, int W, int C, ur_stream_t stream);

/* ---- colour correction of a restored image (between the decoder's conv_out and the egress kernels) ----------------------
 * c fp32 NHWC [N,H,W,ld_c]: the restored image; src 16-bit NHWC [src_n,H,W,ld_s]: the image the encoder saw, image n is corrected
 * against source n % src_n (a task-major K*B batch against B sources); out fp32 NHWC [N,H,W,ld_c], not c.  Channels 0..2 are RGB;
 * channels [3, ld) of c and src are never used in arithmetic and those of out are written as zeros.
 *   wavelet: out = c + L(src - c), L = B_16 B_8 B_4 B_2 B_1, B_r(v)[y,x] = sum over i,j in {-1,0,1} of k_i k_j v[clamp(y + i r), clamp(x + j r)],
 *            k = (1/4, 1/2, 1/4), clamp to the image at every level (replicate border): the restored detail on the source's level-5
 *            low band.  Two launches (the five vertical levels in LDS, then the five horizontal ones); out holds the value between.
 *   adain:   out = (c - mu_c) * (sigma_s / sigma_c) + mu_s per image and channel over the H*W pixels, sigma = sqrt(unbiased variance
 *            + 1e-5); fp64 fixed-order statistics, fp32 (a, b) and out = a*c + b.  ws: ur_color_fix_adain_ws_bytes(N, H, W) bytes,
 *            8-byte aligned (that function returns 0 for a non-positive argument).
 * UR_E_INVALID before any launch for a null pointer, N, src_n, H or W <= 0, N % src_n != 0, ld_c or ld_s < 3, an unknown dtype,
 * out == c, for adain H*W < 2 or a workspace that is too small.  No allocation, no synchronisation, no atomics: the same inputs
 * give the same bits. */
int ur_color_fix_wavelet(const void* c_f32, int ld_c, const void* src_16, int ld_s, float* out, int N, int src_n, int H, int W, int dtype,
                         ur_stream_t stream);
int ur_color_fix_adain(const void* c_f32, int ld_c, const void* src_16, int ld_s, float* out, int N, int src_n, int H, int W, int dtype,
                       void* ws, size_t ws_bytes, ur_stream_t stream);
size_t ur_color_fix_adain_ws_bytes(int N, int H, int W);

/* ---- corruptions of 8-bit images (ImageNet-C semantics; the planner is unirestore_amd/corrupt.py) ---------------------------
 * x u8 [N,H,W,3] contiguous HWC on the device, H and W >= 32, N*H*W*3 < 2^31; out of the same shape, not x: u8 for out_kind 0,
 * fp32 for out_kind 1.  Every primitive computes a value v in fp32 on the 0-255 scale; out_kind 1 stores clamp(v, 0, 255),
 * out_kind 0 the floor of that (truncation, as numpy's cast to uint8).  keys: DEVICE uint32 [N][2] as for ur_keyed_noise; element e
 * of a field takes word e & 3 of the Philox counter (e >> 2, draw, 0, 0) under image n's key, uniforms and normals as
 * ur_keyed_noise's; for the image fields e = (y*W + x)*3 + ch.  All tables are DEVICE memory and read by the kernels.
 *   ur_corrupt_noise  mode 0 gaussian: v = x + c*n (draw 16, c = 255 sigma);  mode 1 speckle: v = x + x*(c*n) (draw 17, c = sigma);
 *       mode 2 impulse: u1 = uniform of draw 18, u2 of draw 19; u1 < c flips the element to 255 if u2 < 0.5 else to 0, any other
 *       element keeps x (c = amount);  mode 3 shot: k = the number of j in [0, 128) with table[x][j] <= (word of draw 20) >> 8, at
 *       most 127, v = (k*255)/c (one correctly rounded division; table uint32 [256][128], row x = floor(2^24 CDF) of Poisson(x*c/255)).
 *   ur_corrupt_filter_sep  v = sum_k taps[k+r] * t[clamp(x+k)], t = sum_k taps[k+r] * x[clamp(y+k)] (rows first, k ascending, fp32
 *       accumulation, replicate border); taps fp32 [2*radius+1]; ws holds t.
 *   ur_corrupt_taps  v = sum over t (ascending) of w_t * x[b(y + ty_t)][b(x + tx_t)] per channel; taps int32 [n_taps][3] = (tx, ty,
 *       the fp32 bits of w), or [N][n_taps][3] with per_image 1; b = replicate (border 0) or reflect-101 (border 1; an index still
 *       outside after one reflection is clamped).  A tap of weight 0 adds nothing: pad shorter lists with (0, 0, 0.0f).
 *   ur_corrupt_zoom  v = (x + sum of the layers) / (n_layers + 1); layers int32 [n_layers][6] = (top, left, ch, cw, oh, ow): the crop
 *       [top, top+ch) x [left, left+cw) resampled bilinearly to oh x ow, of which the top-left H x W is used (a pixel beyond oh x ow
 *       gets nothing from that layer).  Output index o reads position o*(in-1)/(out-1): the cell by integer division, the fraction
 *       (remainder)/(out-1) in fp32; value a + fy*(b - a) with a, b = p0 + fx*(p1 - p0) on the two rows.
 *   ur_corrupt_color  mode 0 contrast: v = (x - mean_c)*a + mean_c, mean_c = the image's exact integer channel sum / (H*W), divided in
 *       fp64 and rounded to fp32;  mode 1 brightness / mode 2 saturate: V = max(r,g,b), delta = V - min, S = delta/V (0 for delta 0),
 *       hue h6 in [0, 6) = 4 + (r-g)/delta if b is the maximum, else 2 + (b-r)/delta if g is, else (g-b)/delta (+6 if negative), 0 for
 *       delta 0; mode 1: V = clamp(V + a, 0, 255), mode 2: S = clamp(S*a + b, 0, 1); back with i = floor(h6), f = h6 - i,
 *       p = V(1-S), q = V(1-fS), t = V(1-(1-f)S): (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q) for i = 0..5.
 *   ur_corrupt_pixelate  box tables int32 [small][2] = (first, count) of the source range an output index of the reduced image
 *       averages, the mean rounded half up to u8: the horizontal pass first (into ws), then the vertical one; ymap [H] / xmap [W]
 *       = the reduced image's row / column a full-size pixel copies.  Integers throughout.
 *   ur_corrupt_fog  a diamond-square map of M x M fp32 cells per image, M = the power of two >= max(H, W, 32): cell (0,0) = 0; for
 *       step = M, M/2, .., 2 with wibble = fp32(100 / decay^level) (fp64 on the host): the centre of every step x step square =
 *       ((c00 + c10) + (c01 + c11))/4 + r, then the midpoint of its top edge = ((centre + the centre above) + (corner + the corner
 *       to the right))/4 + r and of its left edge = ((centre + the centre to the left) + (corner + the corner below))/4 + r,
 *       neighbours wrapping around; r = wibble*(wibble*(2u - 1)), u = the uniform of element y*M + x of draw 21.  Then
 *       v = (x + c*(map[y][x] - min)/(max - min)) * (m/(m + c)), min / max over the whole map, m = the image's largest byte,
 *       c = 255 * the reference's constant.
 * ws: the matching _ws_bytes function's size (0 for a non-positive argument), 8-byte aligned.  UR_E_INVALID before any HIP call
 * for a null pointer, N <= 0, H or W < 32, an image of 2^31 elements or more, out == x, an unknown mode / border / out_kind, a
 * misaligned fp32 out, table or workspace, a table size out of range or a workspace that is too small.  No allocation, no
 * synchronisation, no atomics: the same inputs give the same bits. */
int ur_corrupt_noise(const uint8_t* x, const uint32_t* keys, void* out, int N, int H, int W, int mode, float c, const uint32_t* table,
                     int out_kind, ur_stream_t stream);
int ur_corrupt_filter_sep(const uint8_t* x, const float* taps, int radius, void* out, int N, int H, int W, void* ws, size_t ws_bytes,
                          int out_kind, ur_stream_t stream);
size_t ur_corrupt_filter_sep_ws_bytes(int N, int H, int W);
int ur_corrupt_taps(const uint8_t* x, const int32_t* taps, int n_taps, int per_image, int border, void* out, int N, int H, int W,
                    int out_kind, ur_stream_t stream);
int ur_corrupt_zoom(const uint8_t* x, const int32_t* layers, int n_layers, void* out, int N, int H, int W, int out_kind, ur_stream_t stream);
int ur_corrupt_color(const uint8_t* x, void* out, int N, int H, int W, int mode, float a, float b, void* ws, size_t ws_bytes, int out_kind,
                     ur_stream_t stream);
size_t ur_corrupt_color_ws_bytes(int N, int H, int W);
int ur_corrupt_pixelate(const uint8_t* x, void* out, int N, int H, int W, int small_h, int small_w, const int32_t* hbox, const int32_t* vbox,
                        const int32_t* ymap, const int32_t* xmap, void* ws, size_t ws_bytes, int out_kind, ur_stream_t stream);
size_t ur_corrupt_pixelate_ws_bytes(int N, int H, int small_w);
int ur_corrupt_fog(const uint8_t* x, const uint32_t* keys, void* out, int N, int H, int W, float c, double decay, void* ws, size_t ws_bytes,
                   int out_kind, ur_stream_t stream);
size_t ur_corrupt_fog_ws_bytes(int N, int H, int W);

/* ---- JPEG compression as a degradation: the bytes a baseline JPEG decodes to (the planner is unirestore_amd/jpeg.py) ---------
 * x u8 [N,H,W,3] contiguous HWC RGB on the device, H and W >= 16; out of the same shape, not x.  quality 1..100; subsampling 0
 * (4:4:4) or 2 (4:2:0), Pillow's codes.  out = what Pillow (libjpeg-turbo) reads back from save(quality, subsampling), byte for
 * byte: only the lossy steps are computed, the entropy coder is lossless and absent.  Everything is int32, >> is the arithmetic
 * shift, D(v, n) = (v + (1 << (n-1))) >> n.
 *   tables   the Annex-K luminance and chrominance tables in natural order, entry = clamp((base*s + 50)/100, 1, 255), s = 5000/quality
 *            (integer division) for quality < 50, else 200 - 2*quality; built once per call on the host.
 *   colour   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128<<16) + 32767) >> 16,
 *            Cr = (32768 R - 27439 G - 5329 B + (128<<16) + 32767) >> 16.
 *   planes   Y is padded by edge replication to multiples of 8 in both directions; for 4:4:4 so are Cb and Cr.  For 4:2:0 with
 *            ch = ceil(H/2), cw = ceil(W/2) and chb, cwb their round-ups to 8: the full-size chroma is edge-replicated to 2*ch rows
 *            and 2*cwb columns, reduced with (a00 + a01 + a10 + a11 + bias) >> 2, bias 1 for even output columns and 2 for odd, and
 *            the reduced plane is then edge-replicated downwards from ch to chb rows (rows beyond ch copy the last reduced row).
 *   block    per 8 x 8 block: subtract 128; the forward "islow" DCT (CONST_BITS 13, PASS1_BITS 2), rows then columns, on
 *            t0..t3 = d0+d7, d1+d6, d2+d5, d3+d4, t4..t7 = d3-d4, d2-d5, d1-d6, d0-d7, t10, t13 = t0 +- t3, t11, t12 = t1 +- t2:
 *              o0, o4 = t10 +- t11;  e = 4433 (t12 + t13): o2 = e + 6270 t13, o6 = e - 15137 t12;
 *              z5 = 9633 (t4+t5+t6+t7), z1 = -7373 (t4+t7), z2 = -20995 (t5+t6), z3 = -16069 (t4+t6) + z5, z4 = -3196 (t5+t7) + z5:
 *              o7 = 2446 t4 + z1 + z3, o5 = 16819 t5 + z2 + z4, o3 = 25172 t6 + z2 + z3, o1 = 12299 t7 + z1 + z4;
 *            pass 1 stores o0, o4 shifted left by 2 and the others as D(., 11), pass 2 stores D(o0, 2), D(o4, 2) and the others as
 *            D(., 15): 8 times the DCT.  Quantise with d = q << 3, rounding half away from zero: sign(c) * ((|c| + (d >> 1)) / d);
 *            dequantise with coef * q.  The inverse "islow" DCT, columns with D(., 11) then rows with D(., 18):
 *              e = 4433 (c2 + c6), e2 = e - 15137 c6, e3 = e + 6270 c2, e0, e1 = (c0 +- c4) << 13, t10, t13 = e0 +- e3, t11, t12 = e1 +- e2;
 *              z5 = 9633 (c7+c5+c3+c1), z1 = -7373 (c7+c1), z2 = -20995 (c5+c3), z3 = -16069 (c7+c3) + z5, z4 = -3196 (c5+c1) + z5,
 *              a0 = 2446 c7 + z1 + z3, a1 = 16819 c5 + z2 + z4, a2 = 25172 c3 + z2 + z3, a3 = 12299 c1 + z1 + z4;
 *              outputs 0..7 = t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3;
 *            add 128 and clamp to 0..255 (libjpeg-turbo's SIMD path saturates; plain libjpeg's table wraps).
 *   decode   Y cropped to H x W, chroma to ch x cw.  4:2:0 "fancy" upsampling: the two output rows of a chroma row are
 *            v = 3*this + above and 3*this + below, then the even output column is (3 v + v_left + 8) >> 4 and the odd one
 *            (3 v + v_right + 7) >> 4, neighbours edge-replicated inside ch x cw; cropped to H x W.
 *            R = Y + ((91881 (Cr-128) + 32768) >> 16), G = Y + ((-22554 (Cb-128) - 46802 (Cr-128) + 32768) >> 16),
 *            B = Y + ((116130 (Cb-128) + 32768) >> 16), each clamped to 0..255.
 *   ranges   no int32 product overflows.  The forward DCT's output is 8 times an orthonormal transform of 64 samples in
 *            [-128, 127], so |c| <= 8 * 8 * 128 = 2^13 up to rounding; a pass-1 value is below 4 * 8 sqrt(2) * 128 = 5793, a t4..t7 of
 *            pass 2 below T = 11586, and the crudest bound of an odd output, every term at its maximum with one sign,
 *            (25172 + 2*20995 + 2*16069 + 4*9633) T = 1.6e9, is below 2^31; the even outputs are smaller.  The inverse sees |coef * q| <= |c|/8 + q/2 < 2^11, the range jidctint.c is written for.  The quantiser's division
 *            is a multiply-high by m = ceil(2^32 / d): with n = |c| + (d >> 1) < 2^14 and m d - 2^32 < d <= 2040, n (m d - 2^32) <
 *            2^32, which makes floor(n m / 2^32) = floor(n / d) for every n.
 * ws: ur_jpeg_roundtrip_ws_bytes(N, H, W, subsampling) bytes (the padded u8 planes; 0 for a non-positive argument or an unknown
 * subsampling), 8-byte aligned; nothing in it is read before this call has written it.  UR_E_INVALID before any HIP call for a null
 * pointer, N <= 0, H or W < 16, N*(H+7)*(W+7)*3 >= 2^31, quality outside 1..100, a subsampling other than 0 and 2, out == x, a
 * misaligned workspace or one that is too small.  No allocation, no synchronisation, no atomics: the same inputs give the same bits. */
int ur_jpeg_roundtrip(const uint8_t* x, uint8_t* out, int N, int H, int W, int quality, int subsampling, void* ws, size_t ws_bytes,
                      ur_stream_t stream);
size_t ur_jpeg_roundtrip_ws_bytes(int N, int H, int W, int subsampling);

/* ---- antialiased resize of 8-bit images: the bytes torch's CPU interpolate(uint8, antialias=True) gives, which is what
 * torchvision v2's resize of a uint8 tensor runs (the planner is unirestore_amd/resize.py) ---------------------------------------
 * x u8 [N,H,W,3] contiguous HWC on the device -> out u8 [N,oh,ow,3], not x; H, W, oh and ow >= 2.  Two 1-D passes: ALONG THE WIDTH
 * FIRST, into a u8 intermediate [N,H,ow,3] in ws, then along the height.  A pass whose input and output length are equal is
 * skipped; with both equal out is a copy of x.  The kernels know no filter: the caller builds, per axis n_in -> n_out, in fp64 on
 * the host, and hands over as DEVICE int32 tables
 *   bounds [n_out][2] = (xmin, xsize) and weights [n_out][K], with K and one precision p for the whole axis:
 *     scale = n_in / n_out; isz = 2 (bilinear) or 4 (bicubic); support = isz/2 * scale if scale >= 1 else isz/2;
 *     inv = 1/scale if scale >= 1 else 1; K = ceil(support)*2 + 1.  For output index i: c = scale*(i + 0.5),
 *     xmin = max(int(c - support + 0.5), 0), xsize = min(int(c + support + 0.5), n_in) - xmin,
 *     w_j = f((j + xmin - c + 0.5) * inv) for j < xsize, divided by their sum (added in ascending j); the other slots are 0.
 *     f(t) = 1 - |t| below 1 (bilinear); the Keys cubic with a = -0.5 (bicubic): ((a+2)|t| - (a+3)) t^2 + 1 below 1,
 *     (((|t| - 5)|t| + 8)|t| - 4) a below 2; 0 beyond.
 *     p = the smallest of 0..21 with int(0.5 + wmax * 2^(p+1)) >= 2^15, wmax the largest weight of the axis, else 22;
 *     W_j = int(0.5 + w_j * 2^p), or int(-0.5 + w_j * 2^p) for a negative w_j (both truncate towards zero).
 *   out byte = clamp((2^(p-1) + sum_j W_j * src[xmin + j]) >> p, 0, 255): int32 accumulation, arithmetic shift.
 * The rounded weights of a row need not sum to 2^p, so a constant image does not always come back constant: that is the target.
 * The float path (interpolate(float).round()) and Pillow's BILINEAR are different functions and differ by one in some bytes.
 * A table row with xmin < 0, xsize < 0, xsize > K or xmin + xsize > n_in is read as xsize = 0: no kernel reads outside x, the
 * tables or ws.  The tables of a skipped pass are not read but must still be given.
 * ws: ur_resize_u8_ws_bytes(N, H, W, oh, ow) bytes (the intermediate, rounded up to 8; 0 for a non-positive argument), 8-byte
 * aligned; nothing in it is read before this call has written it.  UR_E_INVALID before any HIP call for a null pointer, N <= 0, a
 * side below 2, N*H*W*3, N*oh*ow*3 or N*H*ow*3 >= 2^31, K outside 1..65536, p outside 1..22, out == x, a misaligned table or
 * workspace, or a workspace that is too small.  No allocation, no synchronisation, no atomics: the same inputs give the same
 * bits. */
int ur_resize_u8(const uint8_t* x, uint8_t* out, int N, int H, int W, int oh, int ow, const int32_t* xbounds, const int32_t* xweights, int xK,
                 int xp, const int32_t* ybounds, const int32_t* yweights, int yK, int yp, void* ws, size_t ws_bytes, ur_stream_t stream);
size_t ur_resize_u8_ws_bytes(int N, int H, int W, int oh, int ow);

/* ---- glass blur, snow and elastic transform: the corruptions that work on float fields between the u8 ends (the planner is
 * unirestore_amd/distort.py; siblings of ur_corrupt_*, whose conventions hold: x u8 [N,H,W,3] HWC on the device, H and W >= 32,
 * N*H*W*3 < 2^31, fp32 values v on the 0-255 scale, out_kind 1 stores clamp(v, 0, 255) as fp32 and out_kind 0 its floor as u8, keys
 * DEVICE uint32 [N][2], uniforms and normals as ur_keyed_noise's) -----------------------------------------------------------------
 * Element e = y*W + x of a per-pixel field [H][W] takes word e & 3 of the Philox counter (e >> 2, draw, 0, 0) under image n's key.
 * Draw numbers: 32..37 glass_blur (iteration i: 32 + 2i for dy, 33 + 2i for dx), 40 snow, 48 / 49 elastic_transform (dy / dx);
 * 0, 1 and 16..21 are taken by ur_keyed_noise's callers and ur_corrupt_*.
 *   glass_blur = ur_corrupt_filter_sep (out_kind 0) -> `iterations` times ur_distort_shuffle -> ur_corrupt_filter_sep.
 *   ur_distort_shuffle  one iteration, u8 -> u8, integers throughout: a pixel with delta <= y < H - delta and delta <= x < W - delta
 *       becomes the whole pixel x[y + dy][x + dx], dy = ((word of `draw` * 2 delta) >> 32) - delta (a 64-bit product), dx the same
 *       from draw + 1: independent integers in [-delta, delta); every other pixel is copied.  delta in 1..4; out != x.
 *   snow = ur_distort_snow_layer -> ur_distort_snow.
 *   ur_distort_snow_layer  field fp32 [N][oh][ow]: layer[y][x] = loc + scale*n, n = the normal of element y*W + x of draw 40; the crop
 *       [top, top+ch) x [left, left+cw) of the layer is resampled bilinearly to oh x ow exactly as a layer of ur_corrupt_zoom is
 *       (position o*(in-1)/(out-1): the cell by integer division, the fraction (remainder)/(out-1) in fp32, a + fy*(b - a) with
 *       a, b = p0 + fx*(p1 - p0)); a value < thr becomes 0, every other one is clamped to [0, 1].  The normals are drawn at the four
 *       source cells; nothing else is stored.  oh >= H, ow >= W, both <= 32768, N*oh*ow < 2^31, scale > 0.
 *   ur_distort_snow  s = sum over t (ascending) of w_t * field[clamp(y + ty_t)][clamp(x + tx_t)] (replicate border of the oh x ow
 *       field; taps int32 [N][n_taps][3] = (tx, ty, the fp32 bits of w) per image, n_taps in 1..64, pad a shorter list with
 *       weight-0 taps), L[y][x] = rint(255*s) (round half to even) as u8 for y < H, x < W, held in ws; then, in a second launch so
 *       that all of L is written before any of it is read, per channel
 *         v = (keep*x + (1 - keep)*max(x, 1.5*g + 127.5)) + (L[y][x] + L[H-1-y][W-1-x]),  g = 0.299 R + 0.587 G + 0.114 B,
 *       keep in [0, 1], N <= 65535.  ws: ur_distort_snow_ws_bytes(N, H, W).
 *   elastic_transform = ur_distort_field -> ur_distort_warp.
 *   ur_distort_field  field fp32 [N][2][H][W], plane 0 = dy (draw 48), plane 1 = dx (draw 49): f = m*(2u - 1), u = the uniform of
 *       element y*W + x; t = sum_k taps_y[k+ry] * f[r(y+k)][x], then field = alpha * sum_k taps_x[k+rx] * t[y][r(x+k)] (k ascending,
 *       fp32), r = the half-sample-symmetric reflection (d c b a | a b c d, periodic).  taps fp32 [2*radius+1], radii in 0..255,
 *       m >= 0.  ws: ur_distort_field_ws_bytes(N, H, W); field is not ws.
 *   ur_distort_warp  per channel the bilinear sample of x at (py, px) = (y + field[n][0][y][x], x + field[n][1][y][x]), each sum
 *       rounded once to fp32 and limited to +-1e6: i = floor(p), f = p - i, rows r(iy), r(iy + 1) and columns r(ix), r(ix + 1) with
 *       the same reflection r, value a + fy*(b - a), a, b = p0 + fx*(p1 - p0).  A field of zeros returns x.
 * UR_E_INVALID before any HIP call for a null pointer, N <= 0, H or W < 32, an image of 2^31 elements or more, out == x, an unknown
 * out_kind, a misaligned fp32 array, table or workspace, a size, radius, delta or constant out of the ranges above, or a workspace
 * that is too small; the _ws_bytes functions return 0 for a non-positive argument.  Workspaces are 8-byte aligned and nothing in
 * them is read before the call has written it.  No allocation, no synchronisation, no atomics: the same inputs give the same bits. */
int ur_distort_shuffle(const uint8_t* x, const uint32_t* keys, uint8_t* out, int N, int H, int W, int delta, uint32_t draw, ur_stream_t stream);
int ur_distort_snow_layer(const uint32_t* keys, float* field, int N, int H, int W, int top, int left, int ch, int cw, int oh, int ow, float loc,
                          float scale, float thr, ur_stream_t stream);
int ur_distort_snow(const uint8_t* x, const float* field, const int32_t* taps, int n_taps, void* out, int N, int H, int W, int oh, int ow,
                    float keep, void* ws, size_t ws_bytes, int out_kind, ur_stream_t stream);
size_t ur_distort_snow_ws_bytes(int N, int H, int W);
int ur_distort_field(const uint32_t* keys, const float* taps_y, int ry, const float* taps_x, int rx, float* field, int N, int H, int W, float m,
                     float alpha, void* ws, size_t ws_bytes, ur_stream_t stream);
size_t ur_distort_field_ws_bytes(int N, int H, int W);
int ur_distort_warp(const uint8_t* x, const float* field, void* out, int N, int H, int W, int out_kind, ur_stream_t stream);

/* ---- NIQE block features (no-reference quality, evaluator side; csrc/niqe.hip) ----------------------------------------------------
 * The natural-scene-statistics features of the NIQE score, as unirestore_amd/niqe.py chains them.  Everything is fp64; no kernel
 * uses atomics and every sum has a fixed order, so the same inputs give the same bits, eagerly and in a graph.  No expression is
 * contracted into a fused multiply-add.  Elements are addressed with 64-bit offsets.
 * ur_niqe_luma: x fp32 NCHW [N,3,H,W] in [0,1] -> y fp64 [N,h,w], the top-left h x w crop (h <= H, w <= W) of
 *     color_space 0 (yiq):   rint(((0.299 R + 0.587 G) + 0.114 B) * 255)
 *     color_space 1 (ycbcr): rint(((16 + 65.481 R) + 128.553 G) + 24.966 B)            (rint: round half to even)
 * ur_niqe_mscn: y fp64 [N,h,w] -> m = (y - mu) / (sqrt(|G*y^2 - mu^2|) + 1), mu = G*y, G the 7 x 7 Gaussian of sigma 7/6 normalised
 *     to sum 1 and applied separably (g_k = exp(-(k-3)^2 / (2 sigma^2)) / sum, the row pass first, taps ascending), with a replicate
 *     border at the edge of the h x w field.  m must not be y.
 * ur_niqe_block_moments: field fp64 [N,h,w], bs 96 or 48, h and w multiples of bs -> moments fp64 [N][blocks][5][6], the blocks in
 *     row-major order.  Fields: M, then M * roll(M, s) for s = (0,1), (1,0), (1,1), (1,-1), roll(M, s)[i][j] =
 *     M[(i - s0) mod bs][(j - s1) mod bs] INSIDE the block.  Moments: the count and the sum of squares of the entries < 0, the
 *     same of the entries > 0, sum |v|, sum v^2.  One workgroup per block, the block in LDS (72 KiB at bs = 96).
 * ur_niqe_halve: y fp64 [N,h,w], h and w even and >= 4 -> out fp64 [N,h/2,w/2] = halve(y / 255) * 255, the antialiased bicubic
 *     (a = -0.5) halving: output o reads inputs 2o-3 .. 2o+4 with the weights (-0.0234375, -0.0703125, 0.2265625, 0.8671875,
 *     0.8671875, 0.2265625, -0.0703125, -0.0234375) / 2, an index outside the axis mirrored with the edge sample repeated
 *     (-1 -> 0, -2 -> 1, n -> n-1); along the rows first (every column's eight row taps, ascending), then along the columns.
 * ur_niqe_fit: moments fp64 [rows][5][6] of blocks of block_pixels pixels -> the 18 features of every row at
 *     features[row * ld + col_off ..]: (alpha, (bl + br) / 2) of M, then (alpha, (br - bl) * mean_ratio[i], bl, br) of each product.
 *     l = sqrt(sum- / n-), r = sqrt(sum+ / n+), gam = l / r, R = (sum|v| / P)^2 / (sum v^2 / P) * (gam^3 + 1)(gam + 1) / (gam^2 + 1)^2;
 *     i = the first index that minimises (rho[i] - R)^2 over the 9801-entry tables, found by bisection of the strictly increasing
 *     rho; alpha = 0.2 + 0.001 i, bl = l * scale[i], br = r * scale[i].  A NaN R (a count of 0) gives NaN features and index -1.
 *     rho, scale, mean_ratio: DEVICE fp64 [9801] = Gamma(2/a)^2 / (Gamma(1/a) Gamma(3/a)), sqrt(Gamma(1/a) / Gamma(3/a)),
 *     Gamma(2/a) / Gamma(1/a), built on the host.  alpha_index: NULL, or int32 [rows][5] that receives i.
 * UR_E_INVALID before any HIP call for a null required pointer or a malformed shape.  Size limits (64-bit arithmetic, before any HIP
 * call; UR_E_UNSUPPORTED beyond): N*h*w < 2^31 - 256 (luma, halve), N * ceil(h/32) * ceil(w/32) < 2^31 - 256 (mscn),
 * N * blocks < 2^31 - 256 (block_moments), rows * 5 < 2^31 - 256 (fit). */
int ur_niqe_luma(const float* x, double* y, int N, int H, int W, int h, int w, int color_space, ur_stream_t stream);
int ur_niqe_mscn(const double* y, double* m, int N, int h, int w, ur_stream_t stream);
int ur_niqe_block_moments(const double* field, double* moments, int N, int h, int w, int bs, ur_stream_t stream);
int ur_niqe_halve(const double* y, double* out, int N, int h, int w, ur_stream_t stream);
int ur_niqe_fit(const double* moments, const double* rho, const double* scale, const double* mean_ratio, double* features,
                int* alpha_index, long long rows, int block_pixels, int ld, int col_off, ur_stream_t stream);

/* ---- RetinaNet scoring of the det output (csrc/detect.hip; the network and the host side are unirestore_amd/detect.py) ----------
 * fp32 throughout, maps NHWC and contiguous.  No allocation, no synchronisation, no global atomics; every floating-point sum in a
 * fixed order: the same inputs give the same bits, and an image's results depend on that image alone.
 * ur_det_prep: x NCHW [N,3,H,W] in [0,1] -> y NHWC [N,HP,WP,3]: (v - mean_c) / std_c (ImageNet), then the half-pixel bilinear resize
 *     to RH x RW with the tables iy int32 [RH] / wy fp32 [RH][2] and ix [RW] / wx [RW][2] (output o reads sources i[o] and
 *     min(i[o] + 1, last) with the weights w[o]), as wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d); zeros beyond RH x RW.
 * ur_upsample_nearest_add_f32: y [N,OH,OW,C] = a [N,OH,OW,C] + b [N,h,w,C] at (iy[oh], ix[ow]); iy int32 [OH] and ix int32 [OW] are
 *     built on the host and must lie inside b.  y is a buffer of its own.
 * ur_groupnorm_relu_f32: GroupNorm of x [N,HW,C] over G groups of C / G neighbouring channels: per (image, group) the mean, then
 *     the biased variance of the centred values, in fp64 in a fixed order; y = (x - mean) / sqrt(var + eps) * gamma_c + beta_c in
 *     fp64, rounded to fp32 once; relu 1: maximum(y, 0), a NaN stays.  Any 4-byte aligned pointers.  y is not x.
 * ur_det_select: logits [N][HWA][K], reg [N][HWA][4] (or NULL).  Per image the candidates are the logits > lt (a NaN is none; -0
 *     equals +0); the first min(k, count) of them in the order (logit descending, flat index ascending) are written in that order to
 *     row n (row stride ld >= k elements) of scores (sigmoid of the logit, evaluated in fp64 and rounded to fp32), anchors (index /
 *     K), labels (index % K) and, unless NULL, index; entries from the count up to k are zero.  counts[n] = min(k, count);
 *     nonfinite[n] = 1 when any logit or any regression of the image is not finite, else 0.  k <= ur_det_select_kmax() = 1024.
 *     The result is exact whatever share of the logits passes.  ws: ur_det_select_ws_bytes(N, HWA * K) bytes, 16-byte aligned.
 * ur_det_decode: for j < counts[n], candidate (n, j) with anchor index an = anchors[n * ld + j]: a = an % A, cell = an / A, anchor =
 *     base[a] (fp32 [A][4], x1 y1 x2 y2) shifted by ((cell % WF) * stride_w, (cell / WF) * stride_h); torchvision's BoxCoder with
 *     weights (1, 1, 1, 1) and dw, dh clamped at log(1000 / 16) on reg[n][an] gives `raw` (or NULL), clamped to [0, img_w] x [0,
 *     img_h] `clipped`, and times (ratio_w, ratio_h) `scaled`: rows of ld boxes, zeros from counts[n] up to k.
 * ur_det_nms: class-aware greedy NMS of the candidates of each image among its M <= ur_det_nms_mmax() = 8192 positions; position p is
 *     a candidate when p % seg < counts[(p / seg) * N + n] (counts int32 [levels][N], seg * levels >= M).  Order: (score descending,
 *     position ascending).  A box is dropped when a kept box of its label has inter / (area_a + area_b - inter) > thresh, areas
 *     and inter as in torchvision's nms, on `boxes`; the first D kept are written: y_boxes (from out_boxes), y_scores, y_labels
 *     (int64), y_keep (the positions; -1 beyond the count), zeros beyond y_count[n].  flags int32 [levels][N] or NULL: any set ->
 *     y_nonfinite[n] = 1 and the image has no detections.  ws: ur_det_nms_ws_bytes(N, M) bytes, 8-byte aligned.
 * UR_E_INVALID before any HIP call for a null required pointer, a size out of range, a misaligned pointer or a small workspace. */
int ur_det_prep(const float* x, float* y, int N, int H, int W, int RH, int RW, int HP, int WP, const int32_t* iy, const float* wy,
                const int32_t* ix, const float* wx, ur_stream_t stream);
int ur_upsample_nearest_add_f32(const float* a, const float* b, float* y, int N, int OH, int OW, int C, int h, int w, const int32_t* iy,
                                const int32_t* ix, ur_stream_t stream);
int ur_groupnorm_relu_f32(const float* x, const float* gamma, const float* beta, float* y, int N, int HW, int C, int G, double eps, int relu,
                          ur_stream_t stream);
int ur_det_select_kmax(void);
long long ur_det_select_ws_bytes(int N, long long L);
int ur_det_select(const float* logits, const float* reg, int N, long long HWA, int K, float lt, int k, float* scores, int32_t* anchors,
                  int32_t* labels, int32_t* index, int ld, int32_t* counts, int32_t* nonfinite, void* ws, long long ws_bytes, ur_stream_t stream);
int ur_det_decode(const float* reg, const int32_t* anchors, const int32_t* counts, const float* base, float* raw, float* clipped,
                  float* scaled, int N, long long HWA, int k, int ld, int A, int WF, int stride_h, int stride_w, float img_h, float img_w,
                  float ratio_h, float ratio_w, ur_stream_t stream);
int ur_det_nms_mmax(void);
long long ur_det_nms_ws_bytes(int N, int M);
int ur_det_nms(const float* boxes, const float* out_boxes, const float* scores, const int32_t* labels, const int32_t* counts,
               const int32_t* flags, int N, int M, int seg, int levels, float thresh, int D, float* y_boxes, float* y_scores,
               long long* y_labels, int32_t* y_keep, int32_t* y_count, int32_t* y_nonfinite, void* ws, long long ws_bytes, ur_stream_t stream);

/* ---- live per-kernel-family timing (HIP events on the launch stream) ------------------------------*/
int ur_profile_enable(int on);
/* writes a JSON object {family: {launches, ms, flops, bytes}} into buf (host); synchronises the events */
int ur_profile_report(char* buf, size_t buf_bytes);

#ifdef __cplusplus
}
#endif
#endif /* UNIRESTORE_HIP_H */
