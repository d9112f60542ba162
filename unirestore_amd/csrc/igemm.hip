// Implicit-GEMM convolution / linear for gfx950: NHWC bf16 activations, [Cout][KH*KW*Cin] bf16 weights,
// v_mfma_f32_32x32x16_bf16 with fp32 accumulate, fused epilogues.  See include/unirestore_hip.h.
//
// Mapping (MI355X-first, not a cuDNN-style port):
//   * GEMM view: M = N*OH*OW output pixels, N = Cout, K = KH*KW*Cin; the K index runs (tap, cin) so every
//     16-byte vector a lane loads is 8 contiguous input channels of ONE pixel (NHWC) or of one weight row.
//   * MFMA "A" operand = weight rows (cout), "B" operand = pixels, so each lane of the 32x32 accumulator
//     holds 4 CONSECUTIVE output channels of one pixel -> 8-byte bf16 stores straight into NHWC.
//   * 256 threads = 4 waves; register-staged global->LDS pipeline (issue tile t+1 loads, compute tile t,
//     write LDS, one barrier per 64-deep K tile), 2 LDS stages.
//   * LDS tile = [row][128 B] with the 16-B slot XOR-swizzled by (row>>1)&7: conflict-free for both the
//     ds_write_b128 staging pattern and the ds_read_b128 fragment pattern of 32-row MFMA operands.
//   * zero padding, stride, nearest-2x upsample and channel concat are address arithmetic in the loader.
//   * block id -> tile map is XCD-aware (blocks that share an activation tile land on one XCD's L2).
#include "igemm_impl.h"

namespace urk {   // the launchers of the instantiation units, one object per 16-bit type (parallel compilation): ConvK::f16 picks
#define UR_DECLARE(name)                                                                                             \
  ConvLaunch name##_bf16(void* k, size_t ws_bytes);                                                                 \
  ConvLaunch name##_f16(void* k, size_t ws_bytes);                                                                  \
  static ConvLaunch name(ConvK& k, size_t ws_bytes) { return (k.f16 ? name##_f16 : name##_bf16)(&k, ws_bytes); }
UR_CONV_LAUNCHERS(UR_DECLARE)
#undef UR_DECLARE
}  // namespace urk

namespace {

// The launcher for k, planned (host only: no HIP call).
ConvLaunch dispatch_conv(ConvK& k, bool pair, size_t ws_bytes) {
  // Nearest-2x upsample + 3x3 with the caller's folded weights (ur_conv_desc.w_up4): four 2x2 phase convs over the SOURCE image on the
  // 8 x 32 halo kernels, 4/9 of the MACs.  The source image must be whole patches; the epilogue writes through a strided view of y
  // (up4_out_view), so the features that index rows of other planes (row sums, LayerNorm folding, transposed columns) and the
  // in-loader GroupNorm stay on the 9-tap path.  Any Cout runs (a ragged last tile on the 128-wide kernel).
  k.fold = 0;
  if (k.w4 && k.ups && k.KH == 3 && k.stride == 1 && k.pad_t == 1 && k.pad_l == 1 && k.kcm && k.staged_ok_ && !pair && k.nbatch == 1 &&
      k.C2 == 0 && k.Cin % 64 == 0 && k.W % 32 == 0 && k.H % 8 == 0 && k.OH == 2 * k.H && k.OW == 2 * k.W && !k.yt && !k.gn_ab && !k.row_stats &&
      !k.ln_stats) {
    k.fold = 1;
    const long long tm = 4ll * k.N * (k.H / 8) * (k.W / 32);
    auto fill = [](long long t) { return (double)t / (double)(((t + 255) / 256) * 256); };
    const bool ok128 = k.Cout % 128 == 0, ok160 = k.Cout % 160 == 0;
    if (ok160 && (!ok128 || fill(tm * (k.Cout / 160)) >= fill(tm * (k.Cout / 128)))) return urk::halo_8x32_160(k, ws_bytes);
    return urk::halo_8x32_128(k, ws_bytes);
  }
  if (k.KH == 3 && k.stride == 1 && k.pad_t == 1 && k.pad_l == 1 && k.kcm && k.staged_ok_ && !pair && k.nbatch == 1 &&
      k.OW % 32 == 0 && k.OH % 8 == 0 && k.OH == (k.ups ? 2 * k.H : k.H) && k.OW == (k.ups ? 2 * k.W : k.W) && !k.yt) {
    // tile width: 128 or 160 output channels, whichever divides Cout; when both do, the one whose tile count fills whole
    // rounds of 256 CUs better (e.g. 1280 channels at 32 x 32: 8 x 160 -> 256 tiles = one round, 10 x 128 -> 320 = two)
    const bool ok128 = k.Cout % 128 == 0, ok160 = k.Cout % 160 == 0;
    const long long tm8 = (long long)k.N * (k.OH / 8) * (k.OW / 32);
    // (<= 128 tiles are split over channel chunks into floor(256 / tiles) workgroups each)
    auto eff = [](long long t) { return t <= 128 ? (double)(t * (256 / t)) / 256.0 : (double)t / (double)(((t + 255) / 256) * 256); };
    const bool use160 = ok160 && (!ok128 || eff(tm8 * (k.Cout / 160)) >= eff(tm8 * (k.Cout / 128)));
    const long long tiles8 = tm8 * (use160 ? k.Cout / 160 : k.Cout / 128);
    if ((ok128 || ok160) && tiles8 >= 64) {
      if (use160) return urk::halo_8x32_160(k, ws_bytes);
      return urk::halo_8x32_128(k, ws_bytes);
    }
  }
  // conv_out layers: <= 32 output channels (fp32 or 16-bit) of a 3x3 / stride 1 / pad 1 conv with chunk-major weights
  if (k.KH == 3 && k.stride == 1 && k.pad_t == 1 && k.pad_l == 1 && k.kcm && !pair && k.nbatch == 1 && !k.ups && k.C2 == 0 &&
      k.Cout <= 32 && k.OW % 32 == 0 && k.OH % 8 == 0 && k.OH == k.H && k.OW == k.W && !k.yt && !k.gn_part && !k.gn_ab && !k.row_stats && !k.ln_stats &&
      !k.bias_img && (long long)k.N * (k.OH / 8) * (k.OW / 32) >= 128)
    return urk::halo_thin_32(k, ws_bytes);
  // (round 6: the 8 x 8 -> 16 x 16 upsampling conv runs on the whole-image tile too - the patch pieces read their nearest source pixel)
  const bool himg_ups = k.ups && k.OH == 16 && k.OW == 16 && k.H == 8 && k.W == 8;
  if (k.KH == 3 && k.stride == 1 && k.pad_t == 1 && k.pad_l == 1 && k.kcm && k.staged_ok_ && !pair && k.nbatch == 1 &&
      ((!k.ups && k.OH == k.H && k.OW == k.W) || himg_ups) && !k.yt && k.Cout % 128 == 0 && k.nk >= 36) {
    // 8 x 8 maps of a few images: a weight stream (csrc/conv_wstream.hip) when the caller packed the fragment-major copy
    if (k.wf && k.OH == 8 && k.OW == 8 && k.N <= 16 && k.Cin % 256 == 0 && k.nk >= 72 && k.y && k.ws && !k.gn_ab && !k.row_stats && !k.ln_stats &&
        (long long)(k.nk / 36) * k.M * k.Cout * 4 <= (long long)ws_bytes)
      return urk::wstream_8x8(k, ws_bytes);
    if (k.OH == 16 && k.OW == 16) return urk::himg_16x16(k, ws_bytes);
    if (k.OH == 8 && k.OW == 8 && k.N % 4 == 0) {
      return urk::himg_8x8x4(k, ws_bytes);
    }
  }
  if (k.KH == 1 && k.stride == 1 && !k.ups && k.C2 == 0 && k.staged_ok_ && k.Cout % 256 == 0 && !k.yt && (k.act == UR_ACT_GEGLU || k.act == UR_ACT_GATE) &&
      (long long)((k.M + 255) / 256) * (k.Cout / 256) * k.nbatch >= 200 && (long long)k.M * k.ldx < (1ll << 31) - 256)
  {
    // 320-wide tiles when they land on whole rounds of CUs (2048 x 10240: 8 x 32 = 256 tiles instead of 320)
    auto fill = [](long long t) { return (double)t / (double)(((t + 255) / 256) * 256); };
    const long long tm = (k.M + 255) / 256;
    if (k.Cout % 320 == 0 && k.nbatch == 1 && !k.bias_img && fill(tm * (k.Cout / 320)) > fill(tm * (k.Cout / 256)))
      return urk::gemm_256x320_pair(k, ws_bytes);
    return urk::gemm_256x256(k, ws_bytes);
  }
  // short-K GEMMs (<= 10 K tiles: per-workgroup prologue/epilogue latency dominates): 128-row tiles, 2 workgroups per CU
  const bool use_v1 = k.KH == 1 && k.nk <= 10;
  const long long blocks128 = (long long)((k.M + 127) / 128) * ((k.Cout + 127) / 128) * k.nbatch;
  // pure GEMMs that will not be split: the LDS-DMA twin of the register-staged kernel (no staging registers / ds_writes)
  const bool g1 = k.KH == 1 && k.stride == 1 && !k.ups && k.C2 == 0 && k.pad_t == 0 && k.pad_l == 0 && k.OH == k.H && k.OW == k.W &&
                  (long long)k.M * k.ldx + k.Ktot < (1ll << 31) - 256;
  auto nosplit = [&](int bm, int bn) { return (long long)((k.M + bm - 1) / bm) * ((k.Cout + bn - 1) / bn) * k.nbatch >= 200 || k.nk < 8 || !k.ws; };
  if (k.KH == 1 && !pair && k.Cout > 64) {
    // too few 128 x 128 tiles to fill 256 CUs and K too short for split-K to pay for its reduce pass: 64 x 64 tiles
    // (>= 128 such tiles run faster unsplit up to K = 3072 than split with a reduce pass: 512 x 1280 x 1280 11.3 vs 14.6 us,
    //  2048 x 1280 x 2560 29 vs 34 us)
    const long long blocks64 = (long long)((k.M + 63) / 64) * ((k.Cout + 63) / 64) * k.nbatch;
    // (grids of <= 256 workgroups - the 8x8 level - are latency-bound per K tile: four ring stages, and K up to 2560 stays unsplit:
    //  512 x 1280 x 1280 12.9 -> 9.1 us, x 2560 20.8 (split + reduce) -> 14.3 us; profiles/r5_wreg_ab.txt)
    if (blocks128 < 200 && g1 && blocks64 >= 128 && blocks64 <= 256 && k.nk >= 8 && k.nk <= 48) return urk::g1_64x64_deep(k, ws_bytes);
    // long-K GEMMs of the 16x16 level: 128 x 64 tiles, three stages, unsplit (2048 x 1280 x 2560 25.9 -> 23.3 us, x 5120 49.1 -> 43.7 us)
    if (g1 && blocks128 < 200 && k.nk > 24 && k.nk <= 96 && (long long)((k.M + 127) / 128) * ((k.Cout + 63) / 64) * k.nbatch >= 256)
      return urk::g1_128x64_deep(k, ws_bytes);
    if (blocks128 < 200 && g1 && ((blocks64 >= 128 && k.nk <= 24) || (blocks64 >= 256 && k.nk <= 48))) return urk::g1_64x64(k, ws_bytes);
    if (blocks128 < 200 && k.nk <= 24) return g1 && nosplit(64, 64) ? urk::g1_64x64(k, ws_bytes) : urk::v1_64x64(k, ws_bytes);
    // 1 < tiles/CU < 2 at 128 x 128: halve the N tile so every CU gets the same work
    if (use_v1 && blocks128 > 256 && blocks128 < 400 && k.Cout % 128 == 0) return g1 && nosplit(128, 64) ? urk::g1_128x64(k, ws_bytes) : urk::v1_128x64(k, ws_bytes);
  }
  if (use_v1) {
    if (pair) return urk::v1_128x128(k, ws_bytes);  // a|g 32-row blocks must sit in one wave tile
    if (k.Cout <= 32) return urk::v1_256x32(k, ws_bytes);
    if (k.Cout <= 64) return urk::v1_128x64(k, ws_bytes);
    if (k.Cout % 160 == 0 && k.Cout % 128 != 0) return g1 && nosplit(128, 160) ? urk::g1_128x160(k, ws_bytes) : urk::v1_128x160(k, ws_bytes);
    return g1 && nosplit(128, 128) ? urk::g1_128x128(k, ws_bytes) : urk::v1_128x128(k, ws_bytes);
  }
  // v2 (LDS-DMA ring).  One workgroup per CU: pick the 256-row / 8-wave tiles when they still fill the chip.
  if (k.Cout <= 32) return urk::v2_256x32(k, ws_bytes);
  if (k.Cout <= 64 && !pair) return urk::v2_128x64(k, ws_bytes);
  const bool n160 = !pair && k.Cout % 160 == 0 && k.Cout % 128 != 0;
  const long long big_tiles = (long long)((k.M + 255) / 256) * ((k.Cout + (n160 ? 159 : 127)) / (n160 ? 160 : 128)) * k.nbatch;
  if (g1 && !pair && big_tiles < 256) {
    // 256-row tiles would leave CUs without a workgroup (e.g. 8192 x 640: 160 tiles): 128-row LDS-DMA tiles, two per CU,
    // in the width that lands closest to whole CUs (8192 x 640 -> 64 x 4 tiles of 160 = 256)
    const long long t160 = k.Cout % 160 == 0 ? (long long)((k.M + 127) / 128) * (k.Cout / 160) : 0;
    const long long t128 = (long long)((k.M + 127) / 128) * ((k.Cout + 127) / 128);
    auto fill = [](long long t) { return t <= 0 ? 0.0 : (double)t / (double)(((t + 255) / 256) * 256); };
    if (t160 >= 200 && fill(t160) >= fill(t128)) return urk::g1_128x160(k, ws_bytes);
    if (t128 >= 200) return urk::g1_128x128(k, ws_bytes);
  }
  if (big_tiles >= 160) {
    // pure GEMMs onto 320/960-wide outputs: two 128 x 160 workgroups per CU beat one 256 x 160 (32768 x 320 x 1280: 41 vs 44.5 us)
    if (n160 && g1) return urk::g1_128x160(k, ws_bytes);
    if (n160) return urk::v2_256x160(k, ws_bytes);
    return urk::v2_256x128(k, ws_bytes);
  }
  // small problems: the register-staged kernel (two workgroups per CU), split-K when few tiles meet a long K
  if (k.Cout % 160 == 0 && k.Cout % 128 != 0 && !pair) return urk::v1_128x160(k, ws_bytes);
  return urk::v1_128x128(k, ws_bytes);
}

}  // namespace

// plan or info != nullptr: only plan the launch (ur_conv2d_plan / ur_conv2d_plan_launch), nothing runs
static int conv_impl(const ur_conv_desc* d, ur_stream_t stream, ur_conv_plan* plan, ur_conv_launch_info* info = nullptr) {
  UR_REQUIRE(d && d->x && d->w, "null x/w");
  UR_REQUIRE(d->KH == d->KW && (d->KH == 1 || d->KH == 3), "only 1x1 and 3x3 kernels");
  UR_REQUIRE(d->C1 > 0 && d->C1 % 8 == 0 && d->C2 % 8 == 0 && d->ldx % 8 == 0, "Cin/ldx must be multiples of 8");
  UR_REQUIRE(d->C2 == 0 || (d->x2 && d->ldx2 % 8 == 0), "virtual concat needs x2");
  UR_REQUIRE(d->Cout > 0 && d->Cout % 4 == 0 && d->ldw % 8 == 0, "Cout%4, ldw%8");
  UR_REQUIRE(d->nbatch >= 1 && d->stride >= 1 && d->OH > 0 && d->OW > 0, "bad dims");
  UR_REQUIRE(d->y || d->yt || d->gn_part, "no output requested");
  UR_REQUIRE_DT(d->dtype);
  const bool pair = d->act == UR_ACT_GEGLU || d->act == UR_ACT_GATE;
  if (pair && d->Cout % 64 != 0)     // (production widths are 128 / 256 / 512 output channels; refused, never computed wrongly)
    return ur::fail(UR_E_UNSUPPORTED, "ur_conv2d_nhwc: pair activations (GEGLU / SimpleGate) need Cout % 64 == 0 (32-row a|g interleave)");
  UR_REQUIRE(!d->y || (d->out_f32 ? d->ldy % 4 == 0 : d->ldy % 4 == 0), "ldy%4");
  UR_REQUIRE(!d->residual || d->ldr % 4 == 0, "ldr%4");
  UR_REQUIRE(!d->yt || (d->t_rows > 0 && d->n_split % 4 == 0 && !pair), "bad transposed-output spec");
  UR_REQUIRE(!d->yt || d->nbatch == 1, "transposed columns (yt) need nbatch == 1 (yt has no batch stride)");
  // Size limits (include/unirestore_hip.h, "size limits"), checked before any int product of the dimensions, one factor at a time
  // (every partial product is below 2^31 before the next int is multiplied in, so no 64-bit product can wrap either):
  //  * output rows M = N * OH * OW: row indices are int and a tile may start up to one tile (<= 256 rows) short of M and run past it.
  //    (OH and OW are the caller's: nothing ties them to H and W, so this is not implied by the bound on x.  Defensive: no caller
  //    of this repository comes near it.);
  //  * x, x2 and w are read through 32-bit element offsets.  (The LDS-DMA kernels read them through raw buffer descriptors whose range
  //    check treats byte offsets >= 0xffffff00 as "read zero" (IG_OOB, csrc/igemm_impl.h), so a source of theirs must end below that
  //    byte.  It always does: the halo / whole-image kernels take images of OH % 8 == 0, OW % 32 == 0 or 8 x 8 / 16 x 16 pixels with
  //    ldx % 8 == 0, whose element count is a multiple of 512, and the pure-GEMM ones keep M * ldx + K < 2^31 - 256 in dispatch_conv;
  //    the kernels that take any other shape use 64-bit pointers.  tests/test_large_tensors_cpu.py pins this.)
  //    The WEIGHTS of the pure-GEMM LDS-DMA kernels had no such guard: with Cout * ldw = 2^31 - 32 in rows of 24 elements the last
  //    four rows started past that byte and read as zeros (those output columns came out as their bias).  Hence the same margin
  //    for w as dispatch_conv keeps for x: a row's last lane offset is its start + 112 bytes, below 0xffffff00 for every ldw.
  //    y, yt, residual, bias rows, the statistics planes and the split-K planes are addressed with 64-bit offsets: no bound of their own;
  //  * a grid of 2^32 threads or more is not refused by the runtime - it wraps, and the workgroups past the wrap never run - so the
  //    tile grid of the launcher that is planned must stay below 2^23 workgroups (checked below, once the plan has counted its tiles).
  UR_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0, "N, H, W must be positive");
  UR_REQUIRE((long long)d->N * d->OH < (1ll << 31) && (long long)d->N * d->OH * d->OW < (1ll << 31) - 512,
             "ur_conv2d_nhwc: too many output rows: N * OH * OW must be below 2^31 - 512");
  UR_REQUIRE(d->ldx > 0 && d->ldx2 >= 0 && d->ldw > 0 && (long long)d->N * d->H < (1ll << 31) && (long long)d->N * d->H * d->W < (1ll << 31) &&
                 (long long)d->N * d->H * d->W * (long long)std::max(d->ldx, d->ldx2) < (1ll << 31),
             "ur_conv2d_nhwc: tensor too large for 32-bit element offsets: N * H * W * max(ldx, ldx2) must be below 2^31");
  UR_REQUIRE((long long)d->Cout * d->ldw < (1ll << 31) - 256,
             "ur_conv2d_nhwc: weights too large for 32-bit element offsets: Cout * ldw must be below 2^31 - 256");

  ConvK k;
  k.x = (const uint16_t*)d->x; k.x2 = (const uint16_t*)d->x2; k.w = (const uint16_t*)d->w; k.bias = d->bias;
  k.res = (const uint16_t*)d->residual; k.y = d->y; k.yt = (uint16_t*)d->yt;
  k.ws = d->workspace;
  k.N = d->N; k.H = d->H; k.W = d->W; k.C1 = d->C1; k.ldx = d->ldx; k.C2 = d->C2; k.ldx2 = d->ldx2;
  k.Cin = d->C1 + d->C2; k.Cout = d->Cout; k.ldw = d->ldw; k.ldy = d->ldy; k.ldr = d->ldr;
  k.KH = d->KH; k.KW = d->KW; k.stride = d->stride; k.pad_t = d->pad_t; k.pad_l = d->pad_l;
  k.OH = d->OH; k.OW = d->OW; k.OHW = d->OH * d->OW; k.ups = d->upsample2x; k.act = d->act; k.out_f32 = d->out_f32;
  k.n_split = d->yt ? d->n_split : d->Cout; k.t_rows = d->t_rows; k.t_ld = d->t_ld;
  k.out_scale = d->out_scale;
  k.M = d->N * d->OH * d->OW; k.Ktot = d->KH * d->KW * k.Cin; k.nk = (k.Ktot + 63) / 64; k.nbatch = d->nbatch;
  k.bs_x = d->bs_x; k.bs_x2 = d->bs_x2; k.bs_w = d->bs_w; k.bs_bias = d->bs_bias; k.bs_y = d->bs_y; k.bs_r = d->bs_r; k.bias_img = d->bias_img_stride;
  UR_REQUIRE(k.M > 0, "empty problem");

  k.kcm = d->k_chunk_major; k.wf = (const uint16_t*)d->w_frag; k.wmajor = 0; k.xgm = 0; k.xbn = 0; k.patch_tw = 0;
  // (w_up4 has no batch stride: a batched / grouped launch never reads it - neither here nor in the per-group launches of the group loop)
  k.w4 = d->upsample2x && d->nbatch == 1 ? (const uint16_t*)d->w_up4 : nullptr; k.fold = 0;
  UR_REQUIRE(!k.kcm || (k.Cin % 64 == 0 && d->C1 % 64 == 0), "k_chunk_major needs C1 and C1+C2 to be multiples of 64");
  k.gn_part = d->gn_part; k.gn_ab = d->gn_ab; k.gn_silu = d->gn_silu; k.f16 = d->dtype == UR_DT_F16; k.gn_fused = 0; k.gn_parts = 0;
  k.ln_parts = d->ln_parts;
  k.row_stats = d->row_stats; k.ln_stats = d->ln_stats; k.ln_colsum = d->ln_colsum; k.ln_eps = d->ln_eps; k.ln_dim = d->ln_dim;
  UR_REQUIRE(!d->ln_stats || (d->ln_colsum && d->ln_dim > 0), "ln_stats needs ln_colsum / ln_dim");
  // feature combinations the specialised epilogues cover (each is one compiled instance; see epi_frag_pass)
  UR_REQUIRE(!(d->bias_img_stride && (pair || d->ln_stats || d->yt)), "per-image bias rows do not combine with pair activations / LayerNorm folding / transposed columns");
  // (a tile that straddles images of another size than its own takes the unstaged epilogue (igemm_epilogue: bias_geom_ok), which
  //  writes no row sums: 2 x 16 x 17 outputs in 128-row tiles would leave the row_stats plane as it was.  The plan does not know the
  //  tile height before dispatch and no caller pairs the two - refused, never computed wrongly.)
  UR_REQUIRE(!(d->bias_img_stride && d->row_stats), "per-image bias rows do not combine with row_stats");
  // staged (LDS-tiled, 16-byte row stores) epilogue: 16-bit y with aligned rows, or no y at all (statistics-only launch)
  k.staged_ok_ = (d->y ? (!d->out_f32 && ((d->ldy | d->bs_y) & 7) == 0) : d->gn_part != nullptr) &&
                 (!d->residual || ((d->ldr | d->bs_r) & 7) == 0);
  UR_REQUIRE(!d->gn_part || (!d->out_f32 && !d->yt), "gn_part needs a plain 16-bit output (or none)");
  // the statistics pass (csrc/norms.hip gn_geom) works on vectors of 8 channels: 4 output channels divided by zero there (SIGFPE
  // while planning) and 12 / 20 would leave their last four channels' sums unwritten.  No fused source is exercised at such a width either, so the rule
  // holds for every source of the partials (refused, never computed wrongly); before dispatch_conv, whose plan sizes the pass
  UR_REQUIRE(!d->gn_part || (pair ? d->Cout / 2 : d->Cout) % 8 == 0, "gn_part needs output channels % 8 == 0 (GroupNorm statistics run on 8-channel vectors)");
  hipStream_t s = (hipStream_t)stream;
  const ConvLaunch launch = dispatch_conv(k, pair, d->workspace_bytes);
  const int kprof = k.fold ? 4 * k.Cin : k.Ktot;      // K the launch executes: a folded upsampling conv runs 4 taps per channel, not 9
  const double flops = 2.0 * k.M * (double)k.Cout * kprof * k.nbatch;
  const double bytes = 2.0 * ((double)k.M * k.Cin + (double)k.Cout * kprof + (double)k.M * k.Cout) * k.nbatch;
  const char* fam = d->KH == 3 ? "conv3x3_igemm" : "gemm1x1_igemm";
  static const bool prof_shapes = getenv("UR_PROF_SHAPES") != nullptr;
  if (prof_shapes) {           // per-shape families for offline analysis (interned strings keep the pointers stable)
    static std::map<std::string, int> interned;
    char buf[128];
    snprintf(buf, sizeof buf, "%s M%d N%d K%d s%d u%d b%d a%d", d->KH == 3 ? "c3" : "g1", k.M, k.Cout, kprof, d->stride, d->upsample2x,
             k.nbatch, d->act);
    fam = interned.emplace(buf, 0).first->first.c_str();
  }
  // (the grid's x dimension is tiles_m * tiles_n; groups and K splits sit in y and z.  Workgroups have at most 512 threads.)
  UR_REQUIRE((long long)k.tiles_m * k.tiles_n < (1ll << 23),
             "ur_conv2d_nhwc: tile grid too large: the planned launcher's row tiles x column tiles must be below 2^23");
  // Grouped 3x3 convolutions whose groups are halo-kernel sized (chunk-major weights, >= 64 channels in, a multiple of 128 out):
  // one halo launch per group on the channel slice instead of the batched generic kernel, which gathers 64-byte runs per pixel and
  // tap (CFRM's AdaNAFV2.group_conv, densified to 128-channel blocks by the caller: 2.19 ms -> 4 x ~0.2 ms at 256 x 256 x 512)
  const bool group_loop = k.nbatch > 1 && d->KH == 3 && k.kcm && k.stride == 1 && !pair && !k.gn_part && !k.row_stats && !k.ln_stats &&
                          !k.yt && !k.gn_ab && !k.out_f32 && k.staged_ok_ && k.Cout % 128 == 0 && !k.bias_img && k.C2 == 0;
  auto group_k = [&](int b) {      // the single-group problem of group b
    ConvK kb = k;
    kb.nbatch = 1; kb.w4 = nullptr;
    kb.x = k.x + b * k.bs_x; kb.w = k.w + b * k.bs_w; kb.bias = k.bias ? k.bias + b * k.bs_bias : nullptr;
    kb.res = k.res ? k.res + b * k.bs_r : nullptr;
    kb.y = reinterpret_cast<uint16_t*>(k.y) + b * k.bs_y;
    kb.bs_x = kb.bs_w = kb.bs_bias = kb.bs_y = kb.bs_r = 0;
    return kb;
  };
  // The extra statistics pass reads y as one dense [M][nbatch * channels] tensor: batches must sit side by side in its rows (the
  // grouped conv's layout), not one after the other (bmm_nt's): no ldy makes that layout dense, so both plans refuse it.
  if (k.gn_part && !k.gn_fused && !group_loop && k.nbatch > 1 && d->y && d->bs_y != (pair ? k.Cout / 2 : k.Cout))
    return ur::fail(UR_E_UNSUPPORTED, "ur_conv2d_nhwc: gn_part of a batched launch that cannot fuse the statistics needs bs_y == output channels per batch");
  if (plan) {      // row-stat planes: one per N tile, or the single one of a split-K reduce pass
    plan->row_stat_parts = d->row_stats ? (k.splitk > 1 ? 1 : k.tiles_n) : 0;
    plan->gn_parts = k.gn_parts; plan->gn_fused = k.gn_fused; plan->prologue_ok = launch.prologue_ok; plan->up4 = k.fold;
  }
  if (info) {      // what runs: the launcher (per group, for the group loop), its split and reduce pass, the GroupNorm pass
    ConvK kb = group_loop ? group_k(0) : k;
    const ConvLaunch l = group_loop ? dispatch_conv(kb, pair, d->workspace_bytes) : launch;
    info->launcher = l.id; info->splitk = kb.splitk; info->nk_per_split = kb.nk_per_split;
    const ReducePlan r = kb.splitk > 1 ? plan_splitk_reduce(kb) : ReducePlan{-1, 0};
    info->reduce = r.kind; info->reduce_ri = r.ri;
    info->gn_pass = k.gn_part && !k.gn_fused && !group_loop;
    info->group_loop = group_loop;
  }
  if (plan) return UR_OK;
  // What the launch refuses, ur_conv2d_plan_launch refuses too: it answers what runs (ur_conv2d_plan only sizes the planes).
  // statistics-only launch: only where the epilogue itself produces the partials
  if (!d->y && d->gn_part && (!k.gn_fused || k.splitk > 1))
    return ur::fail(UR_E_UNSUPPORTED, "ur_conv2d_nhwc: y == NULL needs a launch whose epilogue writes gn_part (see ur_conv2d_plan)");
  if (d->gn_ab && !launch.prologue_ok)
    return ur::fail(UR_E_UNSUPPORTED, "ur_conv2d_nhwc: gn_ab is not supported by this launch (see ur_conv2d_plan.prologue_ok)");
  UR_REQUIRE(!(d->row_stats || d->ln_stats) || (k.staged_ok_ && k.nbatch == 1), "row_stats / ln fusion need a bf16 staged output");
  if (info) return UR_OK;
  // The extra statistics pass needs a dense y.  Checked before anything runs (it used to fail after the conv had written y); the two
  // plans do not refuse it - they report gn_pass / gn_fused for a descriptor whose ldy the caller may still choose.
  const int gn_pass_ctot = (pair ? k.Cout / 2 : k.Cout) * k.nbatch;
  UR_REQUIRE(!(k.gn_part && !k.gn_fused) || (k.y && k.ldy == gn_pass_ctot), "gn_part fallback needs a dense output (ldy == channels)");
  ur::ProfScope prof(fam, flops, bytes, s);
  if (group_loop) {
    for (int b = 0; b < d->nbatch; ++b) {
      ConvK kb = group_k(b);
      const int rcb = dispatch_conv(kb, pair, d->workspace_bytes).launch(&kb, s);
      if (rcb != UR_OK) return rcb;
    }
    return UR_OK;
  }
  const int rc = launch.launch(&k, s);
  if (rc != UR_OK) return rc;
  if (k.gn_part && !k.gn_fused)     // this launch could not fuse the statistics: one extra pass over the (dense, checked above) output
    return ur::gn_stats_launch(k.y, k.gn_part, k.N, k.OHW, gn_pass_ctot, d->dtype, s);
  return UR_OK;
}

extern "C" int ur_conv2d_nhwc(const ur_conv_desc* d, ur_stream_t stream) { return conv_impl(d, stream, nullptr); }

// Host-only plan of the launch of `d` (no kernel runs): partial row-sum planes ([parts][M][2] fp32, one per N tile - the
// partial layout keeps the producer free of atomics), GroupNorm partials per image and who writes them, prologue support.
extern "C" int ur_conv2d_plan(const ur_conv_desc* d, ur_conv_plan* plan) {
  UR_REQUIRE(d && plan, "null pointer");
  ur_conv_desc t = *d;
  if (!t.y && !t.yt && !t.gn_part) t.y = reinterpret_cast<void*>(16);    // any non-null value: only the plan is wanted
  return conv_impl(&t, nullptr, plan);
}

// Host-only plan of which launcher runs `d` and how (no kernel runs, no HIP call; the same workspace rule as the launch).
extern "C" int ur_conv2d_plan_launch(const ur_conv_desc* d, ur_conv_launch_info* info) {
  UR_REQUIRE(d && info, "null pointer");
  ur_conv_desc t = *d;
  if (!t.y && !t.yt && !t.gn_part) t.y = reinterpret_cast<void*>(16);    // any non-null value: only the plan is wanted
  return conv_impl(&t, nullptr, nullptr, info);
}

// The launcher names, stringised from the list the launchers are declared from (they cannot drift apart).
#define UR_LAUNCHER_NAME(name) #name,
static const char* const kLauncherNames[] = {UR_CONV_LAUNCHERS(UR_LAUNCHER_NAME)};
#undef UR_LAUNCHER_NAME
static_assert(sizeof(kLauncherNames) / sizeof(kLauncherNames[0]) == UR_CONV_LAUNCHER_COUNT, "one name per launcher");

extern "C" int ur_conv_launcher_count(void) { return UR_CONV_LAUNCHER_COUNT; }
extern "C" const char* ur_conv_launcher_name(int i) { return i >= 0 && i < UR_CONV_LAUNCHER_COUNT ? kLauncherNames[i] : nullptr; }

extern "C" int ur_gemm_bias_act(const void* x, const void* w, const float* bias, const void* residual, void* y, long long M, int N, int K,
                                int ldx, int ldw, int ldy, int ldr, int act, float* workspace, size_t workspace_bytes, int dtype,
                                ur_stream_t stream) {
  UR_REQUIRE(M > 0 && M < (1ll << 31), "M out of range");
  ur_conv_desc d = {};
  d.x = x; d.w = w; d.bias = bias; d.residual = residual; d.y = y;
  d.workspace = workspace; d.workspace_bytes = workspace_bytes;
  d.N = 1; d.H = 1; d.W = (int)M; d.C1 = K; d.ldx = ldx; d.Cout = N; d.ldw = ldw; d.ldy = ldy; d.ldr = ldr;
  d.KH = d.KW = 1; d.stride = 1; d.OH = 1; d.OW = (int)M; d.act = act; d.out_scale = 1.f; d.nbatch = 1; d.dtype = dtype;
  return conv_impl(&d, stream, nullptr);
}

extern "C" int ur_groupconv3x3_nhwc(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int Cg, int Cog,
                                    int groups, int act, float* workspace, size_t workspace_bytes, int dtype, ur_stream_t stream) {
  UR_REQUIRE(groups >= 1 && Cg % 8 == 0 && Cog % 4 == 0, "groups >= 1, Cg % 8 == 0, Cog % 4 == 0");
  ur_conv_desc d = {};
  d.x = x; d.w = w; d.bias = bias; d.y = y;
  d.workspace = workspace; d.workspace_bytes = workspace_bytes;
  d.N = N; d.H = H; d.W = W; d.C1 = Cg; d.ldx = Cg * groups; d.Cout = Cog; d.ldw = 9 * Cg; d.ldy = Cog * groups;
  d.KH = d.KW = 3; d.stride = 1; d.pad_t = d.pad_l = 1; d.OH = H; d.OW = W; d.act = act; d.out_scale = 1.f; d.nbatch = groups;
  d.bs_x = Cg; d.bs_w = (long long)Cog * 9 * Cg; d.bs_bias = Cog; d.bs_y = Cog; d.dtype = dtype;
  return conv_impl(&d, stream, nullptr);
}
