"""Case table of the scoring kernels at their stated size limits (tests/test_scoring_large_gpu.py; host gate in
tests/test_scoring_large_cpu.py).  Importable without torch: the unit builders below import it when they are called.

The scoring side - the fp32 layers (csrc/f32_layers.hip), LPIPS (csrc/lpips.hip), the classifier (csrc/classify.hip), the
segmenter (csrc/segment.hip), PSNR / SSIM (csrc/metrics.hip) - is tested everywhere else at a few thousand elements.  Every entry point states a size limit (include/
unirestore_hip.h, "size limits" of each section); the cases here launch just below each limit, on tensors whose bytes cross 2^31 or
2^32, and on the paths no small case reaches (the second and third trip of the confusion kernel's chunk loop, its 255 bin passes).

The inputs are periodic, as in tests/large_cases.py: unit i (an image, a row of a 1x1 convolution, an element of a flat tensor) is
a copy of unit i mod P for a small odd P, so blocks straddle the unit boundaries differently in every period, and the fp64
reference with its bound is computed for the P distinct units only, by the existing reference modules.  No tolerance is introduced
here: `build(case)` returns the bound the small-shape test of the same op uses (E32_* x 8 of segment_reference / classify_reference
/ lpips_reference, PSNR_TOL / SSIM_TOL of test_metrics_gpu), and 0 for the exact ops.

A "limit" case sits at the largest count the entry point accepts: `count` is the checked quantity, `limit` the first refused value
(GRID: 2^31 - 256, the 1-D launch limit of csrc/launch_size.h; INT31: 2^31; P28: 2^28).  Where the geometry allows it count ==
limit - 1; where it does not (2^31 - 257 = 3 x 715827797 has no factorisation into a map) count is the largest value of the geometry,
inside the last 256 values below the limit where the launch count itself is at stake, and one more unit (`more`) is refused.
"""
GRID = (1 << 31) - 256           # ur::GRID_1D_LIMIT: work items of a 1-D launch, and the element counts that become one
INT31 = 1 << 31
P28 = 1 << 28
P_IMG, P_FLAT = 3, 771           # periods: images, elements / rows
SC_CHUNK, SC_MAX_BLOCKS = 4096, 1024     # csrc/segment.hip: pixels per chunk of the confusion kernel, its largest grid
TRIP = SC_CHUNK * SC_MAX_BLOCKS          # 4 194 304 pixels: one chunk for each of 1024 blocks


def _c(cid, op, export, props=(), **kw):
    return dict(id=cid, op=op, export=export, props=tuple(props), **kw)


CASES = [
    # ---- csrc/f32_layers.hip ---------------------------------------------------------------------------------------------------------
    _c("add_vec_limit", "add", "ur_add_f32", ("vector", "limit"), n=GRID - 4, count=GRID - 4, limit=GRID, more=dict(n=GRID)),
    _c("add_scalar_limit", "add", "ur_add_f32", ("scalar", "limit"), n=GRID - 3, count=GRID - 3, limit=GRID, more=dict(n=GRID + 1)),
    # 64219 x 32 x 55 x 19 = 2^31 - 288: inside the last block below the limit (`total + 255` does not fit an int from 2^31 - 255 on)
    _c("upsample_c19_limit", "upsample", "ur_upsample_bilinear_ac_f32", ("scalar", "limit"), N=64219, h=8, w=8, C=19, H=32, W=55,
       count=64219 * 32 * 55 * 19, limit=GRID, more=dict(N=64220)),
    _c("upsample_c256_limit", "upsample", "ur_upsample_bilinear_ac_f32", ("vector", "limit"), N=2049, h=8, w=8, C=256, H=46, W=89,
       count=2049 * 46 * 89 * 256, limit=GRID, more=dict(N=2050)),
    _c("maxpool5_c19_limit", "maxpool5", "ur_maxpool5_f32", ("scalar", "limit"), N=64219, H=32, W=55, C=19, count=64219 * 32 * 55 * 19,
       limit=GRID, more=dict(N=64220)),
    _c("maxpool5_c256_limit", "maxpool5", "ur_maxpool5_f32", ("vector", "limit"), N=2049, H=46, W=89, C=256, count=2049 * 46 * 89 * 256,
       limit=GRID, more=dict(N=2050)),
    # a 1 x 1 map: the launch is over all N*C = 2^31 - 257 elements (= limit - 1), each output the one tap inside the map
    _c("maxpool_pad_limit", "maxpool_pad", "ur_maxpool2d_pad_f32", ("limit",), N=715827797, H=1, W=1, C=3, count=GRID - 1, limit=GRID,
       more=dict(N=715827798)),
    # 941 x 99223 x 23 = 2^31 - 259: image n starts at byte 4 * n * P * C, past 2^31 from image 236 on
    _c("avgpool_limit", "avgpool", "ur_avgpool_f32", ("limit", "plane offsets past 2^31 bytes"), N=941, P=99223, C=23, count=941 * 99223 * 23,
       limit=GRID, more=dict(N=942)),
    # 99962 x 31 x 33 x 21 = 2^31 - 2 (2^31 - 1 is prime)
    _c("maxpool2d_limit", "maxpool2d", "ur_maxpool2d_f32", ("limit",), N=99962, H=31, W=33, C=21, count=99962 * 31 * 33 * 21, limit=INT31,
       more=dict(N=99963)),
    # (a) x of 2^24 + 129 rows x 64 channels = 2^32 + 33024 bytes; M % 128 = 1: the last block holds one row, whose taps are the far-end reads
    _c("conv_a_x_past_4g", "conv", "ur_conv2d_f32_res", ("vector", "x past 2^32 bytes", "M tail of 1 row"), unit="row", N=1, H=1, W=(1 << 24) + 129,
       Cin=64, Cout=8, k=1, stride=1, pad=0, res=False, relu=True, tol="1x1_s2_256_512"),
    # (b) 86540 images of 33 x 47 x 4: 2^31 + 93 KiB bytes; K = 36 = two tiles of 16 and a tail of 4, gathered four channels at a time
    _c("conv_b_3x3_s2_past_2g", "conv", "ur_conv2d_f32_res", ("vector", "x past 2^31 bytes", "K tail"), unit="image", N=86540, H=33, W=47, Cin=4,
       Cout=8, k=3, stride=2, pad=1, res=False, relu=True, tol="3x3_s2_128_128"),
    # (c) 10737500 rows x 200 columns = 2^31 + 16352 elements of y and of the residual; 200 = three 64-column tiles and a tail of 8
    _c("conv_c_y_past_2g_elems", "conv", "ur_conv2d_f32_res", ("vector", "y past 2^31 elements", "residual", "Cout tail"), unit="row", N=1, H=1,
       W=10737500, Cin=8, Cout=200, k=1, stride=1, pad=0, res=True, relu=False, tol="1x1_64_256_res_no_relu"),
    # (d) the scalar gather (Cin = 3, as the stems): 115400 images of 33 x 47 x 3 = 2^31 + 333 KiB bytes
    _c("conv_d_cin3_past_2g", "conv", "ur_conv2d_f32_res", ("scalar", "x past 2^31 bytes"), unit="image", N=115400, H=33, W=47, Cin=3, Cout=8,
       k=3, stride=1, pad=1, res=False, relu=True, tol="7x7_s2_3_64"),
    # ---- csrc/segment.hip ------------------------------------------------------------------------------------------------------------
    # N*3*H*W = 2^31 - 2 (2^31 - 1 is prime); the launch is over the N*8*8 outputs, the input is read through 64-bit plane offsets
    _c("seg_prep_limit", "seg_prep", "ur_seg_prep", ("limit",), N=993, H=434, W=1661, OH=8, OW=8, count=993 * 3 * 434 * 1661, limit=INT31,
       more=dict(N=994)),
    # 99223 x 23 x 941 = 2^31 - 259 pixels, avg == NULL; three 16 x 16 maps of 19 classes
    _c("tta_pixels_limit", "tta", "ur_seg_tta_argmax", ("limit", "avg null"), N=99223, C=19, maps=((16, 16), (16, 16), (16, 16)), H=23, W=941,
       avg=False, count=99223 * 23 * 941, limit=GRID, more=dict(N=99224)),
    _c("tta_avg_limit", "tta", "ur_seg_tta_argmax", ("limit", "avg given"), N=64219, C=19, maps=((16, 16), (12, 19), (9, 14)), H=32, W=55,
       avg=True, count=64219 * 32 * 55 * 19, limit=GRID, more=dict(N=64220)),
    _c("confusion_one_trip", "confusion", "ur_seg_confusion", ("trip 1", "2 bin passes"), P=TRIP, C=19, i64=False),
    _c("confusion_second_trip", "confusion", "ur_seg_confusion", ("trip 2", "int64 targets"), P=TRIP + 1, C=19, i64=True),
    _c("confusion_third_trip", "confusion", "ur_seg_confusion", ("trip 3",), P=2 * TRIP + 4097, C=19, i64=False),
    _c("confusion_limit", "confusion", "ur_seg_confusion", ("limit",), P=INT31 - 1, C=19, i64=False, count=INT31 - 1, limit=INT31,
       more=dict(P=INT31)),
    _c("confusion_c255", "confusion", "ur_seg_confusion", ("255 bin passes",), P=5000, C=255, i64=False),
    _c("confusion_c1", "confusion", "ur_seg_confusion", ("C = 1",), P=5000, C=1, i64=False),
    # ---- csrc/classify.hip -----------------------------------------------------------------------------------------------------------
    # 10631 x 3 x 257 x 262 = 2^31 - 386 (H and W >= 224, so the input is the largest of x, tmp and y and its count the binding one)
    _c("classify_prep_limit", "classify_prep", "ur_classify_preprocess", ("limit",), N=10631, H=257, W=262, count=10631 * 3 * 257 * 262,
       limit=GRID, more=dict(N=10632)),
    _c("top1_limit", "top1", "ur_top1_counts", ("limit",), N=21643, C=99223, count=21643 * 99223, limit=GRID, more=dict(N=21644)),
    # ---- csrc/lpips.hip --------------------------------------------------------------------------------------------------------------
    _c("lpips_prep_limit", "lpips_prep", "ur_lpips_prep", ("limit",), N=55245, H=43, W=113, count=55245 * 43 * 113, limit=P28, more=dict(N=55246)),
    _c("lpips_layer_c64", "lpips_layer", "ur_lpips_layer", ("feat past 2^31 elements",), N=1025, P=16401, C=64),
    _c("lpips_layer_c384", "lpips_layer", "ur_lpips_layer", ("feat past 2^31 elements",), N=1025, P=2737, C=384),
    # the largest batch of 31 x 31 images: N*H*W = 2^28 - 287 (the next image is refused); five taps of one chunk each
    _c("lpips_finish_limit", "lpips_finish", "ur_lpips_finish", ("limit",), N=279329, H=31, W=31, count=279329 * 31 * 31, limit=P28, more=dict(N=279330)),
    # ---- csrc/metrics.hip ------------------------------------------------------------------------------------------------------------
    # 4099 images x 3 planes of 296 x 296: 2^32 + 14.6 MB bytes in pred and in target; 5 x 19 tiles per plane, so the second pass
    # adds C*T = 285 partials per image: more than its 256 threads.  (Many small images, not a few large ones: the CPU yardstick
    # runner.ssim of an 11000 x 11000 image takes minutes.)
    _c("metrics_past_4g", "metrics", "ur_image_metrics", ("planes past 2^32 bytes", "C*T above 256"), N=4099, C=3, H=296, W=296, win=7),
]

# exports of the four files that launch a kernel, and what no case runs, with the reason
LAUNCHING_EXPORTS = ("ur_image_metrics", "ur_lpips_prep", "ur_conv2d_f32", "ur_conv2d_f32_res", "ur_maxpool2d_f32", "ur_lpips_layer", "ur_lpips_finish",
                     "ur_classify_preprocess", "ur_maxpool2d_pad_f32", "ur_avgpool_f32", "ur_top1_counts", "ur_seg_prep",
                     "ur_upsample_bilinear_ac_f32", "ur_maxpool5_f32", "ur_add_f32", "ur_seg_tta_argmax", "ur_seg_confusion")
NOT_RUN = {"ur_conv2d_f32": "one call of ur_conv2d_f32_res with res = NULL, nothing of its own"}
TWO_KERNELS = ("ur_add_f32", "ur_upsample_bilinear_ac_f32", "ur_maxpool5_f32", "ur_conv2d_f32_res")      # a float4 and a scalar kernel
PROPERTIES = ("trip 1", "trip 2", "trip 3", "2 bin passes", "255 bin passes", "C = 1", "int64 targets", "avg null", "avg given",
              "x past 2^32 bytes", "x past 2^31 bytes", "y past 2^31 elements", "residual", "K tail", "Cout tail", "M tail of 1 row",
              "feat past 2^31 elements", "planes past 2^32 bytes", "C*T above 256", "plane offsets past 2^31 bytes")
EXACT = ("confusion_limit", "maxpool_pad_limit", "lpips_prep_limit")      # count == limit - 1; the others: the largest count of the geometry
# Not run on a device: ur_top1_counts with N = 1 and C from 2^30 to 2^31 - 257 (where its second kernel's launch count, C, reaches the
# limit and the counts rows start past 2^31 elements) has one wave walk 2^30 logits or more.  Its block count is checked by the host
# program tests/launch_size_main.cpp; its row offsets are 64-bit.
HOST_ONLY = {"ur_top1_counts: C from 2^30 to the launch limit": "one 64-lane block over 2^30 .. 2^31 - 257 logits"}


# One long output axis (N = W = 1): the entries of the callers' align_corners tables - idx [nmaps][H], wt [nmaps][H][2] - lie past
# 2^31: `2 * oy` (upsample, H = 2^30 + 129), `2 * (k * H + oy)` (tta_avg: three maps, H = 2^29 + 129, the largest H whose averaged
# logits of 3 classes stay below the 2^31 - 256 elements) and `k * H + oy` itself (tta_pred: avg NULL, H = 2^30 + 129).  The tables
# are the caller's, so they are made periodic (row oy = row oy mod 771) and so is the output; `long_axis_units` builds the period
# and its fp64 reference.
LONG_AXIS = dict(upsample=dict(H=(1 << 30) + 129, maps=(5,), C=1), tta_avg=dict(H=(1 << 29) + 129, maps=(5, 4, 6), C=3, avg=True),
                 tta_pred=dict(H=(1 << 30) + 129, maps=(5, 4), C=3, avg=False))


def long_axis_units(op):
    """(x or maps [h] / [h, C] fp32, idx [k][P] int32, wt [k][P][2] fp32, ref fp64 [P, 1, C], bnd) for the LONG_AXIS shape of `op`:
    output row r of the period is h0 * src[idx] + h1 * src[idx + 1] with the fp32 table weights, in fp64 (the W axis has one
    column, weights (1, 0)); for tta the mean of the two maps.  The bound is the op's own (UPSAMPLE_TOL / TTA_TOL x max |x|)."""
    import torch
    import segment_reference as SR
    g = torch.Generator().manual_seed(77)
    d = LONG_AXIS[op]
    hs = d["maps"]
    srcs = [3.0 * torch.randn(h, d["C"], generator=g) for h in hs]
    idx = torch.stack([torch.randint(0, h - 1, (P_FLAT,), generator=g, dtype=torch.int32) for h in hs])
    frac = torch.rand(len(hs), P_FLAT, generator=g)
    frac[:, ::7] = 0.0                                         # some rows sit on a source row
    wt = torch.stack([1.0 - frac, frac], dim=2).contiguous()   # fp32 [k][P][2]
    outs = [wt[k, :, 0:1].double() * s.double()[idx[k].long()] + wt[k, :, 1:2].double() * s.double()[idx[k].long() + 1] for k, s in enumerate(srcs)]
    ref = (sum(outs) / len(outs)).view(P_FLAT, 1, d["C"])
    scale = max(float(s.abs().max()) for s in srcs)
    tol = SR.UPSAMPLE_TOL if op == "upsample" else SR.TTA_TOL
    return srcs, idx, wt, ref, torch.full_like(ref, tol * scale)


def by_id(cid):
    return next(c for c in CASES if c["id"] == cid)


def confusion_trips(P):
    """Trips of the chunk loop the busiest block of the confusion kernel makes."""
    chunks = -(-P // SC_CHUNK)
    blocks = min(chunks, SC_MAX_BLOCKS)
    return -(-chunks // blocks)


def bin_passes(C):
    return -(-C * C // 256)


def conv_out(c):
    return (c["H"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1, (c["W"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1


def refusal(c, lib, ptr=256):
    """The return code of case c's entry point on `more` (one unit past the largest accepted shape), with placeholder pointers:
    a refusal returns before any HIP call."""
    d = dict(c, **c["more"])
    p, op = ptr, c["op"]
    if op == "add":
        return lib.ur_add_f32(p, p + 256, p + 512, d["n"], None)
    if op == "upsample":
        return lib.ur_upsample_bilinear_ac_f32(p, p + 256, d["N"], d["h"], d["w"], d["C"], d["H"], d["W"], p, p, p, p, None)
    if op == "maxpool5":
        return lib.ur_maxpool5_f32(p, p + 256, d["N"], d["H"], d["W"], d["C"], None)
    if op == "seg_prep":
        return lib.ur_seg_prep(p, p + 256, d["N"], 3, d["H"], d["W"], d["OH"], d["OW"], p, p, p, p, None)
    if op == "tta":
        m = d["maps"]
        return lib.ur_seg_tta_argmax(p, p, p, 3, d["N"], d["C"], m[0][0], m[0][1], m[1][0], m[1][1], m[2][0], m[2][1], d["H"], d["W"], p, p, p, p,
                                     p + 256, p + 512 if d["avg"] else None, None)
    if op == "confusion":
        return lib.ur_seg_confusion(p, p, int(d["i64"]), d["P"], d["C"], 255, p, 1 << 40, p, None)
    if op == "maxpool_pad":
        return lib.ur_maxpool2d_pad_f32(p, p + 256, d["N"], d["H"], d["W"], d["C"], None)
    if op == "avgpool":
        return lib.ur_avgpool_f32(p, p + 256, d["N"], d["P"], d["C"], None)
    if op == "classify_prep":
        return lib.ur_classify_preprocess(p, p + 256, p + 512, d["N"], 3, d["H"], d["W"], p, p, p, 4, p, p, p, 4, None)
    if op == "top1":
        return lib.ur_top1_counts(p, p, d["N"], d["C"], p, p, None)
    if op == "lpips_prep":
        return lib.ur_lpips_prep(p, p + 256, d["N"], 3, d["H"], d["W"], None)
    if op == "maxpool2d":
        return lib.ur_maxpool2d_f32(p, p + 256, d["N"], d["H"], d["W"], d["C"], None)
    if op == "lpips_finish":
        return lib.ur_lpips_finish(p, 1 << 40, d["N"], d["H"], d["W"], p, None)
    raise KeyError(op)


# ---- the periodic units with their fp64 reference and bound (torch from here on) ------------------------------------------------------
def _seed(c):
    return sum(ord(ch) for ch in c["id"])


def build(c):
    """The P distinct units of case c on the CPU: a dict with
         ins    name -> fp32 tensor [P, ...] in the kernel's layout (what is tiled on the device)
         ref    fp64 [P, R, width]: the reference of the output units (R rows of `width` values per unit)
         bnd    fp64, same shape: the per-element bound (0: bit-equal)
         ref32  (fp32 ops) the same computed by the reference's own fp32 restatement: the host gate asserts |ref32 - ref| <= bnd
       and op-specific extras.  Nothing here depends on the unit COUNT, only on the geometry of one unit."""
    import torch
    import torch.nn.functional as F
    import classify_reference as CR
    import lpips_reference as LR
    import segment_reference as SR
    g = torch.Generator().manual_seed(_seed(c))
    op = c["op"]
    if op == "add":
        a, b = torch.randn(P_FLAT, generator=g), torch.randn(P_FLAT, generator=g)
        return dict(ins=dict(a=a, b=b), ref=(a + b).double().view(P_FLAT, 1, 1), bnd=torch.zeros(P_FLAT, 1, 1, dtype=torch.float64))
    if op == "upsample":
        x = torch.randn(P_IMG, c["C"], c["h"], c["w"], generator=g)
        size = (c["H"], c["W"])
        ref = SR.nhwc(SR.resize_ac(x, size)).reshape(P_IMG, -1, c["C"])
        ref32 = SR.nhwc(SR.resize_ac_einsum32(x, size)).reshape(P_IMG, -1, c["C"])
        return dict(ins=dict(x=SR.nhwc(x)), ref=ref, bnd=torch.full_like(ref, SR.UPSAMPLE_TOL * float(x.abs().max())), ref32=ref32)
    if op in ("maxpool5", "maxpool2d", "maxpool_pad"):
        x = torch.randn(P_IMG, c["C"], c["H"], c["W"], generator=g)
        if op != "maxpool_pad":
            x[1] = -x[1].abs() - 0.5                          # an all-negative image: padding with 0 instead of -inf would win
        y = {"maxpool5": SR.maxpool5, "maxpool2d": LR.pool, "maxpool_pad": CR.maxpool}[op](x)
        ref = SR.nhwc(y).double().reshape(P_IMG, -1, c["C"])
        return dict(ins=dict(x=SR.nhwc(x)), ref=ref, bnd=torch.zeros_like(ref))
    if op == "seg_prep":
        x = SR.images((P_IMG, 3, c["H"], c["W"]), _seed(c))
        size = (c["OH"], c["OW"])
        ref = SR.nhwc(SR.prep(x, size)).reshape(P_IMG, -1, 3)
        return dict(ins=dict(x=x), ref=ref, bnd=torch.full_like(ref, SR.PREP_TOL), ref32=SR.nhwc(SR.prep_einsum32(x, size)).reshape(P_IMG, -1, 3))
    if op == "tta":
        maps = [3.0 * torch.randn(P_IMG, c["C"], h, w, generator=g) for h, w in c["maps"]]
        size = (c["H"], c["W"])
        want = SR.tta_average(maps, size)
        scale = max(float(m.abs().max()) for m in maps)
        ok = SR.decidable(want, SR.TTA_TOL * scale)                                   # [P, H, W]
        pred = want.argmax(dim=1).double().reshape(P_IMG, -1, 1)
        pbnd = torch.where(ok, 0.0, 255.0).double().reshape(P_IMG, -1, 1)             # an undecidable pixel may be any class
        ref = SR.nhwc(want).reshape(P_IMG, -1, c["C"])
        ref32 = SR.nhwc(SR.tta_average_einsum32(maps, size)).reshape(P_IMG, -1, c["C"])
        return dict(ins={f"m{k}": SR.nhwc(m) for k, m in enumerate(maps)}, ref=ref, bnd=torch.full_like(ref, SR.TTA_TOL * scale), ref32=ref32,
                    pred=pred, pred_bnd=pbnd, undecidable=1.0 - float(ok.float().mean()))
    if op == "avgpool":
        x = F.relu(torch.randn(P_IMG, c["C"], c["P"], 1, generator=g)) + 0.01        # (classify_reference.avgpool_case's values)
        ref = CR.avgpool(x).view(P_IMG, 1, c["C"])
        bnd = CR.AVGPOOL_TOL * x.double().abs().mean(dim=(2, 3)).view(P_IMG, 1, c["C"])
        return dict(ins=dict(x=CR.nhwc(x)), ref=ref, bnd=bnd, ref32=CR.avgpool(x, torch.float32).view(P_IMG, 1, c["C"]))
    if op == "classify_prep":
        x = CR.images((P_IMG, 3, c["H"], c["W"]), _seed(c))
        ref = CR.nhwc(CR.preprocess(x)).reshape(P_IMG, -1, 3)
        return dict(ins=dict(x=x), ref=ref, bnd=torch.full_like(ref, CR.PREP_TOL), ref32=CR.nhwc(CR.preprocess_einsum32(x)).reshape(P_IMG, -1, 3))
    if op == "lpips_prep":
        x = LR.images((P_IMG, 3, c["H"], c["W"]), _seed(c))[0]
        ref = LR.nhwc(LR.scale_input(x)).reshape(P_IMG, -1, 3)
        return dict(ins=dict(x=x), ref=ref, bnd=torch.full_like(ref, LR.PREP_TOL),
                    ref32=LR.nhwc(LR.scale_input(x, torch.float32)).reshape(P_IMG, -1, 3))
    if op == "top1":
        P = 7                                                                          # rows per period
        x = torch.randn(P, c["C"], generator=g)
        x[2, 5] = x[2, 900] = 100.0                                                    # a tie: the lowest index
        x[4, c["C"] - 1] = 50.0                                                        # the last class
        x[5, 77] = float("nan")                                                        # NaN is the maximum
        x[5, 4000] = float("nan")                                                      # ... the first one
        want = torch.tensor([5 if i == 2 else c["C"] - 1 if i == 4 else 77 if i == 5 else int(x[i].argmax()) for i in range(P)])
        labels = torch.tensor([int(want[0]), 3, 5, int(want[3]), 0, 77, 12345])        # four hits in seven
        return dict(ins=dict(x=x), pred=want, labels=labels)
    if op == "conv":
        P = P_FLAT if c["unit"] == "row" else P_IMG
        k, cin, cout = c["k"], c["Cin"], c["Cout"]
        h, w = (1, 1) if c["unit"] == "row" else (c["H"], c["W"])
        x = torch.randn(P, cin, h, w, generator=g)
        if cin != 3:
            x = F.relu(x)
        wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        b = 0.1 * torch.randn(cout, generator=g)
        oh, ow = (h + 2 * c["pad"] - k) // c["stride"] + 1, (w + 2 * c["pad"] - k) // c["stride"] + 1
        res = torch.randn(P, cout, oh, ow, generator=g) if c["res"] else None
        ref = CR.nhwc(CR.conv(x, wt, b, c["stride"], c["pad"], res, c["relu"])).reshape(P, -1, cout)
        ref32 = CR.nhwc(CR.conv(x, wt, b, c["stride"], c["pad"], res, c["relu"], torch.float32)).reshape(P, -1, cout)
        bnd = CR.CONV_TOL[c["tol"]] * CR.nhwc(CR.conv_abs(x, wt, b, c["stride"], c["pad"], res)).reshape(P, -1, cout)
        ins = dict(x=CR.nhwc(x))
        if res is not None:
            ins["res"] = CR.nhwc(res)
        return dict(ins=ins, ref=ref, bnd=bnd, ref32=ref32, weight=wt, bias=b)
    if op == "lpips_layer":
        fp, ft = (F.relu(torch.randn(P_IMG, c["C"], c["P"], 1, generator=g)) for _ in range(2))
        lin = torch.rand(c["C"], generator=g) / c["C"]
        fp[0, :, 0, 0] = 0.0                                                           # all zero in one image
        fp[0, :, 1, 0] = 0.0                                                           # ... and in both
        ft[0, :, 1, 0] = 0.0
        ref = LR.layer(fp, ft, lin).view(P_IMG, 1, 1)
        return dict(ins=dict(fp=LR.nhwc(fp), ft=LR.nhwc(ft)), lin=lin, ref=ref, bnd=LR.LAYER_TOL * LR.layer_abs(fp, ft, lin).view(P_IMG, 1, 1),
                    ref32=(((LR.unit(fp) - LR.unit(ft)) ** 2 * lin.view(1, -1, 1, 1)).sum(dim=1).double().mean(dim=(1, 2))).view(P_IMG, 1, 1))
        # (ref32: every pixel in fp32, the pixels added in fp64 - what the kernel does; fp32 sums over 16401 pixels are not its business)
    if op == "lpips_finish":
        # partials of the five taps (one chunk each at 31 x 31: 49, 9, 1, 1, 1 pixels): out = sum over taps, in order, of part / pixels
        parts = torch.rand(P_IMG, 5, generator=g, dtype=torch.float64)
        pixels = (49.0, 9.0, 1.0, 1.0, 1.0)
        out = torch.zeros(P_IMG, dtype=torch.float64)
        for t in range(5):
            out = out + (0.0 + parts[:, t]) / pixels[t]
        return dict(ins=dict(parts=parts), pixels=pixels, ref=out.view(P_IMG, 1, 1), bnd=torch.zeros(P_IMG, 1, 1, dtype=torch.float64))
    if op == "metrics":
        from unirestore_amd import runner
        import test_metrics_gpu as MG
        shape = (P_IMG, c["C"], c["H"], c["W"])
        tgt = torch.rand(shape, generator=g)
        pred = (tgt + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
        ps = runner.psnr_per_image(pred, tgt, 1.0).double().view(P_IMG, 1, 1)
        ss = torch.tensor([runner.ssim(pred[i:i + 1], tgt[i:i + 1], 1.0, c["win"]) for i in range(P_IMG)], dtype=torch.float64).view(P_IMG, 1, 1)
        return dict(ins=dict(pred=pred, target=tgt), psnr=ps, ssim=ss, psnr_bnd=torch.full_like(ps, MG.PSNR_TOL), ssim_bnd=torch.full_like(ss, MG.SSIM_TOL))
    raise KeyError(op)


def confusion_period(c):
    """One period of (pred uint8, target int64 in [0, C) or 255) for a confusion case, numpy.  The period is odd and no multiple of
    the chunk, so every chunk sees another phase; class C - 1 is never a target (an absent row), a fifth of the pixels is ignored."""
    import numpy as np
    rng = np.random.default_rng(_seed(c))
    period = 4999 if c["P"] <= 5000 else 1000003
    C = c["C"]
    target = rng.integers(0, max(C - 1, 1), period)
    target[rng.random(period) < 0.2] = 255
    if C == 255:
        target[target == 255] = 254                           # 255 classes: ignore_index 255 never occurs, class 254 is the "absent" row made present
    pred = rng.integers(0, C, period).astype(np.uint8)
    return pred, target


def confusion_expected(c, pred, target):
    """conf[t][p] of the P-pixel periodic repetition, by numpy.bincount on the period and on its tail."""
    import numpy as np
    C, n = c["C"], len(pred)

    def count(p, t):
        keep = (t >= 0) & (t < C) & (t != 255) & (p < C)
        return np.bincount(t[keep].astype(np.int64) * C + p[keep], minlength=C * C).reshape(C, C)
    q, r = divmod(c["P"], n)
    return q * count(pred, target) + count(pred[:r], target[:r])
