"""Case table of the large-tensor tests (tests/test_large_tensors_gpu.py; CPU gate in tests/test_large_tensors_cpu.py).  Importable
without torch.

Every other parity matrix of the suite launches on a few MiB.  Production launches on far more: the fanned-out decoder batch of
DiffUIE.forward_tasks (3 tasks, B = 8, 512 x 512) has 256-channel maps of 24 x 512 x 512 x 256 = 1.61 G elements = 3.2 GB, and
tiling.task_chunks packs chunks right up to the conv launcher's element limit.  The cases here put one tensor of each launch into
one of three size classes, by the element count E of the launch's largest 16-bit tensor (`big` names it):

  past2g   E a little above 2^30: the tensor's bytes cross 2^31 (signed 32-bit byte offsets);
  limit    the largest E the export accepts for this geometry (include/unirestore_hip.h "size limits"): the bytes end just below
           2^32 (unsigned wrap; the byte offset 0xffffff00 from which the buffer descriptors of csrc/igemm_impl.h read zeros);
  past2^31 E a little above 2^31, only for tensors the export states no element limit for.

The inputs are periodic (tests/large_harness.py): image i is image i mod 3, row i of a Linear is row i mod 771 - odd periods, so
tiles straddle the unit boundaries differently in every period - and the reference is the existing fp64 one of the P distinct units.
Channels are small and the size sits in N (images) or M (rows), so a launch stays at a few 1e12 FLOP.

bf16 only: the fp16 instantiations differ in the conversion instructions, not in any address arithmetic, and every feature is
already crossed with fp16 at small shapes (tests/conv_launcher_cases.py, tests/norm_cases.py, tests/boundary_cases.py).
"""
import conv_launcher_cases as LC

GN_MAX_N = 65535                 # GroupNorm family and ur_avgpool_hw: images are gridDim.y
P_IMG, P_ROW = 3, 771            # periods: images, rows of a Linear
G30, G31 = 1 << 30, 1 << 31
SRC_LIMIT = G31                  # ur_conv2d_nhwc: N*H*W*max(ldx, ldx2) must be below this (32-bit element offsets)
W_LIMIT = G31 - 256              # ur_conv2d_nhwc: Cout*ldw must be below this (its rows are read through buffer descriptors, see IG_OOB_BYTES)
GRID_LIMIT = 1 << 23             # ur_conv2d_nhwc: row tiles x column tiles of the planned launcher must be below this
IG_OOB_BYTES = 0xFFFFFF00        # byte offset the LDS-DMA kernels' buffer descriptors read as zero from (csrc/igemm_impl.h)
DESCRIPTOR_LAUNCHERS = ("halo_8x32_160", "halo_8x32_128", "halo_thin_32", "himg_16x16", "himg_8x8x4", "wstream_8x8", "gemm_256x256",
                        "gemm_256x320_pair", "g1_128x128", "g1_128x160", "g1_128x64", "g1_64x64", "g1_64x64_deep", "g1_128x64_deep")
ROWS_LIMIT = G31 - 512           # ur_conv2d_nhwc: N*OH*OW must be below this
NONE, SILU, GELU, GEGLU, GATE = LC.NONE, LC.SILU, LC.GELU, LC.GEGLU, LC.GATE


def conv(cid, cls, launcher, big, N, H, W, C1, Cout, KH=3, **kw):
    """A conv case: LC.case plus the size class, the tensor that carries the size, and the periodic unit (an image; a row when the
    geometry is a Linear, N = H = 1)."""
    c = LC.case(cid, launcher, N, H, W, C1, Cout, KH, **kw)
    c.update(cls=cls, big=big, unit="row" if (N == 1 and H == 1 and KH == 1) else "image")
    return c


def lin(cid, cls, launcher, big, M, K, Cout, **kw):
    return conv(cid, cls, launcher, big, 1, 1, M, K, Cout, 1, **kw)


def wlin(cid, cls, launcher, M, K, Cout, **kw):
    """A Linear whose WEIGHT is the large tensor: few rows, a long K, many output columns.  The periodic unit is a weight row
    (= an output column): w row j is row j mod 771, and so is bias[j]."""
    c = lin(cid, cls, launcher, "w", M, K, Cout, **kw)
    c["unit"] = "wrow"
    return c


def units(c):
    """(unit count U, period P) of case c."""
    if c["unit"] == "wrow":
        return c["Cout"], P_ROW
    return (c["W"], P_ROW) if c["unit"] == "row" else (c["N"], P_IMG)


def period_case(c):
    """The same geometry with one period of units: the case whose inputs and fp64 reference the existing generators build."""
    if c["unit"] == "wrow":
        return dict(c, Cout=P_ROW)
    if c["unit"] == "row":
        return dict(c, W=P_ROW, OW=P_ROW)
    return dict(c, N=P_IMG)


def elems(c):
    """Element counts of the tensors of case c (x2 and residual only where present)."""
    g = LC.geometry(c)
    M = LC.m_rows(c)
    px = c["N"] * c["H"] * c["W"]
    return dict(x=px * g["ldx"], x2=px * c["C2"], w=c["Cout"] * g["ldw"], y=M * g["ldy"], r=M * g["ldr"], M=M)


def next_unit(c):
    """Case c with one more unit (image or row)."""
    if c["unit"] == "wrow":
        return dict(c, C1=c["C1"] + 8)          # (the weight grows by a K step of 8: Cout rows of 8 elements)
    if c["unit"] == "row":
        return dict(c, W=c["W"] + 1, OW=c["OW"] + 1)
    return dict(c, N=c["N"] + 1)


# 3x3 geometry of the mandatory limit cases: 29 x 43 images, 64 channels in rows of 120 (149640 elements per image; 14351 images are
# 2^31 - 8 elements, so the last pixel's channels start at byte 0xffffff00 - where a buffer descriptor of the LDS-DMA kernels would
# read zeros.  They plan to v2_128x64 / v2_256x* (3x3) and v1_128x64 (1x1), which read through 64-bit pointers.)
G2943 = dict(H=29, W=43, C1=64, ldx_pad=56)

CONV_CASES = [
    # ---- past2g: E a little above 2^30 ------------------------------------------------------------------------------------------
    conv("p_halo128_gnab_gn", "past2g", "halo_8x32_128", "y", 7712, 32, 32, 64, 128, gn_ab=True, gn=True),
    conv("p_halo128_ups", "past2g", "halo_8x32_128", "y", 7712, 16, 16, 64, 128, ups=True, act=GELU),
    conv("p_halo160_res_silu", "past2g", "halo_8x32_160", "y", 6244, 32, 32, 64, 160, res=True, act=SILU),
    conv("p_thin_f32", "past2g", "halo_thin_32", "x", 16388, 32, 32, 64, 8, out_f32=True),
    conv("p_himg16_cat_rowbias", "past2g", "himg_16x16", "x", 32770, 16, 16, 128, 128, C2=128, bias_img=True, act=SILU, ldy_pad=0),
    conv("p_himg8", "past2g", "himg_8x8x4", "x", 65540, 8, 8, 256, 128, res=True),
    conv("p_v2_128x64_gn", "past2g", "v2_128x64", "x", 7177, Cout=64, gn=True, **G2943),
    conv("p_v2_256x128_rowbias", "past2g", "v2_256x128", "y", 6334, Cout=128, bias_img=True, **G2943),
    conv("p_v2_256x160", "past2g", "v2_256x160", "y", 5128, Cout=160, act=SILU, **G2943),
    conv("p_v2_256x32_s2", "past2g", "v2_256x32", "x", 3847, 58, 86, 32, 16, stride=2, ldx_pad=24),
    lin("p_g1_128x128_res", "past2g", "g1_128x128", "y", 7895163, 64, 128, res=True),
    lin("p_g1_128x160", "past2g", "g1_128x160", "y", 6391323, 64, 160, act=GELU),
    lin("p_v1_128x64", "past2g", "v1_128x64", "y", 14913083, 64, 64),
    lin("p_v1_256x32_f32", "past2g", "v1_256x32", "x", 33554435, 32, 8, out_f32=True, ldy_pad=4),
    lin("p_gemm256_gate", "past2g", "gemm_256x256", "y", 7895163, 64, 256, act=GATE),
    lin("p_gemm320_geglu", "past2g", "gemm_256x320_pair", "y", 1687552, 64, 1280, act=GEGLU),
    lin("p_v1_128x128_gate", "past2g", "v1_128x128", "y", 14913083, 64, 128, act=GATE),
    wlin("p_splitk_w", "past2g", "v1_128x128", 128, 65600, 16384),                 # split-K (3 splits at WS_FULL) + plain reduce
    lin("p_v1_128x160_cat", "past2g", "v1_128x160", "x", 2236965, 32, 160, C2=32, ldx_pad=448),
    # ---- limit: the largest unit count the export accepts for the geometry: x below 2^31 elements, w below 2^31 - 256 (the next
    #      unit is refused, or - for the pure-GEMM LDS-DMA launchers, whose own rule is M * ldx + K < 2^31 - 256 - plans to the
    #      register-staged twin) ------------------------------------------------------------------------------------------------
    conv("l_halo128_n16383", "limit", "halo_8x32_128", "x", 16383, 32, 32, 128, 128, res=True),
    conv("l_halo160_n16383", "limit", "halo_8x32_160", "x", 16383, 32, 32, 128, 160, gn=True),
    conv("l_thin_n32767", "limit", "halo_thin_32", "x", 32767, 32, 32, 64, 8, out_f32=True),
    conv("l_himg16_n32767", "limit", "himg_16x16", "x", 32767, 16, 16, 256, 128),
    conv("l_himg8_n131068", "limit", "himg_8x8x4", "x", 131068, 8, 8, 256, 128),
    conv("l_v2_128x64_3x3_n14351", "limit", "v2_128x64", "x", 14351, Cout=64, **G2943),
    conv("l_v1_128x64_1x1_n14351", "limit", "v1_128x64", "x", 14351, Cout=64, KH=1, **G2943),
    conv("l_v2_256x128_n14351", "limit", "v2_256x128", "x", 14351, Cout=128, **G2943),
    conv("l_v2_256x160_n14351", "limit", "v2_256x160", "x", 14351, Cout=160, **G2943),
    conv("l_v2_256x32_s2_n7688", "limit", "v2_256x32", "x", 7688, 58, 86, 32, 16, stride=2, ldx_pad=24),
    lin("l_linear_g1_side", "limit", "g1_128x128", "x", (1 << 25) - 6, 64, 72),
    lin("l_linear_v1_side", "limit", "v1_128x128", "x", (1 << 25) - 5, 64, 72),       # (the first M past the g1 rule, not the last accepted)
    lin("l_v1_128x128", "limit", "v1_128x128", "x", (1 << 25) - 1, 64, 72, res=True),
    lin("l_g1_128x160", "limit", "g1_128x160", "x", (1 << 24) - 3, 64, 160, ldx_pad=64),
    lin("l_gemm256_gate", "limit", "gemm_256x256", "x", (1 << 24) - 3, 64, 256, act=GATE, ldx_pad=64),
    # (320-wide pair tiles are taken only when M / 256 is 64 * an odd number: the largest such M whose x still fits; the next row
    #  plans to gemm_256x256, the same kernel template at 256 columns)
    lin("l_gemm320_geglu", "limit", "gemm_256x320_pair", "x", 1687552, 64, 1280, act=GEGLU, ldx_pad=1208),
    lin("l_v1_128x64", "limit", "v1_128x64", "x", (1 << 25) - 1, 64, 64),
    lin("l_v1_256x32_f32", "limit", "v1_256x32", "x", (1 << 26) - 1, 32, 8, out_f32=True, ldy_pad=4),
    lin("l_v1_128x160_cat", "limit", "v1_128x160", "x", 4473924, 32, 160, C2=32, ldx_pad=448),
    wlin("l_splitk_w", "limit", "v1_128x128", 128, 131064, 16384),
    # a pure-GEMM LDS-DMA launch whose WEIGHT ends just below its limit, in rows of 48 bytes.  (With 89478484 rows = 2^31 - 32 elements,
    # inside the old bound, the last four rows started past byte 0xffffff00 and read as zeros: REFUSED below.)
    wlin("l_w_g1_tail", "limit", "g1_128x128", 8, 24, 89478472),
    # ---- the production shape itself: the 256-channel full-resolution maps of the three-task decode at B = 8 ---------------------------
    conv("prod_n24_512x512_c256", "prod", "halo_8x32_128", "x", 24, 512, 512, 256, 256, act=SILU, ldy_pad=0),
    # ---- y past 2^31 elements: the header states no element limit for y (64-bit offsets in every epilogue) -----------------------------
    lin("e_y_past_2g_elems", "past2^31", "g1_128x128", "y", 15790400, 64, 128),
]

# Shapes just outside a stated limit: (id, case, fragment of the refusal).  Each is an accepted limit case plus one unit.
REFUSED = [
    ("r_3x3_n14352", conv("r", "refused", "", "x", 14352, Cout=64, **G2943), "must be below 2^31"),
    ("r_1x1_n14352", conv("r", "refused", "", "x", 14352, Cout=64, KH=1, **G2943), "must be below 2^31"),
    ("r_linear_m", lin("r", "refused", "", "x", 1 << 25, 64, 64), "must be below 2^31"),
    ("r_x2", lin("r", "refused", "", "x2", 4473925, 32, 160, C2=480), "must be below 2^31"),
    ("r_w", wlin("r", "refused", "", 128, 131072, 16384), "Cout * ldw must be below 2^31 - 256"),
    ("r_w_g1_tail", wlin("r", "refused", "", 8, 24, 89478484), "Cout * ldw must be below 2^31 - 256"),
    ("r_rows", lin("r", "refused", "", "y", G31 - 512, 8, 8), "below 2^31 - 512"),
    ("r_grid", lin("r", "refused", "", "y", 1 << 27, 8, 1024), "tile grid too large"),
    ("r_wrap64", conv("r", "refused", "", "x", 65536, 65536, 65536, 8, 8, 1, ldx_pad=65528), "must be below 2^31"),   # N*H*W*ldx = 2^64
]

# Launchers no case can reach at these sizes, with the reason; tests/test_large_tensors_cpu.py plans the nearest large shape of each
# (`near`) and asserts it lands on `lands`.  All of them need a small tile count, so only an absurd row stride (ldx of millions)
# could make their x large; their w is bounded by the same tile count.
UNREACHABLE = {
    "wstream_8x8": ("8 x 8 maps of at most 16 images", conv("n", "near", "", "x", 65540, 8, 8, 256, 128, wfrag=True), "himg_8x8x4"),
    "g1_64x64": ("fewer than 200 128 x 128 tiles", lin("n", "near", "", "x", 2097153, 512, 128), "g1_128x128"),
    "g1_64x64_deep": ("at most 256 64 x 64 tiles", lin("n", "near", "", "x", 1048577, 1024, 128), "v2_256x128"),
    "g1_128x64_deep": ("fewer than 200 128 x 128 tiles", lin("n", "near", "", "x", 524289, 2048, 128), "v2_256x128"),
    "v1_64x64": ("fewer than 200 128 x 128 tiles", lin("n", "near", "", "x", 4194305, 256, 128, C2=256), "v1_128x128"),
    "g1_128x64": ("between 256 and 400 128 x 128 tiles", lin("n", "near", "", "x", 2097153, 512, 256), "g1_128x128"),
}

# Features the conv cases must cover between them (tests/test_large_tensors_cpu.py)
FEATURES = {
    "staged 16-bit output": lambda c: not c["out_f32"], "fp32 output": lambda c: c["out_f32"], "residual": lambda c: c["res"],
    "x2 virtual concat": lambda c: c["C2"] > 0, "bias_img": lambda c: c["bias_img"], "gn_part": lambda c: c["gn"],
    "gn_ab prologue": lambda c: c["gn_ab"], "upsample2x": lambda c: c["ups"], "stride 2": lambda c: c["stride"] == 2,
    "pair activation": lambda c: LC.is_pair(c),
}
SPLITK_CASES = ("p_splitk_w", "l_splitk_w")      # plan to > 1 split with a reduce pass at WS_FULL (asserted on the host)


# ---- norms and per-channel kernels: they see the same fanned-out decoder batch ------------------------------------------------------
# None of these exports states an element limit (their index arithmetic is 64-bit; include/unirestore_hip.h "size limits"), so each
# runs past2g and past2^31.  U units of R rows of C channels; E = U * R * C is the element count of the 16-bit tensors (for
# ur_spade_modulate E is that of gb, twice as wide; for ur_softmax_rows_f32 that of p, rows of C + 8).
# (e_softmax has more than 2^24 rows and e_layernorm more than 2^28: one grid of 256-thread workgroups cannot hold them, see
#  csrc/norms.hip UR_MAX_BLOCKS)
def _rows(cid, cls, op, U, C):
    return dict(id=cid, cls=cls, op=op, U=U, P=P_ROW, R=1, C=C)


def _imgs(cid, cls, op, U, R, C, **kw):
    return dict(id=cid, cls=cls, op=op, U=U, P=P_IMG, R=R, C=C, **kw)


ROW_CASES = [
    _rows("p_axpy", "past2g", "axpy", 16778000, 64), _rows("e_axpy", "past2^31", "axpy", 33555000, 64),
    _rows("p_spade", "past2g", "spade", 8389000, 64), _rows("e_spade", "past2^31", "spade", 16778000, 64),
    _rows("p_layernorm", "past2g", "layernorm", 16778000, 64), _rows("e_layernorm", "past2^31", "layernorm", 268500000, 8),
    _rows("p_softmax", "past2g", "softmax", 14913100, 64), _rows("e_softmax", "past2^31", "softmax", 29826200, 64),
]
IMG_CASES = [
    _imgs("p_scale", "past2g", "scale", 16778, 1000, 64), _imgs("e_scale", "past2^31", "scale", 33556, 1000, 64),
    _imgs("p_fanout", "past2g", "fanout", 16785, 1000, 64, K=3), _imgs("e_fanout", "past2^31", "fanout", 33561, 1000, 64, K=3),
    _imgs("p_dwconv_strip", "past2g", "dwconv", 16778, 1000, 64, H=25, W=40),
    _imgs("p_dwconv_pixel", "past2g", "dwconv", 17209, 975, 64, H=25, W=39),
    _imgs("e_dwconv_strip", "past2^31", "dwconv", 33556, 1000, 64, H=25, W=40),
    _imgs("p_groupnorm", "past2g", "groupnorm", 16778, 1000, 64, G=8), _imgs("e_groupnorm", "past2^31", "groupnorm", 33556, 1000, 64, G=8),
    _imgs("p_groupnorm_x2", "past2g", "groupnorm", 16778, 1000, 64, G=8, C2=24),          # x 40 + x2 24 channels; E is that of y
    _imgs("p_avgpool", "past2g", "avgpool", 16778, 1000, 64), _imgs("e_avgpool", "past2^31", "avgpool", 33556, 1000, 64),
    # the GroupNorm family's stated limit, N <= 65535 (images are the grid's y dimension), from the accepted side
    _imgs("l_groupnorm_n65535", "limit", "groupnorm", 65535, 257, 64, G=8), _imgs("l_avgpool_n65535", "limit", "avgpool", 65535, 257, 64),
]


def big_elems(c):
    """E of a ROW_CASES / IMG_CASES entry."""
    width = {"spade": 2 * c["C"], "softmax": c["C"] + 8}.get(c["op"], c["C"])
    return c["U"] * c["R"] * width


# ---- boundary kernels on the decode tail and the ingest: the fp32 side crosses 2^32 bytes (E = its element count > 2^30) ------------
# ur_image_unpad_resize_nchw: a real bicubic resize of a crop window (250 x 258 of a 264 x 264 canvas -> 256 x 256), fp32 output, not
# quantised, so every output has the per-element bound of boundary_reference.resize_out_reference.  ur_image_u8_egress: fp32 input
# past 2^32 bytes, three geometries per period (no resize; two downscales of a window), 8-bit slots with slack bytes behind them.
BOUNDARY_CASES = [
    dict(id="b_nhwc_to_nchw_f32", cls="f32past4g", op="layout_out", U=5462, P=P_IMG, R=1, C=3, H=256, W=256, ld=8, f32=0, mul=0.5, add=0.5),
    dict(id="b_nchw_f32_to_nhwc", cls="f32past4g", op="layout_in", U=5462, P=P_IMG, R=256 * 256, C=3, H=256, W=256, Cpad=8),
    dict(id="b_f32_to_bf16_scaled", cls="f32past4g", op="cast", U=134220000, P=P_ROW, R=1, C=4, ld=8, Cpad=8, mul=0.25, kind="rand"),
    dict(id="b_unpad_resize_nchw", cls="f32past4g", op="unpad_resize", U=5462, P=P_IMG, R=3, C=3, XH=264, XW=264, ld=8, CH=250, CW=258,
         OH=256, OW=256, mul=0.5, add=0.5, quantize=0, f32=0, special=False),
    dict(id="b_u8_egress", cls="f32past4g", op="u8_egress", U=8195, P=P_IMG, R=1, C=3, CH=128, CW=128, slack=37,
         geom=[(128, 128, 128, 128), (100, 90, 120, 112), (77, 128, 99, 128)]),
]


def f32_elems(c):
    """Elements of the fp32 tensor of a BOUNDARY_CASES entry."""
    if c["op"] == "unpad_resize":
        return c["U"] * c["C"] * c["OH"] * c["OW"]               # the fp32 NCHW output
    if c["op"] == "u8_egress":
        return c["U"] * c["CH"] * c["CW"] * 8                    # the fp32 NHWC input (ld = 8)
    return c["U"] * (c["ld"] if c["op"] == "cast" else c["C"] * c["H"] * c["W"])
