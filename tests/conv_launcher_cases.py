"""Case table of the conv / GEMM launcher parity matrix (tests/test_conv_launchers_gpu.py).  Importable without torch: the CPU
gate in tests/test_conv_plan_cpu.py plans every case on the host (ur_conv2d_plan_launch) and checks that the table reaches every
launcher of csrc/igemm_impl.h UR_CONV_LAUNCHERS, each case the one it names, and every split / reduce / statistics path.

A case is one ur_conv_desc geometry plus the epilogue features it runs.  Shapes are as small as dispatch_conv (csrc/igemm.hip) allows
for the launcher they name; the features are the ones that launcher's dispatch and plan conditions accept.  Every case runs at three
workspace sizes: WS_FULL (the size ops.workspace passes), "less" (one split fewer than the full plan, only for split launches) and
"none" (a NULL workspace, as C callers may pass), plus any `ws` entries of its own.  `launchers` names the launcher of a workspace
variant where it is not the case's own (the unsplit twin of a split launcher, or the kernel that runs when the weight stream does not fit).

The first 61 cases are the bases of tests/conv_launcher_space.py; the cases with a "+" in their id add features to a base's geometry so
that every feature and feature pair the plan accepts on a launch path is run (the gate in tests/test_conv_plan_cpu.py names what is missing).
"""

MiB = 1 << 20
WS_FULL = 192 * MiB
NONE, SILU, GELU, GEGLU, GATE = 0, 1, 2, 3, 4


def case(cid, launcher, N, H, W, C1, Cout, KH=3, *, C2=0, stride=1, pad=None, ups=False, OH=None, OW=None, act=NONE, kcm=None,
         wfrag=False, bias=True, res=False, bias_img=False, gn=False, gn_ab=False, rows=False, ln=False, yt=None, out_f32=False,
         out_scale=1.0, ldy_pad=8, ldx_pad=0, zero_rows=0, groups=0, bmm=0, ws=(), launchers=None):
    """groups = G: the descriptor ur_groupconv3x3_nhwc builds (C1 = Cg, Cout = Cog per group); bmm = B: the one ops.bmm_nt builds
    (A [B][M][ldx], B [B][N][ldw]).  yt = (n_split, t_rows).  zero_rows: trailing weight rows (and bias) that are zero - padded
    output channels, which must come out exactly 0."""
    pad = (KH // 2, KH // 2) if pad is None else pad
    hin, win = (2 * H, 2 * W) if ups else (H, W)
    OH = (hin + 2 * pad[0] - KH) // stride + 1 if OH is None else OH
    OW = (win + 2 * pad[1] - KH) // stride + 1 if OW is None else OW
    if kcm is None:
        kcm = KH == 3 and C1 % 64 == 0 and (C1 + C2) % 64 == 0
    return dict(id=cid, launcher=launcher, N=N, H=H, W=W, C1=C1, C2=C2, Cout=Cout, KH=KH, stride=stride, pad=pad, ups=ups, OH=OH,
                OW=OW, act=act, kcm=int(kcm), wfrag=wfrag, bias=bias, res=res, bias_img=bias_img, gn=gn, gn_ab=gn_ab, rows=rows, ln=ln,
                yt=yt, out_f32=out_f32, out_scale=out_scale, ldy_pad=ldy_pad, ldx_pad=ldx_pad, zero_rows=zero_rows, groups=groups,
                bmm=bmm, ws=tuple(ws), launchers=dict(launchers or {}))


def is_pair(c):
    return c["act"] in (GEGLU, GATE)


def cout_out(c):
    """Output channels per group / batch of the launch (pair activations halve the GEMM's N)."""
    return c["Cout"] // 2 if is_pair(c) else c["Cout"]


def nbatch(c):
    return c["groups"] or c["bmm"] or 1


def m_rows(c):
    return c["N"] * c["OH"] * c["OW"]


def ldy(c, gn_pass=False):
    """Leading dimension of y: padding columns past the output unless the GroupNorm fallback pass needs a dense output or the
    descriptor is a grouped / batched one (ldy as its wrapper sets it)."""
    if c["groups"]:
        return cout_out(c) * c["groups"]
    if c["bmm"] or gn_pass:
        return cout_out(c) if c["yt"] is None else c["yt"][0]
    width = cout_out(c) if c["yt"] is None else c["yt"][0]
    return width + c["ldy_pad"]


def geometry(c, gn_pass=False):
    """The ur_conv_desc fields of case c that are not pointers (ConvDesc attribute -> value)."""
    g = dict(N=c["N"], H=c["H"], W=c["W"], C1=c["C1"], C2=c["C2"], ldx2=c["C2"], Cout=c["Cout"], KH=c["KH"], KW=c["KH"],
             stride=c["stride"], pad_t=c["pad"][0], pad_l=c["pad"][1], OH=c["OH"], OW=c["OW"], upsample2x=int(c["ups"]), act=c["act"],
             out_f32=int(c["out_f32"]), out_scale=c["out_scale"], nbatch=nbatch(c), k_chunk_major=c["kcm"])
    K = c["KH"] * c["KH"] * (c["C1"] + c["C2"])
    g["ldx"] = c["C1"] + c["ldx_pad"]
    g["ldw"] = K
    g["ldy"] = ldy(c, gn_pass)
    g["ldr"] = cout_out(c) * (c["groups"] or 1) + 8 if c["res"] else 0      # (grouped: the groups' residual columns side by side)
    if c["groups"]:
        G = c["groups"]
        g.update(ldx=c["C1"] * G, ldw=K, bs_x=c["C1"], bs_w=c["Cout"] * K, bs_bias=c["Cout"], bs_y=c["Cout"], bs_r=c["Cout"])
    if c["bmm"]:
        g.update(ldx=c["C1"] + 8, ldw=c["C1"] + 16)
        g.update(bs_x=m_rows(c) * g["ldx"] + 64, bs_w=c["Cout"] * g["ldw"], bs_y=m_rows(c) * c["Cout"])
    if c["yt"] is not None:
        ns, tr = c["yt"]
        g.update(n_split=ns, t_rows=tr, t_ld=tr + 8)
    if c["bias_img"]:
        g["bias_img_stride"] = c["Cout"] * (c["groups"] or 1)
    if c["ln"]:
        g.update(ln_dim=K, ln_parts=2, ln_eps=1e-5)
    if c["gn_ab"]:
        g["gn_silu"] = 1
    return g


P = 16      # placeholder pointer: planning reads no data


def placeholders(c):
    """Non-null placeholder pointers for every input / output case c passes (ConvDesc attribute -> value)."""
    on = dict(x=True, w=True, y=True, x2=c["C2"] > 0, bias=c["bias"], residual=c["res"], gn_part=c["gn"], gn_ab=c["gn_ab"],
              row_stats=c["rows"], ln_stats=c["ln"], ln_colsum=c["ln"], yt=c["yt"] is not None, w_frag=c["wfrag"])
    return {k: (P if v else None) for k, v in on.items()}


def fill(d, c, ptrs, ws_bytes, gn_pass=False):
    """Fill ConvDesc d for case c: geometry, the pointers in ptrs, and a workspace of ws_bytes (None: no workspace; a pointer
    must then be absent from ptrs too)."""
    for k, v in geometry(c, gn_pass).items():
        setattr(d, k, v)
    for k, v in ptrs.items():
        setattr(d, k, v)
    d.workspace_bytes = ws_bytes or 0
    if ws_bytes is None:
        d.workspace = None
    return d


def splitk_bytes(c, splitk):
    """Workspace of `splitk` fp32 partial planes (plan_splitk's rule)."""
    return splitk * nbatch(c) * m_rows(c) * c["Cout"] * 4


def ws_variants(c, splitk_full):
    """(label, workspace bytes or None for a NULL workspace) of case c, given the split count of its full-workspace plan."""
    v = [("full", WS_FULL)]
    if splitk_full > 1:
        v.append(("less", splitk_bytes(c, splitk_full - 1)))
    v.append(("none", None))
    for label, nbytes in c["ws"]:
        v.append((label, nbytes))
    return v


def expected_launcher(c, label):
    return c["launchers"].get(label, c["launcher"])


def _wstream_need(N, cin, cout):
    """Workspace wstream_8x8 needs: nk / 36 partial planes of the 8 x 8 output (dispatch_conv)."""
    return (9 * cin // 64) // 36 * N * 64 * cout * 4


CASES = [
    # ---- 8 x 32 halo patches (halo_8x32_128 / _160): >= 64 patch tiles; <= 128 tiles split over 64-channel chunks
    case("h128_res_silu_gn", "halo_8x32_128", 2, 64, 64, 64, 256, res=True, act=SILU, gn=True),
    case("h128_ups_cat_rowbias_gelu_gnab", "halo_8x32_128", 2, 32, 32, 64, 256, C2=64, ups=True, bias_img=True, act=GELU, gn_ab=True, gn=True),
    case("h128_chunksplit_gnab_res_gn", "halo_8x32_128", 2, 64, 64, 256, 256, res=True, gn_ab=True, gn=True),
    case("h160_res_gelu_gn", "halo_8x32_160", 2, 64, 64, 64, 320, res=True, act=GELU, gn=True),
    case("h160_ups_cat_rowbias_silu_gn", "halo_8x32_160", 2, 32, 32, 64, 320, C2=64, ups=True, bias_img=True, act=SILU, gn=True),
    case("h160_chunksplit_res_gn", "halo_8x32_160", 2, 64, 64, 256, 320, res=True, gn=True),
    # ---- conv_out layers (<= 32 channels, fp32 or 16-bit): padded channels come out exactly 0
    case("thin_c3_f32", "halo_thin_32", 2, 64, 256, 64, 8, zero_rows=5, out_f32=True),
    case("thin_c4_res", "halo_thin_32", 2, 64, 256, 64, 4, res=True),
    case("thin_c8_silu", "halo_thin_32", 2, 64, 256, 64, 8, act=SILU),
    case("thin_c32_f32_res", "halo_thin_32", 2, 64, 256, 64, 32, res=True, out_f32=True, zero_rows=4),
    # ---- whole-image halo tiles (16 x 16: one image per tile; 8 x 8: four), split over channel chunks + the GroupNorm reduce
    case("himg16_n1_res_gn", "himg_16x16", 1, 16, 16, 256, 128, res=True, gn=True),
    case("himg16_n3_cat_rowbias_silu_gn", "himg_16x16", 3, 16, 16, 128, 256, C2=128, bias_img=True, act=SILU, gn=True),
    case("himg16_n4_gelu", "himg_16x16", 4, 16, 16, 256, 128, act=GELU),
    case("himg16_n5_ups_gnab_gn", "himg_16x16", 5, 8, 8, 256, 128, ups=True, gn_ab=True, gn=True),
    case("himg16_n16_res_gn", "himg_16x16", 16, 16, 16, 256, 256, res=True, gn=True),
    case("himg8_n4_res_gn", "himg_8x8x4", 4, 8, 8, 256, 128, res=True, gn=True),
    case("himg8_n16_cat_rowbias_silu_gn", "himg_8x8x4", 16, 8, 8, 128, 256, C2=128, bias_img=True, act=SILU, gn=True),
    # ---- the 8 x 8 weight stream (fragment-major weights); below its workspace need the whole-image tile takes over
    case("wstream_n1_res_gn", "wstream_8x8", 1, 8, 8, 512, 128, wfrag=True, res=True, gn=True,
         launchers={"less": "v1_128x128", "none": "v1_128x128"}),
    case("wstream_n3_cat_rowbias_silu", "wstream_8x8", 3, 8, 8, 256, 128, C2=256, wfrag=True, bias_img=True, act=SILU,
         launchers={"less": "v1_128x128", "none": "v1_128x128"}),
    case("wstream_n4_gn_ws_edge", "wstream_8x8", 4, 8, 8, 512, 128, wfrag=True, gn=True,
         ws=(("need", _wstream_need(4, 512, 128)), ("need_minus_4", _wstream_need(4, 512, 128) - 4)),
         launchers={"need_minus_4": "himg_8x8x4", "less": "himg_8x8x4", "none": "himg_8x8x4"}),
    case("wstream_n5_res_gn", "wstream_8x8", 5, 8, 8, 512, 256, wfrag=True, res=True, gn=True,
         launchers={"less": "v1_128x128", "none": "v1_128x128"}),
    case("wstream_n16_gelu_gn", "wstream_8x8", 16, 8, 8, 512, 128, wfrag=True, act=GELU, gn=True,
         launchers={"less": "himg_8x8x4", "none": "himg_8x8x4"}),
    # ---- 256-row gated GEMM tiles: GEGLU / GATE, ragged M, a K tail shorter than 64
    case("gemm256_geglu_res_rows", "gemm_256x256", 1, 1, 25700, 72, 512, KH=1, act=GEGLU, res=True, rows=True),
    case("gemm256_gate_gnpass", "gemm_256x256", 1, 1, 25700, 72, 512, KH=1, act=GATE, gn=True),
    case("gemm320_geglu_res", "gemm_256x320_pair", 1, 1, 8100, 72, 2560, KH=1, act=GEGLU, res=True),
    case("gemm320_gate_rows", "gemm_256x320_pair", 1, 1, 8100, 72, 2560, KH=1, act=GATE, rows=True),
    # ---- register-staged tiles (v1_*): split-K with every reduce kind, LayerNorm folding, transposed columns, fp32 output
    case("v1_128x128_3x3_split", "v1_128x128", 1, 16, 16, 64, 128, res=True, act=SILU),
    case("v1_128x128_3x3_s2_asym", "v1_128x128", 2, 33, 33, 64, 128, stride=2, pad=(0, 1), OH=16, OW=17, act=GELU),
    case("v1_128x128_3x3_split_gn", "v1_128x128", 1, 16, 16, 128, 128, gn=True, res=True),
    case("v1_128x128_geglu_ktail", "v1_128x128", 1, 1, 1000, 200, 256, KH=1, act=GEGLU, res=True),
    case("v1_128x128_ln_rows_split", "v1_128x128", 1, 1, 250, 2048, 256, KH=1, ln=True, rows=True, res=True),
    case("v1_128x128_yt_split", "v1_128x128", 1, 1, 256, 2048, 256, KH=1, yt=(128, 64)),
    case("v1_128x128_f32_scale_split", "v1_128x128", 1, 1, 250, 2048, 256, KH=1, out_f32=True, out_scale=0.5),
    case("v1_128x160_3x3_split_gn", "v1_128x160", 1, 16, 16, 64, 160, gn=True, res=True),
    case("v1_128x160_cat", "v1_128x160", 1, 1, 4000, 160, 960, KH=1, C2=160, res=True, act=GELU),
    case("v1_128x64_ktail", "v1_128x64", 1, 1, 4100, 200, 64, KH=1, res=True, act=GELU, rows=True),
    case("v1_128x64_gn", "v1_128x64", 4, 32, 32, 200, 64, KH=1, gn=True),
    case("v1_256x32_ragged_n_f32", "v1_256x32", 1, 1, 4100, 200, 20, KH=1, out_f32=True, ldy_pad=4),
    case("v1_256x32_rows_gn", "v1_256x32", 4, 32, 32, 200, 32, KH=1, rows=True, gn=True),
    case("v1_64x64_cat_split", "v1_64x64", 1, 1, 1024, 320, 640, KH=1, C2=320, res=True),
    case("v1_64x64_rows_split", "v1_64x64", 1, 1, 500, 640, 256, KH=1, rows=True, launchers={"none": "g1_64x64"}),
    case("v1_64x64_ln_split", "v1_64x64", 1, 1, 500, 640, 256, KH=1, ln=True, launchers={"none": "g1_64x64"}),
    # ---- LDS-DMA ring (v2_*): small 3x3 convs (split-K + GroupNorm reduce), stride 2, asymmetric padding, fallback GroupNorm pass
    case("v2_256x32_s2_asym_f32", "v2_256x32", 2, 33, 33, 40, 20, stride=2, pad=(1, 0), OH=17, OW=16, out_f32=True, ldy_pad=4),
    case("v2_256x32_split_gn", "v2_256x32", 1, 16, 16, 128, 32, gn=True, res=True),
    case("v2_128x64_split_gn", "v2_128x64", 1, 16, 16, 128, 64, gn=True, act=SILU),
    case("v2_128x64_rows_gelu", "v2_128x64", 1, 16, 16, 128, 64, rows=True, act=GELU, res=True),
    case("v2_256x160_s2_gnpass", "v2_256x160", 1, 406, 406, 32, 160, stride=2, gn=True, res=True, act=SILU),
    case("v2_256x128_asym_f32_scale", "v2_256x128", 2, 144, 144, 32, 128, pad=(0, 1), OH=142, OW=144, out_f32=True, out_scale=0.25),
    case("v2_256x128_rowbias_gn", "v2_256x128", 2, 144, 144, 32, 128, bias_img=True, gn=True),
    # ---- pure GEMM LDS-DMA tiles (g1_*): K tails, ragged M / N, transposed columns, fused GroupNorm sums
    case("g1_128x128_ragged_res_gelu", "g1_128x128", 1, 1, 4100, 200, 1288, KH=1, res=True, act=GELU, out_scale=0.5),
    case("g1_128x128_rows", "g1_128x128", 1, 1, 4100, 200, 1288, KH=1, rows=True),
    case("g1_128x160_ragged", "g1_128x160", 1, 1, 4100, 200, 960, KH=1, res=True, rows=True),
    case("g1_128x64_ragged", "g1_128x64", 1, 1, 4100, 200, 1280, KH=1, res=True, act=SILU),
    case("g1_64x64_ragged_yt", "g1_64x64", 1, 1, 1000, 200, 1288, KH=1, yt=(1032, 100)),
    case("g1_64x64_gn", "g1_64x64", 4, 16, 16, 200, 1288, KH=1, gn=True, res=True),
    case("g1_64x64_deep_ragged_ln", "g1_64x64_deep", 1, 1, 500, 520, 1040, KH=1, ln=True, rows=True),
    case("g1_128x64_deep_ragged", "g1_128x64_deep", 1, 1, 2000, 1608, 1040, KH=1, res=True, act=GELU),
    # ---- batched descriptors: grouped 3x3 (generic kernel; halo loop, one launch per 128-channel group) and bmm_nt strides
    case("group_generic", "v2_128x64", 1, 16, 16, 32, 36, groups=4, act=SILU),
    case("group_halo_loop", "halo_8x32_128", 1, 128, 128, 128, 128, groups=2, act=SILU),
    case("bmm_f32_scale", "g1_64x64", 1, 1, 100, 64, 72, KH=1, bmm=3, out_f32=True, out_scale=0.125, bias=False),
    case("bmm_split", "v1_64x64", 1, 1, 200, 1024, 96, KH=1, bmm=2, bias=False, launchers={"none": "g1_64x64"}),
    # ---- feature pairs (tests/conv_launcher_space.py): the id is "<base id>+<features added>".  A case is its base - geometry AND every
    # feature the base's own line sets, whether or not the base's id spells it (g1_128x128_ragged_res_gelu has out_scale=0.5, g1_64x64_gn
    # has res) - with the features after the "+" switched on as well; its line repeats all of them.  Chosen greedily, so that together with the cases above they run every (launch path, feature) and
    # (launch path, feature pair) the plan accepts with up to two features added to a base; ordered by launcher.
    case("wstream_n3_cat_rowbias_silu+out_f32", "v1_128x128", 3, 8, 8, 256, 128, C2=256, act=SILU, wfrag=True, bias_img=True, out_f32=True),
    case("v1_128x128_3x3_split+bias_img+gn+out_scale", "v1_128x128", 1, 16, 16, 64, 128, act=SILU, res=True, bias_img=True, gn=True, out_scale=0.5),
    case("v1_128x128_3x3_s2_asym+gn+rows", "v1_128x128", 2, 33, 33, 64, 128, stride=2, pad=(0, 1), act=GELU, gn=True, rows=True),
    case("v1_128x128_3x3_s2_asym+res+bias_img+gn+out_scale", "v1_128x128", 2, 33, 33, 64, 128, stride=2, pad=(0, 1), act=GELU, res=True,
         bias_img=True, gn=True, out_scale=0.5),
    case("v1_128x128_3x3_s2_asym+res+bias_img+out_f32+out_scale", "v1_128x128", 2, 33, 33, 64, 128, stride=2, pad=(0, 1), act=GELU, res=True,
         bias_img=True, out_f32=True, out_scale=0.5),
    case("v1_128x128_3x3_s2_asym+res+rows+out_scale", "v1_128x128", 2, 33, 33, 64, 128, stride=2, pad=(0, 1), act=GELU, res=True, rows=True,
         out_scale=0.5),
    case("v1_128x128_3x3_split_gn+rows", "v1_128x128", 1, 16, 16, 128, 128, res=True, gn=True, rows=True),
    case("v1_128x128_ln_rows_split+act+gn+out_scale", "v1_128x128", 1, 1, 250, 2048, 256, KH=1, act=SILU, res=True, gn=True, rows=True, ln=True,
         out_scale=0.5),
    case("v1_128x128_ln_rows_split+act+yt+out_scale", "v1_128x128", 1, 1, 250, 2048, 256, KH=1, act=SILU, res=True, rows=True, ln=True, yt=(128, 50),
         out_scale=0.5),
    case("v1_128x128_f32_scale_split+res+act+yt", "v1_128x128", 1, 1, 250, 2048, 256, KH=1, act=SILU, res=True, yt=(128, 50), out_f32=True,
         out_scale=0.5),
    case("v1_128x160_3x3_split_gn+act+bias_img+out_scale", "v1_128x160", 1, 16, 16, 64, 160, act=SILU, res=True, bias_img=True, gn=True,
         out_scale=0.5),
    case("v1_128x160_3x3_split_gn+act+rows+out_scale", "v1_128x160", 1, 16, 16, 64, 160, act=SILU, res=True, gn=True, rows=True, out_scale=0.5),
    case("v1_128x160_cat+bias_img+gn+out_scale", "v1_128x160", 1, 1, 4000, 160, 960, KH=1, C2=160, act=GELU, res=True, bias_img=True, gn=True,
         out_scale=0.5),
    case("v1_128x160_cat+bias_img+out_f32", "v1_128x160", 1, 1, 4000, 160, 960, KH=1, C2=160, act=GELU, res=True, bias_img=True, out_f32=True),
    case("v1_128x160_cat+gn+rows", "v1_128x160", 1, 1, 4000, 160, 960, KH=1, C2=160, act=GELU, res=True, gn=True, rows=True),
    case("v1_128x160_cat+rows+yt", "v1_128x160", 1, 1, 4000, 160, 960, KH=1, C2=160, act=GELU, res=True, rows=True, yt=(480, 100)),
    case("v1_128x160_cat+yt+out_f32+out_scale", "v1_128x160", 1, 1, 4000, 160, 960, KH=1, C2=160, act=GELU, res=True, yt=(480, 100), out_f32=True,
         out_scale=0.5),
    case("v1_128x64_ktail+gn+ln+out_scale", "v1_128x64", 1, 1, 4100, 200, 64, KH=1, act=GELU, res=True, gn=True, rows=True, ln=True, out_scale=0.5),
    case("v1_128x64_ktail+ln+yt+out_scale", "v1_128x64", 1, 1, 4100, 200, 64, KH=1, act=GELU, res=True, rows=True, ln=True, yt=(32, 100),
         out_scale=0.5),
    case("v1_128x64_gn+res+act+bias_img+out_scale", "v1_128x64", 4, 32, 32, 200, 64, KH=1, act=SILU, res=True, bias_img=True, gn=True, out_scale=0.5),
    case("v1_128x64_gn+rows+ln", "v1_128x64", 4, 32, 32, 200, 64, KH=1, gn=True, rows=True, ln=True),
    case("v1_256x32_ragged_n_f32+res+act+bias_img+out_scale", "v1_256x32", 1, 1, 4100, 200, 20, KH=1, act=SILU, res=True, bias_img=True,
         out_f32=True, out_scale=0.5, ldy_pad=4),
    case("v1_256x32_ragged_n_f32+res+act+yt+out_scale", "v1_256x32", 1, 1, 4100, 200, 20, KH=1, act=SILU, res=True, yt=(8, 100), out_f32=True,
         out_scale=0.5, ldy_pad=4),
    case("v1_256x32_rows_gn+res+act+ln+out_scale", "v1_256x32", 4, 32, 32, 200, 32, KH=1, act=SILU, res=True, gn=True, rows=True, ln=True,
         out_scale=0.5),
    case("v1_64x64_cat_split+act+bias_img+gn+out_scale", "v1_64x64", 1, 1, 1024, 320, 640, KH=1, C2=320, act=SILU, res=True, bias_img=True, gn=True,
         out_scale=0.5),
    case("v1_64x64_cat_split+act+bias_img+out_f32+out_scale", "v1_64x64", 1, 1, 1024, 320, 640, KH=1, C2=320, act=SILU, res=True, bias_img=True,
         out_f32=True, out_scale=0.5),
    case("v1_64x64_cat_split+act+rows+yt+out_scale", "v1_64x64", 1, 1, 1024, 320, 640, KH=1, C2=320, act=SILU, res=True, rows=True, yt=(320, 64),
         out_scale=0.5),
    case("v1_64x64_cat_split+act+yt+out_f32+out_scale", "v1_64x64", 1, 1, 1024, 320, 640, KH=1, C2=320, act=SILU, res=True, yt=(320, 64),
         out_f32=True, out_scale=0.5),
    case("v1_64x64_cat_split+gn+rows", "v1_64x64", 1, 1, 1024, 320, 640, KH=1, C2=320, res=True, gn=True, rows=True),
    case("v1_64x64_rows_split+res+act+gn+ln+out_scale", "v1_64x64", 1, 1, 500, 640, 256, KH=1, act=SILU, res=True, gn=True, rows=True, ln=True,
         out_scale=0.5, launchers={"none": "g1_64x64"}),
    case("v1_64x64_rows_split+res+act+ln+yt+out_scale", "v1_64x64", 1, 1, 500, 640, 256, KH=1, act=SILU, res=True, rows=True, ln=True, yt=(128, 100),
         out_scale=0.5, launchers={"none": "g1_64x64"}),
    case("bmm_split+res+act+out_f32+out_scale", "v1_64x64", 1, 1, 200, 1024, 96, KH=1, act=SILU, bias=False, res=True, out_f32=True, out_scale=0.5,
         bmm=2, launchers={"none": "g1_64x64"}),
    case("v2_256x32_s2_asym_f32+res+act+bias_img+out_scale", "v2_256x32", 2, 33, 33, 40, 20, stride=2, pad=(1, 0), act=SILU, res=True, bias_img=True,
         out_f32=True, out_scale=0.5, ldy_pad=4),
    case("v2_256x32_split_gn+act+bias_img+out_scale", "v2_256x32", 1, 16, 16, 128, 32, act=SILU, res=True, bias_img=True, gn=True, out_scale=0.5),
    case("v2_256x32_split_gn+act+rows+out_scale", "v2_256x32", 1, 16, 16, 128, 32, act=SILU, res=True, gn=True, rows=True, out_scale=0.5),
    case("v2_128x64_split_gn+res+bias_img+out_scale", "v2_128x64", 1, 16, 16, 128, 64, act=SILU, res=True, bias_img=True, gn=True, out_scale=0.5),
    case("v2_128x64_split_gn+rows+out_scale", "v2_128x64", 1, 16, 16, 128, 64, act=SILU, gn=True, rows=True, out_scale=0.5),
    case("group_generic+res+bias_img+out_f32+out_scale", "v2_128x64", 1, 16, 16, 32, 36, act=SILU, res=True, bias_img=True, out_f32=True,
         out_scale=0.5, groups=4),
    case("v2_256x160_s2_gnpass+bias_img+out_scale", "v2_256x160", 1, 406, 406, 32, 160, stride=2, act=SILU, res=True, bias_img=True, gn=True,
         out_scale=0.5),
    case("v2_256x160_s2_gnpass+rows+out_scale", "v2_256x160", 1, 406, 406, 32, 160, stride=2, act=SILU, res=True, gn=True, rows=True, out_scale=0.5),
    case("v2_256x128_asym_f32_scale+res+act+bias_img", "v2_256x128", 2, 144, 144, 32, 128, pad=(0, 1), act=SILU, res=True, bias_img=True,
         out_f32=True, out_scale=0.25),
    case("v2_256x128_rowbias_gn+res+act+out_scale", "v2_256x128", 2, 144, 144, 32, 128, act=SILU, res=True, bias_img=True, gn=True, out_scale=0.5),
    case("gemm256_geglu_res_rows+gn+ln+out_scale", "gemm_256x256", 1, 1, 25700, 72, 512, KH=1, act=GEGLU, res=True, gn=True, rows=True, ln=True,
         out_scale=0.5),
    case("gemm256_geglu_res_rows+ln+out_scale", "gemm_256x256", 1, 1, 25700, 72, 512, KH=1, act=GEGLU, res=True, rows=True, ln=True, out_scale=0.5),
    case("gemm320_geglu_res+gn+rows+ln+out_scale", "gemm_256x320_pair", 1, 1, 8100, 72, 2560, KH=1, act=GEGLU, res=True, gn=True, rows=True, ln=True,
         out_scale=0.5),
    case("gemm320_geglu_res+rows+ln+out_scale", "gemm_256x320_pair", 1, 1, 8100, 72, 2560, KH=1, act=GEGLU, res=True, rows=True, ln=True,
         out_scale=0.5),
    case("g1_128x128_ragged_res_gelu+bias_img+gn", "g1_128x128", 1, 1, 4100, 200, 1288, KH=1, act=GELU, res=True, bias_img=True, gn=True,
         out_scale=0.5),
    case("g1_128x128_ragged_res_gelu+bias_img+out_f32", "g1_128x128", 1, 1, 4100, 200, 1288, KH=1, act=GELU, res=True, bias_img=True, out_f32=True,
         out_scale=0.5),
    case("g1_128x128_ragged_res_gelu+gn+rows+ln", "g1_128x128", 1, 1, 4100, 200, 1288, KH=1, act=GELU, res=True, gn=True, rows=True, ln=True,
         out_scale=0.5),
    case("g1_128x128_ragged_res_gelu+rows+ln", "g1_128x128", 1, 1, 4100, 200, 1288, KH=1, act=GELU, res=True, rows=True, ln=True, out_scale=0.5),
    case("g1_128x128_ragged_res_gelu+yt+out_f32", "g1_128x128", 1, 1, 4100, 200, 1288, KH=1, act=GELU, res=True, yt=(644, 100), out_f32=True,
         out_scale=0.5),
    case("g1_128x160_ragged+act+gn+ln+out_scale", "g1_128x160", 1, 1, 4100, 200, 960, KH=1, act=SILU, res=True, gn=True, rows=True, ln=True,
         out_scale=0.5),
    case("g1_128x160_ragged+act+ln+yt+out_scale", "g1_128x160", 1, 1, 4100, 200, 960, KH=1, act=SILU, res=True, rows=True, ln=True, yt=(480, 100),
         out_scale=0.5),
    case("g1_128x64_ragged+bias_img+gn", "g1_128x64", 1, 1, 4100, 200, 1280, KH=1, act=SILU, res=True, bias_img=True, gn=True),
    case("g1_128x64_ragged+bias_img+out_f32+out_scale", "g1_128x64", 1, 1, 4100, 200, 1280, KH=1, act=SILU, res=True, bias_img=True, out_f32=True,
         out_scale=0.5),
    case("g1_128x64_ragged+gn+rows+ln+out_scale", "g1_128x64", 1, 1, 4100, 200, 1280, KH=1, act=SILU, res=True, gn=True, rows=True, ln=True,
         out_scale=0.5),
    case("g1_128x64_ragged+rows+ln+yt+out_scale", "g1_128x64", 1, 1, 4100, 200, 1280, KH=1, act=SILU, res=True, rows=True, ln=True, yt=(640, 100),
         out_scale=0.5),
    case("g1_128x64_ragged+yt+out_f32", "g1_128x64", 1, 1, 4100, 200, 1280, KH=1, act=SILU, res=True, yt=(640, 100), out_f32=True),
    case("g1_64x64_ragged_yt+out_f32", "g1_64x64", 1, 1, 1000, 200, 1288, KH=1, yt=(1032, 100), out_f32=True),
    case("g1_64x64_gn+act+bias_img+out_scale", "g1_64x64", 4, 16, 16, 200, 1288, KH=1, act=SILU, res=True, bias_img=True, gn=True, out_scale=0.5),
    case("g1_64x64_gn+rows+ln", "g1_64x64", 4, 16, 16, 200, 1288, KH=1, res=True, gn=True, rows=True, ln=True),
    case("g1_64x64_deep_ragged_ln+res+act+gn+out_scale", "g1_64x64_deep", 1, 1, 500, 520, 1040, KH=1, act=SILU, res=True, gn=True, rows=True,
         ln=True, out_scale=0.5),
    case("g1_64x64_deep_ragged_ln+res+act+yt+out_scale", "g1_64x64_deep", 1, 1, 500, 520, 1040, KH=1, act=SILU, res=True, rows=True, ln=True,
         yt=(520, 100), out_scale=0.5),
    case("g1_128x64_deep_ragged+bias_img+gn", "g1_128x64_deep", 1, 1, 2000, 1608, 1040, KH=1, act=GELU, res=True, bias_img=True, gn=True),
    case("g1_128x64_deep_ragged+bias_img+out_f32+out_scale", "g1_128x64_deep", 1, 1, 2000, 1608, 1040, KH=1, act=GELU, res=True, bias_img=True,
         out_f32=True, out_scale=0.5),
    case("g1_128x64_deep_ragged+gn+rows+ln+out_scale", "g1_128x64_deep", 1, 1, 2000, 1608, 1040, KH=1, act=GELU, res=True, gn=True, rows=True,
         ln=True, out_scale=0.5),
    case("g1_128x64_deep_ragged+rows+ln+yt+out_scale", "g1_128x64_deep", 1, 1, 2000, 1608, 1040, KH=1, act=GELU, res=True, rows=True, ln=True,
         yt=(520, 100), out_scale=0.5),
    case("g1_128x64_deep_ragged+yt+out_f32", "g1_128x64_deep", 1, 1, 2000, 1608, 1040, KH=1, act=GELU, res=True, yt=(520, 100), out_f32=True),
    case("h160_ups_cat_rowbias_silu_gn+res+out_scale", "halo_8x32_160", 2, 32, 32, 64, 320, C2=64, ups=True, act=SILU, res=True, bias_img=True,
         gn=True, out_scale=0.5),
    case("h160_chunksplit_res_gn+act+bias_img+out_scale", "halo_8x32_160", 2, 64, 64, 256, 320, act=SILU, res=True, bias_img=True, gn=True,
         out_scale=0.5),
    case("h160_chunksplit_res_gn+act+rows+out_scale", "halo_8x32_160", 2, 64, 64, 256, 320, act=SILU, res=True, gn=True, rows=True, out_scale=0.5),
    case("h128_ups_cat_rowbias_gelu_gnab+res+out_scale", "halo_8x32_128", 2, 32, 32, 64, 256, C2=64, ups=True, act=GELU, res=True, bias_img=True,
         gn=True, gn_ab=True, out_scale=0.5),
    case("h128_chunksplit_gnab_res_gn+act+bias_img+out_scale", "halo_8x32_128", 2, 64, 64, 256, 256, act=SILU, res=True, bias_img=True, gn=True,
         gn_ab=True, out_scale=0.5),
    case("h128_chunksplit_gnab_res_gn+act+rows+out_scale", "halo_8x32_128", 2, 64, 64, 256, 256, act=SILU, res=True, gn=True, gn_ab=True, rows=True,
         out_scale=0.5),
    case("group_halo_loop+res+out_scale", "halo_8x32_128", 1, 128, 128, 128, 128, act=SILU, res=True, out_scale=0.5, groups=2),
    case("thin_c32_f32_res+act+out_scale", "halo_thin_32", 2, 64, 256, 64, 32, act=SILU, res=True, out_f32=True, out_scale=0.5, zero_rows=4),
    case("himg16_n3_cat_rowbias_silu_gn+res+gn_ab+out_scale", "himg_16x16", 3, 16, 16, 128, 256, C2=128, act=SILU, res=True, bias_img=True, gn=True,
         gn_ab=True, out_scale=0.5),
    case("himg16_n4_gelu+res+bias_img+gn_ab+out_scale", "himg_16x16", 4, 16, 16, 256, 128, act=GELU, res=True, bias_img=True, gn_ab=True,
         out_scale=0.5),
    case("himg16_n4_gelu+res+gn_ab+rows+out_scale", "himg_16x16", 4, 16, 16, 256, 128, act=GELU, res=True, gn_ab=True, rows=True, out_scale=0.5),
    case("himg16_n5_ups_gnab_gn+res+act+bias_img+out_scale", "himg_16x16", 5, 8, 8, 256, 128, ups=True, act=SILU, res=True, bias_img=True, gn=True,
         gn_ab=True, out_scale=0.5),
    case("himg16_n5_ups_gnab_gn+res+act+rows+out_scale", "himg_16x16", 5, 8, 8, 256, 128, ups=True, act=SILU, res=True, gn=True, gn_ab=True,
         rows=True, out_scale=0.5),
    case("himg16_n16_res_gn+act+bias_img+gn_ab+out_scale", "himg_16x16", 16, 16, 16, 256, 256, act=SILU, res=True, bias_img=True, gn=True,
         gn_ab=True, out_scale=0.5),
    case("himg8_n4_res_gn+act+rows+out_scale", "himg_8x8x4", 4, 8, 8, 256, 128, act=SILU, res=True, gn=True, rows=True, out_scale=0.5),
    case("himg8_n16_cat_rowbias_silu_gn+res+out_scale", "himg_8x8x4", 16, 8, 8, 128, 256, C2=128, act=SILU, res=True, bias_img=True, gn=True,
         out_scale=0.5),
    case("wstream_n3_cat_rowbias_silu+res+gn+out_scale", "wstream_8x8", 3, 8, 8, 256, 128, C2=256, act=SILU, wfrag=True, res=True, bias_img=True,
         gn=True, out_scale=0.5, launchers={"less": "v1_128x128", "none": "v1_128x128"}),
    case("wstream_n3_cat_rowbias_silu+res+out_scale", "wstream_8x8", 3, 8, 8, 256, 128, C2=256, act=SILU, wfrag=True, res=True, bias_img=True,
         out_scale=0.5, launchers={"less": "v1_128x128", "none": "v1_128x128"}),
]
