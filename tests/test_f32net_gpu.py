"""The fp32 NHWC layers on the GPU (unirestore_amd/f32net.py, csrc/f32_layers.hip): every launcher that LPIPS, the classifier and
the segmenters share, against the fp64 restatement element by element.  The cases, restatements and bounds are those of the three
networks (lpips_reference.py, classify_reference.py, segment_reference.py: 8 x fp32's own measured error, kept honest by the
test_*_cpu.py::test_tolerances_follow_the_measured_fp32_error tests); the max-pools and the sum are compared for equality."""
import math

import pytest
import torch
import torch.nn.functional as F

import classify_reference as CR
import deeplab_reference as DR
import lpips_reference as LR
import segment_reference as SR

pytestmark = pytest.mark.gpu


# ---- the convolution ----------------------------------------------------------------------------------------------------------

# AlexNet's shapes: name -> (conv index whose measured bound applies, N, H, W, Cin, Cout, k, stride, pad, relu, zero bias)
CONV_CASES = {
    "conv1_2x31x31": (0, 2, 31, 31, 3, 64, 11, 4, 2, True, False),              # output 7 x 7, K = 363: a K tail and the scalar gather
    "conv1_1x33x47": (0, 1, 33, 47, 3, 64, 11, 4, 2, True, False),
    "conv1_2x64x64_four_blocks": (0, 2, 64, 64, 3, 64, 11, 4, 2, True, False),  # M = 450: more than one block, the last partial
    "conv2_filter_larger_than_map": (1, 2, 3, 3, 64, 192, 5, 1, 2, True, False),
    "conv2_no_relu": (1, 1, 6, 5, 64, 192, 5, 1, 2, False, False),
    "conv3_1x1_map": (2, 2, 1, 1, 192, 384, 3, 1, 1, True, False),              # eight of nine taps are padding
    "conv3_zero_bias": (2, 1, 5, 4, 192, 384, 3, 1, 1, True, True),
    "conv4_m105": (3, 3, 7, 5, 384, 256, 3, 1, 1, True, False),                 # M = 105 is no tile multiple; K = 3456
    "conv5_two_blocks": (4, 2, 9, 8, 256, 256, 3, 1, 1, True, False),           # M = 144
}


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv2d_f32_matches_fp64_elementwise(name):
    from unirestore_amd import f32net
    idx, n, h, w_, cin, cout, k, stride, pad, relu, zero_bias = CONV_CASES[name]
    g = torch.Generator().manual_seed(len(name) + 17 * idx)
    x = torch.randn(n, cin, h, w_, generator=g)
    if cin != 3:
        x = F.relu(x)                                        # what the later convs see
    wt = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
    b = torch.zeros(cout) if zero_bias else 0.1 * torch.randn(cout, generator=g)
    pc = f32net.PackedConvF32(wt, b, stride, pad, "cuda")
    y = f32net.conv2d_f32(LR.nhwc(x).cuda(), pc, relu=relu)
    want = LR.conv(x, wt, b, stride, pad, relu)
    assert tuple(y.shape) == (n, want.shape[2], want.shape[3], cout)
    ratio = float(((LR.nchw(y.cpu()).double() - want).abs() / LR.conv_abs(x, wt, b, stride, pad)).max())
    print(f"{name}: max |err| / sum|ab| {ratio:.2e} (bound {LR.CONV_TOL[idx]:.2e})")
    assert ratio <= LR.CONV_TOL[idx]
    if relu:
        assert float(y.min()) >= 0.0
    else:
        assert float(y.min()) < 0.0


@pytest.mark.parametrize("name", sorted(CR.CONV_CASES))
def test_conv2d_f32_with_residual_matches_fp64_elementwise(name):
    """The ResNets' shapes, with and without the residual input."""
    from unirestore_amd import f32net
    _n, _h, _w, _cin, cout, _k, stride, pad, has_res, relu = CR.CONV_CASES[name]
    x, wt, b, res = CR.conv_case(name)
    pc = f32net.PackedConvF32(wt, b, stride, pad, "cuda")
    y = f32net.conv2d_f32(CR.nhwc(x).cuda(), pc, None if res is None else CR.nhwc(res).cuda(), relu=relu)
    want = CR.conv(x, wt, b, stride, pad, res, relu)
    assert tuple(y.shape) == (want.shape[0], want.shape[2], want.shape[3], cout) and (res is not None) == has_res
    ratio = float(((CR.nchw(y.cpu()).double() - want).abs() / CR.conv_abs(x, wt, b, stride, pad, res)).max())
    print(f"{name}: max |err| / (sum|ab| + |bias| + |res|) {ratio:.2e} (bound {CR.CONV_TOL[name]:.2e})")
    assert ratio <= CR.CONV_TOL[name]
    assert (float(y.min()) >= 0.0) if relu else (float(y.min()) < 0.0)


def test_null_residual_is_conv2d_f32_bit_for_bit():
    """At the C entry points: ur_conv2d_f32 gives the bits of ur_conv2d_f32_res with a null residual."""
    from unirestore_amd import capi, f32net
    for name in ("1x1_64_256_res_relu", "7x7_s2_3_64", "fc_2048_1000"):
        _n, _h, _w, _cin, _cout, _k, stride, pad, _r, relu = CR.CONV_CASES[name]
        x, wt, b, _res = CR.conv_case(name)
        pc = f32net.PackedConvF32(wt, b, stride, pad, "cuda")
        xg = CR.nhwc(x).cuda()
        n, h, w_, cin = xg.shape
        geometry = (n, h, w_, cin, pc.cout, pc.kh, pc.kw, stride, pad, int(relu), f32net.stream())
        plain = torch.empty(n, (h + 2 * pad - pc.kh) // stride + 1, (w_ + 2 * pad - pc.kw) // stride + 1, pc.cout, device="cuda")
        with_null = torch.empty_like(plain)
        capi.check(capi.lib.ur_conv2d_f32(xg.data_ptr(), pc.w.data_ptr(), pc.bias.data_ptr(), plain.data_ptr(), *geometry))
        capi.check(capi.lib.ur_conv2d_f32_res(xg.data_ptr(), pc.w.data_ptr(), pc.bias.data_ptr(), None, with_null.data_ptr(), *geometry))
        assert torch.equal(plain, with_null) and torch.equal(plain, f32net.conv2d_f32(xg, pc, relu=relu))
    with pytest.raises(ValueError):
        f32net.conv2d_f32(xg, pc, torch.zeros(1, 1, 1, 3, device="cuda"))      # a residual of the wrong shape


# ---- the pools ----------------------------------------------------------------------------------------------------------------

POOL_CASES = {"7x7_to_3x3": (2, 64, 7, 7), "8x9_to_3x4_floor_drops_a_row": (1, 192, 8, 9), "3x3_to_1x1_negative": (2, 5, 3, 3)}


@pytest.mark.parametrize("name", sorted(POOL_CASES))
def test_maxpool2d_f32_is_exact(name):
    from unirestore_amd import f32net
    n, c, h, w_ = POOL_CASES[name]
    x = torch.randn(n, c, h, w_, generator=torch.Generator().manual_seed(len(name)))
    if "negative" in name:
        x = -x.abs() - 0.5                                   # the maximum is not 0: a kernel that starts from 0 fails
    y = f32net.maxpool2d_f32(LR.nhwc(x).cuda()).cpu()
    want = LR.pool(x)
    assert tuple(y.shape) == (n, want.shape[2], want.shape[3], c)
    assert torch.equal(LR.nchw(y), want)


PAD_POOL_CASES = {"17x24_to_9x12": (2, 64, 17, 24), "8x8_to_4x4": (1, 128, 8, 8), "1x1": (2, 5, 1, 1), "16x16_all_negative": (1, 64, 16, 16)}


@pytest.mark.parametrize("name", sorted(PAD_POOL_CASES))
def test_maxpool2d_pad_f32_is_exact(name):
    from unirestore_amd import f32net
    n, c, h, w_ = PAD_POOL_CASES[name]
    x = torch.randn(n, c, h, w_, generator=torch.Generator().manual_seed(len(name)))
    if "negative" in name:
        x = -x.abs() - 0.5                                   # padding with 0 instead of -inf would win at every border
    y = f32net.maxpool2d_pad_f32(CR.nhwc(x).cuda()).cpu()
    want = CR.maxpool(x)
    assert tuple(y.shape) == (n, want.shape[2], want.shape[3], c)
    assert torch.equal(CR.nchw(y), want)
    if "negative" in name:
        assert float(y.max()) < 0


POOL5_CASES = {"1x1": (2, 5, 1, 1), "2x3_window_larger_than_the_map": (1, 8, 2, 3), "7x9": (2, 19, 7, 9), "7x9_c256": (1, 256, 7, 9),
               "6x6_all_negative": (1, 64, 6, 6)}


@pytest.mark.parametrize("name", sorted(POOL5_CASES))
def test_maxpool5_is_exact(name):
    from unirestore_amd import f32net
    n, c, h, w_ = POOL5_CASES[name]
    x = torch.randn(n, c, h, w_, generator=torch.Generator().manual_seed(len(name)))
    if "negative" in name:
        x = -x.abs() - 0.5                                   # padding with 0 instead of -inf would win at every border
    y = f32net.maxpool5_f32(SR.nhwc(x).cuda()).cpu()
    assert torch.equal(SR.nchw(y), SR.maxpool5(x))
    if "negative" in name:
        assert float(y.max()) < 0


@pytest.mark.parametrize("shape", CR.AVGPOOL_CASES, ids=["x".join(map(str, s)) for s in CR.AVGPOOL_CASES])
def test_avgpool_f32_matches_fp64(shape):
    from unirestore_amd import f32net
    x = CR.avgpool_case(shape)
    y = f32net.avgpool_f32(CR.nhwc(x).cuda()).cpu()
    assert tuple(y.shape) == shape[:2]
    ratio = float(((y.double() - CR.avgpool(x)).abs() / x.double().abs().mean(dim=(2, 3))).max())
    print(f"avgpool {shape}: max |err| / mean|x| {ratio:.2e} (bound {CR.AVGPOOL_TOL:.2e})")
    assert ratio <= CR.AVGPOOL_TOL


# ---- the up-sample and the sum ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SR.UPSAMPLE_CASES, ids=["x".join(map(str, c)) for c in SR.UPSAMPLE_CASES])
def test_upsample_matches_fp64(case):
    from unirestore_amd import f32net
    x = SR.upsample_case(case)
    y = f32net.upsample_bilinear_ac_f32(SR.nhwc(x).cuda(), case[4:]).cpu()
    assert tuple(y.shape) == (case[0], case[4], case[5], case[1])
    err = float((SR.nchw(y).double() - SR.resize_ac(x, case[4:])).abs().max() / x.abs().max())
    print(f"upsample {case}: max |err| / max |x| {err:.2e} (bound {SR.UPSAMPLE_TOL:.2e})")
    assert err <= SR.UPSAMPLE_TOL


@pytest.mark.parametrize("c", [19, 256])
def test_upsample_to_the_same_size_is_the_identity(c):
    from unirestore_amd import f32net
    x = torch.randn(2, 5, 7, c, generator=torch.Generator().manual_seed(c)).cuda()
    assert torch.equal(f32net.upsample_bilinear_ac_f32(x, (5, 7)), x)


# One table-driven resize kernel behind two entry points: (N, C, h, w, H, W) of the two networks' UPSAMPLE_CASES, the channel
# count of the buffer the slice is written into and the slice's first channel.
SLICE_CASES = {
    "float4": ((2, 48, 4, 5, 16, 20), 100, 48),
    "scalar_c19": ((1, 19, 3, 4, 12, 16), 71, 48),
    "scalar_c48_in_51_channels": ((1, 48, 3, 4, 12, 16), 51, 3),     # C % 4 == 0 but ldy % 4 != 0: float4 stores would be misaligned
}
SENTINEL = -12345.0


@pytest.mark.parametrize("table", ["align_corners", "half_pixel"])
@pytest.mark.parametrize("name", sorted(SLICE_CASES))
def test_upsample_into_a_slice_is_the_dense_result_bit_for_bit(name, table):
    """Dense (ldy = C: ur_upsample_bilinear_ac_f32 for the align_corners table, ur_dlv3_upsample_f32 for the half-pixel one) and
    into a channel slice of a wider buffer (ur_dlv3_upsample_f32, either table): the same bits, and no other channel is touched."""
    from unirestore_amd import capi, f32net
    case, channels, off = SLICE_CASES[name]
    assert case in DR.UPSAMPLE_CASES
    n, c, h, w_, H, W = case
    x = DR.nhwc(DR.upsample_case(case)).cuda()
    if table == "align_corners":
        dense = f32net.upsample_bilinear_ac_f32(x, (H, W))
        tabs = f32net._device_tables((h,), H, x.device.index), f32net._device_tables((w_,), W, x.device.index)
        want, tol = SR.resize_ac(DR.nchw(x.cpu()), (H, W)), SR.UPSAMPLE_TOL
    else:
        dense = f32net.upsample_bilinear_hp_f32(x, (H, W))
        tabs = f32net._device_tables_hp(((h, H),), x.device.index), f32net._device_tables_hp(((w_, W),), x.device.index)
        want, tol = DR.resize_hp(DR.nchw(x.cpu()), (H, W)), DR.UPSAMPLE_TOL
    assert tuple(dense.shape) == (n, H, W, c)
    err = float((DR.nchw(dense.cpu()).double() - want).abs().max() / x.abs().max())
    print(f"{name} {table}: dense max |err| / max |x| {err:.2e} (bound {tol:.2e})")
    assert err <= tol                                                # (not vacuous: the dense result is the resize)
    buf = torch.full((n, H, W, channels), SENTINEL, device="cuda")
    assert f32net._upsample_bilinear("test", x, (H, W), *tabs, (buf, off), capi.lib.ur_dlv3_upsample_f32) is buf
    assert torch.equal(buf[..., off:off + c], dense)
    rest = torch.cat([buf[..., :off], buf[..., off + c:]], dim=3)
    assert rest.numel() == n * H * W * (channels - c) and bool((rest == SENTINEL).all())


def test_both_preps_reach_one_resize():
    """segment.prep and deeplab.prep are one kernel with two per-channel functors.  The stage in front of the functors is the
    align_corners=True resize of the image, which `upsample_bilinear_ac_f32` computes from the same tables with the same `bilerp`:
    each prep result is that resized image put through its network's arithmetic in fp32, bit for bit; and inverting each
    functor in fp64 on the host recovers it within the side's own PREP_TOL carried to the image (/ 255, x std).  (The inverse
    cannot be exact: both functors round twice.)  The per-network prep tests stay the authority on the values."""
    from unirestore_amd import deeplab, f32net, segment
    shape, s = (2, 3, 64, 96), 0.8
    assert (shape, s) in SR.PREP_CASES and (shape, s) in DR.PREP_CASES
    x = SR.images(shape, sum(shape))
    size = (segment.scaled_size(shape[2], s), segment.scaled_size(shape[3], s))
    resized = f32net.upsample_bilinear_ac_f32(SR.nhwc(x).cuda(), size).cpu()                  # NHWC, R, G, B
    seg, dl = segment.prep(x.cuda(), size).cpu(), deeplab.prep(x.cuda(), size).cpu()
    assert tuple(resized.shape) == tuple(seg.shape) == tuple(dl.shape) == (shape[0], *size, 3)
    mean255, mean, std = (torch.tensor(v, dtype=torch.float32) for v in (SR.MEAN, DR.MEAN, DR.STD))
    assert torch.equal(seg, (resized * 255.0 - mean255).flip(3))
    assert torch.equal(dl, (resized - mean) / std)
    from_seg = (seg.double().flip(3) + mean255.double()) / 255.0
    from_dl = dl.double() * std.double() + mean.double()
    for what, d in (("segment", (from_seg - resized.double()).abs()), ("deeplab", (from_dl - resized.double()).abs()),
                    ("segment vs deeplab", (from_seg - from_dl).abs())):
        e_seg, e_dl = float(d.max()) * 255.0, float((d / std.double()).max())
        print(f"{what}: recovered image off by {float(d.max()):.2e}; as segment's output {e_seg:.2e} (bound {SR.PREP_TOL:.2e}), "
              f"as deeplab's {e_dl:.2e} (bound {DR.PREP_TOL:.2e})")
        assert e_seg <= SR.PREP_TOL and e_dl <= DR.PREP_TOL


def test_add_f32_is_exact():
    from unirestore_amd import f32net
    for shape in ((1, 3, 5, 19), (2, 4, 4, 256)):
        a, b = (torch.randn(shape, generator=torch.Generator().manual_seed(i)) for i in (1, 2))
        assert torch.equal(f32net.add_f32(a.cuda(), b.cuda()).cpu(), a + b)
