"""CPU-side check of the conv / GEMM launch planning (csrc/igemm.hip dispatch_conv and the launchers' plan steps): ur_conv2d_plan on
host-only descriptors (placeholder pointers, nothing runs), one shape per launcher.  The expected (row_stat_parts, gn_parts, gn_fused,
prologue_ok) were recorded before planning was split from launching."""
import pytest

from unirestore_amd import capi

MiB = 1 << 20
P = 16          # any non-null pointer: the plan reads no data
GEGLU = capi.UR_ACT_GEGLU


def _desc(N, H, W, cin, cout, kh, *, c2=0, kcm=0, wfrag=False, act=0, nbatch=1, stride=1, ups=False, **extra):
    d = capi.ConvDesc()
    d.x, d.w, d.y = P, P, P
    d.x2 = P if c2 else None
    d.workspace, d.workspace_bytes = P, 192 * MiB      # ops.workspace's size
    d.N, d.H, d.W = N, H, W
    d.C1, d.ldx, d.C2, d.ldx2 = cin, cin * nbatch, c2, c2
    d.Cout, d.ldw = cout, kh * kh * (cin + c2)
    d.ldy = (cout // 2 if act == GEGLU else cout) * nbatch
    d.KH = d.KW = kh
    d.stride, d.pad_t, d.pad_l = stride, kh // 2, kh // 2
    d.OH, d.OW = (2 * H, 2 * W) if ups else (H // stride, W // stride)
    d.upsample2x, d.act, d.out_scale, d.nbatch = int(ups), act, 1.0, nbatch
    d.k_chunk_major = kcm
    d.w_frag = P if wfrag else None
    if nbatch > 1:
        d.bs_x, d.bs_w, d.bs_bias, d.bs_y, d.bs_r = cin, cout * d.ldw, cout, cout, cout
    for k, v in extra.items():
        setattr(d, k, v)
    return d


def _plan(d):
    p = capi.ConvPlan()
    rc = capi.lib.ur_conv2d_plan(d, p)
    assert rc == 0, capi.lib.ur_last_error()
    return p.row_stat_parts, p.gn_parts, p.gn_fused, p.prologue_ok


# (launcher, descriptor, expected plan of each variant: plain, gn_part, gn_ab + gn_part, row_stats)
CASES = [
    ("halo_8x32_160", dict(N=1, H=64, W=64, cin=640, cout=640, kh=3, kcm=1),
        ((0, 0, 0, 0), (0, 64, 1, 0), (0, 64, 1, 0), (1, 0, 0, 0))),
    ("halo_8x32_128", dict(N=2, H=64, W=64, cin=256, cout=256, kh=3, kcm=1),
        ((0, 0, 0, 1), (0, 64, 1, 1), (0, 64, 1, 1), (1, 0, 0, 1))),
    ("halo_thin_32", dict(N=8, H=64, W=64, cin=320, cout=8, kh=3, kcm=1),
        ((0, 0, 0, 0), (0, 64, 1, 0), (0, 64, 1, 0), (1, 0, 0, 0))),
    ("himg_16x16", dict(N=2, H=16, W=16, cin=1280, cout=1280, kh=3, kcm=1),
        ((0, 0, 0, 1), (0, 16, 1, 1), (0, 16, 1, 1), (1, 0, 0, 1))),
    ("himg_8x8x4", dict(N=4, H=8, W=8, cin=1280, cout=1280, kh=3, kcm=1),
        ((0, 0, 0, 0), (0, 4, 1, 0), (0, 4, 1, 0), (1, 0, 0, 0))),
    ("wstream_8x8", dict(N=4, H=8, W=8, cin=1280, cout=1280, kh=3, kcm=1, wfrag=True),
        ((0, 0, 0, 0), (0, 4, 1, 0), (0, 4, 1, 0), (1, 0, 0, 0))),
    ("wstream_8x8_cpw2", dict(N=8, H=8, W=8, cin=2560, cout=1280, kh=3, kcm=1, wfrag=True),
        ((0, 0, 0, 0), (0, 4, 1, 0), (0, 4, 1, 0), (1, 0, 0, 0))),
    ("gemm_256x256", dict(N=1, H=1, W=4096, cin=1280, cout=4096, kh=1, act=GEGLU),
        ((0, 0, 0, 0), (0, 16, 1, 0), (0, 16, 1, 0), (16, 0, 0, 0))),
    ("gemm_256x320_pair", dict(N=1, H=1, W=4096, cin=1280, cout=10240, kh=1, act=GEGLU),
        ((0, 0, 0, 0), (0, 16, 1, 0), (0, 16, 1, 0), (32, 0, 0, 0))),
    ("v1_128x128", dict(N=1, H=1, W=1024, cin=320, cout=1280, kh=1, act=GEGLU),
        ((0, 0, 0, 0), (0, 8, 1, 0), (0, 8, 1, 0), (10, 0, 0, 0))),
    ("v1_128x160", dict(N=1, H=1, W=8192, cin=160, c2=160, cout=960, kh=1),
        ((0, 0, 0, 0), (0, 64, 1, 0), (0, 64, 1, 0), (6, 0, 0, 0))),
    ("v1_128x64", dict(N=1, H=1, W=4096, cin=320, cout=64, kh=1),
        ((0, 0, 0, 0), (0, 32, 1, 0), (0, 32, 1, 0), (1, 0, 0, 0))),
    ("v1_256x32", dict(N=1, H=1, W=4096, cin=320, cout=32, kh=1),
        ((0, 0, 0, 0), (0, 16, 1, 0), (0, 16, 1, 0), (1, 0, 0, 0))),
    ("v1_64x64", dict(N=1, H=1, W=1024, cin=320, c2=320, cout=640, kh=1),
        ((0, 0, 0, 0), (0, 64, 1, 0), (0, 64, 1, 0), (1, 0, 0, 0))),
    ("g1_64x64_deep", dict(N=8, H=8, W=8, cin=1280, cout=1280, kh=1),
        ((0, 0, 0, 0), (0, 1, 1, 0), (0, 1, 1, 0), (20, 0, 0, 0))),
    ("g1_128x64_deep", dict(N=8, H=16, W=16, cin=2560, cout=1280, kh=1),
        ((0, 0, 0, 0), (0, 2, 1, 0), (0, 2, 1, 0), (20, 0, 0, 0))),
    ("g1_64x64", dict(N=2, H=32, W=32, cin=640, cout=640, kh=1),
        ((0, 0, 0, 0), (0, 16, 1, 0), (0, 16, 1, 0), (10, 0, 0, 0))),
    ("g1_128x64", dict(N=4, H=32, W=32, cin=640, cout=1280, kh=1),
        ((0, 0, 0, 0), (0, 8, 1, 0), (0, 8, 1, 0), (20, 0, 0, 0))),
    ("g1_128x160", dict(N=2, H=64, W=64, cin=320, cout=960, kh=1),
        ((0, 0, 0, 0), (0, 32, 1, 0), (0, 32, 1, 0), (6, 0, 0, 0))),
    ("g1_128x128", dict(N=2, H=64, W=64, cin=320, cout=1280, kh=1),
        ((0, 0, 0, 0), (0, 32, 1, 0), (0, 32, 1, 0), (10, 0, 0, 0))),
    ("v2_256x32", dict(N=1, H=64, W=64, cin=128, cout=32, kh=3),
        ((0, 0, 0, 0), (0, 256, 1, 0), (0, 256, 1, 0), (1, 0, 0, 0))),
    ("v2_128x64", dict(N=1, H=64, W=64, cin=128, cout=64, kh=3),
        ((0, 0, 0, 0), (0, 256, 1, 0), (0, 256, 1, 0), (1, 0, 0, 0))),
    ("v2_256x160", dict(N=4, H=128, W=128, cin=320, cout=960, kh=3),
        ((0, 0, 0, 0), (0, 64, 1, 0), (0, 64, 1, 0), (6, 0, 0, 0))),
    ("v2_256x128", dict(N=4, H=128, W=128, cin=320, cout=1280, kh=3),
        ((0, 0, 0, 0), (0, 64, 1, 0), (0, 64, 1, 0), (10, 0, 0, 0))),
    ("v1_128x160_split", dict(N=1, H=16, W=16, cin=320, cout=320, kh=3),
        ((0, 0, 0, 0), (0, 16, 1, 0), (0, 16, 1, 0), (1, 0, 0, 0))),
    ("grouped_halo", dict(N=1, H=64, W=64, cin=128, cout=128, kh=3, kcm=1, nbatch=4),
        ((0, 0, 0, 0), (0, 64, 0, 0), (0, 64, 0, 0), (1, 0, 0, 0))),
]
VARIANTS = {"plain": {}, "gn": dict(gn_part=P), "gn_ab": dict(gn_ab=P, gn_part=P), "rows": dict(row_stats=P)}


@pytest.mark.parametrize("name,shape,expected", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("dtype", [capi.UR_DT_BF16, capi.UR_DT_F16])
def test_plan_per_launcher(name, shape, expected, dtype):
    for (variant, extra), want in zip(VARIANTS.items(), expected):
        assert _plan(_desc(**shape, dtype=dtype, **extra)) == want, (name, variant)


def test_plan_refusals():
    # pair activations need 32-row a|g blocks: refused by the plan itself
    d = _desc(N=1, H=1, W=1024, cin=320, cout=96, kh=1, act=GEGLU)
    assert capi.lib.ur_conv2d_plan(d, capi.ConvPlan()) == capi.UR_E_UNSUPPORTED
    assert "pair activations (GEGLU / SimpleGate) need Cout % 64 == 0" in capi.lib.ur_last_error().decode()
    # the launch refuses what its plan rules out before it makes any HIP call (no stream, no device needed)
    d = _desc(N=1, H=1, W=4096, cin=320, cout=1280, kh=1, gn_ab=P)
    assert _plan(d)[3] == 0
    assert capi.lib.ur_conv2d_nhwc(d, None) == capi.UR_E_UNSUPPORTED
    assert capi.lib.ur_last_error().decode() == \
        "ur_conv2d_nhwc: gn_ab is not supported by this launch (see ur_conv2d_plan.prologue_ok)"
    d = _desc(N=4, H=8, W=8, cin=320, cout=320, kh=3, y=None, gn_part=P)      # 64-pixel images in 128-row tiles: no per-tile partial
    assert _plan(d)[2] == 0
    assert capi.lib.ur_conv2d_nhwc(d, None) == capi.UR_E_UNSUPPORTED
    assert capi.lib.ur_last_error().decode() == \
        "ur_conv2d_nhwc: y == NULL needs a launch whose epilogue writes gn_part (see ur_conv2d_plan)"
