"""CPU-side check of the conv / GEMM launch planning (csrc/igemm.hip dispatch_conv and the launchers' plan steps): ur_conv2d_plan on
host-only descriptors (placeholder pointers, nothing runs), one shape per launcher.  The expected (row_stat_parts, gn_parts, gn_fused,
prologue_ok) were recorded before planning was split from launching."""
import math
import os
import re

import pytest

import conv_launcher_cases as LC
import conv_launcher_space as LS
from unirestore_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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


# launcher each CASES entry plans to, where its id is not already the launcher's name (the grouped conv: the launcher of each group's
# launch, which needs >= 64 8 x 32 patch tiles for the halo kernel - a 64 x 64 map of one image has 16)
LAUNCHER_OF = {"wstream_8x8_cpw2": "wstream_8x8", "v1_128x160_split": "v1_128x160", "grouped_halo": "v1_128x128"}


def _launcher(d):
    info = capi.ConvLaunchInfo()
    rc = capi.lib.ur_conv2d_plan_launch(d, info)
    assert rc == 0, capi.lib.ur_last_error()
    return capi.launcher_names()[info.launcher], info


@pytest.mark.parametrize("name,shape,expected", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("dtype", [capi.UR_DT_BF16, capi.UR_DT_F16])
def test_plan_per_launcher(name, shape, expected, dtype):
    for (variant, extra), want in zip(VARIANTS.items(), expected):
        assert _plan(_desc(**shape, dtype=dtype, **extra)) == want, (name, variant)
    assert _launcher(_desc(**shape, dtype=dtype))[0] == LAUNCHER_OF.get(name, name)


def test_launcher_names_match_the_list():
    names = capi.launcher_names()
    assert len(names) == capi.lib.ur_conv_launcher_count() == len(set(names)) == 23
    assert capi.lib.ur_conv_launcher_name(-1) is None and capi.lib.ur_conv_launcher_name(len(names)) is None
    src = open(os.path.join(ROOT, "unirestore_amd", "csrc", "igemm_impl.h")).read()
    body = src[src.index("#define UR_CONV_LAUNCHERS(X)"):]
    body = body[:body.index("\n#define", 1)]
    assert re.findall(r"X\((\w+)\)", body) == names


def _plan_case(c, nbytes, dtype):
    d = capi.ConvDesc()
    ptrs = dict(LC.placeholders(c), workspace=LC.P if nbytes is not None else None)
    LC.fill(d, c, ptrs, nbytes)
    d.dtype = dtype
    return _launcher(d)


@pytest.mark.parametrize("dtype", [capi.UR_DT_BF16, capi.UR_DT_F16])
def test_launcher_matrix_covers_every_launcher_and_path(dtype):
    """The GPU parity matrix (tests/conv_launcher_cases.py) on the host: every case plans to the launcher it names at each of its
    workspace sizes, the cases reach every launcher of UR_CONV_LAUNCHERS, and every split / reduce / statistics path occurs."""
    names = capi.launcher_names()
    hit, paths, moved = set(), set(), []
    for c in LC.CASES:
        _, full = _plan_case(c, LC.WS_FULL, dtype)
        for label, nbytes in LC.ws_variants(c, full.splitk):
            name, info = _plan_case(c, nbytes, dtype)
            if name != LC.expected_launcher(c, label):
                moved.append(f"{c['id']} [{label}]: {name}, expected {LC.expected_launcher(c, label)}")
            hit.add(name)
            if info.splitk > 1:
                paths.add(("reduce", info.reduce, info.reduce_ri))
            if info.gn_pass:
                paths.add("gn_pass")
            if info.group_loop:
                paths.add("group_loop")
            if label == "less" and 1 < info.splitk < full.splitk:
                paths.add("workspace-limited split")
            if label == "none":
                assert info.splitk == 1, c["id"]
    missing = sorted(set(names) - hit)
    assert not missing and not moved, f"launchers no case reaches: {missing}; dispatch moved cases:\n" + "\n".join(moved)
    assert hit == set(names)
    want = {("reduce", 0, 0), ("reduce", 1, 0), ("reduce", 2, 4), ("reduce", 2, 2), ("reduce", 2, 1), "gn_pass", "group_loop",
            "workspace-limited split"}
    assert want <= paths, f"paths no case reaches: {want - paths}"


# (path, feature pair) combinations the plan accepts and no case runs: combo id (conv_launcher_space.combo_id) -> reason.  The only
# reasons allowed: the plan accepts the combination only at a shape too large for a few-second test, or the combination has been
# turned into a refusal.  At most 5 % of the reachable pairs, no single feature; an entry that is covered or no longer reachable fails.
EXEMPT = {
}
EXEMPT_CAP = 0.05


def _gate(dtype, pairs):
    reach = {i for i in LS.reachable(capi, dtype) if LS.is_pair_id(i) == pairs}
    cov = LS.covered(capi, dtype) & reach
    what = "pairs" if pairs else "singles"
    print(f"\nconv launcher space [{'fp16' if dtype == capi.UR_DT_F16 else 'bf16'}]: {len(reach)} reachable (path, feature"
          f"{' pair' if pairs else ''}) combinations, {len(cov)} covered")
    exempt = {i for i in EXEMPT if LS.is_pair_id(i) == pairs}
    stale = sorted(i for i in exempt if i in cov or i not in reach)
    assert not stale, f"exemptions that are covered or no longer reachable: {stale}"
    missing = sorted(reach - cov - exempt)
    assert not missing, f"{len(missing)} reachable {what} no case of conv_launcher_cases.CASES runs:\n" + "\n".join(missing)
    return reach, exempt


@pytest.mark.parametrize("dtype", [capi.UR_DT_BF16, capi.UR_DT_F16])
def test_launcher_matrix_covers_every_reachable_feature(dtype):
    """Every (path, feature) the plan accepts on a base case's launcher (tests/conv_launcher_space.py) has a case.  No exemptions."""
    assert not [i for i in EXEMPT if not LS.is_pair_id(i)], "single features cannot be exempted"
    _gate(dtype, pairs=False)


@pytest.mark.parametrize("dtype", [capi.UR_DT_BF16, capi.UR_DT_F16])
def test_launcher_matrix_covers_every_reachable_feature_pair(dtype):
    """Every (path, feature pair) the plan accepts on a base case's launcher has a case, but for the listed exemptions."""
    reach, exempt = _gate(dtype, pairs=True)
    assert len(exempt) <= EXEMPT_CAP * len(reach), f"{len(exempt)} exemptions for {len(reach)} reachable pairs: above 5 %"


def test_launcher_space_is_fixed():
    """The bases are the 61 cases the space was defined on, all still in the table; the enumeration is deterministic."""
    ids = [c["id"] for c in LC.CASES]
    assert len(ids) == len(set(ids)) and set(LS.BASES) <= set(ids)
    assert len(LS.TOGGLES) == 10
    # a "<base>+<features>" id says what the case is: exactly its base with those toggles applied, nothing more and nothing less
    by_id = {c["id"]: c for c in LC.CASES}
    for c in LC.CASES:
        base, *added = c["id"].split("+")
        if added:
            v = by_id[base]
            for f in added:
                v = LS.TOGGLES[f](v)
                assert v is not None, (c["id"], f)
            skip = ("id", "launcher", "launchers")
            assert {k: x for k, x in v.items() if k not in skip} == {k: x for k, x in c.items() if k not in skip}, c["id"]
    assert LS.reachable(capi, capi.UR_DT_BF16) == LS.reachable(capi, capi.UR_DT_BF16)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_comparator_rejects_subtle_errors(dt):
    """The per-element bound of tests/conv_reference.py accepts the fp64 reference after 16-bit rounding and rejects a ragged tile
    corner set to 0, one 64-channel K chunk of one tap missing from one pixel, a halo tile edge read one column off, a NaN in a plane."""
    import torch
    import conv_reference as R
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dt]
    g = torch.Generator().manual_seed(3)
    N, H, W, C, Cout = 1, 8, 64, 128, 40                       # two 8 x 32 patches, two 64-channel chunks, a ragged 40-wide N
    x = torch.randn(N, H, W, C, generator=g).to(tdt).double()
    w = (torch.randn(Cout, 3, 3, C, generator=g) / math.sqrt(9 * C)).to(tdt).double()
    K = 9 * C
    acc = R.conv_nhwc(x, w, 1, (1, 1))
    A = R.conv_nhwc(x.abs(), w.abs(), 1, (1, 1))
    ref, Ao, eps = R.epilogue(acc, A)
    bnd = R.bound(ref, Ao, eps, K, tdt)
    y = ref.to(tdt).double()
    assert R.compare(y, ref, bnd) < 1.0
    bad = y.clone()                                            # (a) last ragged tile: largest element of columns 32..39 of the last rows
    blk = ref[-32:, 32:].abs()
    i = int(blk.argmax())
    bad[ref.shape[0] - 32 + i // 8, 32 + i % 8] = 0
    with pytest.raises(AssertionError):
        R.compare(bad, ref, bnd)
    pix = 3 * W + 17                                           # (b) one pixel without chunk 1 of tap (1, 1) (the centre tap)
    part = x[0, 3, 17, 64:] @ w[:, 1, 1, 64:].t()
    bad = y.clone()
    bad[pix] = (ref[pix] - part).to(tdt).double()
    with pytest.raises(AssertionError):
        R.compare(bad, ref, bnd)
    xs = x.clone()                                             # (c) the pixel at a patch edge (ow = 31) reads its input one column off
    xs[:, :, 1:] = x[:, :, :-1]
    shifted = R.conv_nhwc(xs, w, 1, (1, 1))
    bad = y.clone()
    bad[5 * W + 31] = shifted[5 * W + 31].to(tdt).double()
    with pytest.raises(AssertionError):
        R.compare(bad, ref, bnd)
    yy = y.view(N, H * W, Cout).permute(0, 2, 1)               # (d) GroupNorm plane sums: exact sums pass, one NaN does not
    s, q = yy.sum(-1), (yy * yy).sum(-1)
    assert R.compare_sums(s, q, yy, H * W) < 1.0
    s[0, 7] = float("nan")
    with pytest.raises(AssertionError):
        R.compare_sums(s, q, yy, H * W)


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
    # GroupNorm statistics run on vectors of 8 channels: 4 output channels divided by zero while planning the extra pass (the
    # process died), 12 / 20 would have left the last four channels' sums unwritten.  Refused, whichever source writes the sums.
    for cout in (4, 12, 20):
        d = _desc(N=2, H=64, W=256, cin=64, cout=cout, kh=3, kcm=1, residual=P, ldr=cout + 8, gn_part=P)
        for rc in (capi.lib.ur_conv2d_plan(d, capi.ConvPlan()), capi.lib.ur_conv2d_plan_launch(d, capi.ConvLaunchInfo()),
                   capi.lib.ur_conv2d_nhwc(d, None)):
            assert rc == capi.UR_E_INVALID, cout
            assert "gn_part needs output channels % 8 == 0" in capi.lib.ur_last_error().decode()
    d = _desc(N=2, H=64, W=256, cin=64, cout=8, kh=3, kcm=1, residual=P, ldr=16, gn_part=P)
    assert _plan(d)[1] > 0
    def refused(d, code, words):
        for rc in (capi.lib.ur_conv2d_plan(d, capi.ConvPlan()), capi.lib.ur_conv2d_plan_launch(d, capi.ConvLaunchInfo()),
                   capi.lib.ur_conv2d_nhwc(d, None)):
            assert rc == code, words
            assert words in capi.lib.ur_last_error().decode()

    def accepted(d):
        assert capi.lib.ur_conv2d_plan(d, capi.ConvPlan()) == 0, capi.lib.ur_last_error()
        info = capi.ConvLaunchInfo()
        assert capi.lib.ur_conv2d_plan_launch(d, info) == 0, capi.lib.ur_last_error()
        return info

    # per-image bias rows with row sums: 2 x 16 x 17 outputs in 128-row tiles straddle images, take the unstaged epilogue, and that one
    # writes no row sums (the row_stats plane would stay as it was).  Either feature alone is accepted.
    asym = dict(N=2, H=33, W=33, cin=64, cout=128, kh=3, stride=2, pad_t=0, pad_l=1, OH=16, OW=17, bias=P)
    refused(_desc(**asym, bias_img_stride=128, row_stats=P), capi.UR_E_INVALID, "per-image bias rows do not combine with row_stats")
    accepted(_desc(**asym, bias_img_stride=128))
    accepted(_desc(**asym, row_stats=P))
    # transposed columns of a batched launch: yt has no batch stride, every batch would write the same block
    bmm = dict(N=1, H=1, W=200, cin=1024, cout=96, kh=1)
    yt = dict(yt=P, n_split=48, t_rows=100, t_ld=108)
    refused(_desc(**bmm, nbatch=2, **yt), capi.UR_E_INVALID, "transposed columns (yt) need nbatch == 1")
    accepted(_desc(**bmm, **yt))
    # GroupNorm sums of a batched launch that cannot fuse them (200 rows: no whole tile per image): the extra pass reads one dense
    # [M][nbatch * Cout] tensor, which a batch-major y (bs_y = M * Cout) is not at any ldy; batches side by side (bs_y == Cout) are
    # accepted, planned onto the extra pass, and launched only with a dense ldy - refused before anything runs otherwise
    refused(_desc(**bmm, nbatch=2, gn_part=P, bs_y=200 * 96, ldy=96), capi.UR_E_UNSUPPORTED,
            "gn_part of a batched launch that cannot fuse the statistics needs bs_y == output channels per batch")
    side = _desc(**bmm, nbatch=2, gn_part=P)
    assert (side.bs_y, side.ldy) == (96, 192) and accepted(side).gn_pass == 1 and _plan(side)[2] == 0
    side.ldy = 200
    assert accepted(side).gn_pass == 1
    assert capi.lib.ur_conv2d_nhwc(side, None) == capi.UR_E_INVALID
    assert "gn_part fallback needs a dense output (ldy == channels)" in capi.lib.ur_last_error().decode()
    # what the launch refuses, the launch plan refuses with the same words
    d = _desc(N=1, H=1, W=4096, cin=320, cout=1280, kh=1, gn_ab=P)
    assert capi.lib.ur_conv2d_plan_launch(d, capi.ConvLaunchInfo()) == capi.UR_E_UNSUPPORTED
    assert "gn_ab is not supported by this launch" in capi.lib.ur_last_error().decode()
    d = _desc(N=1, H=1, W=4096, cin=320, cout=1280, kh=1, row_stats=P, out_f32=1)     # row sums are taken from the staged 16-bit tile
    assert capi.lib.ur_conv2d_plan_launch(d, capi.ConvLaunchInfo()) == capi.UR_E_INVALID
    assert "row_stats / ln fusion need a bf16 staged output" in capi.lib.ur_last_error().decode()
    assert capi.lib.ur_conv2d_nhwc(d, None) == capi.UR_E_INVALID
