"""CPU-side checks of the nearest-2x upsample + 3x3 conv fold (ops.up4_fold / up4_pack / wants_up4; csrc/igemm.hip dispatch_conv):
the four 2x2 phase convs are the upsampled 3x3 conv, the packed layout round-trips, and Python and the plan agree on eligibility."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from unirestore_amd import capi, ops

P = 16          # any non-null pointer: the plan reads no data


def _phase_convs(x, w4):
    """x [N,C,H,W], w4 [2][2][Cout][2][2][Cin] (ops.up4_fold) -> [N,Cout,2H,2W]: phase (py, px) is a 2x2 conv over the rows
    (y - 1 + py, y + py) and columns (x - 1 + px, x + px) of the zero-padded low-resolution image, written to (2y + py, 2x + px)."""
    n, c, h, w_ = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros(n, w4.shape[2], 2 * h, 2 * w_)
    for py, px in itertools.product((0, 1), (0, 1)):
        k = w4[py, px].permute(0, 3, 1, 2)                                   # [Cout][Cin][2][2]
        out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + h + 1, px:px + w_ + 1], k)
    return out


@pytest.mark.parametrize("shape", [(1, 3, 5, 1, 1), (2, 5, 4, 2, 3), (1, 8, 6, 5, 7), (2, 4, 3, 8, 32)])
def test_fold_equals_upsampled_conv_fp64(shape):
    n, cin, cout, h, w_ = shape
    g = torch.Generator().manual_seed(1000 * h + w_)
    x = torch.randn(n, cin, h, w_, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    got = _phase_convs(x, ops.up4_fold(w.permute(0, 2, 3, 1)))
    err = (got - ref).abs()
    assert float(err.max()) <= 1e-12 * float(ref.abs().max())
    for sl in (err[:, :, 0], err[:, :, -1], err[:, :, :, 0], err[:, :, :, -1]):          # the four borders (corners included)
        assert float(sl.max()) <= 1e-12 * float(ref.abs().max())
    for cy, cx in itertools.product((0, -1), (0, -1)):
        assert float(err[:, :, cy, cx].max()) <= 1e-12 * float(ref[:, :, cy, cx].abs().max())


def test_fold_row_rule():
    """py = 0: {ky 0} -> a 0, {ky 1, 2} -> a 1; py = 1: {ky 0, 1} -> a 0, {ky 2} -> a 1; the columns likewise."""
    w = torch.zeros(1, 3, 3, 1, dtype=torch.float64)
    for ky, kx in itertools.product(range(3), range(3)):
        w[0, ky, kx, 0] = 10.0 ** ky + 1000.0 * 10.0 ** kx
    w4 = ops.up4_fold(w)[:, :, 0, :, :, 0]
    rows = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    for py, px, a, b in itertools.product((0, 1), repeat=4):
        want = sum(float(w[0, ky, kx, 0]) for ky in rows[py][a] for kx in rows[px][b])
        assert float(w4[py, px, a, b]) == want


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cout,cin", [(8, 64), (32, 192), (160, 128)])
def test_pack_round_trips(dt, cout, cin):
    g = torch.Generator().manual_seed(cout + cin)
    w4 = ops.up4_fold(torch.randn(cout, 3, 3, cin, generator=g))
    packed = ops.up4_pack(w4, dt)
    assert packed.dtype == dt and tuple(packed.shape) == (4, cout, 4 * cin) and packed.is_contiguous()
    assert torch.equal(ops.up4_unpack(packed, cin), w4.to(dt))
    # K tile (chunk * 4 + tap) of phase (py, px), row co = the 64 channels of `chunk` at tap (a, b) = (tap / 2, tap % 2)
    py, px, co, chunk, tap = 1, 0, cout - 1, cin // 64 - 1, 2
    kt = chunk * 4 + tap
    assert torch.equal(packed[py * 2 + px, co, kt * 64:(kt + 1) * 64], w4[py, px, co, tap // 2, tap % 2, chunk * 64:(chunk + 1) * 64].to(dt))


def _desc(n, h, w_, cin, cout, *, c2=0, stride=1, ups=True, kcm=1, up4=True, pad=1, dtype=capi.UR_DT_BF16):
    d = capi.ConvDesc()
    d.x, d.w, d.y = P, P, P
    d.x2 = P if c2 else None
    d.workspace, d.workspace_bytes = P, 192 << 20
    d.N, d.H, d.W = n, h, w_
    d.C1, d.ldx, d.C2, d.ldx2 = cin, cin, c2, c2
    d.Cout, d.ldw, d.ldy = cout, 9 * (cin + c2), cout
    d.KH = d.KW = 3
    d.stride, d.pad_t, d.pad_l = stride, pad, pad
    hin, win = (2 * h, 2 * w_) if ups else (h, w_)
    d.OH, d.OW = (hin + 2 * pad - 3) // stride + 1, (win + 2 * pad - 3) // stride + 1
    d.upsample2x, d.out_scale, d.nbatch, d.k_chunk_major, d.dtype = int(ups), 1.0, 1, kcm, dtype
    d.w_up4 = P if up4 else None
    return d


def _plan(d):
    p, info = capi.ConvPlan(), capi.ConvLaunchInfo()
    assert capi.lib.ur_conv2d_plan(d, p) == 0, capi.lib.ur_last_error()
    assert capi.lib.ur_conv2d_plan_launch(d, info) == 0, capi.lib.ur_last_error()
    return p, capi.launcher_names()[info.launcher], info


GRID = [dict(n=n, h=h, w_=w_, cin=cin, cout=cout, c2=c2, stride=stride, ups=ups)
        for n in (1, 3) for (h, w_) in ((8, 32), (16, 64), (32, 32), (8, 8), (16, 16), (12, 32), (8, 48), (256, 256))
        for (cin, c2) in ((64, 0), (192, 0), (96, 0), (64, 64)) for cout in (32, 160, 256, 320, 640)
        for (stride, ups) in ((1, True), (1, False), (2, False))]


@pytest.mark.parametrize("dtype", [capi.UR_DT_BF16, capi.UR_DT_F16])
def test_wants_up4_agrees_with_the_plan(dtype):
    folded = 0
    for s in GRID:
        kcm = int((s["cin"] + s["c2"]) % 64 == 0 and s["cin"] % 64 == 0)
        pc = ops.PackedConv(w=None, bias=None, cin=s["cin"] + s["c2"], cout=s["cout"], cout_out=s["cout"], k=3, kcm=bool(kcm))
        want = ops.wants_up4(pc, s["n"], s["h"], s["w_"], s["cin"], s["c2"], s["stride"], s["ups"], 1, (1, 1))
        p, name, info = _plan(_desc(**s, kcm=kcm, dtype=dtype))
        assert bool(p.up4) == want, s
        if p.up4:
            folded += 1
            # 160-wide tiles only where they divide Cout (both widths do at 640: the fuller grid wins); any other width runs
            # ragged on the 128-wide tile
            ok = {"halo_8x32_128"} if s["cout"] % 160 else {"halo_8x32_160"} if s["cout"] % 128 else {"halo_8x32_160", "halo_8x32_128"}
            assert name in ok, (s, name)
            assert info.splitk == 1 and info.nk_per_split == 4 * s["cin"] // 64
        # w_up4 changes a plan only by folding it: NULL never folds, and where the plan does not fold, the launcher, its split and the
        # GroupNorm plan are those of the descriptor without w_up4
        p0, name0, info0 = _plan(_desc(**s, kcm=kcm, up4=False, dtype=dtype))
        assert not p0.up4
        if not p.up4:
            assert (name, info.splitk, info.nk_per_split, info.reduce, info.reduce_ri, info.gn_pass, info.group_loop) == \
                   (name0, info0.splitk, info0.nk_per_split, info0.reduce, info0.reduce_ri, info0.gn_pass, info0.group_loop), s
            assert (p.row_stat_parts, p.gn_parts, p.gn_fused, p.prologue_ok) == (p0.row_stat_parts, p0.gn_parts, p0.gn_fused, p0.prologue_ok), s
    assert folded >= 40


def test_plan_refuses_the_fold_where_the_epilogue_cannot_follow():
    """The folded launch writes through a strided view of y: the features that index rows of other planes stay on the old path."""
    base = dict(n=1, h=16, w_=64, cin=64, cout=160)
    assert _plan(_desc(**base))[0].up4 == 1
    for extra in (dict(gn_ab=P), dict(row_stats=P), dict(out_f32=1), dict(pad_t=0)):
        d = _desc(**base)
        for k, v in extra.items():
            setattr(d, k, v)
        p = capi.ConvPlan()
        assert capi.lib.ur_conv2d_plan(d, p) == 0 and p.up4 == 0, extra
    d = _desc(**base)
    d.gn_part = P
    p = _plan(d)[0]
    assert p.up4 == 1 and p.gn_fused == 1 and p.gn_parts == 4 * (16 // 8) * (64 // 32) and p.prologue_ok == 0


@pytest.mark.parametrize("dtype", [capi.UR_DT_BF16, capi.UR_DT_F16])
def test_grouped_launch_never_reads_w_up4(dtype):
    """w_up4 has no batch stride: a grouped upsampling conv (nbatch > 1) plans exactly as without it - no fold at the top level and
    none in the per-group launches of the group loop, whose single-group problems would otherwise be eligible."""
    def grouped(up4):
        d = _desc(1, 64, 64, 128, 128, up4=up4, dtype=dtype)
        d.nbatch, d.ldx, d.ldy = 4, 4 * 128, 4 * 128
        d.bs_x, d.bs_w, d.bs_bias, d.bs_y, d.bs_r = 128, 128 * d.ldw, 128, 128, 128
        return _plan(d)
    (p1, name1, info1), (p0, name0, info0) = grouped(True), grouped(False)
    assert p1.up4 == 0 and p0.up4 == 0
    assert info1.group_loop == 1 and info0.group_loop == 1
    assert (name1, info1.splitk, info1.nk_per_split, info1.reduce, info1.gn_pass) == (name0, info0.splitk, info0.nk_per_split, info0.reduce, info0.gn_pass)
    assert info1.nk_per_split % 9 == 0, "the per-group launch must be the 9-tap one"
    # the same group as a launch of its own does fold: the grouped refusal is about the batch, not the shape
    assert _plan(_desc(1, 64, 64, 128, 128, dtype=dtype))[0].up4 == 1


def test_version_bumped():
    assert capi.lib.ur_version() >= 102
