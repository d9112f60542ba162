"""The folded upsampling conv (ur_conv_desc.w_up4: four 2x2 phase convs on the 8 x 32 halo kernels with NTAP = 4) against fp64,
element by element (-m gpu, bf16 and fp16).

The reference is fp64 of the SAME rounded folded weights and the same 16-bit input (four 2x2 convs over the source image, interleaved);
the bound is the one every conv launcher meets (tests/conv_reference.py) on those operands, K = 4 * Cin:

    |y - ref| <= u_out * |ref| + 4 * sqrt(K) * 2^-24 * A + abs_out

Each case asserts the planned kernel (ur_conv_plan.up4 and the launcher), prefills y - with guard rows before and after the image and
padding columns past Cout - and the GroupNorm plane with NaN, launches twice into fresh buffers and requires bit-identical results,
every output element written and within the bound, everything else untouched, and the 4 x patches GroupNorm partials summed in fp64 equal
to the sums over the stored 16-bit output.
"""
import ctypes
import itertools
import zlib

import pytest
import torch

import conv_reference as R

pytestmark = pytest.mark.gpu
GUARD = 3                       # rows of y before and after the output that must stay untouched
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}

# The smallest shapes at which each mechanism can go wrong: one 8 x 32 source tile / 2 x 2 tiles (interior seams and image borders);
# N = 1 and 3; Cin = 64 (one chunk: the weight ring wraps inside the prologue's reach) and 192 (three chunks: ring and patch double
# buffer wrap); Cout = 32 (ragged N tile), 160 and 320 (one and two N tiles of the 160-wide kernel), 128 and 256 (the 128-wide one);
# with and without bias; with gn; one with a residual (the epilogue reads it through the same strided view as y).
CASES = [
    dict(id="n1_8x32_c64_o32_bias_gn", N=1, H=8, W=32, Cin=64, Cout=32, bias=True, gn=True, res=False, pad_cols=8),
    dict(id="n3_16x64_c192_o160_gn", N=3, H=16, W=64, Cin=192, Cout=160, bias=False, gn=True, res=False, pad_cols=0),
    dict(id="n1_16x64_c64_o320_bias_gn", N=1, H=16, W=64, Cin=64, Cout=320, bias=True, gn=True, res=False, pad_cols=8),
    dict(id="n3_8x32_c192_o160_bias", N=3, H=8, W=32, Cin=192, Cout=160, bias=True, gn=False, res=False, pad_cols=0),
    dict(id="n1_16x64_c192_o32", N=1, H=16, W=64, Cin=192, Cout=32, bias=False, gn=False, res=False, pad_cols=0),
    dict(id="n3_16x64_c64_o256_bias_res_gn", N=3, H=16, W=64, Cin=64, Cout=256, bias=True, gn=True, res=True, pad_cols=8),
    dict(id="n1_8x32_c192_o128_bias", N=1, H=8, W=32, Cin=192, Cout=128, bias=True, gn=False, res=False, pad_cols=0),
]


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    return c


def _nan(n, dtype):
    return torch.full((n,), float("nan"), dtype=dtype, device="cuda")


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _phase_reference(x, w4):
    """x [N,H,W,Cin], w4 [2][2][Cout][2][2][Cin] (fp64, on the GPU) -> (acc, A) [N*2H*2W, Cout] of the four phase convs."""
    N, H, W, _ = x.shape
    Cout = w4.shape[2]
    acc = x.new_zeros(N, 2 * H, 2 * W, Cout)
    A = torch.zeros_like(acc)
    for py, px in itertools.product((0, 1), (0, 1)):
        # source rows y - 1 + py + a: a 2x2 cross-correlation with (1 - py) rows of zeros on top (conv_nhwc pads the far side itself)
        acc[:, py::2, px::2] = R.conv_nhwc(x, w4[py, px], 1, (1 - py, 1 - px), H, W).view(N, H, W, Cout)
        A[:, py::2, px::2] = R.conv_nhwc(x.abs(), w4[py, px].abs(), 1, (1 - py, 1 - px), H, W).view(N, H, W, Cout)
    return acc.view(-1, Cout), A.view(-1, Cout)


def _inputs(c, dt):
    from unirestore_amd import ops
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    N, H, W, Cin, Cout = c["N"], c["H"], c["W"], c["Cin"], c["Cout"]
    t = {"x": torch.randn(N, H, W, Cin, generator=g).to(dt)}
    w = torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5
    t["w"] = w.reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3).reshape(Cout, 9 * Cin).to(dt).contiguous()      # (chunk-major 9-tap rows)
    t["w_up4"] = ops.up4_pack(ops.up4_fold(w), dt)
    if c["bias"]:
        t["bias"] = (torch.randn(1, Cout, generator=g) * 0.5).contiguous()
    if c["res"]:
        t["residual"] = torch.randn(N * 4 * H * W, Cout, generator=g).to(dt)
    return t


def _desc(capi, c, dt, ptrs, ldy, up4=True):
    d = capi.ConvDesc()
    d.dtype = capi.UR_DT_F16 if dt == torch.float16 else capi.UR_DT_BF16
    d.x, d.w, d.bias, d.residual = ptrs["x"], ptrs["w"], ptrs.get("bias"), ptrs.get("residual")
    d.w_up4 = ptrs["w_up4"] if up4 else None
    d.y, d.gn_part = ptrs.get("y", 16), ptrs.get("gn_part", 16 if c["gn"] else None)
    d.N, d.H, d.W = c["N"], c["H"], c["W"]
    d.C1 = d.ldx = c["Cin"]
    d.Cout, d.ldw, d.ldy, d.ldr = c["Cout"], 9 * c["Cin"], ldy, (c["Cout"] if c["res"] else 0)
    d.KH = d.KW = 3
    d.stride = d.pad_t = d.pad_l = 1
    d.OH, d.OW = 2 * c["H"], 2 * c["W"]
    d.upsample2x, d.out_scale, d.nbatch, d.k_chunk_major = 1, 1.0, 1, 1
    return d


def _plan(capi, d):
    p, info = capi.ConvPlan(), capi.ConvLaunchInfo()
    capi.check(capi.lib.ur_conv2d_plan(d, p))
    capi.check(capi.lib.ur_conv2d_plan_launch(d, info))
    return p, capi.launcher_names()[info.launcher], info


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_folded_launch(capi, c, dtype):
    from unirestore_amd import ops
    dt = DTYPES[dtype]
    N, H, W, Cin, Cout = c["N"], c["H"], c["W"], c["Cin"], c["Cout"]
    M, ldy = N * 4 * H * W, Cout + c["pad_cols"]
    t = _inputs(c, dt)
    dev = {k: v.cuda() for k, v in t.items()}
    ptrs = {k: v.data_ptr() for k, v in dev.items()}
    # the plan: the folded kernel with the folded weights, the parent's launch without them, and where the source image is no whole patch
    plan, name, info = _plan(capi, _desc(capi, c, dt, ptrs, ldy))
    assert plan.up4 == 1 and name == ("halo_8x32_160" if Cout % 160 == 0 else "halo_8x32_128"), (c["id"], plan.up4, name)
    assert info.splitk == 1 and info.nk_per_split == 4 * Cin // 64
    patches = (H // 8) * (W // 32)
    if c["gn"]:
        assert plan.gn_fused == 1 and plan.gn_parts == 4 * patches
    plan0, name0, _ = _plan(capi, _desc(capi, c, dt, ptrs, ldy, up4=False))
    assert plan0.up4 == 0
    ragged = _desc(capi, dict(c, W=W + 16), dt, ptrs, ldy)
    assert _plan(capi, ragged)[0].up4 == 0, "W % 32 != 0 must stay on the 9-tap path"

    # reference: fp64 of the same rounded folded weights and the same 16-bit input
    w4 = ops.up4_unpack(t["w_up4"], Cin).double().cuda()
    acc, A = _phase_reference(dev["x"].double(), w4)
    bias = dev["bias"].double().expand(M, Cout) if c["bias"] else None
    res = dev["residual"].double() if c["res"] else None
    ref, Ao, eps = R.epilogue(acc, A, R.NONE, bias, 1.0, res, None)
    bnd = R.bound(ref, Ao, eps, 4 * Cin, dt)

    runs = []
    for _ in range(2):
        b = {"y": _nan((M + 2 * GUARD) * ldy, dt)}
        if c["gn"]:
            b["gn_part"] = torch.full((N, plan.gn_parts, Cout, 2), float("nan"), dtype=torch.float32, device="cuda")
        p = dict(ptrs, y=b["y"].data_ptr() + GUARD * ldy * 2)
        if c["gn"]:
            p["gn_part"] = b["gn_part"].data_ptr()
        d = _desc(capi, c, dt, p, ldy)
        capi.check(capi.lib.ur_conv2d_nhwc(ctypes.byref(d), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        runs.append(b)
    for k in runs[0]:
        assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), (c["id"], k, "not bit-identical between two launches")
    y = runs[0]["y"].view(M + 2 * GUARD, ldy)
    nanbits = _bits(_nan(1, dt))[0]
    assert bool((_bits(y[:GUARD]) == nanbits).all()) and bool((_bits(y[GUARD + M:]) == nanbits).all()), (c["id"], "guard rows written")
    assert bool((_bits(y[:, Cout:]) == nanbits).all()), (c["id"], "padding columns written")
    got = y[GUARD:GUARD + M, :Cout].double()
    assert not bool(torch.isnan(got).any()), (c["id"], "output pixels left unwritten")
    worst = R.compare(got, ref, bnd, f"{c['id']} [{dtype}, {name}] y")
    print(f"\n{c['id']} [{dtype}, {name}]: largest |y - ref| / bound = {worst:.3f}")
    if c["gn"]:
        gp = runs[0]["gn_part"]
        assert not bool(torch.isnan(gp).any()), (c["id"], "GroupNorm partial slots left unwritten")
        s = gp.double().sum(1)                                                  # [N][C][2] over the 4 x patches slots
        yy = got.view(N, 4 * H * W, Cout).permute(0, 2, 1)
        R.compare_sums(s[..., 0], s[..., 1], yy, 4 * H * W, f"{c['id']} [{dtype}] GroupNorm plane (P = {plan.gn_parts})")


def _unfolded_reference(x, w, bias):
    """fp64 9-tap reference of the rounded 3x3 weights w [Cout][3][3][Cin] on the upsampled x: (ref, bound) [M, Cout]."""
    N, H, W, Cin = x.shape
    xu = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    acc = R.conv_nhwc(xu, w, 1, (1, 1), 2 * H, 2 * W)
    A = R.conv_nhwc(xu.abs(), w.abs(), 1, (1, 1), 2 * H, 2 * W)
    return R.epilogue(acc, A, R.NONE, bias, 1.0, None, None)


@pytest.mark.parametrize("exact_fold", [True, False], ids=["exact_fold", "random"])
def test_module_fold_switch(capi, monkeypatch, exact_fold):
    """Upsample2D.run with and without UR_UPS_FOLD=0 on a 2 x 32 x 32 x 64 input.

    exact_fold: the weights are multiples of 1/64 with |w| <= 15/64, so every sum of up to four taps is exact in bf16 and the folded
    and the 9-tap launch share ONE fp64 reference: the two outputs must then agree within the sum of their two bounds against it.
    random: each path meets its own bound against the fp64 reference of its own rounded weights.  Those references differ by the one
    rounding of the tap sums, which no bound on the arithmetic of either launch covers; the two outputs must agree within the sum
    of their two bounds plus exactly that term, |ref_folded - ref_9tap| in fp64 (a wrong phase or tap mapping moves the folded
    output by whole products, far outside it)."""
    from unirestore_amd import ops
    from unirestore_amd.modules import nn as M
    dt = ops.act_dtype()
    g = torch.Generator().manual_seed(7 + exact_fold)
    up = M.Upsample2D(64)
    with torch.no_grad():
        if exact_fold:
            up.conv.weight.copy_(torch.randint(-15, 16, up.conv.weight.shape, generator=g).float() / 64.0)
        else:
            up.conv.weight.copy_(torch.randn(up.conv.weight.shape, generator=g) / 24.0)
        up.conv.bias.copy_(torch.randn(64, generator=g) * 0.5)
    x = torch.randn(2, 32, 32, 64, generator=g).to(dt).cuda()
    pc = up.conv.packed()
    assert ops.conv_plan(x, pc, upsample=True, gn=True, up4=True).up4 == 1
    monkeypatch.setenv("UR_UPS_FOLD", "0")
    y_u = up.run(x)
    assert pc.w_up4 is None, "the 9-tap path must not build the folded weights"
    monkeypatch.delenv("UR_UPS_FOLD")
    y_f = up.run(x)
    torch.cuda.synchronize()
    assert pc.w_up4 is not None and tuple(y_f.shape) == tuple(y_u.shape) == (2, 64, 64, 64)
    bias = pc.bias.double().expand(2 * 64 * 64, 64)
    w9 = pc.w.double().view(64, 1, 9, 64).permute(0, 2, 1, 3).reshape(64, 3, 3, 64)               # chunk-major rows -> [Cout][3][3][Cin]
    ref_u, A_u, eps_u = _unfolded_reference(x.double(), w9, bias)
    bnd_u = R.bound(ref_u, A_u, eps_u, 9 * 64, dt)
    acc, A = _phase_reference(x.double(), ops.up4_unpack(pc.w_up4, 64).double())
    ref_f, A_f, eps_f = R.epilogue(acc, A, R.NONE, bias, 1.0, None, None)
    bnd_f = R.bound(ref_f, A_f, eps_f, 4 * 64, dt)
    got_u, got_f = y_u.double().view(-1, 64), y_f.double().view(-1, 64)
    r_u = R.compare(got_u, ref_u, bnd_u, "9-tap path")
    r_f = R.compare(got_f, ref_f, bnd_f, "folded path")
    print(f"\nUpsample2D 2x32x32x64 [{dt}]: |y - ref| / bound: 9-tap {r_u:.3f}, folded {r_f:.3f}; "
          f"max |folded - 9-tap| = {float((got_f - got_u).abs().max()):.4g}")
    if exact_fold:
        assert torch.equal(ref_f, ref_u) or float((ref_f - ref_u).abs().max()) <= 1e-12 * float(ref_u.abs().max())
        R.compare(got_f, got_u, bnd_f + bnd_u, "folded against 9-tap")
    else:
        wr = (ref_f - ref_u).abs()                                  # what rounding the tap sums once, not per tap, changes (fp64)
        R.compare(got_f, got_u, bnd_f + bnd_u + wr, "folded against 9-tap (+ weight-rounding term)")
        print(f"weight-rounding term: max {float(wr.max()):.4g}, mean {float(wr.mean()):.4g}; mean of the two bounds {float((bnd_f + bnd_u).mean()):.4g}")
    # the statistics both paths hand to the consumer GroupNorm describe their own outputs
    for y in (y_u, y_f):
        plane, parts = ops.gn_of(y)
        s = plane.double().sum(1)
        R.compare_sums(s[..., 0], s[..., 1], y.double().view(2, 64 * 64, 64).permute(0, 2, 1), 64 * 64, "GroupNorm plane")
