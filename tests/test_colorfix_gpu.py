"""The colour fix on the GPU (-m gpu): csrc/colorfix.hip against fp64 element by element through the raw C ABI, and
DiffUIE.set_color_fix through forward, forward_tasks, forward_u8 and `cli restore` on the tiny model.

Op level: the cases are tests/colorfix_cases.py, the fp64 references and the bounds (with their derivations) tests/colorfix_reference.py;
this module only applies them.  Every case runs for a bf16 and an fp16 source with NaN in the padding channels of both inputs, into a
NaN-filled output with guard elements; the output's padding channels must be zero, the guards and the inputs untouched, and a second
call must give the same bits.
Model level (tiny model, 2 steps, 512 x 512 inputs: no resize between the tensors): with the fix on, `forward` must equal the fp64
formula applied to the output with the fix off and the 16-bit image the encoder saw.
"""
import json
import os

import numpy as np
import pytest
import torch

import colorfix_cases as T
import colorfix_reference as R
from restore_worker import tiny_cfg, tiny_model
from test_boundary_launchers_gpu import Buf, _bits, _in
from test_multitask_gpu import tasks_matter_

pytestmark = pytest.mark.gpu
DTYPES = list(T.DTYPES)
F32 = torch.float32
WORST = {}
FN = {"wavelet": "ur_color_fix_wavelet", "adain": "ur_color_fix_adain"}


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    yield c
    if WORST:
        print("\nlargest |y - ref| / bound:")
        for k, r in sorted(WORST.items()):
            print(f"  {k[0]:28s} {k[1]}: {r:.3f}")


def _note(what, dtype, r):
    WORST[(what, dtype)] = max(WORST.get((what, dtype), 0.0), r)


def _launch(capi, mode, cb, ld_c, sb, ld_s, out, n, src_n, h, w, dt):
    code = capi.UR_DT_F16 if dt == torch.float16 else capi.UR_DT_BF16
    stream = torch.cuda.current_stream().cuda_stream
    if mode == "wavelet":
        return capi.lib.ur_color_fix_wavelet(cb.ptr, ld_c, sb.ptr, ld_s, out.ptr, n, src_n, h, w, code, stream)
    ws_bytes = capi.lib.ur_color_fix_adain_ws_bytes(n, h, w)
    ws = Buf((ws_bytes // 4,), torch.int32)
    rc = capi.lib.ur_color_fix_adain(cb.ptr, ld_c, sb.ptr, ld_s, out.ptr, n, src_n, h, w, code, ws.ptr, ws_bytes, stream)
    torch.cuda.synchronize()
    assert ws.guards_ok()
    return rc


def _check(capi, mode, sh, dtype, c, s, what):
    """One case: c fp32 [N,H,W,3], s 16-bit [src_n,H,W,3] (host) -> the kernel's RGB output fp64 [N,H,W,3], checked against fp64."""
    n, src_n, h, w, ld_c, ld_s = sh
    dt = T.DTYPES[dtype]
    cb, sb = _in(T.padded(c, ld_c)), _in(T.padded(s, ld_s))                 # NaN in the padding channels of both inputs
    c_bits, s_bits = _bits(cb.raw).clone(), _bits(sb.raw).clone()
    outs = []
    for _ in range(2):
        out = Buf((n, h, w, ld_c), F32)
        assert _launch(capi, mode, cb, ld_c, sb, ld_s, out, n, src_n, h, w, dt) == 0, capi.lib.ur_last_error()
        torch.cuda.synchronize()
        assert out.guards_ok()
        outs.append(out.t.cpu())
    assert torch.equal(_bits(cb.raw), c_bits) and torch.equal(_bits(sb.raw), s_bits)           # inputs untouched
    y = outs[0]
    assert not torch.isnan(y).any() and torch.equal(_bits(outs[0]), _bits(outs[1]))            # written everywhere; same bits twice
    assert bool((y[..., 3:] == 0).all())                                                       # padding channels: zeros
    c64, s64 = c.double().numpy(), T.source_of(s, n)
    got = y[..., :3].double().numpy()
    ratio = float((np.abs(got - R.fix(mode, c64, s64)) / R.bound(mode, c64, s64)).max())
    _note(what, dtype, ratio)
    assert ratio <= 1.0, (mode, sh, dtype, ratio)
    return got


# ---- op level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("sh", T.SHAPES, ids=T.shape_id)
def test_case_table(capi, sh, mode, dtype):
    c, s = T.make(sh, T.DTYPES[dtype])
    if not T.runs(mode, sh):                                   # adain on a single pixel: refused, nothing written
        n, src_n, h, w, ld_c, ld_s = sh
        cb, sb, out = _in(T.padded(c, ld_c)), _in(T.padded(s, ld_s)), Buf((n, h, w, ld_c), F32)
        assert _launch(capi, mode, cb, ld_c, sb, ld_s, out, n, src_n, h, w, T.DTYPES[dtype]) == capi.UR_E_INVALID
        assert torch.isnan(out.t).all()
        return
    _check(capi, mode, sh, dtype, c, s, mode)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_wrong_source_index_shows(capi, dtype):
    """FANOUT has two distinct sources for four images: reading source n, n / 2 or 0 instead of n % 2 leaves the bound by far."""
    sh = T.FANOUT
    c, s = T.make(sh, T.DTYPES[dtype])
    c64 = c.double().numpy()
    for mode in T.MODES:
        got = _check(capi, mode, sh, dtype, c, s, mode)
        for wrong in (np.array([0, 0, 1, 1]), np.array([0, 0, 0, 0]), np.array([1, 0, 1, 0])):
            s_wrong = s.double().numpy()[wrong]
            assert (np.abs(got - R.fix(mode, c64, s_wrong)) > 1e3 * R.bound(mode, c64, s_wrong)).any(), (mode, wrong)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", T.MODES)
def test_known_answers(capi, mode, dtype):
    sh = (2, 1, 20, 24, 8, 8)
    dt = T.DTYPES[dtype]
    _, s = T.make(sh, dt)
    s32 = s.float().repeat(2, 1, 1, 1)
    # a constant per channel on top of the source comes off again (exactly representable constants: c - s is the constant up to one rounding)
    c = (s32 + torch.tensor([0.25, -0.125, 0.0625])).contiguous()
    got = _check(capi, mode, sh, dtype, c, s, mode + " (known answers)")
    tol = R.bound(mode, c.double().numpy(), T.source_of(s, 2)) + 1e-13
    assert (np.abs(got - s32.double().numpy()) <= tol).all()
    # the source itself is left alone
    got = _check(capi, mode, sh, dtype, s32.contiguous(), s, mode + " (known answers)")
    assert (np.abs(got - s32.double().numpy()) <= R.bound(mode, s32.double().numpy(), T.source_of(s, 2)) + 1e-13).all()
    if mode == "wavelet":
        assert np.array_equal(got, s32.double().numpy())                    # d = 0 exactly, and c + 0 = c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", [(0, 0), (39, 39), (0, 17), (23, 39), (20, 20)], ids=lambda p: f"y{p[0]}x{p[1]}")
def test_impulse(capi, where, dtype):
    """An impulse in s - c at a corner, an edge and the centre of a 40 x 40 plane: the response is the composition of the five clamped
    levels, which no single clamped 63-tap filter gives."""
    sh = (1, 1, 40, 40, 8, 8)
    s = torch.zeros(1, 40, 40, 3, dtype=T.DTYPES[dtype])
    s[0, where[0], where[1]] = torch.tensor([1.0, -0.5, 0.25], dtype=T.DTYPES[dtype])
    c = torch.zeros(1, 40, 40, 3)
    got = _check(capi, "wavelet", sh, dtype, c, s, "wavelet (impulse)")
    assert (got[0, :, :, 0] > 0).sum() > 900 and got[0, :, :, 0].max() < 0.1            # spread over 32 x 32 pixels at the least
    if where != (20, 20):
        one_clamp = R.low_single_clamp(s.double().numpy())
        assert (np.abs(got - one_clamp) > 1e3 * 24 * R.U).any()


def test_ops_color_fix(capi):
    """ops.color_fix: the torch front end gives the C ABI's bits, and refuses what the ABI could not check."""
    from unirestore_amd import ops
    sh = T.FANOUT
    c, s = T.make(sh, torch.float16)
    cd, sd = T.padded(c, 8).cuda(), T.padded(s, 8).cuda()
    for mode in T.MODES:
        y = ops.color_fix(cd, sd, mode)
        assert y.shape == cd.shape and y.dtype == F32 and bool((y[..., 3:] == 0).all())
        ref = R.fix(mode, c.double().numpy(), T.source_of(s, 4))
        assert (np.abs(y[..., :3].double().cpu().numpy() - ref) <= R.bound(mode, c.double().numpy(), T.source_of(s, 4))).all()
        assert torch.equal(ops.color_fix(cd, sd, mode, src_n=2), y)
        one = ops.color_fix(cd, sd, mode, src_n=1)                      # every image against source 0
        assert torch.equal(one[0], y[0]) and not torch.equal(one[1], y[1])
    for bad in (dict(src_n=3), dict(src_n=0), dict(src_n=4)):
        with pytest.raises(ValueError, match="src_n"):
            ops.color_fix(cd, sd, "wavelet", **bad)
    with pytest.raises(ValueError, match="canvas"):
        ops.color_fix(cd, sd[:, :10].contiguous(), "wavelet")
    with pytest.raises(ValueError, match="device"):
        ops.color_fix(cd, sd.cpu(), "adain")
    with pytest.raises(ValueError, match="2 pixels"):
        ops.color_fix(cd[:1, :1, :1].contiguous(), sd[:1, :1, :1].contiguous(), "adain")


# ---- model level -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    p = tasks_matter_(tiny_model(), 3)                  # (the tasks' images differ: a decode that mixed them up must show)
    p.refresh()
    yield p
    from unirestore_amd import ops
    ops.set_dtype("bf16")


def _inputs(b=2, seed=11):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(b, 3, 512, 512, generator=g)
    return img, (torch.randn(b, 4, 64, 64, generator=g), torch.randn(b, 4, 64, 64, generator=g))


def _x0(img, dt):
    """What the encoder saw, widened: round16(2 img - 1) as fp64 NHWC."""
    return (img * 2 - 1).to(dt).double().permute(0, 2, 3, 1).numpy()


def _wiring(mode, p_off, p_on, x0, what, dtype):
    """p_on against the fp64 fix of c = 2 p_off - 1 with the source x0, mapped back by (x + 1) / 2.  Bound: the op bound halved by the
    0.5 of that map, plus 2 u for the two (x + 1) / 2 maps (p_off's and p_on's roundings)."""
    c = 2 * p_off.double().cpu().permute(0, 2, 3, 1).numpy() - 1
    ref = 0.5 * R.fix(mode, c, x0) + 0.5
    bound = 0.5 * R.bound(mode, c, x0) + 2 * R.U
    err = np.abs(p_on.double().cpu().permute(0, 2, 3, 1).numpy() - ref)
    ratio = float((err / bound).max())
    print(f"{what} [{mode}, {dtype}]: largest |y - ref| / bound = {ratio:.3f}")
    return ratio


@pytest.mark.parametrize("dtype", DTYPES)
def test_off_is_off(model, dtype):
    p = model.set_dtype(dtype)
    p.use_graph = True
    img, noise = _inputs()
    p.set_color_fix(None)
    a = p(img, "ir", noise=noise)
    keys = list(p._graphs)
    p.set_color_fix("wavelet")
    p.set_color_fix(None)
    b = p(img, "ir", noise=noise)
    assert torch.equal(a, b) and list(p._graphs) == keys                     # the same bits, under the same graph key
    p.use_graph = False
    assert torch.equal(p(img, "ir", noise=noise), a)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", T.MODES)
def test_forward_is_the_formula(model, mode, dtype):
    p = model.set_dtype(dtype)
    p.use_graph = False
    img, noise = _inputs()
    x0 = _x0(img, T.DTYPES[dtype])
    p_off = p.set_color_fix(None)(img, "ir", noise=noise)
    p_on = p.set_color_fix(mode)(img, "ir", noise=noise)
    assert not torch.equal(p_on, p_off)
    ratio = _wiring(mode, p_off, p_on, x0, "forward", dtype)
    swapped = _wiring(mode, p_off, p_on, x0[::-1].copy(), "forward, sources swapped", dtype)
    assert swapped > 1e3                                                     # image n against source n, not the other one
    assert ratio <= 1.0, ratio
    # captured == eager, bit for bit, and a replay too
    p.use_graph = True
    assert torch.equal(p(img, "ir", noise=noise), p_on) and torch.equal(p(img, "ir", noise=noise), p_on)
    assert any(k[-1] == mode for k in p._graphs)
    p.set_color_fix(None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", T.MODES)
def test_forward_tasks_is_the_formula(model, mode, dtype):
    p = model.set_dtype(dtype)
    p.use_graph = False
    img, noise = _inputs()
    x0 = _x0(img, T.DTYPES[dtype])
    off = p.set_color_fix(None).forward_tasks(img, ["ir", "seg"], noise=noise)
    on = p.set_color_fix(mode).forward_tasks(img, ["ir", "seg"], noise=noise)
    assert not torch.equal(off["ir"], off["seg"])
    ratios = {t: _wiring(mode, off[t], on[t], x0, f"forward_tasks[{t}]", dtype) for t in ("ir", "seg")}
    assert _wiring(mode, off["seg"], on["ir"], x0, "forward_tasks, tasks crossed", dtype) > 1e3
    assert max(ratios.values()) <= 1.0, ratios
    p.use_graph = True
    cap = p.forward_tasks(img, ["ir", "seg"], noise=noise)
    assert all(torch.equal(cap[t], on[t]) for t in on)
    p.set_color_fix(None)


SIZES_U8 = [(300, 500), (480, 800), (500, 850)]                             # one canvas: 512 x 896


def _u8(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]


def _per_image(p, images, task, noise):
    """Slot i of forward(u8 / 255, quantize=True) * 255 on [x_i] * N: same batch size, same slot, same noise."""
    out = []
    for i, t in enumerate(images):
        x = (t.permute(2, 0, 1)[None].float() / 255).expand(len(images), -1, -1, -1).contiguous()
        out.append(p(x, task, noise=noise, quantize=True)[i].mul(255).round().to(torch.uint8).permute(1, 2, 0))
    return out


@pytest.mark.parametrize("mode", T.MODES)
def test_forward_u8(model, mode):
    from unirestore_amd.modules.model import canvas_of
    assert {canvas_of(h, w) for h, w in SIZES_U8} == {(512, 896)}
    p = model.set_dtype("bf16").set_color_fix(mode)
    a, b, c = _u8(SIZES_U8, 31)
    g = torch.Generator().manual_seed(32)
    noise = (torch.randn(3, 4, 64, 112, generator=g), torch.randn(3, 4, 64, 112, generator=g))
    p.use_graph = False
    want = _per_image(p, [a, b, c], "ir", noise)
    want2 = _per_image(p, [c, a, b], "ir", noise)
    off = p.set_color_fix(None).forward_u8([a, b, c], "ir", noise=noise)
    p.set_color_fix(mode)
    p.use_graph = True
    c0 = p.graph_captures
    got = p.forward_u8([a, b, c], "ir", noise=noise)
    got2 = p.forward_u8([c, a, b], "ir", noise=noise)                        # other sizes per slot: the same graph
    assert p.graph_captures == c0 + 1 and ("u8", 3, 512, 896, "ir", p.dtype, None, mode) in p._graphs
    for i, (y, w_, t) in enumerate(zip(got + got2, want + want2, [a, b, c, c, a, b])):
        assert y.shape == t.shape and torch.equal(y, w_.to(y.device)), (i, int((y.int() - w_.to(y.device).int()).abs().max()))
    assert any(not torch.equal(y, o) for y, o in zip(got, off))              # and the fix is in it
    p.use_graph = False
    both = p.forward_u8([a, b, c], ["ir", "seg"], noise=noise)
    for t in ("ir", "seg"):
        single = p.forward_u8([a, b, c], t, noise=noise)
        assert all(torch.equal(x, y) for x, y in zip(both[t], single)), t
    assert all(torch.equal(x, y) for x, y in zip(both["ir"], got))
    p.set_color_fix(None)


def test_restore_command(tmp_path):
    from unirestore_amd import cli, imageio
    (tmp_path / "in").mkdir()
    for i, t in enumerate(_u8([(96, 80), (100, 84), (90, 76), (96, 80)], 41)):
        imageio.save_u8(t, str(tmp_path / "in" / f"p{i}.png"))

    def run(name, flag):
        res = cli.restore(cli.apply_color_fix(tiny_cfg(), flag), str(tmp_path / "in"), str(tmp_path / name), batch=4, model=tiny_model())
        assert res["images"] == 4 and res["output_finite"] and res["graphs_captured"] == 1, res
        return {f: open(os.path.join(tmp_path / name, f), "rb").read() for f in sorted(os.listdir(tmp_path / name))}
    plain, fixed, again = run("plain", None), run("fixed", "wavelet"), run("again", "wavelet")
    assert sorted(plain) == sorted(fixed) == [f"p{i}.png" for i in range(4)]
    assert all(plain[f] != fixed[f] for f in plain)                          # the flag changes every file
    assert fixed == again                                                     # and two runs write the same bytes
    assert run("none", "none") == plain
    print("restore --color-fix:", json.dumps({f: len(v) for f, v in fixed.items()}))
