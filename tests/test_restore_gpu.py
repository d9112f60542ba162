"""Restoring image files on the GPU: mixed-size 8-bit batches through one captured graph.

Op level: the two ragged 8-bit boundary kernels against the fp32-tensor kernels they generalise (bit for bit) and against
torch on the CPU (the bounds of tests/test_ops_gpu.py's test_image_resize_reflect_pad / test_image_unpad_resize_quantize).
Model level (tiny model, 2 steps): DiffUIE.forward_u8 against `forward` on the same-size batches a ragged batch is made of
(exactly), one graph per canvas, the fp32 oracle (the one oracle run of this file), several tasks, tiling, errors.
The command: `cli restore` on seven PNGs over two canvases, in process and through torch.distributed.run.
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from golden_util import rel_l2
from restore_worker import tiny_cfg, tiny_model
from test_modules_gpu import TOL
from test_multitask_gpu import _pair

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = ["bf16", "fp16"]
TOL_16 = {"bf16": 3e-3, "fp16": 4e-4}                      # TOL_BF16 of tests/test_ops_gpu.py per dtype: one 16-bit rounding
# (canvas, [(H, W), ...]): three sizes that share 640 x 512 with a second 96 x 80 image; no resize; no padding
GEOMETRIES = [((640, 512), [(96, 80), (100, 84), (90, 76), (96, 80)]),
              ((512, 704), [(512, 700), (512, 700)]),
              ((512, 512), [(512, 512), (64, 64), (70, 70)])]


@pytest.fixture(scope="module")
def M():
    import unirestore_amd.modules as m
    return m


@pytest.fixture(scope="module")
def ops():
    from unirestore_amd import ops as o
    yield o
    o.set_dtype("bf16")


def _u8(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]


def _ragged(M, ops, images, canvas):
    """(slots uint8 [N, CH*CW*3] with stale bytes behind every image, device geom, plans)."""
    slots = torch.full((len(images), canvas[0] * canvas[1] * 3), 0xA5, dtype=torch.uint8)
    plans = [M.resize_pad_plan(*t.shape[:2]) for t in images]
    for i, t in enumerate(images):
        slots[i, :t.numel()] = t.reshape(-1)
        assert (plans[i][0] + plans[i][2], plans[i][1] + plans[i][3]) == canvas
    geom = ops.ragged_geometry([tuple(t.shape[:2]) + p[:2] for t, p in zip(images, plans)], canvas)
    return slots.cuda(), geom.cuda(), plans


def _nchw01(t):
    return t.permute(2, 0, 1)[None].float() / 255


# ---- op level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("canvas,sizes", GEOMETRIES)
def test_ingest_equals_resize_pad_and_torch(M, ops, dtype, canvas, sizes):
    ops.set_dtype(dtype)
    images = _u8(sizes, 11 + canvas[1])
    slots, geom, plans = _ragged(M, ops, images, canvas)
    y = ops.image_u8_ingest(slots, geom, canvas)
    assert y.shape == (len(images), *canvas, 8) and y.dtype == ops.act_dtype() and float(y[..., 3:].float().abs().max()) == 0.0
    for n, (t, plan) in enumerate(zip(images, plans)):
        want = ops.image_resize_pad(_nchw01(t).cuda(), *plan)
        assert torch.equal(y[n:n + 1], want), (n, tuple(t.shape), float((y[n:n + 1].float() - want.float()).abs().max()))
        rh, rw, ph, pw = plan                                             # independent of the existing kernel: torch on the CPU
        ref = _nchw01(t)
        if (rh, rw) != tuple(t.shape[:2]):
            ref = F.interpolate(ref, (rh, rw), mode="bicubic", align_corners=False, antialias=False)
        if ph or pw:
            ref = F.pad(ref, (0, pw, 0, ph), mode="reflect")
        ref = ref * 2 - 1
        got = y[n:n + 1, ..., :3].float().cpu().permute(0, 3, 1, 2)
        err = (float((got - ref).abs().max()), rel_l2(got, ref))
        print(f"ingest vs torch [{dtype}] {tuple(t.shape[:2])} -> {canvas}: max abs {err[0]:.3e} rel-L2 {err[1]:.3e}")
        assert err[0] < 8e-3 and err[1] < TOL_16[dtype], (n, err)
    assert not torch.equal(y[0], y[3]) if len(images) == 4 else True          # same size, different content


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("canvas,sizes", GEOMETRIES)
def test_egress_equals_unpad_resize_and_torch(M, ops, dtype, f32, canvas, sizes):
    dt = ops.set_dtype(dtype)
    n = len(sizes)
    x = torch.randn(n, *canvas, 8, generator=torch.Generator().manual_seed(canvas[0] + n)) * 0.6
    x = x if f32 else x.to(dt).float()
    xd = (x if f32 else x.to(dt)).cuda()
    _, geom, plans = _ragged(M, ops, _u8(sizes, 1), canvas)
    out, flags = ops.image_u8_egress(xd, 3, geom, mul=0.5, add=0.5)
    assert out.dtype == torch.uint8 and out.shape == (n, canvas[0] * canvas[1] * 3) and flags.tolist() == [0] * n
    for i, ((h, w), plan) in enumerate(zip(sizes, plans)):
        got = out[i, :h * w * 3].reshape(h, w, 3)
        want = ops.image_unpad_resize(xd[i:i + 1], 3, plan[:2], (h, w), mul=0.5, add=0.5, quantize=True)
        want = want.mul(255).round().to(torch.uint8)[0].permute(1, 2, 0)
        assert torch.equal(got, want), (i, (h, w), int((got.int() - want.int()).abs().max()))
        ref = (x[i:i + 1, ..., :3] * 0.5 + 0.5)[:, :plan[0], :plan[1]].permute(0, 3, 1, 2)
        if plan[:2] != (h, w):
            ref = F.interpolate(ref, (h, w), mode="bicubic", align_corners=False, antialias=False)
        qref = ref.mul(255).round().clamp(0, 255)[0].permute(1, 2, 0)
        d = (got.cpu().float() - qref).abs()
        print(f"egress vs torch [{dtype}, f32={f32}] {canvas} -> {(h, w)}: max {float(d.max())} codes, differing {float((d > 0).float().mean()):.2e}")
        assert float(d.max()) <= 1 and float((d > 0).float().mean()) < 2e-3, i     # a rounding tie may flip one code value


@pytest.mark.parametrize("dtype", DTYPES)
def test_egress_nonfinite_flags(M, ops, dtype):
    ops.set_dtype(dtype)
    canvas, sizes = (640, 512), [(96, 80), (100, 84), (90, 76)]
    _, geom, plans = _ragged(M, ops, _u8(sizes, 2), canvas)
    rh, rw = plans[1][:2]
    assert rh < canvas[0]                                                      # image 1 has padding rows to poison
    x = (torch.randn(3, *canvas, 8, generator=torch.Generator().manual_seed(4)) * 0.6).cuda()
    clean, flags = ops.image_u8_egress(x, 3, geom, mul=0.5, add=0.5)
    assert flags.tolist() == [0, 0, 0]
    pad = x.clone()
    pad[1, rh:, :, :3] = float("nan")                                          # outside [0:RH_1, 0:RW_1]: never read
    pad[1, rh, 5, 1] = float("inf")
    out, flags = ops.image_u8_egress(pad, 3, geom, mul=0.5, add=0.5)
    assert flags.tolist() == [0, 0, 0] and torch.equal(out[1, :100 * 84 * 3], clean[1, :100 * 84 * 3])
    def tap(dst, size_in, size_out):                                           # the source index bicubic tap 1 of output `dst` reads
        return int(math.floor(size_in / size_out * (dst + 0.5) - 0.5))
    bad = x.clone()
    bad[1, tap(50, rh, 100), tap(40, rw, 84), 0] = float("nan")
    bad[1, tap(10, rh, 100), tap(20, rw, 84), 2] = float("inf")
    out, flags = ops.image_u8_egress(bad, 3, geom, mul=0.5, add=0.5)
    assert flags.tolist() == [0, 1, 0]
    assert torch.equal(out[0, :96 * 80 * 3], clean[0, :96 * 80 * 3]) and torch.equal(out[2, :90 * 76 * 3], clean[2, :90 * 76 * 3])
    img1, was = out[1, :100 * 84 * 3].reshape(100, 84, 3).clone(), clean[1, :100 * 84 * 3].reshape(100, 84, 3)
    assert int(img1[50, 40, 0]) == 0 and int(img1[10, 20, 2]) == 0             # a non-finite sample is stored as code 0
    changed = img1 != was
    changed[50, 40, 0] = changed[10, 20, 2] = False
    assert int(changed.sum()) == 0            # 6x downscale: the 4 x 4 taps of neighbouring outputs do not overlap


def test_ragged_argument_errors(M, ops):
    ops.set_dtype("bf16")
    canvas = (640, 512)
    slots, geom, _ = _ragged(M, ops, _u8([(96, 80), (100, 84)], 3), canvas)
    x = torch.zeros(2, *canvas, 8, device="cuda")
    with pytest.raises(ValueError, match="does not fit"):
        ops.ragged_geometry([(641, 80, 641, 512)], canvas)                     # H > CH
    too_tall = geom.clone()
    too_tall[1, 0] = 641
    for bad_geom, word in ((too_tall, "does not fit"), (geom.float(), "int32"), (geom[:, :3].contiguous(), "int32"),
                           (geom[:1], "int32"), (geom.cpu(), "current device"), (geom.t().contiguous().t(), "contiguous")):
        with pytest.raises(ValueError, match=word):
            ops.image_u8_ingest(slots, bad_geom, canvas)
        if bad_geom.shape[0] == 2:
            with pytest.raises(ValueError, match=word):
                ops.image_u8_egress(x, 3, bad_geom)
    with pytest.raises(ValueError, match="uint8"):
        ops.image_u8_ingest(slots.float(), geom, canvas)
    with pytest.raises(ValueError, match="current device"):
        ops.image_u8_ingest(slots.cpu(), geom, canvas)
    with pytest.raises(ValueError, match="slot_bytes"):
        ops.image_u8_ingest(slots[:, :1000].contiguous(), geom, canvas)
    with pytest.raises(ValueError, match="nonfinite"):
        ops.image_u8_egress(x, 3, geom, nonfinite=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="NHWC"):
        ops.image_u8_egress(x.cpu().numpy(), 3, geom)
    # a table row that reaches the kernel unchecked is not followed: zeros in, nothing out but flag 2
    y = ops.image_u8_ingest(slots, too_tall, canvas, validate=False)
    assert float(y[1].float().abs().max()) == 0.0 and float(y[0].float().abs().max()) > 0
    out = torch.full((2, canvas[0] * canvas[1] * 3), 7, dtype=torch.uint8, device="cuda")
    _, flags = ops.image_u8_egress(x, 3, too_tall, out=out, validate=False)
    assert flags.tolist() == [0, 2] and int(out[1].min()) == int(out[1].max()) == 7


# ---- model level ------------------------------------------------------------------------------------------------------------
SIZES_A = [(96, 80), (100, 84), (90, 76)]                                     # canvas 640 x 512, latent 80 x 64


def _abc(seed=5):
    imgs = _u8(SIZES_A, seed)
    g = torch.Generator().manual_seed(seed + 100)
    return imgs, (torch.randn(3, 4, 80, 64, generator=g), torch.randn(3, 4, 80, 64, generator=g))


def _same_size_reference(p, images, task, noise):
    """Slot i of forward on [x_i, x_i, x_i] as fp32 / 255: same batch size, same slot, same noise."""
    out = []
    for i, t in enumerate(images):
        y = p(_nchw01(t).expand(len(images), -1, -1, -1).contiguous(), task, noise=noise, quantize=True)
        out.append(y[i].mul(255).round().to(torch.uint8).permute(1, 2, 0))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_graph", [False, True])
def test_ragged_batch_equals_same_size_batches(M, use_graph, dtype):
    _, p = _pair(M, dtype=dtype, use_graph=use_graph)
    images, noise = _abc()
    got = p.forward_u8(images, "ir", noise=noise)
    want = _same_size_reference(p, images, "ir", noise)
    for i, (g, w, t) in enumerate(zip(got, want, images)):
        assert g.dtype == torch.uint8 and g.is_cuda and g.shape == t.shape
        assert torch.equal(g, w), (i, int((g.int() - w.int()).abs().max()), float((g != w).float().mean()))
    dev = p.forward_u8([t.cuda() for t in images], "ir", noise=noise)            # device inputs: the same
    assert all(torch.equal(a, b) for a, b in zip(dev, got)) and p.u8_nonfinite() == [False] * 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_graph_per_canvas(M, dtype):
    _, p = _pair(M, dtype=dtype, use_graph=True)
    (a, b, c), noise = _abc()
    b2 = _u8([(96, 80)], 77)[0]
    x32 = torch.rand(1, 3, 96, 80, generator=torch.Generator().manual_seed(1))
    n32 = (noise[0][:1], noise[1][:1])
    before32 = p(x32, "ir", noise=n32)
    n0, c0 = len(p._graphs), p.graph_captures
    first = p.forward_u8([a, b, c], "ir", noise=noise)
    assert len(p._graphs) == n0 + 1
    second = p.forward_u8([c, a, b2], "ir", noise=noise)                          # other sizes per slot, same N and canvas
    assert len(p._graphs) == n0 + 1 and p.graph_captures == c0 + 1
    assert all(torch.equal(g, w) for g, w in zip(second, _same_size_reference(p, [c, a, b2], "ir", noise)))
    assert all(torch.equal(g, w) for g, w in zip(p.forward_u8([a, b, c], "ir", noise=noise), first))
    n1 = len(p._graphs)                                                        # (_same_size_reference captured fp32 graphs)
    wide = _u8([(80, 96), (84, 100), (80, 96)], 8)                             # canvas 512 x 640
    nw = (noise[0].transpose(2, 3).contiguous(), noise[1].transpose(2, 3).contiguous())
    out = p.forward_u8(wide, "ir", noise=nw)
    assert len(p._graphs) == n1 + 1 and [tuple(o.shape) for o in out] == [(80, 96, 3), (84, 100, 3), (80, 96, 3)]
    assert ("u8", 3, 640, 512, "ir", p.dtype, None) in p._graphs and ("u8", 3, 512, 640, "ir", p.dtype, None) in p._graphs
    assert torch.equal(p(x32, "ir", noise=n32), before32)                      # forward's own graphs are untouched


def test_against_the_fp32_oracle(M):
    """The one oracle run of this file: the ragged batch, image by image (the oracle has no ragged batch).
    ||g - q(o)|| <= fwd_img * ||o|| + sqrt(numel) / 255: the project's bound on the unquantised image, plus half a code value
    for each of the two roundings (the clamp moves nothing apart)."""
    o, p = _pair(M, dtype="bf16", use_graph=True)
    images, noise = _abc()
    with torch.no_grad():
        oracle = [o(_nchw01(t), "ir", noise=(noise[0][i:i + 1], noise[1][i:i + 1]))[0] for i, t in enumerate(images)]
    for dtype in DTYPES:
        p.set_dtype(dtype)
        got = p.forward_u8(images, "ir", noise=noise)
        for i, (g, oi) in enumerate(zip(got, oracle)):
            q = oi.mul(255).round().clamp(0, 255).div(255)
            gf = g.cpu().permute(2, 0, 1).float() / 255
            err, bound = float((gf - q).norm()), TOL[dtype]["fwd_img"] * float(oi.norm()) + math.sqrt(oi.numel()) / 255
            print(f"forward_u8 vs oracle [{dtype}] image {i} {tuple(g.shape)}: ||g - q(o)|| = {err:.4f}, bound {bound:.4f} "
                  f"(unquantised part {TOL[dtype]['fwd_img'] * float(oi.norm()):.4f})")
            assert err <= bound, (dtype, i, err, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_graph", [False, True])
def test_several_tasks(M, use_graph, dtype):
    """forward_u8(x, [ir, seg])[t] == forward_u8(x, t), exactly, on weights whose tasks matter: one restoration, and the decoder
    tail of each task at the batch size of the single-task call (a fanned-out K * N tail, as forward_tasks runs it, differs from
    it in 20 % of the bf16 samples by up to 2 code values: the conv launchers plan a batch of 6 differently from a batch of 3)."""
    _, p = _pair(M, dtype=dtype, use_graph=use_graph)                           # weights whose tasks matter (tasks_matter_)
    images, noise = _abc()
    both = p.forward_u8(images, ["ir", "seg"], noise=noise)
    assert list(both) == ["ir", "seg"] and p.u8_nonfinite() == [False] * 3
    ir, seg = p.forward_u8(images, "ir", noise=noise), p.forward_u8(images, "seg", noise=noise)
    assert not all(torch.equal(a, b) for a, b in zip(ir, seg))                  # the tasks do matter
    for name, single in (("ir", ir), ("seg", seg)):
        for i, (g, w) in enumerate(zip(both[name], single)):
            assert torch.equal(g, w), (name, i, int((g.int() - w.int()).abs().max()), float((g != w).float().mean()))
    preds, z0, zt = p.forward_u8(images, ["seg"], noise=noise, return_latents=True)
    assert all(torch.equal(a, b) for a, b in zip(preds["seg"], seg)) and z0.shape == zt.shape == (3, 4, 80, 64)
    if use_graph:                                                              # one graph for the task tuple, replayed
        n = p.graph_captures
        again = p.forward_u8(images, ["ir", "seg"], noise=noise)
        assert p.graph_captures == n and all(torch.equal(a, b) for t in both for a, b in zip(again[t], both[t]))


def test_several_tasks_restore_once(M, monkeypatch):
    """Several tasks share ONE encode and ONE denoise loop (eager run with counting wrappers, as test_multitask_gpu.py counts)."""
    steps = 2
    _, p = _pair(M, steps=steps)
    images, noise = _abc()
    calls = dict(encode=0, unet=0)
    enc, unet = p.ae.encode_run, p.base_model.run
    monkeypatch.setattr(p.ae, "encode_run", lambda *a, **k: (calls.__setitem__("encode", calls["encode"] + 1), enc(*a, **k))[1])
    monkeypatch.setattr(p.base_model, "run", lambda *a, **k: (calls.__setitem__("unet", calls["unet"] + 1), unet(*a, **k))[1])
    p.forward_u8(images, ["ir", "cls", "seg"], noise=noise)
    assert calls == dict(encode=1, unet=steps)


def test_tiling_and_errors(M):
    _, p = _pair(M, use_graph=True)
    p.set_latent_tiling(32, 24)
    images, noise = _abc()
    assert p._tile_plan(80, 64) is not None                                    # latent 80 x 64: 3 x 3 tiles of 32
    got = p.forward_u8(images, "ir", noise=noise)
    assert all(torch.equal(g, w) for g, w in zip(got, _same_size_reference(p, images, "ir", noise)))
    assert ("u8", 3, 640, 512, "ir", p.dtype, (32, 24)) in p._graphs and p.u8_nonfinite() == [False] * 3
    p.set_latent_tiling(None)
    with pytest.raises(ValueError, match="640x512.*512x640|512x640.*640x512"):
        p.forward_u8(images[:2] + _u8([(80, 96)], 1), "ir")
    with pytest.raises(KeyError):
        p.forward_u8(images, "deblur")
    with pytest.raises(KeyError):
        p.forward_u8(images, ["ir", "deblur"])
    with pytest.raises(ValueError):
        p.forward_u8([], "ir")
    with pytest.raises(ValueError, match="uint8"):
        p.forward_u8([images[0].float()], "ir")
    with pytest.raises(ValueError, match="noise"):
        p.forward_u8(images, "ir", noise=(noise[0][:2], noise[1][:2]))


def test_fp16_overflow_is_loud(M, monkeypatch):
    """An 8-bit image cannot carry the NaN that forward's check looks for: the egress flags do."""
    _, p = _pair(M, dtype="fp16", use_graph=False)
    images, noise = _abc()
    p.forward_u8(images, "ir", noise=noise)
    from unirestore_amd import ops
    real = ops.image_u8_egress

    def poisoned(x, *a, **k):
        x = x.clone()
        x[2, 3, 4, 1] = float("inf")
        return real(x, *a, **k)
    monkeypatch.setattr(ops, "image_u8_egress", poisoned)
    with pytest.raises(FloatingPointError, match="fp16 activation overflow"):
        p.forward_u8(images, "ir", noise=noise)
    assert p.u8_nonfinite() == [False, False, True]
    p.check_fp16_overflow = False
    p.forward_u8(images, "ir", noise=noise)


# ---- the command ------------------------------------------------------------------------------------------------------------
FOLDER = [("a0", (96, 80)), ("a1", (100, 84)), ("b0", (80, 96)), ("a2", (90, 76)), ("a3", (96, 80)), ("b1", (80, 96)), ("a4", (100, 84))]


def _folder(path):
    from unirestore_amd import imageio
    path.mkdir()
    for (stem, _), t in zip(FOLDER, _u8([hw for _, hw in FOLDER], 21)):
        imageio.save_u8(t, str(path / f"{stem}.png"))
    return sorted(str(path / f"{stem}.png") for stem, _ in FOLDER)


def _read(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def test_restore_command(tmp_path):
    from unirestore_amd import cli, imageio
    paths = _folder(tmp_path / "in")
    sizes = [hw for _, hw in imageio.scan(paths)]
    plan = imageio.plan_batches(sizes, 3)
    assert imageio.graphs_implied(plan) == 2 and [len(b.members) for b in plan] == [3, 3, 2] and [b.valid for b in plan] == [3, 2, 2]
    res = cli.restore(tiny_cfg(), str(tmp_path / "in"), str(tmp_path / "out"), batch=3, model=tiny_model())
    print("cli restore:", json.dumps(res))
    assert res["images"] == 7 and res["input_sizes"] == 4 and res["canvases"] == 2 and res["graphs_captured"] == 2
    assert res["output_finite"] and res["images_timed"] == 2 and res["images_per_s"] > 0
    first = _read(tmp_path / "out")
    assert sorted(first) == sorted(f"{stem}.png" for stem, _ in FOLDER)
    # every file is forward_u8 on its batch of the plan with the documented noise
    model = tiny_model()
    for b in plan:
        images = [imageio.load_u8(paths[i]) for i in b.members]
        got = model.forward_u8(images, "ir", noise=cli.restore_noise(7, b.index, len(b.members), b.canvas))
        for i, g in list(zip(b.members, got))[:b.valid]:
            out = imageio.load_u8(str(tmp_path / "out" / os.path.basename(paths[i])))
            assert tuple(out.shape[:2]) == sizes[i] and torch.equal(out, g.cpu()), paths[i]
    cli.restore(tiny_cfg(), str(tmp_path / "in"), str(tmp_path / "out2"), batch=3, model=tiny_model())
    assert _read(tmp_path / "out2") == first                                   # a second run writes identical bytes
    both = cli.restore(tiny_cfg(), str(tmp_path / "in"), str(tmp_path / "out3"), tasks="ir,seg", batch=3, model=model)
    assert both["tasks"] == ["ir", "seg"] and sorted(os.listdir(tmp_path / "out3")) == ["ir", "seg"]
    assert _read(tmp_path / "out3" / "ir").keys() == first.keys() == _read(tmp_path / "out3" / "seg").keys()
    # the same through the launcher of tests/test_dist_gpu.py
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29553", os.path.join(HERE, "restore_worker.py"), str(tmp_path / "in"), str(tmp_path / "out4"), "3"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=os.path.dirname(HERE))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.stdout[-1000:], r.stderr[-2000:])
    v = json.loads(lines[-1])
    assert v["images"] == 7 and v["graphs_captured"] == 2 and v["n_gpus"] == 1, v
    assert _read(tmp_path / "out4") == first
