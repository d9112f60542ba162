"""Per-image seeded noise on the GPU: the HIP generator against the numpy / fp64 reference, its independence of the slot, its
wiring into forward / forward_tasks / forward_u8 (eager and captured), and `restore --noise image` / `--samples` on files.

Tiny model of tests/restore_worker.py at 2 steps; every reference block is computed once per process.
"""
import functools
import os

import numpy as np
import pytest
import torch

import keyed_noise_reference as ref
from restore_worker import tiny_cfg, tiny_model

pytestmark = pytest.mark.gpu

SEEDS = [0, 2 ** 32 + 5, 2 ** 64 - 1]
# the issue's shapes, and one that needs more than one block per image (4096 counters = 16 blocks)
SHAPES = [(1, 4, 1, 1), (3, 4, 8, 8), (2, 3, 5, 7), (1, 1, 1, 3), (2, 4, 64, 64)]
SENTINEL = 0x5A5A5A5A


def _seeds_for(shape):
    i = SHAPES.index(shape)
    return [SEEDS[(i + j) % 3] for j in range(shape[0])]


@functools.lru_cache(maxsize=None)
def _reference(shape, draw, kind):
    out = ref.keyed_noise(_seeds_for(shape), draw, shape[1:], kind)
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def ops():
    from unirestore_amd import ops as o
    yield o
    o.set_dtype("bf16")


def _keys(ops, seeds):
    return ops.noise_keys(seeds).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_bits_equal_the_reference_exactly(ops, shape):
    """Raw words, both draws; written into a fresh tensor, and into a guarded buffer at byte offsets 0, 4 (off 16 bytes: the
    4-byte store path) and 16.  (2,3,5,7) has count % 4 = 1, so image 1 starts off 16 bytes and both images end in a tail."""
    keys, total = _keys(ops, _seeds_for(shape)), int(np.prod(shape))
    for draw in (0, 1):
        want = _reference(shape, draw, "bits")
        got = ops.keyed_noise(keys, draw, shape[1:], kind="bits")
        assert got.dtype == torch.int32 and tuple(got.shape) == shape and got.is_cuda
        assert np.array_equal(_u32(got), want), (shape, draw)
        for off in (0, 1, 4):
            buf = torch.full((off + total + 8,), SENTINEL, dtype=torch.int32, device="cuda")
            assert buf.data_ptr() % 16 == 0
            out = ops.keyed_noise(keys, draw, shape[1:], kind="bits", out=buf[off:off + total])
            assert out.data_ptr() == buf.data_ptr() + 4 * off
            host = buf.cpu().numpy()
            assert np.array_equal(host[off:off + total].view(np.uint32), want.reshape(-1)), (shape, draw, off)
            assert (host[:off] == SENTINEL).all() and (host[off + total:] == SENTINEL).all(), (shape, draw, off)
    assert not np.array_equal(_reference(shape, 0, "bits"), _reference(shape, 1, "bits"))


@pytest.mark.parametrize("shape", SHAPES)
def test_normals_against_fp64(ops, shape):
    """max |kernel - fp64| <= 1e-5, derived and not measured: theta = 2 pi u rounded to fp32 is off by <= 6.5e-7 (half an ulp at
    6.28 plus the constant's rounding); times r <= 5.77 that is 3.8e-6; a few ulp in log / sqrt / sincos add about 2e-6 (numpy
    fp32 on the CPU measures 2.4e-6 over 65 536 values).  A failure means a fast intrinsic crept in."""
    keys = _keys(ops, _seeds_for(shape))
    for draw in (0, 1):
        want = _reference(shape, draw, "normal")
        got = ops.keyed_noise(keys, draw, shape[1:])
        assert got.dtype == torch.float32 and tuple(got.shape) == shape
        g = got.cpu().numpy().astype(np.float64)
        err = float(np.abs(g - want).max())
        print(f"keyed_noise normal {shape} draw {draw}: max abs err vs fp64 {err:.3e}, max |v| {float(np.abs(g).max()):.3f}")
        assert np.isfinite(g).all() and float(np.abs(g).max()) <= 5.77
        assert err <= 1e-5, (shape, draw, err)
        buf = torch.full((1 + got.numel() + 4,), float("nan"), device="cuda")       # the 4-byte store path gives the same bits
        off = ops.keyed_noise(keys, draw, shape[1:], out=buf[1:1 + got.numel()])
        assert torch.equal(off, got) and bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[1 + got.numel():]).all())


def test_slot_independence(ops):
    s = 2 ** 32 + 5
    for kind in ("bits", "normal"):
        for draw in (0, 1):
            alone = ops.keyed_noise(_keys(ops, [s]), draw, (4, 8, 8), kind=kind)
            third = ops.keyed_noise(_keys(ops, [77, 0, s]), draw, (4, 8, 8), kind=kind)
            assert torch.equal(alone[0], third[2]), (kind, draw)
            assert not torch.equal(third[0], third[2]) and not torch.equal(third[1], third[2])


def test_op_argument_errors_on_the_device(ops):
    keys = _keys(ops, [1, 2])
    with pytest.raises(ValueError, match="current device"):
        ops.keyed_noise(keys.cpu(), 0, (4, 8, 8))
    for shape in ((4, 8), (4, 0, 8), (4, 8, 8, 8)):
        with pytest.raises(ValueError, match="shape"):
            ops.keyed_noise(keys, 0, shape)
    with pytest.raises(ValueError, match="draw"):
        ops.keyed_noise(keys, -1, (4, 8, 8))
    with pytest.raises(ValueError, match="out"):
        ops.keyed_noise(keys, 0, (4, 8, 8), out=torch.empty(2 * 256, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        ops.keyed_noise(keys, 0, (4, 8, 8), out=torch.empty(100, device="cuda"))
    uk = keys.view(torch.uint32)                                                 # a uint32 table is the same table
    assert torch.equal(ops.keyed_noise(uk, 1, (4, 8, 8)), ops.keyed_noise(keys, 1, (4, 8, 8)))


# ---- the model ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return tiny_model()


def _u8(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]


def _flat(result):
    """(preds, z0, zt) -> a flat list of tensors: preds is a tensor, a list (forward_u8), or {task: either}."""
    preds, z0, zt = result
    out = []
    for v in (preds.values() if isinstance(preds, dict) else [preds]):
        out += list(v) if isinstance(v, (list, tuple)) else [v]
    return out + [z0, zt]


def _assert_same(a, b, what):
    a, b = _flat(a), _flat(b)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(x, y), (what, i, float((x.float() - y.float()).abs().max()))


def _entry(model, name):
    """(call(**draws) -> (preds, z0, zt), latent shape (C, H, W), N) of one public entry point on its smallest input."""
    if name == "forward_u8":                                                     # two sizes that share the 640 x 512 canvas
        images = _u8([(96, 80), (100, 84)], 5)
        return (lambda **kw: model.forward_u8(images, "ir", return_latents=True, **kw)), (4, 80, 64), 2
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(6))     # canvas 512 x 512
    if name == "forward_tasks":
        return (lambda **kw: model.forward_tasks(x, ["ir", "seg"], return_latents=True, **kw)), (4, 64, 64), 2
    return (lambda **kw: model(x, "ir", return_latents=True, **kw)), (4, 64, 64), 2


S1, S2 = [2 ** 32 + 5, 2 ** 64 - 1], [0, 2 ** 32 + 5]


@pytest.mark.parametrize("name", ["forward", "forward_tasks", "forward_u8"])
def test_seeds_equal_the_generated_noise(ops, model, name):
    """forward(seeds=S) == forward(noise=(keyed_noise(S, 0), keyed_noise(S, 1))) bit for bit in images, z0 and zt: eager, and
    captured - where two seed lists share ONE graph and each replay equals its eager result."""
    call, lat, n = _entry(model, name)
    model.set_latent_tiling(None).set_color_fix(None)

    def given(seeds):
        keys = _keys(ops, seeds)
        return ops.keyed_noise(keys, 0, lat), ops.keyed_noise(keys, 1, lat)
    try:
        model.use_graph = False
        eager = {tuple(s): call(seeds=s) for s in (S1, S2)}
        _assert_same(eager[tuple(S1)], call(noise=given(S1)), f"{name} eager")
        assert not torch.equal(eager[tuple(S1)][1], eager[tuple(S2)][1])        # other seeds, other z0
        model.use_graph = True
        graphs, captures = len(model._graphs), model.graph_captures
        for s in (S1, S2, S1):
            _assert_same(call(seeds=s), eager[tuple(s)], f"{name} captured {s}")
        assert model.graph_captures == captures + 1 and len(model._graphs) == graphs + 1
        assert sum(1 for k in model._graphs if k[-1] == "seeded") == 1
        _assert_same(call(noise=given(S2)), eager[tuple(S2)], f"{name} captured, noise given")
        assert model.graph_captures == captures + 2                              # the unseeded graph is another one
        assert sum(1 for k in model._graphs if k[-1] == "seeded") == 1
    finally:
        model.use_graph = True


@pytest.mark.parametrize("option,use_graph", [("tiling", False), ("wavelet", True), ("adain", False)])
def test_seeds_with_tiling_and_colour_fix(ops, model, option, use_graph):
    call, lat, n = _entry(model, "forward")
    keys = _keys(ops, S1)
    try:
        model.use_graph = use_graph
        if option == "tiling":
            model.set_latent_tiling(32, 24)
            assert model._tile_plan(64, 64) is not None                           # 3 x 3 tiles of 32
        else:
            model.set_color_fix(option)
        _assert_same(call(seeds=S1), call(noise=(ops.keyed_noise(keys, 0, lat), ops.keyed_noise(keys, 1, lat))), option)
    finally:
        model.set_latent_tiling(None).set_color_fix(None)
        model.use_graph = True


def test_seed_argument_errors(model):
    x = torch.rand(2, 3, 64, 64)
    noise = (torch.zeros(2, 4, 64, 64), torch.zeros(2, 4, 64, 64))
    images = _u8([(96, 80), (100, 84)], 5)
    for call in (lambda **kw: model(x, "ir", **kw), lambda **kw: model.forward_tasks(x, ["ir", "seg"], **kw),
                 lambda **kw: model.forward_u8(images, "ir", **kw)):
        with pytest.raises(ValueError, match="exclude"):
            call(seeds=[1, 2], noise=noise)
        for bad in ([1], [1, 2, 3]):
            with pytest.raises(ValueError, match="one per image"):
                call(seeds=bad)
        with pytest.raises(ValueError, match="2\\^64"):
            call(seeds=[1, 2 ** 64])


# ---- the command ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restored(tmp_path_factory, model):
    """`restore --batch 2` of the list files `X, Y` and `Y, X` (one 640 x 512 canvas) under both noise modes, and of `X` alone
    with --samples 2: {run: {file name: bytes}}, each run once."""
    from unirestore_amd import cli, imageio
    root = tmp_path_factory.mktemp("keyed_noise")
    (root / "in").mkdir()
    for stem, t in zip(("X", "Y"), _u8([(96, 80), (100, 84)], 21)):
        imageio.save_u8(t, str(root / "in" / f"{stem}.png"))
    lists = dict(xy="X.png\nY.png\n", yx="Y.png\nX.png\n", x="X.png\n")
    for name, text in lists.items():
        (root / "in" / f"{name}.txt").write_text(text)
    model.set_latent_tiling(None).set_color_fix(None)
    model.use_graph = True
    runs = {}
    for run, lst, kw in (("image_xy", "xy", dict(noise="image")), ("image_yx", "yx", dict(noise="image")),
                         ("batch_xy", "xy", {}), ("batch_yx", "yx", {}), ("samples_x", "x", dict(noise="image", samples=2))):
        out = root / run
        res = cli.restore(tiny_cfg(), str(root / "in" / f"{lst}.txt"), str(out), batch=2, model=model, **kw)
        assert res["output_finite"] and res["noise"] == kw.get("noise", "batch") and res["samples"] == kw.get("samples", 1)
        assert res["images"] == 2 and res["graphs_captured"] == 1
        runs[run] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    return runs


def test_restore_image_noise_ignores_the_list_order(restored):
    """The test that fails without the feature: with --noise image a file's bytes do not depend on its slot."""
    assert sorted(restored["image_xy"]) == sorted(restored["image_yx"]) == ["X.png", "Y.png"]
    assert restored["image_xy"]["X.png"] == restored["image_yx"]["X.png"]
    assert restored["image_xy"]["Y.png"] == restored["image_yx"]["Y.png"]
    assert restored["image_xy"]["X.png"] != restored["image_xy"]["Y.png"]


def test_restore_batch_noise_depends_on_the_slot(restored):
    """The default is today's behaviour: the slot's slice of one host draw per batch, so the same pair in the other order differs."""
    assert sorted(restored["batch_xy"]) == sorted(restored["batch_yx"]) == ["X.png", "Y.png"]
    assert restored["batch_xy"]["X.png"] != restored["batch_yx"]["X.png"]
    assert restored["batch_xy"]["Y.png"] != restored["batch_yx"]["Y.png"]
    assert restored["batch_xy"]["X.png"] != restored["image_xy"]["X.png"]


def test_restore_samples(restored):
    got = restored["samples_x"]
    assert sorted(got) == ["X.s0.png", "X.s1.png"] and got["X.s0.png"] != got["X.s1.png"]
    assert got["X.s0.png"] == restored["image_xy"]["X.png"]                       # sample 0 at batch size 2 is the K = 1 file
