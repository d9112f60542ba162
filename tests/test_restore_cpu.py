"""Restoring image files, the parts that need no GPU: canvases, the batch plan, 8-bit file I/O, `cli restore` argument errors,
the list-file dataset of `validate`.  (tests/test_restore_gpu.py holds the kernels, DiffUIE.forward_u8 and the command.)"""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from tiny_cfg import model_kwargs
from unirestore_amd import cli, imageio
from unirestore_amd.modules.model import canvas_of, resize_pad_plan

CANVASES = {(512, 896): [(300, 500), (480, 800), (500, 850)], (640, 512): [(96, 80), (100, 84), (90, 76)],
            (512, 640): [(80, 96), (84, 100)], (512, 512): [(64, 64), (70, 70), (512, 512)], (512, 704): [(511, 700), (512, 700)],
            (640, 640): [(600, 600)], (768, 1280): [(720, 1280)]}
ALL_SIZES = [hw for v in CANVASES.values() for hw in v]


def _cfg(**over):
    return dict(seed_everything=7, trainer=dict(precision="bf16-mixed"),
                model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=model_kwargs(2))), **over)


@pytest.mark.parametrize("canvas,sizes", sorted(CANVASES.items()))
def test_canvas_known_answers(canvas, sizes):
    for h, w in sizes:
        rh, rw, ph, pw = resize_pad_plan(h, w)
        assert canvas_of(h, w) == (rh + ph, rw + pw) == canvas, (h, w)
        assert h <= rh <= canvas[0] and w <= rw <= canvas[1]                 # the resize only ever scales up
        assert ph < rh and pw < rw                                            # a reflect pad the kernels accept


def _rand_sizes(rng, n):
    pool = ALL_SIZES + [(rng.randint(40, 900), rng.randint(40, 900)) for _ in range(6)]
    return [rng.choice(pool) for _ in range(n)]


def test_plan_batches_properties():
    rng = random.Random(20)
    for trial in range(60):
        n, batch = rng.randint(1, 40), rng.randint(1, 9)
        sizes = _rand_sizes(rng, n)
        whole = imageio.plan_batches(sizes, batch)
        assert whole == imageio.plan_batches(list(sizes), batch)               # same arguments, same plan
        assert [b.index for b in whole] == list(range(len(whole)))
        assert [b.members[0] for b in whole] == sorted(b.members[0] for b in whole)
        for world in (1, 2, 3, 8):
            parts = [imageio.plan_batches(sizes, batch, r, world) for r in range(world)]
            assert sorted((b for p in parts for b in p), key=lambda b: b.index) == whole      # the union does not depend on world
            for r, p in enumerate(parts):
                assert [b.index % world for b in p] == [r] * len(p)
        written = [i for b in whole for i in b.members[:b.valid]]
        assert sorted(written) == list(range(n))                              # every input exactly once
        full = set()
        for b in whole:
            assert 1 <= b.valid <= len(b.members) <= batch
            assert all(canvas_of(*sizes[i]) == b.canvas for i in b.members)
            assert list(b.members[:b.valid]) == sorted(b.members[:b.valid])   # input order inside a group
            assert all(i == b.members[b.valid - 1] for i in b.members[b.valid:])   # padding repeats the last image
            if len(b.members) > b.valid:                                      # padded only behind a full batch of the canvas
                assert len(b.members) == batch and b.canvas in full
            elif b.valid < batch:
                assert b.canvas not in full
            if b.valid == batch:
                full.add(b.canvas)
        assert imageio.graphs_implied(whole) == len({(len(b.members), b.canvas) for b in whole})


def test_plan_batches_example_and_errors():
    sizes = [(300, 500), (64, 64), (480, 800), (70, 70), (500, 850), (512, 512), (300, 500)]
    plan = imageio.plan_batches(sizes, 2)
    assert [(b.canvas, b.members, b.valid) for b in plan] == [((512, 896), (0, 2), 2), ((512, 512), (1, 3), 2),
                                                              ((512, 896), (4, 6), 2), ((512, 512), (5, 5), 1)]
    assert imageio.graphs_implied(plan) == 2
    assert [b.members for b in imageio.plan_batches(sizes[:3], 8)] == [(0, 2), (1,)]      # short groups run at their own size
    for bad in (dict(batch=0), dict(batch=2, rank=2, world=2), dict(batch=2, rank=-1), dict(batch=2, world=0)):
        with pytest.raises(ValueError):
            imageio.plan_batches(sizes, **bad)


def _png(path, arr, mode=None):
    Image.fromarray(arr, mode).save(path)
    return str(path)


def test_load_save_u8(tmp_path):
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    t = imageio.load_u8(_png(tmp_path / "rgb.png", rgb))
    assert t.dtype == torch.uint8 and tuple(t.shape) == (37, 53, 3) and np.array_equal(t.numpy(), rgb)
    imageio.save_u8(t, str(tmp_path / "again.png"))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "again.png")), rgb)             # RGB round-trips exactly
    grey = rng.integers(0, 256, (20, 31), dtype=np.uint8)
    rgba = rng.integers(0, 256, (20, 31, 4), dtype=np.uint8)
    deep = rng.integers(0, 65536, (20, 31), dtype=np.uint16)
    files = [_png(tmp_path / "grey.png", grey), _png(tmp_path / "rgba.png", rgba), _png(tmp_path / "deep.png", deep)]
    pal = Image.fromarray(rgb).convert("P", palette=Image.ADAPTIVE, colors=17)
    pal.save(tmp_path / "pal.png")
    files.append(str(tmp_path / "pal.png"))
    assert [Image.open(f).mode for f in files] == ["L", "RGBA", "I;16", "P"]
    for f in files:
        t = imageio.load_u8(f)
        want = np.asarray(Image.open(f).convert("RGB"))
        assert t.dtype == torch.uint8 and t.shape[2] == 3 and np.array_equal(t.numpy(), want), f
    assert imageio.scan(files + [str(tmp_path / "rgb.png")]) == [(f, (20, 31)) for f in files[:3]] + [(files[3], (37, 53)),
                                                                                                      (str(tmp_path / "rgb.png"), (37, 53))]
    with pytest.raises(ValueError):
        imageio.save_u8(t.float(), str(tmp_path / "no.png"))


def test_list_inputs(tmp_path):
    d = tmp_path / "in"
    (d / "sub").mkdir(parents=True)
    for name in ("b.png", "a.PNG", "c.jpg", "notes.txt", "sub/deep.png"):
        (d / name).write_bytes(b"")
    assert [os.path.basename(p) for p in imageio.list_inputs(str(d))] == ["a.PNG", "b.png", "c.jpg"]      # sorted, not recursive
    lst = tmp_path / "list.txt"
    lst.write_text(f"in/a.PNG in/hq_a.png 3\n\n# comment\n{d / 'b.png'}\n")
    assert imageio.list_inputs(str(lst)) == [str(tmp_path / "in" / "a.PNG"), str(d / "b.png")]


def test_prefetcher_order_and_errors(tmp_path):
    rng = np.random.default_rng(1)
    arrs = [rng.integers(0, 256, (8 + i, 9, 3), dtype=np.uint8) for i in range(5)]
    paths = [_png(tmp_path / f"{i}.png", a) for i, a in enumerate(arrs)]
    plan = [imageio.Batch(0, (512, 512), (0, 1), 2), imageio.Batch(1, (512, 512), (2, 3), 2), imageio.Batch(2, (512, 512), (4, 4), 1)]
    with imageio.io_pool() as pool:
        got = list(imageio.Prefetcher(plan, paths, pool))
        assert [b for b, _ in got] == plan
        for b, imgs in got:
            assert all(np.array_equal(t.numpy(), arrs[i]) for i, t in zip(b.members, imgs))
        with pytest.raises(FileNotFoundError):
            list(imageio.Prefetcher(plan, paths[:4] + [str(tmp_path / "gone.png")], pool))
    assert imageio.IO_THREADS <= 4


def test_restore_argument_errors_need_no_gpu(tmp_path):
    src, out, empty = tmp_path / "in", tmp_path / "out", tmp_path / "empty"
    src.mkdir(), empty.mkdir()
    _png(src / "a.png", np.zeros((8, 8, 3), np.uint8))
    r = cli.resolve(_cfg())
    ok = dict(inp=str(src), output=str(out))
    paths, which = cli.check_restore_args(r, **ok)
    assert paths == [str(src / "a.png")] and which == "ir"
    assert cli.check_restore_args(r, **ok, tasks="seg,ir")[1] == ("seg", "ir")
    cases = [(dict(ok, inp=str(tmp_path / "nowhere")), FileNotFoundError, "--input"),
             (dict(ok, inp=None), FileNotFoundError, "--input"),
             (dict(ok, inp=str(empty)), ValueError, "--input"),
             (dict(ok, task="deblur"), KeyError, "--task"),
             (dict(ok, tasks="ir,deblur"), KeyError, "--tasks"),
             (dict(ok, tasks="ir,ir"), ValueError, "--tasks"),
             (dict(ok, task="ir", tasks="ir,seg"), ValueError, "--task and --tasks"),
             (dict(ok, output=str(src)), ValueError, "--output"),
             (dict(ok, output=None), ValueError, "--output"),
             (dict(ok, batch=0), ValueError, "--batch")]
    for kw, exc, word in cases:
        with pytest.raises(exc) as e:
            cli.check_restore_args(r, **kw)
        assert word in str(e.value), (kw, str(e.value))
    _png(src / "a.jpg", np.zeros((8, 8, 3), np.uint8))                         # a.png and a.jpg: both would become a.png
    with pytest.raises(ValueError) as e:
        cli.check_restore_args(r, **ok)
    assert "--input" in str(e.value) and "a.png" in str(e.value)
    # the command itself raises the same before it looks for a GPU
    with pytest.raises(ValueError) as e:
        cli.restore(_cfg(), str(src), str(out), task="ir", tasks="ir,seg")
    assert "--task and --tasks" in str(e.value)
    with pytest.raises(FileNotFoundError):
        cli.main(["restore", "--config", _write_cfg(tmp_path), "--input", str(tmp_path / "nowhere"), "--output", str(out)])
    assert not out.exists()


def _write_cfg(tmp_path):
    import yaml
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(_cfg()))
    return str(p)


def test_restore_noise_depends_on_seed_and_index_only():
    a, b = cli.restore_noise(7, 3, 2, (640, 512))
    assert tuple(a.shape) == tuple(b.shape) == (2, 4, 80, 64) and not torch.equal(a, b)
    a2, b2 = cli.restore_noise(7, 3, 2, (640, 512))
    assert torch.equal(a, a2) and torch.equal(b, b2)
    assert not torch.equal(a, cli.restore_noise(7, 4, 2, (640, 512))[0]) and not torch.equal(a, cli.restore_noise(8, 3, 2, (640, 512))[0])


def test_image_list_files(tmp_path):
    from unirestore_amd.data import ImageListFiles, SyntheticImages
    rng = np.random.default_rng(9)
    shapes = [(40, 56), (32, 32), (40, 56)]
    lines = []
    for i, (h, w) in enumerate(shapes):
        for kind in ("lq", "hq"):
            _png(tmp_path / f"{kind}_{i}.png", rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        lines.append(f"lq_{i}.png hq_{i}.png {i}")
    (tmp_path / "val.txt").write_text("\n".join(lines) + "\n")
    ds = ImageListFiles(str(tmp_path / "val.txt"), batch_size=2)
    got = list(ds.batches())
    assert len(ds) == len(got) == 2
    (lq, hq, gt, names, task), second = got
    assert lq.dtype == hq.dtype == torch.float32 and tuple(lq.shape) == tuple(hq.shape) == (2, 3, 40, 56)
    assert gt is None and names == ["lq_0", "lq_2"] and task == "ir"
    assert tuple(second[0].shape) == (1, 3, 32, 32) and second[3] == ["lq_1"]
    want = torch.from_numpy(np.array(Image.open(tmp_path / "hq_2.png"))).permute(2, 0, 1).float() / 255
    assert torch.equal(hq[1], want) and 0 <= float(lq.min()) and float(lq.max()) <= 1
    with pytest.raises(ValueError):
        next(ds.batches(0, 2))
    r = cli.resolve(_cfg(data=dict(class_path="unirestore_amd.data.ImageListFiles",
                                   init_args=dict(list_file=str(tmp_path / "val.txt"), batch_size=2))))
    assert r["data_class"] == "unirestore_amd.data.ImageListFiles" and ImageListFiles(**r["data_args"]).batch_size == 2
    r = cli.resolve(_cfg(data=dict(class_path="data.DatasetEngine", init_args=dict(task="ir", val=dict(batch_size=3)))))
    assert r["data_class"] == "unirestore_amd.data.SyntheticImages" and SyntheticImages(**r["data_args"]).batch_size == 3


def test_new_symbols_are_declared():
    from unirestore_amd import capi
    assert {"ur_image_u8_ingest", "ur_image_u8_egress"} <= set(capi.SIGNATURES) and capi.lib.ur_version() >= 101
    # arguments are checked before any HIP call: these return UR_E_INVALID on a machine without a GPU as well
    assert capi.lib.ur_image_u8_ingest(None, 12, None, None, 1, 2, 2, 8, 2.0, -1.0, 0, None) == capi.UR_E_INVALID
    assert "ur_image_u8_ingest" in capi.lib.ur_last_error().decode()
    assert capi.lib.ur_image_u8_ingest(1, 11, 1, 1, 1, 2, 2, 8, 2.0, -1.0, 0, None) == capi.UR_E_INVALID       # slot < canvas
    assert "slot_bytes" in capi.lib.ur_last_error().decode()
    assert capi.lib.ur_image_u8_egress(1, 1, 1, 12, 1, 1, 0, 3, 2, 2, 8, 0.5, 0.5, 0, None) == capi.UR_E_INVALID  # N = 0
    assert capi.lib.ur_image_u8_egress(1, 1, 1, 12, 1, 1, 1, 3, 2, 2, 8, 0.5, 0.5, 7, None) == capi.UR_E_INVALID  # dtype
    assert capi.lib.ur_image_u8_egress(1, 1, 1, 12, 1, None, 1, 3, 2, 2, 8, 0.5, 0.5, 0, None) == capi.UR_E_INVALID  # no flags
