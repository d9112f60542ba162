"""The resize kernels (csrc/resize.hip) against the numpy restatement of resize_reference.py, byte for byte, and the layers above them
(ops.resize_u8, resize.resize_u8, resize.around, corrupt.degrade, distort.degrade, jpeg.degrade, the two datasets, cli.validate, cli corrupt / jpeg).
The cases are resize_cases.py; test_resize_cpu.py holds the restatement against torch's CPU kernel.  Every launch goes through the C
ABI on guarded buffers: guards, the input and the tables untouched, and a second launch into a dirtied output and a dirtied
workspace bit-identical (nothing in the workspace is read before it is written)."""
import json
import os

import numpy as np
import pytest
import torch

import resize_cases as cases
import resize_reference as ref
from test_boundary_launchers_gpu import Buf

pytestmark = pytest.mark.gpu

_REF = {}                       # (shape, kind, size, mode) -> the restatement's bytes: computed once, shared, read-only


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    return c


def _stream():
    return torch.cuda.current_stream().cuda_stream


def reference(shape, kind, size, mode):
    key = (shape, kind, size, mode)
    if key not in _REF:
        _REF[key] = ref.resize(cases.images(shape, kind), size, mode)
        _REF[key].setflags(write=False)
    return _REF[key]


def _table(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    b = Buf(tuple(t.shape), t.dtype, fill=t.cuda())
    b.orig = t
    return b


def launch(capi, x, size, mode, dirt=None, stream=None):
    """ur_resize_u8 of the host u8 batch x on guarded buffers, the tables from the RESTATEMENT (not from the planner under test);
    dirt: a byte to fill the output and the workspace with first.  -> (out on the host, input and tables untouched and all guards
    intact)."""
    n, h, w, _ = x.shape
    oh, ow = size
    xb, xw, xk, xp = ref.axis_tables(w, ow, mode)
    yb, yw, yk, yp = ref.axis_tables(h, oh, mode)
    ins = [_table(x.numpy()), _table(xb), _table(xw), _table(yb), _table(yw)]
    out = Buf((n, oh, ow, 3), torch.uint8)
    nbytes = capi.lib.ur_resize_u8_ws_bytes(n, h, w, oh, ow)
    assert nbytes >= n * h * ow * 3 and nbytes % 8 == 0
    ws = Buf((nbytes,), torch.uint8)                 # (64 guard bytes in front: still 8-byte aligned)
    if dirt is not None:
        out.t.fill_(dirt)
        ws.t.fill_(dirt)
    torch.cuda.synchronize()
    rc = capi.lib.ur_resize_u8(ins[0].ptr, out.ptr, n, h, w, oh, ow, ins[1].ptr, ins[2].ptr, xk, xp, ins[3].ptr, ins[4].ptr, yk, yp, ws.ptr, nbytes,
                               _stream() if stream is None else stream)
    assert rc == 0, (x.shape, size, mode, capi.lib.ur_last_error())
    torch.cuda.synchronize()
    ok = all(b.guards_ok() for b in ins + [out, ws]) and all(torch.equal(b.t.cpu().view(torch.uint8), b.orig.view(torch.uint8)) for b in ins)
    return out.t.cpu(), ok


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: "%dx%dx%d-%dx%d" % (c[0] + c[1]))
@pytest.mark.parametrize("mode", cases.MODES)
def test_equals_the_restatement_in_every_byte(capi, mode, case):
    shape, size = case
    for kind in cases.KINDS:
        what = (shape, size, kind, mode)
        x = torch.from_numpy(cases.images(shape, kind))
        got, ok = launch(capi, x, size, mode)
        again, ok2 = launch(capi, x, size, mode, dirt=0x5A)
        assert ok and ok2, what
        want = reference(shape, kind, size, mode)
        assert tuple(got.shape) == want.shape, what
        wrong = int((got.numpy() != want).sum())
        print(f"{what}: {wrong} of {want.size} bytes differ from the restatement")
        assert wrong == 0, (what, wrong, int(np.abs(got.numpy().astype(int) - want).max()))
        assert torch.equal(got, again), what
        if ref.torch_cpu_exact():
            assert np.array_equal(got.numpy(), ref.torch_resize(x.numpy(), size, mode)), what
    if size == shape[1:]:
        assert torch.equal(got, x)                   # both passes skipped: a copy


def test_an_image_alone_equals_itself_in_a_batch(capi):
    x = torch.from_numpy(cases.images((3, 45, 37)))
    assert not torch.equal(x[0], x[1]) and not torch.equal(x[1], x[2])
    for mode in cases.MODES:
        for size in ((29, 50), (45, 20), (60, 37)):
            batch, ok = launch(capi, x, size, mode)
            assert ok
            for i in range(3):
                alone, ok2 = launch(capi, x[i:i + 1].contiguous(), size, mode)
                assert ok2 and torch.equal(batch[i:i + 1], alone), (mode, size, i)


def test_wrapper_planner_and_stream_equal_the_raw_call(capi):
    from unirestore_amd import ops
    from unirestore_amd import resize as rz
    x = torch.from_numpy(cases.images((2, 40, 52)))
    dev = x.cuda()
    side = torch.cuda.Stream()
    for mode in cases.MODES:
        for size in ((17, 31), (40, 31), (17, 52), (40, 52), (80, 104), (33, 60)):
            raw, ok = launch(capi, x, size, mode)
            assert ok
            got = rz.resize_u8(dev, size, mode)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (2, *size, 3) and got.is_contiguous() and torch.equal(got.cpu(), raw), (mode, size)
            axes = [tuple(torch.from_numpy(t).cuda() if isinstance(t, np.ndarray) else t for t in rz.axis_tables(a, b, mode))
                    for a, b in ((52, size[1]), (40, size[0]))]
            into = torch.full((2, *size, 3), 9, dtype=torch.uint8, device="cuda")
            assert ops.resize_u8(dev, size, *axes, out=into) is into and torch.equal(into.cpu(), raw), (mode, size)
            with torch.cuda.stream(side):            # the wrapper launches on the current stream
                on_side = rz.resize_u8(dev, size, mode)
            side.synchronize()
            assert torch.equal(on_side.cpu(), raw), (mode, size)
    assert torch.equal(rz.resize_u8(dev, (17, 31)).cpu(), launch(capi, x, (17, 31), "bilinear")[0])          # bilinear is the default
    axes = [tuple(torch.from_numpy(t).cuda() if isinstance(t, np.ndarray) else t for t in rz.axis_tables(a, b)) for a, b in ((52, 31), (40, 17))]
    with pytest.raises(ValueError, match="out"):
        ops.resize_u8(dev, (17, 31), *axes, out=torch.zeros(2, 17, 31, 3, device="cuda"))
    with pytest.raises(ValueError, match="bounds"):
        ops.resize_u8(dev, (17, 31), axes[1], axes[0])                                                        # the axes swapped
    with pytest.raises(ValueError, match="weights"):
        ops.resize_u8(dev, (17, 31), (axes[0][0], axes[0][1].cpu(), *axes[0][2:]), axes[1])
    with pytest.raises(ValueError, match="p must"):
        ops.resize_u8(dev, (17, 31), (*axes[0][:3], 23), axes[1])
    with pytest.raises(ValueError, match="K must"):
        ops.resize_u8(dev, (17, 31), axes[0], (*axes[1][:2], 0, axes[1][3]))
    with pytest.raises(ValueError, match="size"):
        rz.resize_u8(dev, (1, 31))
    with pytest.raises(ValueError, match=">= 2"):
        rz.resize_u8(torch.zeros(1, 1, 40, 3, dtype=torch.uint8, device="cuda"), (20, 20))


def _hand(x, sizes, inner, mode="bilinear"):
    """The wrapper by hand: the restatement down, `inner` (device u8 batch of one -> device u8) at that size, the restatement back."""
    n, h, w, _ = x.shape
    out = []
    for i in range(n):
        small = torch.from_numpy(ref.resize(x[i:i + 1].numpy(), sizes[i], mode)).cuda()
        out.append(ref.resize(inner(small, i).cpu().numpy(), (h, w), mode))
    return torch.from_numpy(np.concatenate(out))


def test_around_groups_by_size_in_input_order():
    from unirestore_amd import resize as rz
    x = torch.from_numpy(cases.images((5, 40, 52)))
    sizes = [(20, 26), (33, 43), (20, 26), (40, 52), (33, 43)]
    calls = []

    def fn(batch, idx):
        calls.append((tuple(batch.shape), list(idx)))
        return 255 - batch
    got = rz.around(x.cuda(), sizes, fn)
    assert calls == [((2, 20, 26, 3), [0, 2]), ((2, 33, 43, 3), [1, 4]), ((1, 40, 52, 3), [3])]
    assert got.dtype == torch.uint8 and got.shape == x.shape and torch.equal(got.cpu(), _hand(x, sizes, lambda s, i: 255 - s))
    assert torch.equal(got[3].cpu(), 255 - x[3])                                     # its size is the input's: two copies around fn
    with pytest.raises(ValueError, match="sizes"):
        rz.around(x.cuda(), sizes[:4], fn)
    with pytest.raises(ValueError, match="fn must return"):
        rz.around(x.cuda(), sizes, lambda b, i: b.float())


@pytest.mark.parametrize("name", ("contrast", "pixelate", "gaussian_blur", "gaussian_noise"))
def test_degrade_equals_the_composition_by_hand(name):
    """Both sides run the same corruption kernel on the same bytes: equal, not close."""
    from unirestore_amd import corrupt as cr
    from unirestore_amd import resize as rz
    x = torch.from_numpy(cases.images((3, 96, 128)))
    dev = x.cuda()
    seeds, stems = [5, 6, 7], ["p", "q", "r"]
    assert torch.equal(cr.degrade(dev, name, 3, seeds, stems), cr.corrupt(dev, name, 3, seeds, stems))            # resize=None: corrupt itself
    assert torch.equal(cr.degrade(dev, name, 3, 9), cr.corrupt(dev, name, 3, 9))
    edges = [rz.draw_short_edge(s, t, 32, 96) for s, t in zip(seeds, stems)]
    sizes = [ref.short_edge_size(96, 128, e) for e in edges]
    assert all(32 <= e < 96 for e in edges) and len(set(edges)) > 1, edges
    for sev in (2, 5):
        got = cr.degrade(dev, name, sev, seeds, stems, resize=(32, 96))
        want = _hand(x, sizes, lambda small, i: cr.corrupt(small, name, sev, seeds[i:i + 1], stems[i:i + 1]))
        assert got.dtype == torch.uint8 and got.shape == dev.shape and got.is_contiguous()
        assert torch.equal(got.cpu(), want), (name, sev, int((got.cpu() != want).sum()))
        assert not torch.equal(got, cr.corrupt(dev, name, sev, seeds, stems))                                     # the wrapper changes the result
        alone = cr.degrade(dev[2:3].contiguous(), name, sev, seeds[2:], stems[2:], resize=(32, 96))               # alone = inside the batch
        assert torch.equal(alone, got[2:3]), (name, sev)
    assert torch.equal(cr.degrade(dev, "clean", 3, seeds, stems, resize=(32, 96)), dev)


def test_jpeg_degrade_equals_the_composition_by_hand():
    from unirestore_amd import jpeg
    from unirestore_amd import resize as rz
    x = torch.from_numpy(cases.images((3, 96, 128)))
    dev = x.cuda()
    seeds, stems = [5, 6, 7], ["p", "q", "r"]
    assert torch.equal(jpeg.degrade(dev, 25, seeds, stems, None), jpeg.roundtrip(dev, 25))
    sizes = [ref.short_edge_size(96, 128, rz.draw_short_edge(s, t, 16, 96)) for s, t in zip(seeds, stems)]
    got = jpeg.degrade(dev, 25, seeds, stems, (16, 96))
    want = _hand(x, sizes, lambda small, i: jpeg.roundtrip(small, 25))
    assert got.shape == dev.shape and torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    assert torch.equal(jpeg.degrade(dev[1:2].contiguous(), "25", seeds[1:2], stems[1:2], (16, 96), "4:2:0"), got[1:2])
    assert not torch.equal(jpeg.degrade(dev, 25, seeds, stems, (16, 96), "4:4:4"), got)


@pytest.mark.parametrize("name", ("glass_blur", "snow", "elastic_transform"))
def test_distort_degrade_equals_the_composition_by_hand(name):
    """Both sides run the same resize and distortion kernels on the same bytes: equal, not close.  40 x 32 with [32, 40) is the
    smallest shape with all three situations in one batch: a draw equal to the short side (both resizes are copies), a draw above
    it (a real resize: 32 is the smallest side distort takes, so it enlarges), and groups of different resized shapes."""
    from unirestore_amd import distort as ds
    from unirestore_amd import resize as rz
    dev = torch.randint(0, 256, (3, 40, 32, 3), generator=torch.Generator().manual_seed(31), dtype=torch.uint8).cuda()
    seeds, stems = [5, 6, 7], ["p", "q", "r"]                                        # these draw the short edges 38, 39 and 32
    edges = [rz.draw_short_edge(s, t, 32, 40) for s, t in zip(seeds, stems)]
    assert edges[2] == 32 and len(set(edges)) == 3, edges
    got = ds.degrade(dev, name, 3, seeds, stems, resize=(32, 40))
    want = []
    for i, e in enumerate(edges):
        small = rz.resize_u8(dev[i:i + 1].contiguous(), rz.short_edge_size(40, 32, e))
        assert (e > 32) == (small.shape != dev[i:i + 1].shape)
        want.append(rz.resize_u8(ds.distort(small, name, 3, seeds[i:i + 1], stems[i:i + 1]), (40, 32)))
    want = torch.cat(want)
    assert got.dtype == torch.uint8 and got.shape == dev.shape and got.is_contiguous()
    assert torch.equal(got, want), (name, int((got != want).sum()))
    assert torch.equal(got[2:3], ds.distort(dev[2:3].contiguous(), name, 3, seeds[2:], stems[2:]))   # the copies change nothing
    assert torch.equal(ds.degrade(dev, name, 3, seeds, stems), ds.distort(dev, name, 3, seeds, stems))   # resize=None: distort itself


SIZES = [("a0", (96, 128)), ("a1", (64, 80)), ("b0", (96, 128)), ("a2", (64, 80)), ("a3", (96, 128))]


def _folder(path, entries=SIZES):
    from unirestore_amd import imageio
    path.mkdir()
    for stem, hw in entries:
        g = torch.Generator().manual_seed(100 + sum(map(ord, stem)))
        imageio.save_u8(torch.randint(0, 256, (*hw, 3), generator=g, dtype=torch.uint8), str(path / f"{stem}.png"))
    return path


def test_datasets_yield_lq_of_hq_s_shape(tmp_path):
    from unirestore_amd import corrupt as cr
    from unirestore_amd import data, imageio, jpeg
    src = _folder(tmp_path / "clean")
    d = data.CorruptedImageFiles(str(src), corruptions="contrast,gaussian_noise,clean", severity="mixed", batch_size=2, seed=11, resize=[32, 64])
    seen = []
    for lq, hq, gt, names, task in d.batches(device="cuda"):
        name, sev = d.last
        assert d.resize == (32, 64) and lq.shape == hq.shape and lq.dtype == torch.float32 and lq.is_contiguous()
        u8 = torch.stack([imageio.load_u8(str(src / f"{st}.png")) for st in names]).cuda()
        assert torch.equal(lq.cpu(), cr.degrade(u8, name, sev, 11, names, resize=(32, 64)).cpu().permute(0, 3, 1, 2).float().div(255))
        assert name == "clean" or not torch.equal(lq.cpu(), cr.corrupt(u8, name, sev, 11, names).cpu().permute(0, 3, 1, 2).float().div(255))
        seen += names
    assert sorted(seen) == sorted(st for st, _ in SIZES)
    j = data.JpegImageFiles(str(src), quality=25, batch_size=3, resize=[16, 64], seed=11)
    for lq, hq, gt, names, task in j.batches(device="cuda"):
        u8 = torch.stack([imageio.load_u8(str(src / f"{st}.png")) for st in names]).cuda()
        assert j.last == ("jpeg", 25) and lq.shape == hq.shape
        assert torch.equal(lq.cpu(), jpeg.degrade(u8, 25, 11, names, (16, 64)).cpu().permute(0, 3, 1, 2).float().div(255))


def test_validate_reports_resize(tmp_path):
    from restore_worker import tiny_cfg, tiny_model
    from unirestore_amd import cli
    src = _folder(tmp_path / "clean", [(f"v{i}", (64, 64)) for i in range(4)])
    cfg = tiny_cfg()
    cfg["data"] = dict(class_path="unirestore_amd.data.CorruptedImageFiles",
                       init_args=dict(source=str(src), corruptions="contrast,pixelate", severity=3, batch_size=2, seed=3, resize=[32, 64]))
    res = cli.validate(cfg, model=tiny_model())
    print("validate:", json.dumps(res))
    assert res["resize"] == [32, 64] and res["images"] == 4 == sum(v["images"] for v in res["by_corruption"].values()) and res["output_finite"]
    cfg["data"]["init_args"].pop("resize")
    assert "resize" not in cli.validate(cfg, model=tiny_model())
    cfg["data"] = dict(class_path="unirestore_amd.data.JpegImageFiles", init_args=dict(source=str(src), quality=[10], batch_size=2, resize=[16, 64]))
    assert cli.validate(cfg, model=tiny_model())["resize"] == [16, 64]


def _read(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def test_cli_files_depend_on_the_file_alone(tmp_path, capsys):
    from unirestore_amd import cli, imageio
    from unirestore_amd import corrupt as cr
    from unirestore_amd import jpeg
    entries = [("X", (96, 128)), ("Y", (96, 128)), ("Z", (96, 128))]
    src = _folder(tmp_path / "xyz", entries)
    which = "contrast,gaussian_noise"
    r1 = cli.corrupt_files(str(src), str(tmp_path / "o1"), which, 3, seed=9, batch=1, resize="32,96")
    r3 = cli.corrupt_files(str(src), str(tmp_path / "o3"), which, 3, seed=9, batch=3, resize=(32, 96))
    plain = cli.corrupt_files(str(src), str(tmp_path / "o0"), which, 3, seed=9, batch=3)
    assert r1["resize"] == r3["resize"] == [32, 96] and "resize" not in plain
    assert r1["folders"] == plain["folders"] == ["contrast_3", "gaussian_noise_3"]              # folder names and pairs.txt: unchanged
    for f in r1["folders"]:
        a, b, c = _read(tmp_path / "o1" / f), _read(tmp_path / "o3" / f), _read(tmp_path / "o0" / f)
        assert sorted(a) == sorted(c) == ["X.png", "Y.png", "Z.png", "pairs.txt"] and a == b and a["pairs.txt"] == c["pairs.txt"]
        assert all(a[k] != c[k] for k in a if k.endswith(".png")), f
        for stem in "XYZ":
            clean = imageio.load_u8(str(src / f"{stem}.png"))[None].cuda()
            want = cr.degrade(clean, f.rsplit("_", 1)[0], 3, 9, [stem], resize=(32, 96))[0].cpu()
            assert torch.equal(imageio.load_u8(str(tmp_path / "o1" / f / f"{stem}.png")), want), (f, stem)
    assert cli.main(["corrupt", "--input", str(src), "--output", str(tmp_path / "o4"), "--corruptions", "contrast", "--seed", "9", "--batch", "2",
                     "--resize", "32,96"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["resize"] == [32, 96] and line["folders"] == ["contrast_3"]
    assert _read(tmp_path / "o4" / "contrast_3") == _read(tmp_path / "o1" / "contrast_3")
    # jpeg
    assert cli.main(["jpeg", "--input", str(src), "--output", str(tmp_path / "j1"), "--quality", "25", "--seed", "9", "--batch", "1", "--resize", "16,96"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["resize"] == [16, 96] and line["seed"] == 9 and line["folders"] == ["jpeg_q25"]
    j3 = cli.jpeg_files(str(src), str(tmp_path / "j3"), "25", batch=3, resize=(16, 96), seed=9)
    assert j3["resize"] == [16, 96] and _read(tmp_path / "j1" / "jpeg_q25") == _read(tmp_path / "j3" / "jpeg_q25")
    assert "resize" not in cli.jpeg_files(str(src), str(tmp_path / "j0"), "25", batch=3)
    clean = imageio.load_u8(str(src / "Y.png"))[None].cuda()
    assert torch.equal(imageio.load_u8(str(tmp_path / "j1" / "jpeg_q25" / "Y.png")), jpeg.degrade(clean, 25, 9, ["Y"], (16, 96))[0].cpu())
