"""CPU-side checks of the antialiased 8-bit resize: the numpy restatement of the specification (resize_reference.py) against torch's
CPU interpolate(uint8, antialias=True) byte for byte on the case list of resize_cases.py, the planner's tables against the
restatement's, known answers of unirestore_amd.resize, and every refusal of the C ABI, of ops.resize_u8, of corrupt.degrade and
jpeg.degrade, of the two datasets and of the two CLI checkers (all before any HIP call)."""
import os

import numpy as np
import pytest
import torch

import resize_cases as cases
import resize_reference as ref
from unirestore_amd import resize as rz

AXES = [(93, 32), (32, 93), (67, 23), (23, 67), (67, 66), (93, 94), (52, 31), (40, 17), (128, 8), (96, 6), (32, 64), (512, 128), (128, 512),
        (512, 511), (37, 50), (45, 29), (52, 52), (2, 2), (2, 7), (300, 2)]


@pytest.mark.skipif(not ref.torch_cpu_exact(), reason="torch's integer uint8 resize needs an AVX2 or AVX512 build; this host reports "
                    + torch.backends.cpu.get_cpu_capability())
@pytest.mark.parametrize("mode", cases.MODES)
def test_restatement_equals_torch_cpu_byte_for_byte(mode):
    """No case may be left out: the cap on differing bytes is zero."""
    wrong, total = [], 0
    todo = [(shape, size, "random") for shape in cases.CPU_SHAPES for size in cases.CPU_SIZES] + \
           [(shape, size, kind) for shape, size in cases.CASES for kind in cases.KINDS]
    for shape, size, kind in todo:
        x = cases.images(shape, kind)
        mine, theirs = ref.resize(x, size, mode), ref.torch_resize(x, size, mode)
        assert mine.shape == theirs.shape == (shape[0], *size, 3)
        total += mine.size
        if not np.array_equal(mine, theirs):
            wrong.append((shape, size, kind, int((mine != theirs).sum())))
    print(f"{mode}: {len(todo)} cases, {total} bytes, {len(wrong)} cases differ from torch")
    assert len(todo) == 36 + 36 and not wrong, wrong[:10]
    # the wrapper's round trip, down and back, at four short edges
    x = cases.images((1, 96, 128))
    for s in (32, 47, 64, 95):
        small = ref.short_edge_size(96, 128, s)
        down = ref.resize(x, small, mode)
        assert np.array_equal(down, ref.torch_resize(x, small, mode)), s
        assert np.array_equal(ref.resize(down, (96, 128), mode), ref.torch_resize(down, (96, 128), mode)), s


def test_the_float_path_is_another_function():
    """Why the integer path is the target: interpolate(float).round() is not the same bytes."""
    if not ref.torch_cpu_exact():
        pytest.skip("needs torch's integer uint8 path (AVX2 / AVX512)")
    import torch.nn.functional as F
    x = cases.images((1, 67, 93))
    f = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2).float(), size=(23, 32), mode="bilinear", antialias=True).round().clamp(0, 255)
    f = f.permute(0, 2, 3, 1).to(torch.uint8).numpy()
    u = ref.resize(x, (23, 32))
    d = np.abs(f.astype(int) - u.astype(int))
    print(f"float path vs uint8 path: {int((d != 0).sum())} of {d.size} bytes differ, max {int(d.max())}")
    assert d.max() == 1 and (d != 0).sum() > 0


@pytest.mark.parametrize("mode", cases.MODES)
def test_axis_tables_equal_the_restatement(mode):
    for n_in, n_out in AXES:
        b, w, k, p = rz.axis_tables(n_in, n_out, mode)
        rb, rw, rk, rp = ref.axis_tables(n_in, n_out, mode)
        assert (k, p) == (rk, rp), (n_in, n_out)
        assert b.dtype == np.int32 and w.dtype == np.int32 and b.shape == (n_out, 2) and w.shape == (n_out, k), (n_in, n_out)
        assert np.array_equal(b, rb) and np.array_equal(w, rw), (n_in, n_out)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 1] <= k).all() and (b[:, 0] + b[:, 1] <= n_in).all(), (n_in, n_out)
        assert all((w[i, b[i, 1]:] == 0).all() for i in range(n_out)), (n_in, n_out)            # nothing beyond xsize
        assert abs(w.sum(1) - (1 << p)).max() <= k, (n_in, n_out)                                # rounded: near 2^p, not always equal
        assert not b.flags.writeable and not w.flags.writeable
    assert rz.axis_tables(93, 32, mode)[0] is rz.axis_tables(93, 32, mode)[0]                   # built once


def test_known_answers():
    # K = ceil(support) * 2 + 1 and the precision p of a few axes: a 16 x reduction, 4 x, a non-integer one, an enlargement, a copy
    pinned = {("bilinear", 128, 8): (33, 18), ("bicubic", 128, 8): (65, 18), ("bilinear", 512, 128): (9, 16), ("bilinear", 93, 32): (7, 16),
              ("bicubic", 93, 32): (13, 16), ("bilinear", 128, 512): (3, 14), ("bicubic", 32, 93): (5, 14), ("bilinear", 52, 52): (3, 14)}
    for (mode, n_in, n_out), kp in pinned.items():
        assert rz.axis_tables(n_in, n_out, mode)[2:] == kp, (mode, n_in, n_out)
    b, w, k, p = rz.axis_tables(52, 52, "bilinear")                                             # equal lengths: the identity
    assert np.array_equal(b[:, 0], np.arange(52)) and (w[:, 0] == 1 << 14).all() and not w[:, 1:].any()
    b, w, k, p = rz.axis_tables(8, 4, "bilinear")                                               # 2 x: (1, 3, 3, 1) / 8 inside
    assert np.array_equal(b[1], (1, 4)) and np.array_equal(w[1, :4] * 8, np.array([1, 3, 3, 1]) << p)
    assert (rz.axis_tables(93, 32, "bicubic")[1] < 0).any() and (rz.axis_tables(93, 32, "bilinear")[1] >= 0).all()
    with pytest.raises(ValueError, match="mode"):
        rz.axis_tables(8, 4, "nearest")
    with pytest.raises(ValueError, match="positive"):
        rz.axis_tables(0, 4, "bilinear")
    # a constant does not always come back constant: the rounded weights of a row need not sum to 2^p
    sums = rz.axis_tables(93, 32, "bicubic")[1].sum(1)
    assert sums.min() < 1 << 16 < sums.max()


def test_short_edge_size():
    for h, w, s, want in ((96, 128, 48, (48, 64)),          # landscape: the height is the short side
                          (128, 96, 48, (64, 48)),          # portrait
                          (80, 80, 33, (33, 33)),           # square: the width counts as the short side
                          (67, 93, 40, (40, 55)),           # 40 * 93 / 67 = 55.52: truncated
                          (93, 67, 40, (55, 40)),
                          (512, 768, 128, (128, 192)), (100, 333, 64, (64, 213)), (96, 128, 200, (200, 266))):
        assert rz.short_edge_size(h, w, s) == want == ref.short_edge_size(h, w, s), (h, w, s)
    try:
        from torchvision.transforms.v2 import functional as TF
    except Exception:
        return
    for h, w, s in ((96, 128, 48), (128, 96, 48), (67, 93, 40), (100, 333, 64), (80, 80, 33)):
        assert tuple(TF.resize(torch.zeros(3, h, w, dtype=torch.uint8), (s,)).shape[-2:]) == rz.short_edge_size(h, w, s), (h, w, s)


def test_draw_short_edge():
    draws = [rz.draw_short_edge(42, f"img{i}", 128, 512) for i in range(1000)]
    assert min(draws) >= 128 and max(draws) < 512 and all(isinstance(d, int) for d in draws)
    assert draws == [rz.draw_short_edge(42, f"img{i}", 128, 512) for i in range(1000)]           # a function of (seed, stem) alone
    assert draws != [rz.draw_short_edge(43, f"img{i}", 128, 512) for i in range(1000)]
    assert rz.draw_short_edge(42, "a", 128, 512) != rz.draw_short_edge(42, "b", 128, 512) or \
        rz.draw_short_edge(42, "a", 128, 512) != rz.draw_short_edge(42, "c", 128, 512)
    # spread over the range: every eighth of it is hit about 125 times (binomial sd 10.5: 70..180 is beyond 5 sd), both ends reached
    hist = np.histogram(draws, bins=8, range=(128, 512))[0]
    assert hist.min() >= 70 and hist.max() <= 180, hist
    assert min(draws) < 140 and max(draws) >= 500 and len(set(draws)) > 300
    assert {rz.draw_short_edge(1, f"s{i}", 32, 34) for i in range(64)} == {32, 33}
    assert rz.draw_short_edge(1, "s", 32, 33) == 32
    with pytest.raises(ValueError, match="empty"):
        rz.draw_short_edge(1, "s", 32, 32)
    from unirestore_amd import corrupt as cr
    assert rz.draw_short_edge(42, "a", 0, 1 << 20) != cr.draw_severity(42, "a") and cr.corruption_seed(42, "a") == cr.corruption_seed(42, "a")


def test_check_range():
    assert rz.check_range((128, 512), 32) == (128, 512) and rz.check_range([32, 33], 32) == (32, 33) and rz.check_range("128,512", 32) == (128, 512)
    assert rz.check_range(" 40 , 96 ", 32) == (40, 96) and rz.check_range((np.int64(40), 96), 32) == (40, 96)
    for bad in ("128", "128,", "a,b", "128,512,600", "12.5,40", "-3,40", 128, (128,), (128, 512, 600), (128.0, 512), (True, 512), None):
        with pytest.raises(ValueError, match="two integers"):
            rz.check_range(bad, 32)
    for bad in ((64, 64), (96, 32), "64,64"):
        with pytest.raises(ValueError, match="below hi"):
            rz.check_range(bad, 32)
    with pytest.raises(ValueError, match=">= 32"):
        rz.check_range((31, 96), 32)
    with pytest.raises(ValueError, match=">= 16"):
        rz.check_range("15,96", 16)


def test_per_image_and_the_sizes_the_wrapper_draws():
    assert rz.per_image("who", 3, 7, None) == ([7, 7, 7], ["", "", ""])
    assert rz.per_image("who", 2, np.int64(7), ("a", "b")) == ([7, 7], ["a", "b"])
    seeds, stems = [5, 6, 7], ["p", "q", "r"]
    assert rz.per_image("who", 3, seeds, stems) == (seeds, stems) and rz.per_image("who", 3, iter(seeds), iter(stems)) == (seeds, stems)
    for bad in ((3, [5, 6], stems), (3, seeds, ["p", "q"]), (2, seeds, None), (3, 5, ["p"]), (1, [], None)):
        with pytest.raises(ValueError, match=r"jpeg\.degrade: \d images but \d seeds and \d stems"):
            rz.per_image("jpeg.degrade", *bad)
    # what `inside` hands to `around`: every image's own draw, whatever the batch around it
    for h, w in ((40, 32), (32, 48)):
        sizes = rz.drawn_sizes(h, w, seeds, stems, 32, 40)
        assert sizes == [rz.short_edge_size(h, w, rz.draw_short_edge(s, t, 32, 40)) for s, t in zip(seeds, stems)]
        assert all(min(s) == rz.draw_short_edge(sd, st, 32, 40) for s, sd, st in zip(sizes, seeds, stems)) and len(set(sizes)) == 3
        assert rz.drawn_sizes(h, w, seeds[1:2], stems[1:2], 32, 40) == sizes[1:2]
    assert rz.drawn_sizes(40, 32, seeds, stems, 32, 40)[2] == (40, 32)                            # a draw of the short side: no resize


def test_c_abi_refuses_wrong_arguments_before_the_gpu():
    from unirestore_amd import capi
    size = capi.lib.ur_resize_u8_ws_bytes
    rows = cases.refusals(size)
    labels = [label for label, _ in rows]
    for must in ("null x", "null out", "null workspace", "null width bounds", "null width weights", "null height bounds", "null height weights",
                 "N = 0", "H = 1", "W = 1", "oh = 1", "ow = 1", "width K = 0", "height K = 0", "width p = 0", "height p = 23",
                 "workspace one byte short", "out == x"):
        assert must in labels, must
    for label, args in rows:
        assert capi.lib.ur_resize_u8(*args) == capi.UR_E_INVALID, label
        assert b"ur_resize_u8" in capi.lib.ur_last_error(), (label, capi.lib.ur_last_error())
    # the intermediate [N, H, ow, 3], rounded up to 8 bytes
    assert size(2, 67, 93, 23, 32) == 2 * 67 * 32 * 3 and size(1, 23, 32, 67, 93) == (23 * 93 * 3 + 7) // 8 * 8 and size(1, 2, 2, 2, 2) == 16
    assert size(0, 8, 8, 8, 8) == 0 and size(1, -1, 8, 8, 8) == 0 and size(1, 8, 0, 8, 8) == 0 and size(1, 8, 8, 0, 8) == 0 and size(1, 8, 8, 8, -2) == 0


def test_python_layers_refuse_wrong_arguments():
    from unirestore_amd import corrupt as cr
    from unirestore_amd import jpeg, ops
    u8 = torch.zeros(1, 40, 52, 3, dtype=torch.uint8)
    for bad in (torch.zeros(1, 40, 52, 3), torch.zeros(40, 52, 3, dtype=torch.uint8), torch.zeros(1, 40, 52, 4, dtype=torch.uint8), None):
        with pytest.raises(ValueError, match="uint8"):
            rz.resize_u8(bad, (20, 26))
        with pytest.raises(ValueError, match="uint8"):
            ops.resize_u8(bad, (20, 26), None, None)
        with pytest.raises(ValueError, match="uint8"):
            rz.around(bad, [(20, 26)], lambda b, i: b)
    for bad in ((1, 26), (20, 1), (20,), 20, (20.0, 26), (True, 26), None, (0, 0)):
        with pytest.raises(ValueError, match="size"):
            rz.resize_u8(u8, bad)
    with pytest.raises(ValueError, match="mode"):
        rz.resize_u8(u8, (20, 26), "nearest")
    # corrupt.degrade / jpeg.degrade: the range is checked before the images are looked at
    for bad, what in (((31, 96), ">= 32"), ((96, 96), "below hi"), ((128,), "two integers"), ("128", "two integers"), (128, "two integers")):
        with pytest.raises(ValueError, match=what):
            cr.degrade(u8, "contrast", 3, 42, ["a"], resize=bad)
    for bad, what in (((15, 96), ">= 16"), ((96, 40), "below hi"), ((40, 96, 3), "two integers")):
        with pytest.raises(ValueError, match=what):
            jpeg.degrade(u8, 50, 42, ["a"], bad)
    with pytest.raises(NotImplementedError, match="snow"):
        cr.degrade(u8, "snow", 3, 42, ["a"], resize=(32, 96))
    with pytest.raises(ValueError, match="unknown corruption"):
        cr.degrade(u8, "sleet", 3, 42, ["a"], resize=(32, 96))
    with pytest.raises(ValueError, match="severity"):
        cr.degrade(u8, "contrast", 6, 42, ["a"], resize=(32, 96))
    with pytest.raises(ValueError, match="quality"):
        jpeg.degrade(u8, 0, 42, ["a"], (16, 96))
    with pytest.raises(ValueError, match="subsampling"):
        jpeg.degrade(u8, 50, 42, ["a"], (16, 96), "4:2:2")
    with pytest.raises(ValueError, match="uint8"):
        cr.degrade(u8.float(), "contrast", 3, 42, ["a"], resize=(32, 96))
    with pytest.raises(ValueError, match="uint8"):
        jpeg.degrade(u8.float(), 50, 42, ["a"], (16, 96))


def _png(path, shape=(32, 40), seed=0):
    from PIL import Image
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (*shape, 3), dtype=np.uint8)).save(path)


def test_datasets_take_resize_last_and_check_it(tmp_path):
    import inspect

    from unirestore_amd import cli, data
    src = tmp_path / "clean"
    src.mkdir()
    for i in range(3):
        _png(src / f"im{i}.png", seed=i)
    assert list(inspect.signature(data.CorruptedImageFiles.__init__).parameters)[-1] == "resize"
    assert list(inspect.signature(data.JpegImageFiles.__init__).parameters)[-2:] == ["resize", "seed"]
    assert data.CorruptedImageFiles(str(src), "fog").resize is None and data.JpegImageFiles(str(src)).resize is None
    d = data.CorruptedImageFiles(str(src), "fog", resize=[128, 512])
    assert d.resize == (128, 512) and d.last is None and len(d) == 1
    j = data.JpegImageFiles(str(src), quality=10, resize=(16, 64), seed=7)
    assert j.resize == (16, 64) and j.seed == 7 and data.JpegImageFiles(str(src)).seed == 42
    for bad, what in (((31, 96), ">= 32"), ((96, 96), "below hi"), ([128], "two integers"), (128, "two integers")):
        with pytest.raises(ValueError, match=what):
            data.CorruptedImageFiles(str(src), "fog", resize=bad)
    for bad, what in (((15, 96), ">= 16"), ((96, 20), "below hi"), ("x", "two integers")):
        with pytest.raises(ValueError, match=what):
            data.JpegImageFiles(str(src), resize=bad)
    cfg = dict(model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=dict(cnet=dict(num_inference_steps=1)))),
               data=dict(class_path="unirestore_amd.data.CorruptedImageFiles", init_args=dict(source=str(src), resize=[128, 512])))
    assert cli.resolve(cfg)["data_args"]["resize"] == [128, 512]


def test_cli_resize_argument_errors(tmp_path, capsys):
    import inspect

    from unirestore_amd import cli
    src = tmp_path / "clean"
    src.mkdir()
    _png(src / "a.png")
    out = str(tmp_path / "out")
    for fn in (cli.check_corrupt_args, cli.corrupt_files, cli.check_jpeg_args):
        assert list(inspect.signature(fn).parameters)[-1] == "resize", fn
    assert list(inspect.signature(cli.jpeg_files).parameters)[-2:] == ["resize", "seed"]
    # what the checkers return is what it was
    assert cli.check_corrupt_args(str(src), out, "fog", resize="32,96") == cli.check_corrupt_args(str(src), out, "fog")
    assert cli.check_jpeg_args(str(src), out, "10", resize="16,96") == cli.check_jpeg_args(str(src), out, "10")
    assert cli.check_corrupt_args(str(src), out, "fog", resize=(128, 512))[1] == ["fog"]
    for bad, what in (("128", "two integers"), ("a,b", "two integers"), ("128,512,9", "two integers"), ("96,96", "below hi"), ("512,128", "below hi"),
                      ("31,96", ">= 32")):
        with pytest.raises(ValueError, match="--resize") as e:
            cli.check_corrupt_args(str(src), out, "fog", resize=bad)
        assert what in str(e.value), (bad, str(e.value))
    for bad, what in (("40", "two integers"), ("40,40", "below hi"), ("15,96", ">= 16")):
        with pytest.raises(ValueError, match="--resize") as e:
            cli.check_jpeg_args(str(src), out, "10", resize=bad)
        assert what in str(e.value), (bad, str(e.value))
    assert cli.check_jpeg_args(str(src), out, "10", resize="16,32")[1] == [10]                   # 16 is enough for the JPEG round trip
    # refused before a GPU is looked for
    for argv in (["corrupt", "--input", str(src), "--output", out, "--corruptions", "fog", "--resize", "31,96"],
                 ["corrupt", "--input", str(src), "--output", out, "--corruptions", "fog", "--resize", "96"],
                 ["jpeg", "--input", str(src), "--output", out, "--quality", "10", "--resize", "64,32"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
        assert "--resize" in capsys.readouterr().err
    assert not os.path.exists(out)


def test_the_modules_around_it_are_what_they_were():
    from unirestore_amd import corrupt as cr
    from unirestore_amd import jpeg
    assert len(cr.NAMES) == 13 and cr.UNBUILT == ("glass_blur", "snow", "frost", "spatter", "elastic_transform", "jpeg_compression")
    assert jpeg.MIN_SIDE == 16 and rz.MIN_SIDE == 2 and sorted(rz.MODES) == ["bicubic", "bilinear"]
