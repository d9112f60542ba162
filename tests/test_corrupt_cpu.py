"""CPU-side checks of the corruptions: the fp64 reference (corrupt_reference.py) against independent implementations where this
machine has them (scipy, Pillow, colorsys), the host-side builders of unirestore_amd.corrupt against the reference's restatements,
known answers, subsets, the seeded choices, and every refusal of the C ABI and of `cli corrupt` (all before any HIP call).
OpenCV and skimage are not assumed: the defocus kernel, reflect-101 and s&p are restated from their documentation."""
import colorsys
import math
import os

import numpy as np
import pytest

import corrupt_cases as cases
import corrupt_reference as ref
from unirestore_amd import corrupt as cr

SEVS = (1, 2, 3, 4, 5)


def test_names_constants_and_subsets():
    assert len(cr.NAMES) == 13 and len(cr.UNBUILT) == 6 and set(cr.NAMES) | set(cr.UNBUILT) == set(cr.ALL) and len(cr.ALL) == 19
    assert set(cr.SEVERITY) == set(cr.NAMES) == set(ref.NAMES)
    for name in cr.NAMES:
        if name != "zoom_blur":
            assert tuple(cr.SEVERITY[name]) == tuple(ref.C[name]), name
    assert cr.expand("common") == ["gaussian_noise", "shot_noise", "impulse_noise", "defocus_blur", "motion_blur", "zoom_blur", "fog",
                                   "brightness", "contrast", "pixelate"]
    assert cr.skipped("common") == ["glass_blur", "snow", "frost", "elastic_transform", "jpeg_compression"]
    assert cr.expand("validation") == ["speckle_noise", "gaussian_blur", "saturate"] and cr.skipped("validation") == ["spatter"]
    assert cr.expand("noise") == ["gaussian_noise", "shot_noise", "impulse_noise"] and cr.skipped("noise") == []
    assert cr.expand("blur") == ["defocus_blur", "motion_blur", "zoom_blur"] and cr.skipped("blur") == ["glass_blur"]
    assert cr.expand("weather") == ["fog", "brightness"] and cr.skipped("weather") == ["snow", "frost"]
    assert cr.expand("digital") == ["contrast", "pixelate"] and cr.skipped("digital") == ["elastic_transform", "jpeg_compression"]
    assert sorted(cr.expand("all")) == sorted(cr.NAMES) and sorted(cr.skipped("all")) == sorted(cr.UNBUILT)
    assert cr.expand("fog,motion_blur,fog") == ["fog", "motion_blur"] and cr.expand(["noise", "clean"])[-1] == "clean"
    assert "clean" not in cr.expand("all")
    with pytest.raises(ValueError, match="nonsense"):
        cr.expand("nonsense")
    with pytest.raises(ValueError):
        cr.expand("")


@pytest.mark.parametrize("name", cr.UNBUILT)
def test_unbuilt_corruptions_are_named(name):
    with pytest.raises(NotImplementedError, match=name):
        cr.expand(name)
    with pytest.raises(NotImplementedError, match=name):
        cr.corrupt(None, name, 3, 42)


def test_known_answers():
    assert cr.corruption_seed(42, "photo") == 10502507413119121937
    from unirestore_amd import cli
    assert cr.corruption_seed(42, "photo") != cli.image_seed(42, "photo")
    assert abs(cr.motion_angle(42, "photo") - 5.203469683048375) < 1e-12 and cr.motion_angle(42, "photo") == ref.motion_angle(42, "photo")
    assert all(-45.0 <= cr.motion_angle(s, f"f{s}") < 45.0 for s in range(200))
    assert [len(cr.zoom_factors(s)) for s in SEVS] == [12, 16, 11, 13, 11]
    assert all(cr.zoom_factors(s)[0] == 1.0 for s in SEVS)
    # 32 x 32 at severity 5 (radius 20, sigma 15), angle 0: the shift reaches the width at tap 32 of 41, the rest is dropped
    taps = cr.motion_taps(32, 32, 20, 15, 0.0)
    g = np.exp(-np.arange(41.0) ** 2 / 450.0)
    assert taps.shape == (32, 3) and np.array_equal(taps[:, 0], np.arange(32.0)) and not taps[:, 1].any()
    assert np.allclose(taps[:, 2], g[:32] / g.sum(), rtol=1e-14, atol=0) and abs(taps[:, 2].sum() - 0.9717839776211201) < 1e-12
    assert len(cr.motion_taps(64, 96, 20, 15, 0.0)) == 41 and abs(cr.motion_taps(64, 96, 20, 15, 30.0)[:, 2].sum() - 1.0) < 1e-12
    # a disk that stays inside its grid keeps its sum through the smoothing; radius 8 and 10 touch the edge, where the reflected
    # border counts the neighbouring column twice (as cv2.GaussianBlur's default border does)
    sums = [cr.disk_kernel(*cr.SEVERITY["defocus_blur"][s - 1]).sum() for s in SEVS]
    assert all(abs(v - 1.0) < 1e-12 for v in sums[:3]) and all(1.0 < v < 1.02 for v in sums[3:])
    assert [cr.disk_kernel(*cr.SEVERITY["defocus_blur"][s - 1]).shape[0] for s in SEVS] == [17, 17, 17, 17, 21]


def test_builders_agree_with_the_reference_restatements():
    for s in SEVS:
        assert np.abs(cr.gaussian_taps(ref.C["gaussian_blur"][s - 1]) - ref.gaussian_taps(ref.C["gaussian_blur"][s - 1])).max() < 1e-16
        assert np.abs(cr.disk_kernel(*ref.C["defocus_blur"][s - 1]) - ref.disk_kernel(*ref.C["defocus_blur"][s - 1])).max() < 1e-16
        assert np.array_equal(cr.zoom_factors(s), ref.C["zoom_blur"][s - 1])
        for angle in (-44.9, -10.0, 0.0, 5.2, 44.9):
            for h, w in ((32, 32), (33, 47), (64, 96)):
                mine, theirs = cr.motion_taps(h, w, *ref.C["motion_blur"][s - 1], angle), ref.motion_shifts(h, w, *ref.C["motion_blur"][s - 1], angle)
                assert len(mine) == len(theirs) and all((-t[0], -t[1]) == (d[0], d[1]) and abs(t[2] - d[2]) < 1e-16 for t, d in zip(mine, theirs))
    k = cr.disk_kernel(3, 0.1)
    taps = cr.kernel_taps(k)
    assert taps.shape == (289, 3) and tuple(taps[0][:2]) == (-8, -8) and tuple(taps[-1][:2]) == (8, 8) and taps[1][0] == -7
    packed = cr.pack_taps(taps)
    assert packed.dtype == np.int32 and np.array_equal(packed[:, 2].view(np.float32), taps[:, 2].astype(np.float32))


def test_gaussian_blur_reference_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    x = cases.images((2, 33, 47))[1]
    for s in SEVS:
        sigma = ref.C["gaussian_blur"][s - 1]
        theirs = np.stack([ndi.gaussian_filter(x[..., c].astype(np.float64), sigma, mode="nearest", truncate=4.0) for c in range(3)], -1)
        assert np.abs(ref.gaussian_blur(x, s)[0] - theirs).max() < 1e-11           # 255 * a few hundred fp64 roundings


def test_zoom_layers_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for shape in cases.SHAPES:
        x = cases.images(shape)[0].astype(np.float64)
        h, w = x.shape[:2]
        for s in SEVS:
            table = cr.zoom_layers(h, w, cr.zoom_factors(s))
            for z, (top, left, ch, cw, oh, ow) in zip(ref.C["zoom_blur"][s - 1], table):
                assert oh >= h and ow >= w and (top, left) == ((h - ch) // 2, (w - cw) // 2)
                theirs = ndi.zoom(x[top:top + ch, left:left + cw], (z, z, 1), order=1)
                assert theirs.shape[:2] == (oh, ow)
                assert np.abs(theirs[:h, :w] - ref.zoom_layer(x, z)).max() < 1e-9


def test_pixelate_reference_and_tables_against_pillow():
    Image = pytest.importorskip("PIL.Image")
    for shape in cases.SHAPES + [(1, 37, 51), (1, 45, 33), (1, 101, 67)]:
        x = cases.images(shape)[0]
        h, w = x.shape[:2]
        for s in SEVS:
            c = ref.C["pixelate"][s - 1]
            theirs = np.asarray(Image.fromarray(x).resize((int(w * c), int(h * c)), Image.BOX).resize((w, h), Image.NEAREST))
            assert np.array_equal(ref.pixelate(x, s)[0], theirs.astype(np.float64)), (shape, s)
            sh, sw, hbox, vbox, ymap, xmap = cr.pixelate_tables(h, w, c)           # the tables the kernel applies, in numpy
            rows = np.stack([(2 * x[:, f:f + n].astype(np.int64).sum(1) + n) // (2 * n) for f, n in hbox], 1)
            small = np.stack([(2 * rows[f:f + n].sum(0) + n) // (2 * n) for f, n in vbox], 0)
            assert (sh, sw) == small.shape[:2] and np.array_equal(small[ymap][:, xmap], theirs), (shape, s)


def test_hsv_round_trip_against_colorsys():
    grid = cases.colour_grid()[0].reshape(-1, 3) / 255.0
    assert any(p[0] == p[1] == p[2] for p in grid) and any(p[0] == p[1] != p[2] for p in grid) and any(p[1] == p[2] != p[0] for p in grid)
    hsv = ref.rgb2hsv(grid)
    theirs = np.array([colorsys.rgb_to_hsv(*p) for p in grid])
    d = np.abs(hsv - theirs)
    d[:, 0] = np.minimum(d[:, 0], 1.0 - d[:, 0])                                   # the hue is a circle
    assert d.max() < 1e-14
    assert np.abs(ref.hsv2rgb(hsv) - np.array([colorsys.hsv_to_rgb(*p) for p in hsv])).max() < 1e-14
    assert np.abs(ref.hsv2rgb(hsv) - grid).max() < 1e-14
    x = cases.colour_grid()[0]
    for s in SEVS:                                   # a grey pixel stays grey under brightness; severity 1-3 of saturate keep it too
        grey = (x[..., 0] == x[..., 1]) & (x[..., 1] == x[..., 2])
        v = ref.brightness(x, s)[0][grey]
        assert np.array_equal(v[:, 0], v[:, 1]) and np.array_equal(v[:, 1], v[:, 2])
        assert np.abs(v[:, 0] - np.minimum(x[grey][:, 0] + 255.0 * ref.C["brightness"][s - 1], 255.0)).max() < 1e-4


def test_poisson_table_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    for c in ref.C["shot_noise"]:
        t = cr.poisson_table(c).astype(np.int64)
        assert t.shape == (256, 128) and (np.diff(t, axis=1) >= 0).all() and (t[0] == 1 << 24).all() and t.max() <= 1 << 24
        theirs = np.floor(stats.poisson.cdf(np.arange(128)[None, :], np.arange(256)[:, None] * c / 255.0) * 2.0 ** 24).astype(np.int64)
        # two fp64 evaluations of the CDF differ by ~1e-15 (and by the 3.2e-14 of mass beyond k = 127), so a floor can fall on the
        # other side of an integer, by one, in a few entries - chiefly where the CDF is within 2^-24 of 1
        assert np.abs(t - theirs).max() <= 1 and (t != theirs).mean() < 2e-3, c


def test_reference_properties():
    x = cases.images((1, 33, 47))[0]
    key = cr.corruption_seed(42, "a")
    for s in SEVS:
        v, bound = ref.impulse_noise(x, s, key)
        flipped = v != x
        assert not bound.any() and set(np.unique(v[flipped])) <= {0.0, 255.0}
        assert abs(flipped.mean() - ref.C["impulse_noise"][s - 1] * (1 - 1 / 256)) < 0.02      # a flip to the value it had is not seen
        dark, c = x // 4, ref.C["shot_noise"][s - 1]     # below 64 the clip at 255 is out of reach: 255 Poisson(x c / 255) / c has
        v, _ = ref.shot_noise(dark, s, key, cr.poisson_table(c))      # mean x and variance 255 x / c; four standard errors
        assert abs(v.mean() - dark.mean()) < 4.0 * math.sqrt(255.0 * dark.mean() / c / dark.size)
        assert not ref.shot_noise(np.zeros_like(x), s, key, cr.poisson_table(ref.C["shot_noise"][s - 1]))[0].any()
    for name in ref.NAMES:                              # every op, every severity: finite, inside [0, 255], a positive or zero bound
        for s in (1, 5):
            v, bound = ref.run(name, x, s, key=key, angle=12.5, table=cr.poisson_table(ref.C["shot_noise"][s - 1]))
            assert v.shape == x.shape == bound.shape and np.isfinite(v).all() and v.min() >= 0 and v.max() <= 255
            assert (bound >= 0).all() and bound.max() < 0.05 and (name in ref.EXACT) == (not bound[v < 255].any() or name == "shot_noise"), name
    flat = np.full((32, 32, 3), 77, dtype=np.uint8)     # a constant image passes every blur and pixelate unchanged
    for name in ("gaussian_blur", "motion_blur", "zoom_blur", "pixelate", "contrast"):
        v, _ = ref.run(name, flat, 2, angle=30.0)
        assert np.abs(v - 77).max() < 1e-9, name


def test_choices_are_seeded_and_order_free(tmp_path):
    names = cr.expand("common")
    stems = [f"file{i:04d}" for i in range(3000)]
    picks = {st: cr.choose(42, st, names, "mixed") for st in stems}
    assert picks == {st: cr.choose(42, st, names, "mixed") for st in reversed(stems)}
    assert picks != {st: cr.choose(43, st, names, "mixed") for st in stems}
    sev = np.bincount([p[1] for p in picks.values()], minlength=6)[1:] / len(stems)
    assert np.abs(sev - np.array(cr.MIXED_P)).max() < 0.04                        # 3000 draws: 4 standard deviations of p = 0.4
    assert {p[0] for p in picks.values()} == set(names)
    assert all(cr.choose(42, st, names, 4)[1] == 4 for st in stems[:10])
    with pytest.raises(ValueError):
        cr.choose(42, "a", names, 6)
    # the plan of a file list: the same (corruption, severity) per file whatever the order and the batch size
    paths = [str(tmp_path / f"{st}.png") for st in stems[:40]]
    sizes = [(32 + i % 2, 40) for i in range(40)]

    def assignment(order, batch):
        plan = cr.plan_files([paths[i] for i in order], [sizes[i] for i in order], names, "mixed", 42, batch)
        assert all(len(idx) <= batch for _, _, idx in plan) and sorted(i for _, _, idx in plan for i in idx) == list(range(40))
        for name, sev, idx in plan:
            assert len({sizes[order[i]] for i in idx}) == 1
        return {paths[order[i]]: (name, sev) for name, sev, idx in plan for i in idx}
    assert assignment(list(range(40)), 8) == assignment(list(reversed(range(40))), 3) == {p: picks[cr.stem_of(p)] for p in paths}


def test_c_abi_refuses_wrong_arguments_before_the_gpu():
    from unirestore_amd import capi
    rows = cases.refusals()
    assert len(rows) > 120 and {fn for _, fn, _ in rows} == {k for k in capi.SIGNATURES if k.startswith("ur_corrupt") and not k.endswith("_bytes")}
    for label, fn, args in rows:
        assert getattr(capi.lib, fn)(*args) == capi.UR_E_INVALID, label
        assert fn.encode() in capi.lib.ur_last_error(), (label, capi.lib.ur_last_error())
    for fn in ("ur_corrupt_filter_sep_ws_bytes", "ur_corrupt_color_ws_bytes", "ur_corrupt_pixelate_ws_bytes", "ur_corrupt_fog_ws_bytes"):
        f = getattr(capi.lib, fn)
        assert f(0, 32, 32) == 0 and f(2, -1, 32) == 0 and f(2, 32, 0) == 0 and f(2, 33, 47) > 0, fn
    assert capi.lib.ur_corrupt_filter_sep_ws_bytes(2, 33, 47) == 2 * 33 * 47 * 3 * 4
    assert capi.lib.ur_corrupt_fog_ws_bytes(1, 33, 47) >= 64 * 64 * 4 and capi.lib.ur_corrupt_fog_ws_bytes(1, 64, 96) >= 128 * 128 * 4


def test_ops_and_planner_refuse_wrong_arguments_before_the_gpu():
    import torch
    from unirestore_amd import ops
    with pytest.raises(ValueError, match="severity"):
        cr.corrupt(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), "fog", 6, 42)
    with pytest.raises(ValueError, match="severity"):
        cr.corrupt(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), "fog", "3", 42)
    with pytest.raises(ValueError, match="unknown corruption"):
        cr.corrupt(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), "rain", 3, 42)
    for bad in (torch.zeros(1, 32, 32, 3), torch.zeros(32, 32, 3, dtype=torch.uint8), torch.zeros(1, 32, 32, 4, dtype=torch.uint8),
                torch.zeros(1, 3, 32, 32, dtype=torch.uint8).permute(0, 2, 3, 1), None):
        with pytest.raises(ValueError, match="uint8"):
            ops.check_u8_images("corrupt", bad)


def _png(path, shape=(32, 40), seed=0):
    from PIL import Image
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (*shape, 3), dtype=np.uint8)).save(path)


def test_cli_corrupt_argument_errors(tmp_path, capsys):
    from unirestore_amd import cli
    src = tmp_path / "clean"
    src.mkdir()
    _png(src / "a.png")
    _png(src / "b.png", seed=1)
    out = str(tmp_path / "out")
    paths, names, sev = cli.check_corrupt_args(str(src), out, "fog,noise", "mixed")
    assert [os.path.basename(p) for p in paths] == ["a.png", "b.png"] and sev == "mixed"
    assert names == ["fog", "gaussian_noise", "shot_noise", "impulse_noise"]
    assert cli.check_corrupt_args(str(src), out, "fog", "4")[2] == 4
    with pytest.raises(ValueError, match="--corruptions"):
        cli.check_corrupt_args(str(src), out, None)
    with pytest.raises(ValueError, match="--corruptions"):
        cli.check_corrupt_args(str(src), out, "rain")
    with pytest.raises(ValueError, match="clean"):
        cli.check_corrupt_args(str(src), out, "fog,clean")
    with pytest.raises(NotImplementedError, match="snow"):
        cli.check_corrupt_args(str(src), out, "snow")
    for bad in ("0", "6", "2.5", "mix"):
        with pytest.raises(ValueError, match="--severity"):
            cli.check_corrupt_args(str(src), out, "fog", bad)
    with pytest.raises(ValueError, match="--batch"):
        cli.check_corrupt_args(str(src), out, "fog", 3, batch=0)
    with pytest.raises(FileNotFoundError, match="--input"):
        cli.check_corrupt_args(str(tmp_path / "nowhere"), out, "fog")
    with pytest.raises(ValueError, match="--output"):
        cli.check_corrupt_args(str(src), None, "fog")
    with pytest.raises(ValueError, match="--output"):
        cli.check_corrupt_args(str(src), str(src), "fog")
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no image"):
        cli.check_corrupt_args(str(empty), out, "fog")
    lst = tmp_path / "pairs.txt"                     # an `lq hq label` list: only the hq column is read
    lst.write_text("# comment\nlq/a.png clean/a.png 0\nlq/b.png clean/b.png 1\n")
    assert cli.check_corrupt_args(str(lst), out, "fog")[0] == [str(src / "a.png"), str(src / "b.png")]
    lst.write_text("x/a.png clean/a.png\ny/a.png clean/a.png\n")
    with pytest.raises(ValueError, match="stem"):
        cli.check_corrupt_args(str(lst), out, "fog")
    lst.write_text("clean/a.png\nclean/missing.png\n")
    with pytest.raises(FileNotFoundError, match="missing"):
        cli.check_corrupt_args(str(lst), out, "fog")
    # `corrupt` needs no --config; the other commands still do
    for argv in (["corrupt", "--input", str(tmp_path / "nowhere"), "--output", out, "--corruptions", "fog"],
                 ["corrupt", "--input", str(src), "--output", out], ["validate"], ["restore", "--input", str(src), "--output", out],
                 ["print_config"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
    assert "--config" in capsys.readouterr().err


def test_corrupted_image_files_plans_without_a_gpu(tmp_path):
    from unirestore_amd import cli, data
    src = tmp_path / "clean"
    src.mkdir()
    for i in range(7):
        _png(src / f"im{i}.png", shape=(32, 40) if i % 3 else (36, 32), seed=i)
    d = data.CorruptedImageFiles(str(src), corruptions="common", severity="mixed", batch_size=2, seed=7)
    assert d.skipped == cr.skipped("common") and len(d) == len(d._plan()) >= 4
    assert sorted(i for _, _, idx in d._plan() for i in idx) == list(range(7))
    assert len(data.CorruptedImageFiles(str(src), batch_size=2, num_batches=2)) == 2
    with pytest.raises(ValueError, match="shard"):
        next(d.batches(0, 2))
    with pytest.raises(NotImplementedError, match="frost"):
        data.CorruptedImageFiles(str(src), corruptions="frost")
    with pytest.raises(ValueError, match="severity"):
        data.CorruptedImageFiles(str(src), severity=0)
    assert cli.DATA_CLASSES["unirestore_amd.data.CorruptedImageFiles"].endswith("CorruptedImageFiles")
