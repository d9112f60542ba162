"""CPU-side checks of glass blur, snow and elastic transform: every stage of the fp64 reference (distort_reference.py) against scipy
in fp64, the host-side planner of unirestore_amd.distort against the reference's restatements and scipy's own output shapes, the
cap on the share of ambiguous intermediate elements, and every refusal of the C ABI, of distort.distort, of `cli distort` and of
data.DistortedImageFiles (all before any HIP call)."""
import os

import numpy as np
import pytest

import corrupt_reference as cref
import distort_cases as cases
import distort_reference as ref
import keyed_noise_reference as kn
from unirestore_amd import corrupt as cr
from unirestore_amd import distort as ds

SEVS = cases.SEVS
TOL = 1e-9                      # 0-255 scale; fp64 sums of <= 100 terms err by ~1e-12: a thousandfold margin
KEY = cr.corruption_seed(42, "img0")


# ------------------------------------------------------------------------------------------ 1. reference stages against scipy
def test_gaussians_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for shape in cases.SHAPES:
        x = cases.images(shape)[0]
        h, w = x.shape[:2]
        for s in SEVS:
            sigma = ref.C["glass_blur"][s - 1][0]
            theirs = np.stack([ndi.gaussian_filter(x[..., c].astype(np.float64), sigma, mode="nearest", truncate=4.0) for c in range(3)], -1)
            assert np.abs(ref.gaussian_u8(x, sigma)[0] - theirs).max() < TOL, (shape, s)
        f = np.random.default_rng(h + w).uniform(-255.0, 255.0, (h, w))
        mine = ref.filter_reflect(ref.filter_reflect(f, ref.elastic_taps(h), 0), ref.elastic_taps(w), 1)
        theirs = ndi.gaussian_filter(f, (0.01 * h, 0.01 * w), mode="reflect", truncate=3.0)
        assert np.abs(mine - theirs).max() < TOL, shape
    assert [len(ref.elastic_taps(n)) // 2 for n in (32, 33, 47, 64, 96, 512)] == [1, 1, 1, 2, 3, 15]      # the radii differ per axis


def test_elastic_field_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for shape in cases.SHAPES:
        h, w = shape[1:]
        for s in SEVS:
            field, bound = ref.elastic_field(h, w, s, KEY)
            m, alpha = float(np.float32(0.005 * h)), float(np.float32(ref.C["elastic_transform"][s - 1]))
            for plane, draw in ((0, 48), (1, 49)):
                f = m * (2.0 * kn.uniforms(kn.words(KEY, draw, h * w)).reshape(h, w) - 1.0)
                theirs = alpha * ndi.gaussian_filter(f, (0.01 * h, 0.01 * w), mode="reflect", truncate=3.0)
                assert np.abs(field[plane] - theirs).max() < TOL, (shape, s, plane)
            assert 0 < bound < 1e-4 and np.abs(field).max() <= 0.15 * h


def test_zoom_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for shape in cases.SHAPES:
        h, w = shape[1:]
        layer = np.random.default_rng(h * w).normal(0.55, 0.3, (h, w))
        for s in SEVS:
            zoom = ref.C["snow"][s - 1][2]
            top, left, ch, cw, oh, ow = ref.snow_geometry(h, w, zoom)
            theirs = ndi.zoom(layer[top:top + ch, left:left + cw, None], (zoom, zoom, 1), order=1)[..., 0]
            assert theirs.shape == (oh, ow) and oh >= h and ow >= w, (shape, s)
            assert 255.0 * np.abs(ref.zoom_linear(layer[top:top + ch, left:left + cw], oh, ow) - theirs).max() < TOL, (shape, s)
    assert ref.snow_geometry(33, 47, 4.5)[4] == 36                               # more rows than the image has


def test_warp_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for shape in cases.SHAPES:
        x = cases.images(shape)[0]
        h, w = x.shape[:2]
        yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        for kind in ("zero", "smooth", "outward"):
            field = cases.warp_field(1, h, w, kind)[0].astype(np.float64)
            py, px = yy + field[0], xx + field[1]
            if kind == "outward":                        # coordinates beyond both edges of both axes, by more than a period too
                assert py.min() < -h and py.max() > 2 * h and px.min() < -w and px.max() > 2 * w
            theirs = np.stack([ndi.map_coordinates(x[..., c].astype(np.float64), [py, px], order=1, mode="reflect") for c in range(3)], -1)
            mine, bound = ref.warp(x, field)
            assert np.abs(mine - theirs).max() < TOL, (shape, kind)
            assert bound.shape == x.shape and bound.max() < 0.2
            if kind == "zero":
                assert np.array_equal(mine, x.astype(np.float64))
    assert list(ref.reflect_sym(np.arange(-9, 9), 4)) == [0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0]


def test_shuffle_is_the_references_gather():
    """The offsets are integers in [-delta, delta), zero outside the interior, and the gather reads the previous image."""
    for shape in cases.SHAPES:
        h, w = shape[1:]
        a = cases.images(shape)[0]
        for delta in cases.DELTAS:
            dy, dx = ref.shuffle_offsets(h, w, KEY, delta, 32)
            inner = np.zeros((h, w), bool)
            inner[delta:h - delta, delta:w - delta] = True
            assert not dy[~inner].any() and not dx[~inner].any()
            assert set(np.unique(dy[inner])) == set(np.unique(dx[inner])) == set(range(-delta, delta)) and not np.array_equal(dy, dx)
            out = ref.shuffle(a, KEY, delta, 32)
            assert np.array_equal(out[~inner], a[~inner])
            for y, x in ((delta, delta), (h - delta - 1, w - delta - 1), (h // 2, w // 3)):
                assert np.array_equal(out[y, x], a[y + dy[y, x], x + dx[y, x]])
            assert not np.array_equal(ref.shuffle_offsets(h, w, KEY, delta, 34)[0], dy)
    assert inner.sum() == (64 - 8) * (96 - 8) and ref.shuffle_offsets(32, 32, KEY, 4, 32)[0][4:28, 4:28].shape == (24, 24)


# ------------------------------------------------------------------------------------------ 2. planner tables
def test_names_and_severity_constants():
    assert ds.NAMES == ("glass_blur", "snow", "elastic_transform") == ref.NAMES and set(ds.SEVERITY) == set(ds.NAMES)
    for name in ds.NAMES:
        assert tuple(ds.SEVERITY[name]) == tuple(ref.C[name]), name
    assert ds.SEVERITY["elastic_transform"] == (12.5, 16.25, 21.25, 25.0, 30.0)
    assert ds.expand("all") == list(ds.NAMES) and ds.expand("snow,glass_blur,snow") == ["snow", "glass_blur"] and ds.expand(["all", "snow"]) == list(ds.NAMES)
    assert (ds.DRAW_GLASS, ds.DRAW_SNOW, ds.DRAW_ELASTIC) == (ref.DRAW["glass"], ref.DRAW["snow"], ref.DRAW["elastic_dy"]) == (32, 40, 48)
    used = set(range(32, 38)) | {40, 48, 49}
    assert not used & (set(cref.DRAW.values()) | {0, 1}) and ref.DRAW["elastic_dx"] == 49
    # the older module is what it was
    assert len(cr.NAMES) == 13 and cr.UNBUILT == ("glass_blur", "snow", "frost", "spatter", "elastic_transform", "jpeg_compression")
    assert not set(ds.NAMES) & set(cr.NAMES) and cr.skipped("common") == ["glass_blur", "snow", "frost", "elastic_transform", "jpeg_compression"]
    for name in ds.NAMES:
        with pytest.raises(NotImplementedError, match="unirestore_amd.distort"):
            cr.check_name(name)


def test_planner_tables_against_the_reference_and_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for shape in cases.SHAPES + [(1, 512, 512), (1, 200, 333)]:
        h, w = shape[1:]
        for s in SEVS:
            zoom, radius, sigma = ref.C["snow"][s - 1][2], ref.C["snow"][s - 1][4], ref.C["snow"][s - 1][5]
            g = ds.snow_geometry(h, w, zoom)
            assert g == ref.snow_geometry(h, w, zoom) and all(isinstance(v, int) for v in g)
            top, left, ch, cw, oh, ow = g
            assert ndi.zoom(np.zeros((ch, cw, 1)), (zoom, zoom, 1), order=1).shape == (oh, ow, 1) and oh >= h and ow >= w
            for angle in (-135.0, -120.3, -90.0, -61.7, -45.0001):
                mine, theirs = cr.motion_taps(oh, ow, radius, sigma, angle), cref.motion_shifts(oh, ow, radius, sigma, angle)
                assert len(mine) == len(theirs) <= 41 and all((-t[0], -t[1]) == (d[0], d[1]) and abs(t[2] - d[2]) < 1e-16 for t, d in zip(mine, theirs))
        ty, tx = ds.elastic_taps(h, w)
        assert len(ty) == 2 * int(0.03 * h + 0.5) + 1 and len(tx) == 2 * int(0.03 * w + 0.5) + 1
        assert np.abs(ty - ref.elastic_taps(h)).max() < 1e-16 and np.abs(tx - ref.elastic_taps(w)).max() < 1e-16
        impulse = np.zeros((h, w))
        impulse[h // 2, w // 2] = 1.0                    # scipy's own kernel: the response to an impulse far from the border
        resp = ndi.gaussian_filter(impulse, (0.01 * h, 0.01 * w), mode="reflect", truncate=3.0)
        ry, rx = len(ty) // 2, len(tx) // 2
        assert np.abs(resp[h // 2 - ry:h // 2 + ry + 1, w // 2 - rx:w // 2 + rx + 1] - np.outer(ty, tx)).max() < 1e-15
    assert max(len(t) // 2 for t in ds.elastic_taps(512, 512)) == 15


def test_snow_angle_depends_on_seed_and_stem_alone():
    angles = [ds.snow_angle(s, f"f{s}") for s in range(300)]
    assert all(-135.0 <= a < -45.0 for a in angles) and min(angles) < -125.0 and max(angles) > -55.0 and len(set(angles)) == 300
    assert ds.snow_angle(42, "photo") == ref.snow_angle(42, "photo") == ds.snow_angle(42, "photo")
    assert ds.snow_angle(42, "photo") != ds.snow_angle(43, "photo") and ds.snow_angle(42, "photo") != ds.snow_angle(42, "photo2")
    assert abs((ds.snow_angle(42, "photo") + 90.0) - cr.motion_angle(42, "photo")) > 1e-6           # a draw of its own, not motion blur's


# ------------------------------------------------------------------------------------------ 3. the cap on ambiguous elements
def test_share_of_ambiguous_intermediate_elements_is_capped():
    """Over all `random` cases at most 1 % of the elements of a quantised intermediate (glass: the floor between the blurs; snow:
    the threshold of the layer and the rounding of L) are ambiguous, so the masks decide little of what the GPU tests compare.
    On the reference alone.  The constant-255 image is wholly ambiguous in glass's floor (255 * the sum of the taps straddles 255,
    in fp64 as in fp32): it runs WITHOUT the cap, here and on the GPU, and only its mask keeps the comparison honest."""
    worst = {}
    for name in ("glass_blur", "snow"):
        for shape in cases.SHAPES:
            x = cases.images(shape)
            for s in SEVS:
                for seed in cases.SEED_SETS:
                    for i, st in enumerate(cases.stems(shape[0])):
                        v, bound, info = ref.run(name, x[i], s, cr.corruption_seed(seed, st), ref.snow_angle(seed, st))
                        worst[name] = max(worst.get(name, 0.0), info["share"])
                        assert info["share"] <= 0.01, (name, shape, s, seed, i, info["share"])
                        assert v.shape == x[i].shape == bound.shape and v.min() >= 0 and v.max() <= 255 and (bound > 0).all()
    print("largest share of ambiguous intermediate elements:", {k: f"{100 * v:.3f} %" for k, v in worst.items()})
    for name, shape, s, seed in cases.UNCAPPED:          # above the cap, and said so (distort_cases.py)
        share = ref.run(name, cases.images(shape)[0], s, cr.corruption_seed(seed, "img0"), ref.snow_angle(seed, "img0"))[2]["share"]
        print("uncapped", name, shape, s, seed, f"{100 * share:.3f} %")
        assert share > 0.01
    assert ref.snow_layer(32, 32, 1, cr.corruption_seed(131, "img0"))[2].sum() == 1      # the cell within its bound of the threshold
    white = cases.images((2, 33, 47), "white")[0]
    for s in SEVS:
        assert ref.glass_blur(white, s, KEY)[2]["share"] > 0.99
        assert ref.snow(white, s, KEY, -90.0)[2]["share"] <= 0.01


def test_reference_properties():
    black = np.zeros((33, 47, 3), dtype=np.uint8)
    x = cases.images((1, 33, 47))[0]
    for s in SEVS:
        assert not ref.glass_blur(black, s, KEY)[0].any() and not ref.elastic_transform(black, s, KEY)[0].any()
        keep = float(np.float32(ref.C["snow"][s - 1][6]))
        v, _, _ = ref.snow(black, s, KEY, -100.0)
        flakes = v[..., 0] - (1 - keep) * 127.5
        free = v[..., 0] < 255.0                       # not clamped
        assert np.array_equal(v[..., 0], v[..., 1]) and np.array_equal(v[..., 1], v[..., 2]) and free.mean() > 0.5
        assert np.abs(flakes - np.rint(flakes))[free].max() < 1e-9 and flakes.min() >= 0 and flakes.max() > 0          # integers: L + L rotated
        assert np.abs(flakes - flakes[::-1, ::-1]).max() < 1e-9
        field, e_l, amb, kept, exact = ref.snow_layer(33, 47, s, KEY)
        thr = float(np.float32(ref.C["snow"][s - 1][3]))
        assert field.shape == ref.snow_geometry(33, 47, ref.C["snow"][s - 1][2])[4:] and 0 < e_l < 1e-5
        assert ((field == 0) | (field >= thr)).all() and field.max() <= 1.0 and 0.0 < (field > 0).mean() < 0.6
        assert exact.mean() > 0.5 and set(np.unique(field[exact])) <= {0.0, 1.0} and not (exact & amb).any()
        for name in ref.NAMES:
            v, bound, info = ref.run(name, x, s, KEY, -77.0)
            assert np.isfinite(v).all() and v.min() >= 0 and v.max() <= 255 and (bound > 0).all() and np.median(bound) < 0.05, (name, s)
            assert not np.array_equal(v, ref.run(name, x, s, cr.corruption_seed(7, "img0"), -77.0)[0]), (name, s)


# ------------------------------------------------------------------------------------------ 4. refusals
def test_c_abi_refuses_wrong_arguments_before_the_gpu():
    from unirestore_amd import capi
    rows = cases.refusals()
    exports = {k for k in capi.SIGNATURES if k.startswith("ur_distort")}
    assert len(rows) > 90 and {fn for _, fn, _ in rows} == {k for k in exports if not k.endswith("_bytes")} and len(exports) == 7
    assert not any(k.startswith("ur_corrupt") for k in exports)
    for label, fn, args in rows:
        assert getattr(capi.lib, fn)(*args) == capi.UR_E_INVALID, label
        assert fn.encode() in capi.lib.ur_last_error(), (label, capi.lib.ur_last_error())
    assert {fn for fn, _ in cases.valid_calls()} == {fn for _, fn, _ in rows}
    for fn in cases.WS_BYTES:
        f = getattr(capi.lib, fn)
        assert f(0, 32, 32) == 0 and f(2, -1, 32) == 0 and f(2, 32, 0) == 0 and f(2, 33, 47) > 0, fn
    assert capi.lib.ur_distort_snow_ws_bytes(2, 33, 47) == (2 * 33 * 47 + 7) // 8 * 8
    assert capi.lib.ur_distort_field_ws_bytes(2, 33, 47) == 2 * 2 * 33 * 47 * 4


def test_planner_refuses_wrong_arguments_before_the_gpu():
    import torch
    img = torch.zeros(1, 32, 32, 3, dtype=torch.uint8)
    for name in ("frost", "spatter"):
        with pytest.raises(NotImplementedError, match=name):
            ds.distort(None, name, 3, 42)
        with pytest.raises(NotImplementedError, match=name):
            ds.expand(name)
        with pytest.raises(NotImplementedError, match=name):
            ds.degrade(None, name, 3, 42, resize=(32, 64))
    for name in ("rain", "fog", "jpeg_compression", "clean", "common"):
        with pytest.raises(ValueError, match="unknown corruption"):
            ds.distort(img, name, 3, 42)
    with pytest.raises(ValueError, match="no corruption"):
        ds.expand("")
    for bad in (0, 6, "3", 2.0, True):
        with pytest.raises(ValueError, match="severity"):
            ds.distort(img, "snow", bad, 42)
    for bad in (torch.zeros(1, 32, 32, 3), torch.zeros(32, 32, 3, dtype=torch.uint8), None):       # (no GPU is looked at before this)
        with pytest.raises(ValueError, match="uint8"):
            ds.distort(bad, "glass_blur", 3, 42)
    with pytest.raises(ValueError, match="resize"):
        ds.degrade(img, "snow", 3, 42, resize=(16, 64))


def _png(path, shape=(32, 40), seed=0):
    from PIL import Image
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (*shape, 3), dtype=np.uint8)).save(path)


def test_cli_distort_argument_errors(tmp_path, capsys):
    from unirestore_amd import cli
    src = tmp_path / "clean"
    src.mkdir()
    _png(src / "a.png")
    _png(src / "b.png", seed=1)
    out = str(tmp_path / "out")
    paths, names, sev = cli.check_distort_args(str(src), out, "snow,glass_blur", "mixed")
    assert [os.path.basename(p) for p in paths] == ["a.png", "b.png"] and sev == "mixed" and names == ["snow", "glass_blur"]
    assert cli.check_distort_args(str(src), out, "all", "4")[1:] == (list(ds.NAMES), 4)
    with pytest.raises(ValueError, match="--corruptions"):
        cli.check_distort_args(str(src), out, None)
    for bad in ("rain", "fog", "common", "clean"):
        with pytest.raises(ValueError, match="--corruptions"):
            cli.check_distort_args(str(src), out, bad)
    with pytest.raises(NotImplementedError, match="frost"):
        cli.check_distort_args(str(src), out, "snow,frost")
    for bad in ("0", "6", "2.5", "mix"):
        with pytest.raises(ValueError, match="--severity"):
            cli.check_distort_args(str(src), out, "snow", bad)
    with pytest.raises(ValueError, match="--batch"):
        cli.check_distort_args(str(src), out, "snow", 3, batch=0)
    with pytest.raises(ValueError, match="--resize"):
        cli.check_distort_args(str(src), out, "snow", 3, resize="16,64")
    with pytest.raises(FileNotFoundError, match="--input"):
        cli.check_distort_args(str(tmp_path / "nowhere"), out, "snow")
    with pytest.raises(ValueError, match="--output"):
        cli.check_distort_args(str(src), None, "snow")
    with pytest.raises(ValueError, match="--output"):
        cli.check_distort_args(str(src), str(src), "snow")
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no image"):
        cli.check_distort_args(str(empty), out, "snow")
    for argv in (["distort", "--input", str(tmp_path / "nowhere"), "--output", out, "--corruptions", "snow"],      # no --config is needed
                 ["distort", "--input", str(src), "--output", out], ["distort", "--input", str(src), "--output", out, "--corruptions", "spatter"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
    assert "arguments are required" not in capsys.readouterr().err


def test_distorted_image_files_plans_without_a_gpu(tmp_path):
    from unirestore_amd import cli, data
    src = tmp_path / "clean"
    src.mkdir()
    for i in range(7):
        _png(src / f"im{i}.png", shape=(32, 40) if i % 3 else (36, 32), seed=i)
    d = data.DistortedImageFiles(str(src), corruptions="all", severity="mixed", batch_size=2, seed=7)
    assert d.names == list(ds.NAMES) and d.skipped == [] and len(d) == len(d._plan()) >= 4
    assert sorted(i for _, _, idx in d._plan() for i in idx) == list(range(7))
    assert all(name in ds.NAMES and (name, sev) == ds.choose(7, f"im{idx[0]}", d.names, "mixed") for name, sev, idx in d._plan())
    assert len(data.DistortedImageFiles(str(src), batch_size=2, num_batches=2)) == 2 and isinstance(d, data.CorruptedImageFiles)
    with pytest.raises(ValueError, match="shard"):
        next(d.batches(0, 2))
    with pytest.raises(NotImplementedError, match="frost"):
        data.DistortedImageFiles(str(src), corruptions="frost")
    with pytest.raises(ValueError, match="unknown corruption"):
        data.DistortedImageFiles(str(src), corruptions="fog")
    with pytest.raises(ValueError, match="severity"):
        data.DistortedImageFiles(str(src), severity=0)
    with pytest.raises(ValueError, match="resize"):
        data.DistortedImageFiles(str(src), resize=[16, 64])
    assert cli.DATA_CLASSES["unirestore_amd.data.DistortedImageFiles"].endswith("DistortedImageFiles")
    assert data.CorruptedImageFiles(str(src), corruptions="weather").skipped == ["snow", "frost"]       # the older class is what it was
