"""The corruption kernels (csrc/corrupt.hip) against the fp64 reference of corrupt_reference.py, element by element, and the layers
above them (corrupt.corrupt, data.CorruptedImageFiles, cli.validate, cli corrupt).  The cases, bounds and the reference are stated in
corrupt_cases.py / corrupt_reference.py; this file launches and compares.  Every launch goes through the C ABI on guarded buffers:
guards and inputs untouched, a second launch bit-identical, the fp32 values (out_kind 1) within the derived bound, the bytes
(out_kind 0) equal to the floor of the fp32 values of the same arguments, and within 1 of (for the integer ops: equal to) the
reference's bytes."""
import json
import os

import numpy as np
import pytest
import torch

import corrupt_cases as cases
import corrupt_reference as ref
from test_boundary_launchers_gpu import Buf

pytestmark = pytest.mark.gpu

SEVS = (1, 2, 3, 4, 5)
KEYED = ("gaussian_noise", "speckle_noise", "impulse_noise", "shot_noise", "fog", "motion_blur")      # what a seed changes
WORST = {}                      # op -> largest |value - reference| / bound seen
_REF = {}                       # (op, shape, kind, severity, seed) -> (values fp64 [N,H,W,3], bounds): computed once, shared, read-only


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    yield c
    if WORST:
        print("\nlargest |value - fp64 reference| / bound per corruption:")
        for name, r in sorted(WORST.items()):
            print(f"  {name:16s} {r:.3f}")


@pytest.fixture(scope="module")
def cr():
    from unirestore_amd import corrupt
    return corrupt


def _stream():
    return torch.cuda.current_stream().cuda_stream


def reference(cr, name, shape, kind, sev, seed):
    key = (name, shape, kind, sev, seed if name in KEYED else None)
    if key not in _REF:
        x = cases.images(shape, kind)
        rows = [ref.run(name, x[i], sev, key=cr.corruption_seed(seed, st), angle=ref.motion_angle(seed, st),
                        table=cr.poisson_table(ref.C["shot_noise"][sev - 1])) for i, st in enumerate(cases.stems(shape[0]))]
        v, b = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        v.setflags(write=False)
        b.setflags(write=False)
        _REF[key] = (v, b)
    return _REF[key]


def _table(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    b = Buf(tuple(t.shape), t.dtype, fill=t.cuda())
    b.orig = t
    return b


def launch(capi, cr, name, sev, x, seeds, stems, out_kind):
    """Corruption `name` of the u8 batch x (host tensor) through the primitives of the C ABI, every buffer guarded.
    -> (out tensor on the host, inputs untouched and all guards intact)."""
    from unirestore_amd import ops
    n, h, w, _ = x.shape
    lib, c = capi.lib, cr.SEVERITY[name][sev - 1]
    xb = _table(x.numpy())
    out = Buf(tuple(x.shape), torch.float32 if out_kind else torch.uint8)
    ins, ws, args = [xb], None, (n, h, w)

    def keys():
        ins.append(_table(ops.noise_keys([cr.corruption_seed(s, t) for s, t in zip(seeds, stems)]).numpy()))
        return ins[-1].ptr

    def tab(a):
        ins.append(_table(a))
        return ins[-1].ptr

    def work(nbytes):
        nonlocal ws
        ws = Buf(((nbytes + 7) // 8 * 2,), torch.int32)
        return ws.ptr, nbytes
    if name in cr.NOISE_MODES:
        mode = cr.NOISE_MODES[name]
        rc = lib.ur_corrupt_noise(xb.ptr, keys(), out.ptr, *args, mode, 255.0 * c if mode == 0 else float(c),
                                  tab(cr.poisson_table(c).view(np.int32)) if mode == 3 else None, out_kind, _stream())
    elif name == "gaussian_blur":
        taps = cr.gaussian_taps(c).astype(np.float32)
        rc = lib.ur_corrupt_filter_sep(xb.ptr, tab(taps), len(taps) // 2, out.ptr, *args, *work(lib.ur_corrupt_filter_sep_ws_bytes(*args)), out_kind,
                                       _stream())
    elif name == "defocus_blur":
        taps = cr.pack_taps(cr.kernel_taps(cr.disk_kernel(*c)))
        rc = lib.ur_corrupt_taps(xb.ptr, tab(taps), len(taps), 0, 1, out.ptr, *args, out_kind, _stream())
    elif name == "motion_blur":
        lists = [cr.motion_taps(h, w, c[0], c[1], cr.motion_angle(s, t)) for s, t in zip(seeds, stems)]
        taps = np.zeros((n, max(len(t) for t in lists), 3))
        for i, t in enumerate(lists):
            taps[i, :len(t)] = t
        rc = lib.ur_corrupt_taps(xb.ptr, tab(cr.pack_taps(taps)), taps.shape[1], 1, 0, out.ptr, *args, out_kind, _stream())
    elif name == "zoom_blur":
        layers = cr.zoom_layers(h, w, cr.zoom_factors(sev))
        rc = lib.ur_corrupt_zoom(xb.ptr, tab(layers), len(layers), out.ptr, *args, out_kind, _stream())
    elif name in cr.COLOR_MODES:
        a, b = (c, 0.0) if name == "contrast" else (255.0 * c, 0.0) if name == "brightness" else c
        rc = lib.ur_corrupt_color(xb.ptr, out.ptr, *args, cr.COLOR_MODES[name], a, b, *work(lib.ur_corrupt_color_ws_bytes(*args)), out_kind, _stream())
    elif name == "pixelate":
        sh, sw, hbox, vbox, ymap, xmap = cr.pixelate_tables(h, w, c)
        rc = lib.ur_corrupt_pixelate(xb.ptr, out.ptr, *args, sh, sw, tab(hbox), tab(vbox), tab(ymap), tab(xmap),
                                     *work(lib.ur_corrupt_pixelate_ws_bytes(n, h, sw)), out_kind, _stream())
    else:
        rc = lib.ur_corrupt_fog(xb.ptr, keys(), out.ptr, *args, 255.0 * c[0], float(c[1]), *work(lib.ur_corrupt_fog_ws_bytes(*args)), out_kind,
                                _stream())
    assert rc == 0, (name, sev, lib.ur_last_error())
    torch.cuda.synchronize()
    ok = all(b.guards_ok() for b in ins + [out] + ([ws] if ws is not None else [])) and \
        all(torch.equal(b.t.cpu().view(torch.uint8), b.orig.view(torch.uint8)) for b in ins)          # inputs and tables as they were
    return out.t.cpu(), ok


def check(capi, cr, name, shape, kind, sev, seed):
    x = torch.from_numpy(cases.images(shape, kind))
    stems, seeds = cases.stems(shape[0]), [seed] * shape[0]
    val, ok1 = launch(capi, cr, name, sev, x, seeds, stems, 1)
    again, ok2 = launch(capi, cr, name, sev, x, seeds, stems, 1)
    u8, ok3 = launch(capi, cr, name, sev, x, seeds, stems, 0)
    what = (name, shape, kind, sev, seed)
    assert ok1 and ok2 and ok3, what                                   # guards and inputs
    assert torch.equal(val.view(torch.int32), again.view(torch.int32)), what          # a second launch: the same bits
    v = val.double().numpy()
    want, bound = reference(cr, name, shape, kind, sev, seed)
    err = np.abs(v - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if bound.any() else (0.0 if not err.any() else float("inf"))
    WORST[name] = max(WORST.get(name, 0.0), float(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0).max()))
    print(f"{name} {shape} {kind} severity {sev} seed {seed}: max |err| {err.max():.3e}, max bound {bound.max():.3e}, max ratio {ratio:.3f}")
    assert (err <= bound).all(), (what, float(err.max()), float(bound.max()))
    assert v.min() >= 0.0 and v.max() <= 255.0, what
    assert np.array_equal(u8.numpy(), np.floor(v).astype(np.uint8)), what              # the bytes are the floor of the values
    want_u8 = np.floor(want).astype(np.int64)
    diff = np.abs(u8.numpy().astype(np.int64) - want_u8)
    assert diff.max() <= (0 if name in ref.EXACT else 1), (what, int(diff.max()))


@pytest.mark.parametrize("name", ref.NAMES)
def test_against_fp64(capi, cr, name):
    for shape in cases.SHAPES:
        for sev in SEVS:
            for seed in cases.SEED_SETS if name in KEYED else cases.SEED_SETS[:1]:
                check(capi, cr, name, shape, "random", sev, seed)
    for kind in cases.KINDS[1:]:                     # constant 0, constant 255, the grey ramp
        for sev in SEVS:
            check(capi, cr, name, (2, 33, 47), kind, sev, cases.SEED_SETS[0])


def test_untouched_pixels_come_out_equal(capi, cr):
    """impulse noise keeps every element it does not flip; brightness / saturate / contrast keep a black image black."""
    x = torch.from_numpy(cases.images((2, 33, 47)))
    v, _ = launch(capi, cr, "impulse_noise", 3, x, [42, 42], cases.stems(2), 0)
    changed = v != x
    assert 0.02 < float(changed.float().mean()) < 0.2 and set(v[changed].unique().tolist()) <= {0, 255}
    zero = torch.zeros(1, 32, 32, 3, dtype=torch.uint8)
    for name in ("gaussian_blur", "defocus_blur", "motion_blur", "zoom_blur", "contrast", "saturate", "pixelate", "speckle_noise", "shot_noise"):
        assert not launch(capi, cr, name, 5, zero, [42], ["z"], 0)[0].any(), name


@pytest.mark.parametrize("name", ref.NAMES)
def test_an_image_alone_equals_itself_in_a_batch(cr, name):
    x = torch.from_numpy(cases.images((3, 40, 32))).cuda()
    seeds, stems = [5, 6, 7], ["p", "q", "r"]
    for sev in (2, 5):
        batch = cr.corrupt(x, name, sev, seeds, stems)
        alone = cr.corrupt(x[2:3].contiguous(), name, sev, seeds[2:], stems[2:])
        assert batch.dtype == torch.uint8 and batch.shape == x.shape and torch.equal(batch[2:3], alone), (name, sev)
        if name in KEYED:                            # the same image under another image's seed differs
            assert not torch.equal(cr.corrupt(x[2:3].contiguous(), name, sev, seeds[:1], stems[:1]), alone), (name, sev)


@pytest.mark.parametrize("name", ("shot_noise", "motion_blur", "fog", "saturate"))
def test_planner_equals_the_primitives_chained_by_hand(capi, cr, name):
    """corrupt.corrupt (one op per group) against `launch`, which drives the C ABI itself."""
    shape = (2, 33, 47)
    x = torch.from_numpy(cases.images(shape))
    for sev in (1, 4):
        for kind in (0, 1):
            by_hand, ok = launch(capi, cr, name, sev, x, [42, 43], cases.stems(2), kind)
            got = cr.corrupt(x.cuda(), name, sev, [42, 43], cases.stems(2), out_kind=kind).cpu()
            assert ok and got.dtype == by_hand.dtype and torch.equal(got.view(torch.uint8), by_hand.view(torch.uint8)), (name, sev, kind)
    assert torch.equal(cr.corrupt(x.cuda(), "clean", 3, 42).cpu(), x)
    with pytest.raises(ValueError, match="32"):
        cr.corrupt(torch.zeros(1, 31, 40, 3, dtype=torch.uint8, device="cuda"), name, 3, 42)
    with pytest.raises(ValueError, match="seeds"):
        cr.corrupt(x.cuda(), name, 3, [1, 2, 3])


SIZES = [("a0", (40, 32)), ("a1", (33, 47)), ("b0", (40, 32)), ("a2", (33, 47)), ("a3", (40, 32)), ("b1", (64, 96)), ("a4", (40, 32))]


def _folder(path, entries=SIZES):
    from unirestore_amd import imageio
    path.mkdir()
    for i, (stem, hw) in enumerate(entries):
        g = torch.Generator().manual_seed(100 + sum(map(ord, stem)))
        imageio.save_u8(torch.randint(0, 256, (*hw, 3), generator=g, dtype=torch.uint8), str(path / f"{stem}.png"))
    return path


def test_corrupted_image_files(cr, tmp_path):
    from unirestore_amd import data, imageio
    src = _folder(tmp_path / "clean")
    d = data.CorruptedImageFiles(str(src), corruptions="fog,motion_blur,shot_noise,clean", severity="mixed", batch_size=2, seed=11)
    seen = []
    for lq, hq, gt, names, task in d.batches(device="cuda"):
        name, sev = d.last
        assert gt is None and task == "ir" and lq.shape == hq.shape and lq.dtype == torch.float32 and lq.shape[1] == 3 and len(names) <= 2
        u8 = torch.stack([imageio.load_u8(str(src / f"{st}.png")) for st in names])
        assert hq.is_cuda and hq.is_contiguous() and lq.is_contiguous()
        assert torch.equal(hq.cpu(), u8.permute(0, 3, 1, 2).float().div(255))            # the values ImageListFiles yields
        assert torch.equal(lq.cpu(), cr.corrupt(u8.cuda(), name, sev, 11, names).cpu().permute(0, 3, 1, 2).float().div(255))
        for st in names:                             # homogeneous in (shape, corruption, severity), each chosen from (seed, stem)
            assert cr.choose(11, st, d.names, "mixed") == (name, sev) and dict(SIZES)[st] == tuple(hq.shape[2:])
        seen += names
    assert sorted(seen) == sorted(st for st, _ in SIZES)
    lst = tmp_path / "list.txt"                      # an `lq hq label` list: the hq column
    lst.write_text("".join(f"nowhere/{st}.png clean/{st}.png 0\n" for st, _ in SIZES[:3]))
    d2 = data.CorruptedImageFiles(str(lst), corruptions="pixelate", severity=2, batch_size=8)
    got = list(d2.batches(device="cuda"))
    assert sorted(n for b in got for n in b[3]) == ["a0", "a1", "b0"] and d2.last == ("pixelate", 2)


def test_validate_reports_by_corruption(tmp_path):
    from restore_worker import tiny_cfg, tiny_model
    from unirestore_amd import cli
    src = _folder(tmp_path / "clean", [(f"v{i}", (64, 64)) for i in range(6)])
    cfg = tiny_cfg()
    cfg["data"] = dict(class_path="unirestore_amd.data.CorruptedImageFiles",
                       init_args=dict(source=str(src), corruptions="weather,digital", severity="mixed", batch_size=2, seed=3))
    res = cli.validate(cfg, model=tiny_model())
    print("validate:", json.dumps(res))
    by = res["by_corruption"]
    assert res["images"] == 6 == sum(v["images"] for v in by.values()) and res["output_finite"]
    assert res["skipped"] == ["snow", "frost", "elastic_transform", "jpeg_compression"]
    assert all(k.split("/")[0] in ("fog", "brightness", "contrast", "pixelate") and 1 <= int(k.split("/")[1]) <= 5 for k in by)
    assert abs(sum(v["psnr"] * v["images"] for v in by.values()) / 6 - res["val_lq/psnr"]) < 1e-9
    assert abs(sum(v["ssim"] * v["images"] for v in by.values()) / 6 - res["val_lq/ssim"]) < 1e-9
    json.dumps(res)
    # any other data class: the keys of the result are what they were
    cfg["data"] = dict(class_path="unirestore_amd.data.SyntheticImages", init_args=dict(resolution=[64, 64], batch_size=2, num_batches=2))
    plain = cli.validate(cfg, model=tiny_model())
    assert sorted(plain) == sorted(["config", "dtype", "n_gpus", "denoise_steps", "images_per_s", "output_finite", "val_lq/psnr",
                                    "val_lq/ssim", "images"]) and plain["images"] == 4


def _read(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def test_cli_corrupt_writes_files_that_depend_on_the_file_alone(tmp_path, capsys):
    from unirestore_amd import cli, data
    entries = [("X", (40, 32)), ("Y", (40, 32)), ("Z", (33, 47))]
    xy = _folder(tmp_path / "xy", entries[:2])
    xyz = _folder(tmp_path / "xyz", entries)
    yx = tmp_path / "yx.txt"
    yx.write_text("xy/Y.png\nxy/X.png\n")
    which = "fog,motion_blur,impulse_noise,pixelate"
    res = cli.corrupt_files(str(xy), str(tmp_path / "o1"), which, "mixed", seed=9, batch=2)
    cli.corrupt_files(str(yx), str(tmp_path / "o2"), which, "mixed", seed=9, batch=1)
    cli.corrupt_files(str(xyz), str(tmp_path / "o3"), which, "mixed", seed=9, batch=3)
    assert res["images"] == 2 and res["corruptions"] == which.split(",") and res["skipped"] == []
    folders = sorted(os.listdir(tmp_path / "o1"))
    assert folders == res["folders"] and {f.rsplit("_", 1)[0] for f in folders} == set(which.split(","))
    found = 0
    for f in folders:
        a, b, c = _read(tmp_path / "o1" / f), _read(tmp_path / "o2" / f), _read(tmp_path / "o3" / f)
        for png in (k for k in a if k.endswith(".png")):
            assert a[png] == b[png] == c[png], (f, png)                            # order, batching and a third file change nothing
            found += 1
        pairs = data.ImageListFiles(str(tmp_path / "o1" / f / "pairs.txt"), batch_size=4)
        for lq, hq, _, names, _ in pairs.batches(device="cuda"):
            assert lq.shape == hq.shape and not torch.equal(lq, hq) and set(names) <= {"X", "Y"}
    assert found == 2 * 4
    other = cli.corrupt_files(str(xy), str(tmp_path / "o4"), "fog", 3, seed=10)
    assert other["folders"] == ["fog_3"] and _read(tmp_path / "o4" / "fog_3")["X.png"] != \
        _read(cli.corrupt_files(str(xy), str(tmp_path / "o5"), "fog", 3, seed=9)["output"] + "/fog_3")["X.png"]
    assert cli.main(["corrupt", "--input", str(xy), "--output", str(tmp_path / "o6"), "--corruptions", "digital", "--severity", "2"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["folders"] == ["contrast_2", "pixelate_2"] and line["skipped"] == ["elastic_transform", "jpeg_compression"]
