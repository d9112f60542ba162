"""The glass blur / snow / elastic transform kernels (csrc/distort.hip) against the fp64 reference of distort_reference.py, element
by element: every stage alone from host-made inputs, the three pipelines end to end, and the layers above them (distort.distort,
distort.degrade, data.DistortedImageFiles, cli.validate, cli distort).  The cases, bounds, masks and the reference are stated in
distort_cases.py / distort_reference.py; this file launches and compares.  Every launch goes through the C ABI on guarded buffers:
guards and inputs untouched, a second launch bit-identical, the fp32 values (out_kind 1) within the derived bound plus the propagated
ambiguity mask, the bytes (out_kind 0) equal to the floor of the fp32 values of the same arguments."""
import json
import os

import numpy as np
import pytest
import torch

import corrupt_reference as cref
import distort_cases as cases
import distort_reference as ref
from test_boundary_launchers_gpu import Buf

pytestmark = pytest.mark.gpu

SEVS = cases.SEVS
WORST = {}                      # stage or pipeline -> largest |value - reference| / bound seen
_REF = {}                       # (name, shape, kind, severity, seed) -> (values, bounds, masks): computed once, shared, read-only


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    yield c
    if WORST:
        print("\nlargest |value - fp64 reference| / bound per stage:")
        for name, r in sorted(WORST.items()):
            print(f"  {name:20s} {r:.3f}")


@pytest.fixture(scope="module")
def ds():
    from unirestore_amd import distort
    return distort


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _table(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    b = Buf(tuple(t.shape), t.dtype, fill=t.cuda())
    b.orig = t
    return b


def _keys(seeds, stems):
    from unirestore_amd import corrupt, ops
    return _table(ops.noise_keys([corrupt.corruption_seed(s, t) for s, t in zip(seeds, stems)]).numpy())


def _work(nbytes):
    return Buf(((nbytes + 7) // 8 * 2,), torch.int32)


def _done(ins, outs):
    """After the launch: every guard intact, inputs and tables as they were."""
    torch.cuda.synchronize()
    return all(b.guards_ok() for b in ins + outs) and all(torch.equal(b.t.cpu().view(torch.uint8), b.orig.view(torch.uint8)) for b in ins)


def _note(stage, err, bound):
    WORST[stage] = max(WORST.get(stage, 0.0), float((err / np.maximum(bound, 1e-300)).max()))


# ---- the primitives through the C ABI -------------------------------------------------------------------------------------------
def shuffle(capi, x, seeds, stems, delta, draw):
    n, h, w, _ = x.shape
    xb, kb, out = _table(x), _keys(seeds, stems), Buf(tuple(x.shape), torch.uint8)
    rc = capi.lib.ur_distort_shuffle(xb.ptr, kb.ptr, out.ptr, n, h, w, delta, draw, _stream())
    assert rc == 0, capi.lib.ur_last_error()
    return out.t.cpu().numpy(), _done([xb, kb], [out])


def snow_layer(capi, n, h, w, seeds, stems, geometry, loc, scale, thr):
    kb, field = _keys(seeds, stems), Buf((n, geometry[4], geometry[5]), torch.float32)
    rc = capi.lib.ur_distort_snow_layer(kb.ptr, field.ptr, n, h, w, *geometry, loc, scale, thr, _stream())
    assert rc == 0, capi.lib.ur_last_error()
    return field.t.cpu().numpy(), _done([kb], [field])


def snow_blend(capi, x, field, taps, keep, out_kind):
    n, h, w, _ = x.shape
    xb, fb, tb = _table(x), _table(field), _table(taps)
    out, ws = Buf(tuple(x.shape), torch.float32 if out_kind else torch.uint8), _work(capi.lib.ur_distort_snow_ws_bytes(n, h, w))
    rc = capi.lib.ur_distort_snow(xb.ptr, fb.ptr, tb.ptr, taps.shape[1], out.ptr, n, h, w, field.shape[1], field.shape[2], keep, ws.ptr,
                                  capi.lib.ur_distort_snow_ws_bytes(n, h, w), out_kind, _stream())
    assert rc == 0, capi.lib.ur_last_error()
    return out.t.cpu().numpy(), _done([xb, fb, tb], [out, ws])


def elastic_field(capi, n, h, w, seeds, stems, ty, tx, m, alpha):
    kb, tyb, txb = _keys(seeds, stems), _table(ty.astype(np.float32)), _table(tx.astype(np.float32))
    field, ws = Buf((n, 2, h, w), torch.float32), _work(capi.lib.ur_distort_field_ws_bytes(n, h, w))
    rc = capi.lib.ur_distort_field(kb.ptr, tyb.ptr, len(ty) // 2, txb.ptr, len(tx) // 2, field.ptr, n, h, w, m, alpha, ws.ptr,
                                   capi.lib.ur_distort_field_ws_bytes(n, h, w), _stream())
    assert rc == 0, capi.lib.ur_last_error()
    return field.t.cpu().numpy(), _done([kb, tyb, txb], [field, ws])


def warp(capi, x, field, out_kind):
    n, h, w, _ = x.shape
    xb, fb, out = _table(x), _table(field), Buf(tuple(x.shape), torch.float32 if out_kind else torch.uint8)
    rc = capi.lib.ur_distort_warp(xb.ptr, fb.ptr, out.ptr, n, h, w, out_kind, _stream())
    assert rc == 0, capi.lib.ur_last_error()
    return out.t.cpu().numpy(), _done([xb, fb], [out])


def gaussian(capi, x, sigma, out_kind):
    """ur_corrupt_filter_sep with gaussian_blur's taps: the first and the last step of glass blur."""
    from unirestore_amd import corrupt
    n, h, w, _ = x.shape
    taps = corrupt.gaussian_taps(sigma).astype(np.float32)
    xb, tb, out = _table(x), _table(taps), Buf(tuple(x.shape), torch.float32 if out_kind else torch.uint8)
    ws = _work(capi.lib.ur_corrupt_filter_sep_ws_bytes(n, h, w))
    rc = capi.lib.ur_corrupt_filter_sep(xb.ptr, tb.ptr, len(taps) // 2, out.ptr, n, h, w, ws.ptr, capi.lib.ur_corrupt_filter_sep_ws_bytes(n, h, w),
                                        out_kind, _stream())
    assert rc == 0, capi.lib.ur_last_error()
    return out.t.cpu().numpy(), _done([xb, tb], [out, ws])


def snow_taps(ds, geometry, sev, seeds, stems):
    from unirestore_amd import corrupt
    radius, sigma = ds.SEVERITY["snow"][sev - 1][4:6]
    lists = [corrupt.motion_taps(geometry[4], geometry[5], radius, sigma, ds.snow_angle(s, t)) for s, t in zip(seeds, stems)]
    taps = np.zeros((len(lists), max(len(t) for t in lists), 3))
    for i, t in enumerate(lists):
        taps[i, :len(t)] = t
    return corrupt.pack_taps(taps)


def launch(capi, ds, name, sev, x, seeds, stems, out_kind):
    """Corruption `name` of the u8 batch x (numpy) through the primitives of the C ABI chained by hand, every buffer guarded.
    -> (out on the host, inputs untouched and all guards intact)."""
    n, h, w, _ = x.shape
    c = ds.SEVERITY[name][sev - 1]
    if name == "glass_blur":
        a, ok = gaussian(capi, x, c[0], 0)
        for i in range(c[2]):
            a, ok_i = shuffle(capi, a, seeds, stems, c[1], ds.DRAW_GLASS + 2 * i)
            ok = ok and ok_i
        out, ok2 = gaussian(capi, a, c[0], out_kind)
        return out, ok and ok2
    if name == "snow":
        geometry = ds.snow_geometry(h, w, c[2])
        field, ok = snow_layer(capi, n, h, w, seeds, stems, geometry, c[0], c[1], c[3])
        out, ok2 = snow_blend(capi, x, field, snow_taps(ds, geometry, sev, seeds, stems), c[6], out_kind)
        return out, ok and ok2
    ty, tx = ds.elastic_taps(h, w)
    field, ok = elastic_field(capi, n, h, w, seeds, stems, ty, tx, 0.005 * h, c)
    out, ok2 = warp(capi, x, field, out_kind)
    return out, ok and ok2


# ---- 1. every stage alone, from host-made inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_shuffle_is_byte_exact(capi, shape):
    from unirestore_amd import corrupt
    x, stems = cases.images(shape), cases.stems(shape[0])
    for seed in cases.SEED_SETS:
        for delta in cases.DELTAS:
            for draw in cases.DRAW_PAIRS:
                got, ok = shuffle(capi, x, [seed] * shape[0], stems, delta, draw)
                again, ok2 = shuffle(capi, x, [seed] * shape[0], stems, delta, draw)
                want = np.stack([ref.shuffle(x[i], corrupt.corruption_seed(seed, st), delta, draw) for i, st in enumerate(stems)])
                assert ok and ok2 and np.array_equal(got, again) and np.array_equal(got, want), (shape, seed, delta, draw)
        assert not np.array_equal(got, x)


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_snow_layer_stage(capi, ds, shape):
    from unirestore_amd import corrupt
    n, h, w = shape
    stems = cases.stems(n)
    for sev in SEVS:
        loc, scale, zoom, thr = ds.SEVERITY["snow"][sev - 1][:4]
        geometry = ds.snow_geometry(h, w, zoom)
        for seed in cases.SEED_SETS + tuple(c[3] for c in cases.UNCAPPED if c[1] == shape and c[2] == sev):
            got, ok = snow_layer(capi, n, h, w, [seed] * n, stems, geometry, loc, scale, thr)
            again, ok2 = snow_layer(capi, n, h, w, [seed] * n, stems, geometry, loc, scale, thr)
            assert ok and ok2 and np.array_equal(got.view(np.int32), again.view(np.int32)), (shape, sev, seed)
            for i, st in enumerate(stems):
                want, e_l, amb, kept, exact = ref.snow_layer(h, w, sev, corrupt.corruption_seed(seed, st))
                v = got[i].astype(np.float64)
                err = np.abs(v - want)
                other = np.abs(v - np.where(want == 0.0, kept, 0.0))        # an ambiguous cell may take either branch
                _note("snow_layer", np.where(amb, 0.0, err), e_l)
                print(f"snow_layer {shape} severity {sev} seed {seed} image {i}: max |err| {np.where(amb, 0.0, err).max():.3e}, bound {e_l:.3e}, "
                      f"ambiguous cells {int(amb.sum())}")
                assert (np.where(amb, np.minimum(err, other), err) <= e_l).all(), (shape, sev, seed, i, float(err.max()))
                assert v.min() >= 0.0 and v.max() <= 1.0 and v.shape == tuple(geometry[4:]) and np.array_equal(v[exact], want[exact])


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_snow_stage_on_a_host_made_field(capi, ds, shape):
    n, h, w = shape
    x, stems = cases.images(shape), cases.stems(n)
    for sev in SEVS:
        zoom, radius, sigma, keep = ds.SEVERITY["snow"][sev - 1][2], *ds.SEVERITY["snow"][sev - 1][4:]
        geometry = ds.snow_geometry(h, w, zoom)
        field = cases.snow_field(n, geometry[4], geometry[5], sev)
        for seed in cases.SEED_SETS:
            taps = snow_taps(ds, geometry, sev, [seed] * n, stems)
            val, ok1 = snow_blend(capi, x, field, taps, keep, 1)
            again, ok2 = snow_blend(capi, x, field, taps, keep, 1)
            u8, ok3 = snow_blend(capi, x, field, taps, keep, 0)
            assert ok1 and ok2 and ok3 and np.array_equal(val.view(np.int32), again.view(np.int32)), (shape, sev, seed)
            assert np.array_equal(u8, np.floor(val).astype(np.uint8)), (shape, sev, seed)
            for i, st in enumerate(stems):
                shifts = cref.motion_shifts(geometry[4], geometry[5], radius, sigma, ref.snow_angle(seed, st))
                want, bound, info = ref.snow_blend(x[i], field[i].astype(np.float64), shifts, keep)
                err = np.abs(val[i].astype(np.float64) - want)
                _note("snow", err, bound)
                print(f"snow stage {shape} severity {sev} seed {seed} image {i}: max |err| {err.max():.3e}, ambiguous roundings "
                      f"{100 * info['share']:.3f} %, max |err| where the mask is 0: {err[info['mask'] == 0].max():.3e}")
                assert (err <= bound).all(), (shape, sev, seed, i, float(err.max()))
                assert info["share"] <= 0.01


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_elastic_field_stage(capi, ds, shape):
    from unirestore_amd import corrupt
    n, h, w = shape
    stems = cases.stems(n)
    ty, tx = ds.elastic_taps(h, w)
    for sev in SEVS:
        for seed in cases.SEED_SETS:
            got, ok = elastic_field(capi, n, h, w, [seed] * n, stems, ty, tx, 0.005 * h, ds.SEVERITY["elastic_transform"][sev - 1])
            again, ok2 = elastic_field(capi, n, h, w, [seed] * n, stems, ty, tx, 0.005 * h, ds.SEVERITY["elastic_transform"][sev - 1])
            assert ok and ok2 and np.array_equal(got.view(np.int32), again.view(np.int32)), (shape, sev, seed)
            for i, st in enumerate(stems):
                want, bound = ref.elastic_field(h, w, sev, corrupt.corruption_seed(seed, st))
                err = np.abs(got[i].astype(np.float64) - want)
                _note("elastic_field", err, bound)
                print(f"elastic field {shape} severity {sev} seed {seed} image {i}: max |err| {err.max():.3e}, bound {bound:.3e}, max |d| {np.abs(want).max():.2f}")
                assert (err <= bound).all(), (shape, sev, seed, i, float(err.max()), bound)
                assert np.abs(want).max() > 0.05 and not np.array_equal(got[i][0], got[i][1])


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_warp_stage_on_host_made_fields(capi, shape):
    n, h, w = shape
    x = cases.images(shape)
    for kind in ("zero", "smooth", "outward"):
        field = cases.warp_field(n, h, w, kind)
        val, ok1 = warp(capi, x, field, 1)
        again, ok2 = warp(capi, x, field, 1)
        u8, ok3 = warp(capi, x, field, 0)
        assert ok1 and ok2 and ok3 and np.array_equal(val.view(np.int32), again.view(np.int32)), (shape, kind)
        assert np.array_equal(u8, np.floor(val).astype(np.uint8)), (shape, kind)
        if kind == "zero":                               # an all-zero field returns x exactly
            assert np.array_equal(u8, x) and np.array_equal(val, x.astype(np.float32))
        for i in range(n):
            want, bound = ref.warp(x[i], field[i].astype(np.float64))
            err = np.abs(val[i].astype(np.float64) - want)
            _note("warp", err, bound)
            print(f"warp {shape} {kind} image {i}: max |err| {err.max():.3e}, max bound {bound.max():.3e}")
            assert (err <= bound).all(), (shape, kind, i, float(err.max()))


# ---- 2. the three pipelines end to end ----------------------------------------------------------------------------------------------
def reference(name, shape, kind, sev, seed):
    from unirestore_amd import corrupt
    key = (name, shape, kind, sev, seed)
    if key not in _REF:
        x = cases.images(shape, kind)
        rows = [ref.run(name, x[i], sev, corrupt.corruption_seed(seed, st), ref.snow_angle(seed, st)) for i, st in enumerate(cases.stems(shape[0]))]
        def mask_of(r):                                  # [H, W] (snow, elastic) or [H, W, 3] (glass) -> [H, W, 3]
            m = r[2]["mask"]
            return np.broadcast_to(m[..., None] if m.ndim == 2 else m, x[0].shape)
        out = (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([mask_of(r) for r in rows]))
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def check(capi, ds, name, shape, kind, sev, seed):
    x = cases.images(shape, kind)
    stems, seeds = cases.stems(shape[0]), [seed] * shape[0]
    val, ok1 = launch(capi, ds, name, sev, x, seeds, stems, 1)
    again, ok2 = launch(capi, ds, name, sev, x, seeds, stems, 1)
    u8, ok3 = launch(capi, ds, name, sev, x, seeds, stems, 0)
    what = (name, shape, kind, sev, seed)
    assert ok1 and ok2 and ok3, what                                   # guards and inputs
    assert np.array_equal(val.view(np.int32), again.view(np.int32)), what          # a second launch: the same bits
    v = val.astype(np.float64)
    want, bound, mask = reference(name, shape, kind, sev, seed)
    err = np.abs(v - want)
    _note(name, err, bound)
    print(f"{name} {shape} {kind} severity {sev} seed {seed}: max |err| {err.max():.3e}, max bound {bound.max():.3e}, max ratio "
          f"{float((err / bound).max()):.3f}, elements under a mask {100 * float((mask > 0).mean()):.2f} %")
    assert (err <= bound).all(), (what, float(err.max()), float(bound.max()))
    assert v.min() >= 0.0 and v.max() <= 255.0, what
    assert np.array_equal(u8, np.floor(v).astype(np.uint8)), what              # the bytes are the floor of the values
    diff = np.abs(u8.astype(np.int64) - np.floor(want).astype(np.int64))
    sure = mask < 1
    assert not sure.any() or diff[sure].max() <= 1, (what, int(diff[sure].max()))


@pytest.mark.parametrize("name", ref.NAMES)
def test_against_fp64(capi, ds, name):
    for shape in cases.SHAPES:
        for sev in SEVS:
            for seed in cases.SEED_SETS:
                check(capi, ds, name, shape, "random", sev, seed)
    for kind in cases.KINDS[1:]:                     # constant 0, constant 255 (wholly ambiguous in glass's floor: no cap), the grey ramp
        for sev in SEVS:
            check(capi, ds, name, (2, 33, 47), kind, sev, cases.SEED_SETS[0])
    for uncapped, shape, sev, seed in cases.UNCAPPED:  # above the cap (distort_cases.py): the propagated masks at work, no cap
        if uncapped == name:
            check(capi, ds, name, shape, "random", sev, seed)


# ---- 3. properties --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.NAMES)
def test_an_image_alone_equals_itself_in_a_batch(ds, name):
    x = torch.from_numpy(cases.images((3, 40, 32))).cuda()
    seeds, stems = [5, 6, 7], ["p", "q", "r"]
    for sev in (2, 5):
        batch = ds.distort(x, name, sev, seeds, stems)
        alone = ds.distort(x[2:3].contiguous(), name, sev, seeds[2:], stems[2:])
        assert batch.dtype == torch.uint8 and batch.shape == x.shape and torch.equal(batch[2:3], alone), (name, sev)
        assert not torch.equal(ds.distort(x[2:3].contiguous(), name, sev, seeds[:1], stems[:1]), alone), (name, sev)       # another image's seed
        assert torch.equal(ds.distort(x, name, sev, seeds, stems), batch)


@pytest.mark.parametrize("name", ref.NAMES)
def test_planner_equals_the_primitives_chained_by_hand(capi, ds, name):
    shape = (2, 33, 47)
    x = cases.images(shape)
    for sev in (1, 4):
        for kind in (0, 1):
            by_hand, ok = launch(capi, ds, name, sev, x, [42, 43], cases.stems(2), kind)
            got = ds.distort(torch.from_numpy(x).cuda(), name, sev, [42, 43], cases.stems(2), out_kind=kind).cpu().numpy()
            assert ok and got.dtype == by_hand.dtype and np.array_equal(got.view(np.uint8), by_hand.view(np.uint8)), (name, sev, kind)
    with pytest.raises(ValueError, match="32"):
        ds.distort(torch.zeros(1, 31, 40, 3, dtype=torch.uint8, device="cuda"), name, 3, 42)
    with pytest.raises(ValueError, match="seeds"):
        ds.distort(torch.from_numpy(x).cuda(), name, 3, [1, 2, 3])


def test_black_images(capi, ds):
    """glass_blur and elastic_transform keep a black image black; snow on it is (1 - keep) * 127.5 plus the flakes: the bytes L of
    the layer and of its 180-degree rotation, integers."""
    zero = np.zeros((1, 32, 32, 3), dtype=np.uint8)
    for sev in SEVS:
        assert not launch(capi, ds, "glass_blur", sev, zero, [42], ["z"], 0)[0].any()
        assert not launch(capi, ds, "elastic_transform", sev, zero, [42], ["z"], 0)[0].any()
        keep = float(np.float32(ds.SEVERITY["snow"][sev - 1][6]))
        v = launch(capi, ds, "snow", sev, zero, [42], ["z"], 1)[0][0].astype(np.float64)
        flakes = v[..., 0] - (1.0 - keep) * 127.5
        free = v[..., 0] < 255.0
        assert np.array_equal(v[..., 0], v[..., 1]) and np.array_equal(v[..., 1], v[..., 2]) and flakes.max() > 0
        assert np.abs(flakes - np.rint(flakes))[free].max() < 1e-4 and np.abs(flakes - flakes[::-1, ::-1]).max() < 1e-4, sev


def test_degrade_bytes_do_not_depend_on_the_batch(ds):
    x = torch.from_numpy(cases.images((3, 40, 32))).cuda()
    seeds, stems = [5, 6, 7], ["p", "q", "r"]
    for name in ds.NAMES:
        batch = ds.degrade(x, name, 3, seeds, stems, resize=(32, 40))
        assert batch.dtype == torch.uint8 and batch.shape == x.shape
        for i in range(3):
            assert torch.equal(ds.degrade(x[i:i + 1].contiguous(), name, 3, seeds[i:i + 1], stems[i:i + 1], resize=(32, 40)), batch[i:i + 1]), (name, i)
        assert torch.equal(ds.degrade(x, name, 3, seeds, stems), ds.distort(x, name, 3, seeds, stems))


# ---- 4. files ---------------------------------------------------------------------------------------------------------------------------
def _folder(path, entries):
    from unirestore_amd import imageio
    path.mkdir()
    for stem, hw in entries:
        g = torch.Generator().manual_seed(100 + sum(map(ord, stem)))
        imageio.save_u8(torch.randint(0, 256, (*hw, 3), generator=g, dtype=torch.uint8), str(path / f"{stem}.png"))
    return path


def _read(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def test_distorted_image_files_through_validate(ds, tmp_path):
    from restore_worker import tiny_cfg, tiny_model
    from unirestore_amd import cli, data, imageio
    src = _folder(tmp_path / "clean", [(f"v{i}", (64, 64)) for i in range(6)])
    d = data.DistortedImageFiles(str(src), corruptions="all", severity="mixed", batch_size=2, seed=3)
    seen = []
    for lq, hq, gt, names, task in d.batches(device="cuda"):
        name, sev = d.last
        u8 = torch.stack([imageio.load_u8(str(src / f"{st}.png")) for st in names])
        assert gt is None and task == "ir" and lq.shape == hq.shape and lq.dtype == torch.float32 and len(names) <= 2
        assert torch.equal(lq.cpu(), ds.distort(u8.cuda(), name, sev, 3, names).cpu().permute(0, 3, 1, 2).float().div(255))
        assert all(ds.choose(3, st, d.names, "mixed") == (name, sev) for st in names)
        seen += names
    assert sorted(seen) == [f"v{i}" for i in range(6)]
    cfg = tiny_cfg()
    cfg["data"] = dict(class_path="unirestore_amd.data.DistortedImageFiles",
                       init_args=dict(source=str(src), corruptions="snow,elastic_transform,glass_blur", severity="mixed", batch_size=2, seed=3))
    res = cli.validate(cfg, model=tiny_model())
    print("validate:", json.dumps(res))
    by = res["by_corruption"]
    assert res["images"] == 6 == sum(v["images"] for v in by.values()) and res["output_finite"] and res["skipped"] == []
    assert all(k.split("/")[0] in ds.NAMES and 1 <= int(k.split("/")[1]) <= 5 for k in by) and len(by) >= 2
    picks = [ds.choose(3, f"v{i}", ["snow", "elastic_transform", "glass_blur"], "mixed") for i in range(6)]
    assert {k: v["images"] for k, v in by.items()} == {f"{n}/{s}": picks.count((n, s)) for n, s in set(picks)}
    assert abs(sum(v["psnr"] * v["images"] for v in by.values()) / 6 - res["val_lq/psnr"]) < 1e-9


def test_cli_distort_writes_files_that_depend_on_the_file_alone(tmp_path, capsys):
    from unirestore_amd import cli, data
    entries = [("X", (40, 32)), ("Y", (40, 32)), ("Z", (33, 47))]
    xy = _folder(tmp_path / "xy", entries[:2])
    xyz = _folder(tmp_path / "xyz", entries)
    yx = tmp_path / "yx.txt"
    yx.write_text("xy/Y.png\nxy/X.png\n")
    res = cli.distort_files(str(xy), str(tmp_path / "o1"), "all", "mixed", seed=9, batch=2)
    cli.distort_files(str(yx), str(tmp_path / "o2"), "all", "mixed", seed=9, batch=1)
    cli.distort_files(str(xyz), str(tmp_path / "o3"), "all", "mixed", seed=9, batch=3)
    cli.distort_files(str(xy), str(tmp_path / "o1b"), "all", "mixed", seed=9, batch=2)                  # a rerun
    assert res["images"] == 2 and res["corruptions"] == ["glass_blur", "snow", "elastic_transform"] and res["skipped"] == []
    folders = sorted(os.listdir(tmp_path / "o1"))
    assert folders == res["folders"] and {f.rsplit("_", 1)[0] for f in folders} == set(res["corruptions"])
    found = 0
    for f in folders:
        a, b, c, again = (_read(tmp_path / o / f) for o in ("o1", "o2", "o3", "o1b"))
        assert a == again and "pairs.txt" in a                                      # a rerun writes equal bytes
        for png in (k for k in a if k.endswith(".png")):
            assert a[png] == b[png] == c[png], (f, png)                            # order, batching and a third file change nothing
            found += 1
        lines = a["pairs.txt"].decode().splitlines()
        assert sorted(l.split()[0] for l in lines) == sorted(k for k in a if k.endswith(".png")) and all(os.path.isabs(l.split()[1]) for l in lines)
        for lq, hq, _, names, _ in data.ImageListFiles(str(tmp_path / "o1" / f / "pairs.txt"), batch_size=4).batches(device="cuda"):
            assert lq.shape == hq.shape and not torch.equal(lq, hq) and set(names) <= {"X", "Y"}
    assert found == 2 * 3
    other = cli.distort_files(str(xy), str(tmp_path / "o4"), "snow", 3, seed=10, resize="32,40")
    assert other["folders"] == ["snow_3"] and other["resize"] == [32, 40] and _read(tmp_path / "o4" / "snow_3")["X.png"] != \
        _read(cli.distort_files(str(xy), str(tmp_path / "o5"), "snow", 3, seed=9, resize="32,40")["output"] + "/snow_3")["X.png"]
    assert cli.main(["distort", "--input", str(xy), "--output", str(tmp_path / "o6"), "--corruptions", "glass_blur,snow", "--severity", "2"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["folders"] == ["glass_blur_2", "snow_2"] and line["skipped"] == [] and line["images"] == 2
