"""Keyed noise without a GPU: the reference generator against published and recorded answers, the seed of a file, what the
`restore` plan does to seeds and names, and every argument error that is raised before a GPU is looked at."""
import ctypes
import os

import numpy as np
import pytest
import torch

import keyed_noise_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


# ---- the generator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,counter,want", [
    ((0, 0), (0, 0, 0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 2, (0xffffffff,) * 4, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_random123_known_answers(key, counter, want):
    assert _hex(ref.philox4x32_10(np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32))) == want


def test_layout_known_answers():
    seed = 2 ** 32 + 5
    assert ref.key_of(seed).tolist() == [5, 1]
    assert _hex(ref.words(seed, 0, 4)) == "009b863c a701829e cdd07445 6fcd431d"
    assert _hex(ref.words(seed, 1, 16)[12:16]) == "7ee89035 68127fa1 781846a7 5432528b"
    # element e = counter e >> 2, word e & 3: a shorter count is a prefix, the draw is counter word 1
    assert np.array_equal(ref.words(seed, 1, 14), ref.words(seed, 1, 16)[:14])
    ctr = np.array([3, 1, 0, 0], dtype=np.uint32)
    assert np.array_equal(ref.philox4x32_10(ctr, ref.key_of(seed)), ref.words(seed, 1, 16)[12:16])


def test_reference_normals():
    u = ref.uniforms(np.array([0, 0xffffffff, 0x1ff, 0x200], dtype=np.uint32))
    assert u.tolist() == [2.0 ** -24, 1 - 2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -24]
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)              # 24 significant bits: exact in fp32
    v = ref.normals(7, 0, 65536)
    assert np.isfinite(v).all() and np.abs(v).max() <= ref.MAX_ABS < 5.77
    assert abs(v.mean()) < 4 / 256 and abs(v.std() - 1) < 0.02                     # 4 sigma of the mean of 65 536 normals
    w = ref.words(7, 0, 4)
    ua, ub = ref.uniforms(w[:2])
    r = np.sqrt(-2 * np.log(ua))
    assert np.allclose(v[:2], [r * np.cos(2 * np.pi * ub), r * np.sin(2 * np.pi * ub)], rtol=0, atol=1e-15)
    out = ref.keyed_noise([7, 9], 0, (2, 3, 5))
    assert out.shape == (2, 2, 3, 5) and np.array_equal(out[0].reshape(-1), v[:30])
    assert np.array_equal(ref.keyed_noise([9], 0, (2, 3, 5))[0], out[1])            # an image's noise is its seed's alone


# ---- ops ----------------------------------------------------------------------------------------------------------------------
def test_noise_keys():
    from unirestore_amd import ops
    k = ops.noise_keys([0, 2 ** 32 + 5, 2 ** 64 - 1, 0x89abcdef01234567])
    assert k.dtype == torch.int32 and tuple(k.shape) == (4, 2) and not k.is_cuda
    assert k.numpy().view(np.uint32).tolist() == [[0, 0], [5, 1], [0xffffffff, 0xffffffff], [0x01234567, 0x89abcdef]]
    assert ops.noise_keys(np.array([3], dtype=np.int64)).tolist() == [[3, 0]]
    for bad in ([-1], [2 ** 64], [1, 2 ** 64 + 1], [1.5], ["7"], [None], [True], []):
        with pytest.raises(ValueError, match="noise_keys"):
            ops.noise_keys(bad)


def test_keyed_noise_argument_errors_before_the_gpu():
    from unirestore_amd import ops
    keys = ops.noise_keys([1, 2])
    with pytest.raises(ValueError, match="kind"):
        ops.keyed_noise(keys, 0, (4, 8, 8), kind="uniform")
    for bad in (keys.float(), keys[:, :1].contiguous(), keys.reshape(-1), keys[:0], keys.t().contiguous().t(), [[1, 2]]):
        with pytest.raises(ValueError, match="keys"):
            ops.keyed_noise(bad, 0, (4, 8, 8))


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """UR_E_INVALID comes from the argument checks, which run before the first HIP call: no GPU is needed to see them."""
    from unirestore_amd import capi
    buf = (ctypes.c_uint32 * 8)()
    p = ctypes.addressof(buf)
    bad = [(None, 0, p, 1, 4, 0), (p, 0, None, 1, 4, 0), (p, 0, p, 0, 4, 0), (p, 0, p, -1, 4, 0), (p, 0, p, 1, 0, 0),
           (p, 0, p, 1, -4, 0), (p, 0, p, 1, 2 ** 34 + 1, 0), (p, 0, p, 1, 4, 2), (p, 0, p, 1, 4, -1)]
    for args in bad:
        assert capi.lib.ur_keyed_noise(*args, None) == capi.UR_E_INVALID, args
        assert b"ur_keyed_noise" in capi.lib.ur_last_error()
    assert list(buf) == [0] * 8


def test_model_seed_arguments():
    import unirestore_amd.modules as M
    keys = M.DiffUIE._seed_keys([5, 2 ** 64 - 1], None, 2)
    assert keys.tolist() == [[5, 0], [-1, -1]] and M.DiffUIE._seed_keys(None, None, 2) is None
    with pytest.raises(ValueError, match="exclude"):
        M.DiffUIE._seed_keys([1, 2], (torch.zeros(1), torch.zeros(1)), 2)
    for bad in ([1], [1, 2, 3], []):
        with pytest.raises(ValueError, match="one per image"):
            M.DiffUIE._seed_keys(bad, None, 2)
    with pytest.raises(ValueError, match="2\\^64"):
        M.DiffUIE._seed_keys([1, -2], None, 2)
    assert M.DiffUIE._seeded_key(None) == () and M.DiffUIE._seeded_key(keys) == ("seeded",)


# ---- the command --------------------------------------------------------------------------------------------------------------
def test_image_seed():
    from unirestore_amd import cli
    assert cli.image_seed(42, "photo", 0) == 14853340700088893816
    seeds = {cli.image_seed(s, stem, k) for s in (42, 43) for stem in ("photo", "photo2", "phot") for k in (0, 1, 10)}
    assert len(seeds) == 18 and all(0 <= v < 2 ** 64 for v in seeds)
    assert cli.image_seed(4, "2\x003", 0) != cli.image_seed(42, "3", 0)


def _seeds_by_name(stems, sizes, batch, world=1, samples=1, seed=7):
    """{output name: seed} over the plans of all ranks, as `restore --noise image` hands them to forward_u8, and the valid slots."""
    from unirestore_amd import cli, imageio
    units = cli.plan_samples([f"/in/{s}.png" for s in stems], samples)
    planned = [hw for hw in sizes for _ in range(samples)]
    out, written = {}, []
    for rank in range(world):
        for b in imageio.plan_batches(planned, batch, rank, world):
            seeds = cli.batch_seeds(seed, units, b.members)
            assert len(seeds) == len(b.members)
            for slot, (i, s) in enumerate(zip(b.members, seeds)):
                name = cli.output_name(units[i][1], units[i][2], samples)
                assert out.setdefault(name, s) == s                                  # a repeated slot carries the repeated seed
                assert s == cli.image_seed(seed, units[i][1], units[i][2])
                if slot < b.valid:
                    written.append(name)
    assert len(written) == len(set(written)) == len(stems) * samples
    return out


def test_seeds_do_not_depend_on_the_plan():
    stems = ["a0", "a1", "b0", "a2", "a3", "b1", "a4"]
    sizes = [(96, 80), (100, 84), (80, 96), (90, 76), (96, 80), (80, 96), (100, 84)]           # two canvases, a padded batch at 3
    base = _seeds_by_name(stems, sizes, 3)
    assert sorted(base) == sorted(f"{s}.png" for s in stems) and len(set(base.values())) == 7
    for batch, world in ((1, 1), (2, 1), (8, 1), (3, 2), (2, 3)):
        assert _seeds_by_name(stems, sizes, batch, world) == base
    order = [4, 0, 6, 2, 1, 5, 3]
    assert _seeds_by_name([stems[i] for i in order], [sizes[i] for i in order], 3) == base     # list order
    more = _seeds_by_name(["_new"] + stems + ["zz"], [(96, 80)] + sizes + [(80, 96)], 3)       # unrelated files
    assert {k: more[k] for k in base} == base
    assert _seeds_by_name(stems, sizes, 3, seed=8)["a0.png"] != base["a0.png"]


def test_samples_planning_and_names():
    from unirestore_amd import cli, imageio
    assert cli.plan_samples(["/x/a.png", "/y/b.jpg"], 2) == [("/x/a.png", "a", 0), ("/x/a.png", "a", 1), ("/y/b.jpg", "b", 0),
                                                           ("/y/b.jpg", "b", 1)]
    assert cli.plan_samples(["/x/a.png"]) == [("/x/a.png", "a", 0)]
    assert cli.output_name("a", 0, 1) == "a.png" and [cli.output_name("a", k, 3) for k in range(3)] == ["a.s0.png", "a.s1.png", "a.s2.png"]
    stems, sizes = ["a", "b", "c"], [(96, 80), (80, 96), (96, 80)]
    k3 = _seeds_by_name(stems, sizes, 2, samples=3)
    assert sorted(k3) == sorted(f"{s}.s{k}.png" for s in stems for k in range(3)) and len(set(k3.values())) == 9
    k1 = _seeds_by_name(stems, sizes, 2)
    assert all(k3[f"{s}.s0.png"] == k1[f"{s}.png"] for s in stems)                             # sample 0 is the K = 1 seed
    # the samples of an input are consecutive slots of its canvas group (a's and c's share one; b's last batch is padded)
    plan = imageio.plan_batches([hw for hw in sizes for _ in range(3)], 2)
    assert [b.members for b in plan] == [(0, 1), (2, 6), (3, 4), (5, 5), (7, 8)]


def test_restore_argument_errors(tmp_path, capsys):
    from unirestore_amd import cli
    assert cli.check_noise_args() == ("batch", 1) and cli.check_noise_args("image", 4) == ("image", 4)
    with pytest.raises(ValueError, match="--noise"):
        cli.check_noise_args("slot", 1)
    for bad in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError, match="--samples"):
            cli.check_noise_args("image", bad)
    with pytest.raises(ValueError, match="--samples 2 needs --noise image"):
        cli.check_noise_args("batch", 2)
    # restore() and the command line refuse before the config, the inputs or a GPU are looked at
    with pytest.raises(ValueError, match="needs --noise image"):
        cli.restore({}, str(tmp_path / "missing"), str(tmp_path / "out"), samples=2)
    cfg = os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")
    for argv, word in ((["--samples", "2"], "needs --noise image"), (["--noise", "image", "--samples", "0"], "--samples 0"),
                       (["--noise", "slot"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            cli.main(["restore", "--config", cfg, "--input", str(tmp_path / "missing"), "--output", str(tmp_path / "out")] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
