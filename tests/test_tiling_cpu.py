"""Tile plan of tiled latent sampling (unirestore_amd/tiling.py): origins, coverage and blend weights, on the host."""
import copy

import numpy as np
import pytest

from unirestore_amd.tiling import axis_origins, check_tile_stride, default_tile_stride, latent_tile_plan


def test_one_tile_for_a_512px_latent():
    origins, (th, tw), wn = latent_tile_plan(64, 64, 64, 48)
    assert origins == [(0, 0)] and (th, tw) == (64, 64)
    assert wn.dtype == np.float32 and wn.shape == (1, 64, 64)
    assert (wn == 1.0).all()


def test_hand_worked_80x64_tile32_stride24():
    assert axis_origins(80, 32, 24) == ([0, 24, 48], 32)
    assert axis_origins(64, 32, 24) == ([0, 24, 32], 32)
    origins, (th, tw), wn = latent_tile_plan(80, 64, 32, 24)
    assert origins == [(y, x) for y in (0, 24, 48) for x in (0, 24, 32)]      # row-major, y then x
    assert (th, tw) == (32, 32) and wn.shape == (9, 32, 32)


def test_hand_worked_128x256_tile64_stride48():
    assert axis_origins(128, 64, 48) == ([0, 48, 64], 64)
    assert axis_origins(256, 64, 48) == ([0, 48, 96, 144, 192], 64)
    origins, _, wn = latent_tile_plan(128, 256, 64, 48)
    assert len(origins) == 15 and wn.shape == (15, 64, 64)


def test_short_axis_is_one_clamped_tile():
    origins, (th, tw), wn = latent_tile_plan(40, 100, 64, 48)
    assert (th, tw) == (40, 64)
    assert origins == [(0, 0), (0, 36)]
    assert wn.shape == (2, 40, 64)


def test_exact_fit_has_no_duplicate_edge_tile():
    assert axis_origins(112, 64, 48) == ([0, 48], 64)                  # 48 + 64 == 112: the flush tile is the second one
    assert axis_origins(96, 32, 32) == ([0, 32, 64], 32)


@pytest.mark.parametrize("lh,lw,tile,stride", [(80, 64, 32, 24), (128, 256, 64, 48), (128, 128, 64, 48), (208, 120, 64, 48),
                                               (40, 100, 64, 48), (96, 96, 32, 8), (72, 72, 64, 64)])
def test_coverage_and_normalisation(lh, lw, tile, stride):
    origins, (th, tw), wn = latent_tile_plan(lh, lw, tile, stride)
    total = np.zeros((lh, lw), np.float64)
    cover = np.zeros((lh, lw), np.int64)
    for k, (y, x) in enumerate(origins):
        assert 0 <= y and y + th <= lh and 0 <= x and x + tw <= lw
        total[y:y + th, x:x + tw] += wn[k]
        cover[y:y + th, x:x + tw] += 1
    assert (cover >= 1).all()
    assert np.abs(total - 1).max() < 1e-6
    for k, (y, x) in enumerate(origins):
        single = cover[y:y + th, x:x + tw] == 1
        assert (wn[k][single] == np.float32(1.0)).all()
        assert (wn[k] > 0).all()


def test_origins_are_multiples_of_8():
    for lh, lw in ((80, 64), (128, 256), (208, 120), (96, 200)):
        origins, (th, tw), _ = latent_tile_plan(lh, lw, 64, 48)
        assert all(y % 8 == 0 and x % 8 == 0 for y, x in origins) and th % 8 == 0 and tw % 8 == 0


def test_weights_follow_the_gaussian_spec():
    """Independent fp64 evaluation of the spec: w = g(i) g(j), g = exp(-(i-(n-1)/2)^2 / (2 (0.1 n)^2)), normalised per pixel."""
    lh, lw, n = 80, 64, 32
    origins, _, wn = latent_tile_plan(lh, lw, n, 24)
    i = np.arange(n, dtype=np.float64)
    g = np.exp(-(i - (n - 1) / 2) ** 2 / (2 * (0.1 * n) ** 2))
    w = g[:, None] * g[None, :]
    acc = np.zeros((lh, lw))
    cover = np.zeros((lh, lw))
    for y, x in origins:
        acc[y:y + n, x:x + n] += w
        cover[y:y + n, x:x + n] += 1
    for k, (y, x) in enumerate(origins):
        ref = np.where(cover[y:y + n, x:x + n] == 1, 1.0, w / acc[y:y + n, x:x + n]).astype(np.float32)
        np.testing.assert_array_equal(wn[k], ref)


@pytest.mark.parametrize("tile,stride", [(60, 48), (64, 44), (24, 8), (64, 0), (64, 72), (0, 0), (-64, 48), (64.0, 48), (None, 48)])
def test_bad_tile_or_stride_raises(tile, stride):
    with pytest.raises(ValueError):
        latent_tile_plan(128, 128, tile, stride)
    with pytest.raises(ValueError):
        check_tile_stride(tile, stride)


def test_default_stride():
    assert default_tile_stride(64) == 48 and default_tile_stride(32) == 24
    for t in range(32, 257, 8):
        check_tile_stride(t, default_tile_stride(t))


_BASE = {"model": {"class_path": "unirestore_amd.runner.LitUniFIE",
                   "init_args": {"model_kwargs": {"cnet": {"type": "scedit", "num_inference_steps": 20}}}}}


def _cfg(**cnet):
    cfg = copy.deepcopy(_BASE)
    cfg["model"]["init_args"]["model_kwargs"]["cnet"].update(cnet)
    return cfg


def test_cli_resolves_tile_keys():
    from unirestore_amd import cli
    assert "tile_size" not in cli.resolve(_cfg())["model_kwargs"]["cnet"]                      # off unless asked for
    cn = cli.resolve(_cfg(tile_size=64))["model_kwargs"]["cnet"]
    assert (cn["tile_size"], cn["tile_stride"]) == (64, 48)
    cn = cli.resolve(_cfg(tile_size=96, tile_stride=64))["model_kwargs"]["cnet"]
    assert (cn["tile_size"], cn["tile_stride"]) == (96, 64)
    for bad in (dict(tile_size=60), dict(tile_size=64, tile_stride=80), dict(tile_stride=48)):
        with pytest.raises(ValueError):
            cli.resolve(_cfg(**bad))


def test_cli_override_reaches_the_config(tmp_path):
    from unirestore_amd import cli
    p = tmp_path / "c.yaml"
    p.write_text("model:\n  class_path: unirestore_amd.runner.LitUniFIE\n  init_args:\n    model_kwargs:\n"
                 "      cnet: {type: scedit, num_inference_steps: 20}\n")
    cfg = cli.load_config(str(p), ["model.init_args.model_kwargs.cnet.tile_size=64",
                                   "model.init_args.model_kwargs.cnet.tile_stride=32"])
    cn = cli.resolve(cfg)["model_kwargs"]["cnet"]
    assert (cn["tile_size"], cn["tile_stride"]) == (64, 32)
