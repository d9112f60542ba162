"""Host side of the colour fix (no GPU needed): the reference module against itself, the kernel's arithmetic emulated in numpy fp32
against the bound, what the case table covers, the refusals of the C ABI, and the switches (DiffUIE.set_color_fix, cnet.color_fix,
--color-fix).  tests/test_colorfix_gpu.py launches the kernels."""
import glob
import os

import numpy as np
import pytest
import torch

import colorfix_cases as T
import colorfix_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


def _data(sh, dtype="bf16", seed=0):
    c, s = T.make(sh, T.DTYPES[dtype], seed)
    return c.double().numpy(), T.source_of(s, sh[0])


# ---- the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh", T.SHAPES, ids=T.shape_id)
def test_both_wavelet_forms_agree(sh):
    c, s = _data(sh)
    assert np.abs(c).max() < 2 and np.abs(s).max() <= 1
    assert np.abs(R.wavelet(c, s) - R.wavelet_atrous(c, s)).max() <= 1e-12


@pytest.mark.parametrize("sh", T.SHAPES, ids=T.shape_id)
def test_low_band_of_a_constant_is_that_constant(sh):
    for k in (0.3, -1.0, 0.7071067811865476):
        v = np.full((sh[0], sh[2], sh[3], 3), k)
        assert np.array_equal(R.low(v), v)
        v32 = v.astype(np.float32)
        assert np.array_equal(R.emulate_wavelet_f32(np.zeros_like(v32), v32), v32)        # and in the kernel's fp32 order


def test_composed_taps():
    w = R.composed_taps()
    assert w.shape == (63,) and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1]) and (w > 0).all()


def test_clamp_at_every_level_is_not_one_clamp():
    """The definition clamps at the image edge at every level.  One 63-tap filter with one clamp agrees with it more than 31 pixels from
    every border and nowhere near one: a row of the case table tells the two apart by far more than the bound."""
    sh = T.STRIPS[0]
    c, s = _data(sh)
    d = s - c
    a, b = R.low(d), R.low_single_clamp(d)
    h = R.HALO
    assert np.abs(a - b)[:, h:-h, h:-h].max() <= 1e-14
    assert np.abs(a - b).max() > 1e3 * R.wavelet_bound(c, s).max()
    for small in T.SMALL[1:]:
        c, s = _data(small)
        assert np.abs(R.low(s - c) - R.low_single_clamp(s - c)).max() > 1e3 * R.wavelet_bound(c, s).max(), small


@pytest.mark.parametrize("dtype", list(T.DTYPES))
@pytest.mark.parametrize("sh", T.SHAPES, ids=T.shape_id)
def test_fp32_emulation_within_the_wavelet_bound(sh, dtype):
    c, s = T.make(sh, T.DTYPES[dtype])
    c64, s64 = c.double().numpy(), T.source_of(s, sh[0])
    got = R.emulate_wavelet_f32(c.numpy(), s64.astype(np.float32))
    ratio = float((np.abs(got.astype(np.float64) - R.wavelet(c64, s64)) / R.wavelet_bound(c64, s64)).max())
    WORST[dtype] = max(WORST.get(dtype, 0.0), ratio)
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("sh", T.SHAPES + [(1, 1, 70, 300, 8, 8), (1, 1, 300, 7, 8, 8)], ids=T.shape_id)
def test_strips_halos_and_the_in_place_walk_change_no_value(sh):
    """The kernel's tiling (windows that end at the image edge, taps clamped to the window, the carry of the in-place row pass) with
    its own strip sizes, in numpy fp32: bit-equal to the whole-canvas emulation on every case."""
    c, s = T.make(sh, torch.bfloat16)
    s32 = T.source_of(s, sh[0]).astype(np.float32)
    whole = R.emulate_wavelet_f32(c.numpy(), s32)
    assert np.array_equal(R.emulate_wavelet_strips_f32(c.numpy(), s32, T.VR, T.HR, T.HC, T.HALO), whole)
    assert np.array_equal(R.emulate_wavelet_strips_f32(c.numpy(), s32, 40, 3, 31, T.HALO), whole)      # any strip sizes >= the halo


def test_adain_reference_and_bound():
    sh = T.FANOUT
    c, s = _data(sh)
    out = R.adain(c, s)
    a, b = R.adain_coefficients(c, s)
    assert np.abs(out - (a * c + b)).max() <= 1e-14
    assert np.abs(out.mean(axis=(1, 2)) - s.mean(axis=(1, 2))).max() <= 1e-14
    sd = np.sqrt(out.var(axis=(1, 2), ddof=1))
    assert np.abs(sd / np.sqrt(s.var(axis=(1, 2), ddof=1) + R.EPS) - 1).max() < 1e-3         # up to the 1e-5 under c's root
    # the fp32 arithmetic of the kernel (fp64 statistics, then a_f c + b_f rounded at every step) stays inside the bound
    c32 = c.astype(np.float32)
    got = (a.astype(np.float32) * c32 + b.astype(np.float32)).astype(np.float64)
    assert (np.abs(got - out) <= R.adain_bound(c, s)).all()


def test_known_answers_in_fp64():
    sh = T.FANOUT
    c, s = _data(sh)
    k = np.array([0.25, -0.125, 0.0625])
    assert np.abs(R.wavelet(s + k, s) - s).max() <= 1e-15
    assert np.abs(R.adain(s + k, s) - s).max() <= 1e-14
    assert np.array_equal(R.wavelet(s, s), s) and np.abs(R.adain(s, s) - s).max() <= 1e-14


def test_print_worst_ratio():
    """Not a check of its own: the largest |emulation - ref| / bound seen above (run with -s)."""
    print("\nwavelet, numpy fp32 in the kernel's order, largest |y - ref| / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})


# ---- the case table --------------------------------------------------------------------------------------------------------------
def test_every_property_is_held_by_a_case():
    for name, holds in T.PROPERTIES.items():
        assert any(holds(sh) for sh in T.SHAPES), f"no case with: {name}"


def test_strip_cases_match_the_kernel_constants():
    src = open(os.path.join(ROOT, "unirestore_amd", "csrc", "colorfix.hip")).read()
    for name, v in (("CF_VR", T.VR), ("CF_VC", T.VC), ("CF_HR", T.HR), ("CF_HC", T.HC), ("CF_HALO", T.HALO)):
        assert f"constexpr int {name} = {v};" in src, name
    assert T.HALO == R.HALO == sum(R.LEVELS)
    for sh in T.STRIPS:
        p = T.plan(sh)
        assert p["rows"]["interior"] and p["cols"]["interior"] and (p["rows"]["ragged"] or p["cols"]["ragged"])
        assert sh[2] <= 200 and sh[3] <= 200
    assert any(T.plan(sh)["rows"]["ragged"] for sh in T.STRIPS) and any(T.plan(sh)["cols"]["ragged"] for sh in T.STRIPS)
    assert not T.runs("adain", T.SMALL[0]) and all(T.runs("adain", sh) for sh in T.SHAPES[1:])
    c, s = T.make(T.FANOUT, torch.bfloat16)
    assert not torch.equal(s[0], s[1])                                      # distinct sources


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------------
REFUSALS = T.refusals()


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    return c


@pytest.mark.parametrize("fn,args", [(r[1], r[2]) for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusal(capi, fn, args):
    """One wrong argument in an otherwise valid call: UR_E_INVALID from the host-side check, before anything is launched."""
    assert getattr(capi.lib, fn)(*args) == capi.UR_E_INVALID, (fn, args)
    assert capi.lib.ur_last_error().decode().startswith("ur_color_fix_")


def test_workspace_size(capi):
    f = capi.lib.ur_color_fix_adain_ws_bytes
    assert f(0, 8, 8) == 0 and f(1, 0, 8) == 0 and f(1, 8, -1) == 0
    assert f(1, 8, 8) == 12 * 8 + 6 * 4 and f(3, 128, 128) == 3 * (12 * 8 + 6 * 4)
    assert f(2, 512, 512) == 2 * (16 * 12 * 8 + 6 * 4) and f(1, 129, 128) == 2 * 12 * 8 + 6 * 4
    assert f(8, 1024, 1024) % 8 == 0


# ---- the switches -------------------------------------------------------------------------------------------------------------
def test_set_color_fix():
    from tiny_cfg import TINY, model_kwargs
    from unirestore_amd.modules import DiffUIE
    m = DiffUIE(**model_kwargs(1), **TINY)
    assert m.color_fix is None
    m._graphs["sentinel"] = 1
    assert m.set_color_fix("wavelet") is m and m.color_fix == "wavelet" and not m._graphs
    m._graphs["sentinel"] = 1
    assert m.set_color_fix("adain").color_fix == "adain" and not m._graphs
    m._graphs["sentinel"] = 1
    assert m.set_color_fix(None).color_fix is None and not m._graphs
    for bad in ("none", "Wavelet", "", 1, True, "luma"):
        with pytest.raises(ValueError, match="wavelet"):
            m.set_color_fix(bad)
    assert m.color_fix is None
    kw = model_kwargs(1)
    kw["cnet"]["color_fix"] = "adain"
    assert DiffUIE(**kw, **TINY).color_fix == "adain"
    kw["cnet"]["color_fix"] = None
    assert DiffUIE(**kw, **TINY).color_fix is None
    kw["cnet"]["color_fix"] = "median"
    with pytest.raises(ValueError):
        DiffUIE(**kw, **TINY)


def test_entry_points_keep_their_defaults():
    import inspect
    from unirestore_amd.modules.model import SkipConnectedAutoEncoder as AE
    assert inspect.signature(AE.encode_run).parameters["return_input"].default is False
    for f in (AE.decode_run, AE.decode_run_tasks):
        p = inspect.signature(f).parameters
        assert p["color_src"].default is None and p["color_fix"].default is None


def test_config_key_and_flag():
    from unirestore_amd import cli
    from restore_worker import tiny_cfg
    for path in sorted(glob.glob(os.path.join(ROOT, "configs", "*.yaml"))):      # absent from every committed file
        cfg = cli.load_config(path)
        assert "color_fix" not in cfg["model"]["init_args"]["model_kwargs"]["cnet"]
        assert "color_fix" not in cli.resolve(cfg)["model_kwargs"]["cnet"]
    for mode in ("wavelet", "adain", None):
        cfg = tiny_cfg()
        cfg["model"]["init_args"]["model_kwargs"]["cnet"]["color_fix"] = mode
        assert cli.resolve(cfg)["model_kwargs"]["cnet"]["color_fix"] == mode
    cfg = tiny_cfg()
    cfg["model"]["init_args"]["model_kwargs"]["cnet"]["color_fix"] = "none"       # a YAML string, not null
    with pytest.raises(ValueError, match="cnet.color_fix"):
        cli.resolve(cfg)
    # the flag overrides the config, "none" turns a configured fix off, no flag leaves the config alone
    cn = lambda cfg: cfg["model"]["init_args"]["model_kwargs"]["cnet"]
    assert "color_fix" not in cn(cli.apply_color_fix(tiny_cfg(), None))
    assert cn(cli.apply_color_fix(tiny_cfg(), "wavelet"))["color_fix"] == "wavelet"
    cfg = tiny_cfg()
    cn(cfg)["color_fix"] = "adain"
    assert cn(cli.apply_color_fix(cfg, None))["color_fix"] == "adain"
    assert cn(cli.apply_color_fix(cfg, "wavelet"))["color_fix"] == "wavelet"
    assert cn(cli.apply_color_fix(cfg, "none"))["color_fix"] is None
    with pytest.raises(ValueError, match="--color-fix"):
        cli.apply_color_fix(tiny_cfg(), "luma")
    cfg = tiny_cfg()
    cfg["model"]["init_args"]["model_kwargs"]["cnet"] = None
    with pytest.raises(ValueError, match="cnet"):
        cli.apply_color_fix(cfg, "wavelet")


@pytest.mark.parametrize("command", ["validate", "restore", "print_config"])
def test_command_line_flag(command, tmp_path, capsys):
    """Both commands take --color-fix {none,wavelet,adain}; print_config shows what they would run."""
    import json
    import yaml
    from unirestore_amd import cli
    from restore_worker import tiny_cfg
    p = tmp_path / "tiny.yaml"
    p.write_text(yaml.safe_dump(tiny_cfg()))
    with pytest.raises(SystemExit):
        cli.main([command, "--config", str(p), "--color-fix", "luma"])
    capsys.readouterr()
    if command != "print_config":
        return
    for flag, want in (("wavelet", "wavelet"), ("adain", "adain"), ("none", None)):
        assert cli.main(["print_config", "--config", str(p), "--color-fix", flag]) == 0
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["model_kwargs"]["cnet"]["color_fix"] == want
    assert cli.main(["print_config", "--config", str(p)]) == 0
    assert "color_fix" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])["model_kwargs"]["cnet"]
    assert cli.main(["print_config", "--config", str(p), "--set", "model.init_args.model_kwargs.cnet.color_fix=adain", "--color-fix", "wavelet"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["model_kwargs"]["cnet"]["color_fix"] == "wavelet"


def test_ops_color_fix_refuses_before_touching_a_device():
    from unirestore_amd import ops
    c, s = torch.zeros(1, 4, 4, 8), torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16)
    for args in ((c, s, "luma"), (c, s, None), (c.double(), s, "wavelet"), (c[0], s, "wavelet"), (c, s.float(), "adain"),
                 (c[..., :4], s, "wavelet"), (c, s[:, :, :, :4], "wavelet"), ("c", s, "wavelet")):
        with pytest.raises(ValueError, match="color_fix"):
            ops.color_fix(*args)
