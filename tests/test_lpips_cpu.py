"""LPIPS, host side: the weight loader, the C ABI's argument checks (they fail before any HIP call: null / dummy pointers are
never dereferenced), properties of the fp64 restatement (tests/lpips_reference.py), the measurement the GPU tolerances come
from, and the caller's switch."""
import math

import pytest
import torch

import lpips_reference as R
from unirestore_amd import capi

DUMMY = 0x1000        # never dereferenced


def _save(tmp_path, asd, lsd):
    a, l = tmp_path / "alexnet.pth", tmp_path / "alex_lin.pth"
    torch.save(asd, a)
    torch.save(lsd, l)
    return str(a), str(l)


def _dicts(seed=3):
    from unirestore_amd import lpips
    return lpips.random_state_dicts(seed)


# ---- the loader ---------------------------------------------------------------------------------------------------------------

def test_loader_reads_the_two_real_key_layouts_and_ignores_the_classifier(tmp_path):
    from unirestore_amd import f32net, lpips
    asd, lsd = _dicts()
    asd["classifier.1.weight"], asd["classifier.1.bias"] = torch.zeros(8, 16), torch.zeros(8)      # torchvision's file has them
    w = lpips.load_weights(*_save(tmp_path, asd, lsd), dev="cpu")
    assert len(w.convs) == len(w.lins) == 5
    for i, (idx, cout, cin, k, stride, pad) in enumerate(lpips.CONVS):
        pc = w.convs[i]
        assert (pc.cout, pc.cin, pc.kh, pc.kw, pc.stride, pc.pad) == (cout, cin, k, k, stride, pad)
        kpad, cpad = f32net.wpack_dims(cin, cout, k, k)
        assert tuple(pc.w.shape) == (kpad, cpad) and kpad % 16 == 0 and cpad % 64 == 0 and kpad >= cin * k * k and cpad >= cout
        src = asd[f"features.{idx}.weight"]
        for (o, c, y, x) in ((0, 0, 0, 0), (cout - 1, cin - 1, k - 1, k - 1), (cout // 2, cin // 2, 1, 2)):
            assert pc.w[(y * k + x) * cin + c, o] == src[o, c, y, x]                  # row (kh, kw, cin), column cout
        assert not pc.w[cin * k * k:].any() and not pc.w[:, cout:].any()              # the padding is zeros
        assert torch.equal(pc.bias, asd[f"features.{idx}.bias"])
        assert torch.equal(w.lins[i], lsd[f"lin{i}.model.1.weight"].reshape(-1)) and w.lins[i].shape == (cout,)
        assert torch.equal(w.cpu[f"conv{i}.weight"], src)
    assert not any(k.startswith("classifier") for k in w.cpu)


BROKEN = [
    ("a", "features.6.weight", "drop", "missing"),
    ("a", "features.0.bias", "drop", "missing"),
    ("l", "lin3.model.1.weight", "drop", "missing"),
    ("a", "features.3.weight", torch.zeros(192, 64, 3, 3), "shape"),
    ("a", "features.10.bias", torch.zeros(255), "shape"),
    ("l", "lin0.model.1.weight", torch.zeros(64), "shape"),
    ("l", "lin2.model.1.weight", "negative", "negative"),
]


@pytest.mark.parametrize("which,key,what,word", BROKEN, ids=[f"{k}-{w}" for _, k, _, w in BROKEN])
def test_loader_rejects_a_wrong_file_and_names_the_key(tmp_path, which, key, what, word):
    from unirestore_amd import lpips
    asd, lsd = _dicts()
    d = asd if which == "a" else lsd
    if isinstance(what, str) and what == "drop":
        del d[key]
    elif isinstance(what, str) and what == "negative":
        d[key] = d[key].clone()
        d[key][0, 5, 0, 0] = -1e-3
    else:
        d[key] = what
    a, l = _save(tmp_path, asd, lsd)
    with pytest.raises(ValueError) as e:
        lpips.load_weights(a, l, dev="cpu")
    msg = str(e.value)
    assert key in msg and word in msg and (a if which == "a" else l) in msg, msg


def test_random_weights_have_the_loaders_structure():
    from unirestore_amd import lpips
    a, b = lpips.random_weights(5, dev="cpu"), lpips.random_weights(5, dev="cpu")
    assert all(torch.equal(a.cpu[k], b.cpu[k]) for k in a.cpu) and sorted(a.cpu) == sorted(R.weights_cpu())
    assert all(bool((l >= 0).all()) for l in a.lins)
    assert "no real weights" in lpips.random_weights.__doc__ or "NOT" in lpips.random_state_dicts.__doc__


# ---- C ABI argument checks ----------------------------------------------------------------------------------------------------

def _invalid(fn, *args):
    assert getattr(capi.lib, fn)(*args) == capi.UR_E_INVALID
    return capi.lib.ur_last_error().decode()


def test_prep_rejects_bad_arguments_before_any_hip_call():
    for args, word in (((DUMMY, DUMMY, 2, 3, 30, 64), "H and W"), ((DUMMY, DUMMY, 2, 3, 64, 30), "H and W"),
                       ((DUMMY, DUMMY, 2, 1, 64, 64), "C must be 3"), ((DUMMY, DUMMY, 2, 4, 64, 64), "C must be 3"),
                       ((DUMMY, DUMMY, 0, 3, 64, 64), "N must"), ((None, DUMMY, 2, 3, 64, 64), "null"),
                       ((DUMMY, None, 2, 3, 64, 64), "null")):
        msg = _invalid("ur_lpips_prep", *args, None)
        assert "ur_lpips_prep" in msg and word in msg, msg


def test_conv_rejects_bad_arguments_before_any_hip_call():
    good = dict(x=DUMMY, w=DUMMY, bias=DUMMY, y=DUMMY, N=1, H=8, W=8, Cin=4, Cout=8, KH=3, KW=3, stride=1, pad=1, relu=1)
    for kw, word in ((dict(x=None), "null"), (dict(w=None), "null"), (dict(bias=None), "null"), (dict(y=None), "null"),
                     (dict(N=0), "N, H and W"), (dict(Cin=0), "Cin"), (dict(Cout=0), "Cin"), (dict(stride=0), "stride"),
                     (dict(pad=-1), "stride"), (dict(H=2, KH=5, pad=1), "smaller than the filter"), (dict(w=DUMMY + 4), "aligned")):
        msg = _invalid("ur_conv2d_f32", *dict(good, **kw).values(), None)
        assert "ur_conv2d_f32" in msg and word in msg, msg


def test_pool_and_layer_reject_bad_arguments_before_any_hip_call():
    for args, word in (((None, DUMMY, 1, 7, 7, 64), "null"), ((DUMMY, DUMMY, 1, 2, 7, 64), "H and W"), ((DUMMY, DUMMY, 1, 7, 7, 0), "N and C")):
        msg = _invalid("ur_maxpool2d_f32", *args, None)
        assert "ur_maxpool2d_f32" in msg and word in msg, msg
    need = 2 * capi.lib.ur_lpips_layer_parts(15 * 11) * 8
    for args, word in (((None, DUMMY, 2, 165, 64, DUMMY, need), "null"), ((DUMMY, None, 2, 165, 64, DUMMY, need), "null"),
                       ((DUMMY, DUMMY, 2, 165, 64, None, need), "null"), ((DUMMY, DUMMY, 0, 165, 64, DUMMY, need), "N must"),
                       ((DUMMY, DUMMY, 2, 0, 64, DUMMY, need), "P and C"), ((DUMMY, DUMMY, 2, 165, 64, DUMMY, need - 1), "workspace too small")):
        msg = _invalid("ur_lpips_layer", *args, None)
        assert "ur_lpips_layer" in msg and word in msg, msg


def test_finish_rejects_bad_arguments_and_a_short_workspace():
    need = capi.lib.ur_lpips_ws_size(2, 64, 80)
    assert need > 0 and need % 8 == 0
    for args, word in (((None, need, 2, 64, 80, DUMMY), "null"), ((DUMMY, need, 2, 64, 80, None), "null"),
                       ((DUMMY, need, 2, 30, 80, DUMMY), "H and W"), ((DUMMY, need, 0, 64, 80, DUMMY), "N must"),
                       ((DUMMY, need - 1, 2, 64, 80, DUMMY), "workspace too small"), ((DUMMY, 0, 2, 64, 80, DUMMY), "workspace too small")):
        msg = _invalid("ur_lpips_finish", *args, None)
        assert "ur_lpips_finish" in msg and word in msg, msg


def test_workspace_size_and_tap_geometry():
    from unirestore_amd import lpips
    ws = capi.lib.ur_lpips_ws_size
    assert ws(1, 31, 31) == (1 + 1 + 1 + 1 + 1) * 8                     # 49, 9, 1, 1, 1 pixels: one partial each
    assert ws(3, 31, 31) == 3 * ws(1, 31, 31)
    for bad in ((0, 64, 64), (1, 30, 64), (1, 64, 30)):
        assert ws(*bad) == capi.UR_E_INVALID and "ur_lpips_ws_size" in capi.lib.ur_last_error().decode()
    for h, w in ((31, 31), (33, 47), (96, 80), (512, 512)):
        x = torch.zeros(1, 3, h, w, dtype=torch.float64)
        taps = R.features(x, {k: torch.zeros_like(v, dtype=torch.float64) for k, v in R.weights_cpu().items()})
        total = 0
        for t, f in enumerate(taps):
            assert lpips.tap_hw(h, w, t) == tuple(f.shape[2:])                     # the planner's geometry is torch's
            total += lpips.layer_parts(f.shape[2] * f.shape[3])
        assert ws(1, h, w) == total * 8
    assert lpips.tap_hw(31, 31, 4) == (1, 1) and lpips.MIN_HW == 31
    assert lpips.layer_parts(64) == 1 and lpips.layer_parts(65) == 2


# ---- the fp64 restatement -----------------------------------------------------------------------------------------------------

def test_reference_identity_symmetry_and_sign():
    w = R.weights_cpu()
    for shape in ((2, 3, 31, 31), (1, 3, 40, 57)):
        a, b = R.images(shape, 21)
        assert bool((R.lpips(a, a.clone(), w) == 0).all())                         # exactly
        ab, ba = R.lpips(a, b, w), R.lpips(b, a, w)
        assert torch.equal(ab, ba)                                                 # (u - v)^2 == (v - u)^2 bit for bit
        assert bool((ab > 0).all()) and bool(torch.isfinite(ab).all())


def test_reference_hand_case():
    """31 x 31, every lin weight 1.  conv1 channel 0 copies the scaled R of the window's centre pixel, channel 1 the scaled G,
    every other weight is 0; conv2..5 are zero filters with bias 1, so taps 2..5 are the same for both images and add nothing.
    pred is pure red, target pure green: after ReLU tap 1 is (a, 0, 0, ...) against (0, b, 0, ...) at all 49 pixels with
    a = (1 + .030) / .458, b = (1 + .088) / .448, and the metric is (a / (a + 1e-10))^2 + (b / (b + 1e-10))^2."""
    w = {}
    for i, (co, ci, k, _s, _p) in enumerate(R.CONVS):
        w[f"conv{i}.weight"], w[f"conv{i}.bias"] = torch.zeros(co, ci, k, k), torch.zeros(co) if i == 0 else torch.ones(co)
        w[f"lin{i}"] = torch.ones(co)
    w["conv0.weight"][0, 0, 5, 5] = 1.0
    w["conv0.weight"][1, 1, 5, 5] = 1.0
    pred, tgt = torch.zeros(1, 3, 31, 31), torch.zeros(1, 3, 31, 31)
    pred[:, 0], tgt[:, 1] = 1.0, 1.0
    taps = R.features(torch.cat([pred, tgt]), w)
    a, b = (1 + .030) / .458, (1 + .088) / .448
    assert tuple(taps[0].shape) == (2, 64, 7, 7) and tuple(taps[4].shape) == (2, 256, 1, 1)
    assert float((taps[0][0, 0] - a).abs().max()) < 1e-15 and not taps[0][0, 1:].any() and not taps[0][1, 0].any()
    want = (a / (a + 1e-10)) ** 2 + (b / (b + 1e-10)) ** 2
    got = float(R.lpips(pred, tgt, w)[0])
    assert abs(got - want) < 1e-14 and abs(got - 2.0) < 1e-9, (got, want)


def test_reference_zero_feature_vector_is_not_nan():
    f0, f1 = torch.zeros(1, 4, 1, 2), torch.zeros(1, 4, 1, 2)
    f1[0, :, 0, 0] = torch.tensor([3.0, 0, 4.0, 0])                     # pixel 0: zero against (.6, 0, .8, 0); pixel 1: zero against zero
    v = R.layer(f0, f1, torch.tensor([1.0, 1, 2, 1]))
    assert torch.isfinite(v).all() and abs(float(v[0]) - (0.36 + 2 * 0.64) / 2) < 1e-9


# ---- where the GPU tolerances come from ---------------------------------------------------------------------------------------

def test_tolerances_follow_the_measured_fp32_error():
    """Measures fp32's own error on the end-to-end cases (the figures in lpips_reference.py's table) and holds the constants to
    them: every GPU bound (8 x the recorded e32) must still be >= 4 x what is measured here, so the constants cannot drift loose
    from the yardstick - and the recorded e32 must not be far above the measurement either."""
    ms = {shape: R.measure_e32(shape) for shape in R.E2E_CASES}
    for shape, m in ms.items():
        print(shape, "metric %.2e prep %.2e layer %.2e conv" % (m["metric"], m["prep"], m["layer"]), " ".join("%.2e" % c for c in m["conv"]))
    metric = max(m["metric"] for m in ms.values())
    convs = [max(m["conv"][i] for m in ms.values()) for i in range(5)]
    lay = max(m["layer"] for m in ms.values())
    prep = max(m["prep"] for m in ms.values())
    assert R.METRIC_TOL == 8 * R.E32_METRIC and R.LAYER_TOL == 8 * R.E32_LAYER and R.PREP_TOL == 8 * R.E32_PREP
    assert R.CONV_TOL == tuple(8 * e for e in R.E32_CONV)
    for name, tol, e32 in [("metric", R.METRIC_TOL, metric), ("layer", R.LAYER_TOL, lay), ("prep", R.PREP_TOL, prep)] + \
                          [(f"conv{i + 1}", R.CONV_TOL[i], convs[i]) for i in range(5)]:
        assert tol >= 4 * e32, (name, tol, e32)
        assert tol <= 16 * e32, (name, tol, e32)                  # nor twice as loose as 8 x what fp32 really does
        assert math.isfinite(e32) and e32 > 0


# ---- the caller ---------------------------------------------------------------------------------------------------------------

class _StubModel:
    pass


def test_litunifie_without_lpips_keeps_todays_keys():
    from unirestore_amd.runner import LitUniFIE
    lit = LitUniFIE({}, model=_StubModel())
    assert lit.lpips_weights is None and set(lit.totals) == {"psnr", "ssim", "images"}
    assert lit.metrics() == {"val_lq/psnr": 0.0, "val_lq/ssim": 0.0, "images": 0}


def test_cli_lpips_flag(tmp_path):
    import inspect

    from unirestore_amd import cli
    assert inspect.signature(cli.validate).parameters["lpips"].default is None
    a, l = _save(tmp_path, *_dicts())
    assert cli.check_lpips_arg(f"{a},{l}") == (a, l)
    for bad in (a, f"{a},{l},{l}", f"{a},", f"{a},{tmp_path / 'nope.pth'}"):
        with pytest.raises(ValueError):
            cli.check_lpips_arg(bad)
    with pytest.raises(SystemExit):                      # an argument error, before the model is built
        cli.main(["validate", "--config", "configs/val_pir_256_4step.yaml", "--lpips", f"{a},{tmp_path / 'nope.pth'}"])
    with pytest.raises(SystemExit):
        cli.main(["restore", "--config", "configs/val_pir_256_4step.yaml", "--lpips", f"{a},{l}"])
