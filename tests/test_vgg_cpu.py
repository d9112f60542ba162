"""Host-only checks of the VGG scorer (unirestore_amd/vgg.py, tests/vgg_reference.py): the plan of all eight architectures, the
stand-in state dict's layout, the weight loader on both wrappings and its refusals, the column permutation of classifier.0 and the
Linear's weight layout, the yardstick's recorded constants are current, its network cases are decidable, the --vgg argument, and
every launcher's size limits."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import classify_reference as CR
import vgg_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the plan -----------------------------------------------------------------------------------------------------------------------

def test_plan_of_every_arch():
    from unirestore_amd import vgg
    assert set(vgg.ARCHS) == {"vgg11", "vgg13", "vgg16", "vgg19", "vgg11_bn", "vgg13_bn", "vgg16_bn", "vgg19_bn"}
    assert vgg.conv_indices("vgg16") == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert vgg.conv_indices("vgg16_bn")[-1] == 40 and vgg.conv_indices("vgg16_bn")[:3] == [0, 3, 7]
    assert vgg.conv_indices("vgg11") == [0, 3, 6, 8, 11, 13, 16, 18]
    for arch, count in (("vgg11", 8), ("vgg13", 10), ("vgg16", 13), ("vgg19", 16)):
        for name in (arch, arch + "_bn"):
            steps = vgg.plan(name)
            assert len(vgg.conv_indices(name)) == count and sum(s[0] == "pool" for s in steps) == 5 and steps[-1][0] == "pool"
            convs = [s for s in steps if s[0] == "conv"]
            assert convs[0][4] == 3 and convs[-1][3] == 512 and all(a[3] == b[4] for a, b in zip(convs, convs[1:]))
            assert all((s[2] == s[1] + 1) if name.endswith("_bn") else s[2] is None for s in convs)
    for bad in ("vgg12", "resnet50", None, 16):
        with pytest.raises(ValueError, match="unknown VGG arch"):
            vgg.plan(bad)


def test_random_state_dict_is_the_layout_and_the_sizes_are_read_back():
    from unirestore_amd import vgg
    sd = vgg.random_state_dict("vgg16_bn", 1, 7, 32)
    assert len(sd) == 13 * 7 + 6
    assert tuple(sd["features.0.weight"].shape) == (64, 3, 3, 3) and tuple(sd["features.40.weight"].shape) == (512, 512, 3, 3)
    assert tuple(sd["features.41.running_var"].shape) == (512,) and "features.42.weight" not in sd
    assert tuple(sd["classifier.0.weight"].shape) == (32, 25088) and tuple(sd["classifier.3.weight"].shape) == (32, 32)
    assert tuple(sd["classifier.6.weight"].shape) == (7, 32) and tuple(sd["classifier.6.bias"].shape) == (7,)
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), vgg.random_state_dict("vgg16_bn", 1, 7, 32).values()))
    sd = vgg.random_state_dict("vgg16", 1, 7, 32)
    assert len(sd) == 13 * 2 + 6 and sorted(int(k.split(".")[1]) for k in sd if k.startswith("features.") and k.endswith(".weight")) == \
        [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    w = vgg.VGGWeights("vgg16", sd, "cpu")
    assert (w.hidden, w.num_classes, w.arch, w.device) == (32, 7, "vgg16", torch.device("cpu"))
    assert set(w.convs) == {f"features.{i}" for i in vgg.conv_indices("vgg16")} and set(w.linears) == set(vgg.LINEAR_KEYS)
    assert set(w.cpu) == set(sd) and all(torch.equal(w.cpu[k], sd[k]) for k in sd)
    c = w.convs["features.28"]
    assert (c.kh, c.kw, c.stride, c.pad, c.cin, c.cout) == (3, 3, 1, 1, 512, 512)
    assert (w.linears["classifier.0"].k, w.linears["classifier.0"].n, w.linears["classifier.0"].splits) == (25088, 32, 49)
    assert vgg.linear_wpack_dims(25088, 4096) == (25088, 4096, 49) and vgg.linear_wpack_dims(7, 5) == (64, 32, 1)
    assert vgg.linear_wpack_dims(1000, 200) == (1024, 224, 2) and vgg.linear_wpack_dims(512, 1)[2] == 1 and vgg.linear_wpack_dims(513, 1)[2] == 2


def test_bn_fold_equals_conv_then_batch_norm():
    from unirestore_amd import f32net, vgg
    sd = vgg.random_state_dict("vgg11_bn", 3, 5, 16)
    w = vgg.VGGWeights("vgg11_bn", sd, "cpu")
    x = torch.randn(1, 3, 6, 7, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    p = lambda k: sd[k].double()                                  # noqa: E731
    want = F.batch_norm(F.conv2d(x, p("features.0.weight"), p("features.0.bias"), padding=1), p("features.1.running_mean"),
                        p("features.1.running_var"), p("features.1.weight"), p("features.1.bias"), False, 0.1, R.BN_EPS)
    fw, fb = vgg.fold_bn_bias(*(sd[f"features.{k}"] for k in ("0.weight", "0.bias", "1.weight", "1.bias", "1.running_mean", "1.running_var")))
    assert float((F.conv2d(x, fw, fb, padding=1) - want).abs().max()) < 1e-12 * float(want.abs().max())
    assert torch.equal(w.convs["features.0"].w, f32net.pack_conv_weight(fw.float())) and torch.equal(w.convs["features.0"].bias, fb.float())


# ---- the loader -----------------------------------------------------------------------------------------------------------------

def test_load_weights_reads_both_wrappings_and_refuses_bad_files(tmp_path, monkeypatch):
    from unirestore_amd import vgg
    sd = vgg.random_state_dict("vgg11_bn", 3, 5, 16)
    a = vgg.VGGWeights("vgg11_bn", sd, "cpu")
    plain, lit = tmp_path / "plain.pth", tmp_path / "lit.ckpt"
    torch.save(sd, str(plain))
    torch.save({"state_dict": {f"model.{k}": v for k, v in sd.items()}}, str(lit))
    for path in (plain, lit):
        b = vgg.load_weights("vgg11_bn", str(path), "cpu")
        assert set(a.cpu) == set(b.cpu) and all(torch.equal(a.cpu[k], b.cpu[k]) for k in a.cpu) and (b.hidden, b.num_classes) == (16, 5)
        assert all(torch.equal(a.convs[k].w, b.convs[k].w) and torch.equal(a.convs[k].bias, b.convs[k].bias) for k in a.convs)
        assert all(torch.equal(a.linears[k].w, b.linears[k].w) and torch.equal(a.linears[k].bias, b.linears[k].bias) for k in a.linears)
    monkeypatch.setattr(vgg.f32net, "read_state_dict", lambda path: pytest.fail("the file was read for an unknown arch"))
    with pytest.raises(ValueError, match="vgg12"):
        vgg.load_weights("vgg12", str(plain), "cpu")
    monkeypatch.undo()
    monkeypatch.setattr(vgg, "PackedConvF32", lambda *a, **k: pytest.fail("a convolution was packed for a bad state dict"))
    monkeypatch.setattr(vgg, "PackedLinearF32", lambda *a, **k: pytest.fail("a Linear was packed for a bad state dict"))
    for key in ("features.0.weight", "features.0.bias", "features.1.running_var", "features.25.weight", "features.26.bias", "classifier.0.weight",
                "classifier.0.bias", "classifier.3.weight", "classifier.6.weight", "classifier.6.bias"):
        torch.save({k: v for k, v in sd.items() if k != key}, str(plain))
        with pytest.raises(ValueError) as e:
            vgg.load_weights("vgg11_bn", str(plain), "cpu")
        assert "plain.pth" in str(e.value) and key in str(e.value)
        if key in ("classifier.0.weight", "classifier.6.weight"):
            continue                                               # their first axes are the hidden width and the class count
        with pytest.raises(ValueError) as e:
            vgg.VGGWeights("vgg11_bn", dict(sd, **{key: torch.zeros(*sd[key].shape, 2)}), "cpu", source="bad.pth")
        assert "bad.pth" in str(e.value) and key in str(e.value) and "shape" in str(e.value)
        for value in (float("nan"), float("inf")):
            poisoned = dict(sd, **{key: sd[key].clone()})
            poisoned[key].view(-1)[-1] = value
            with pytest.raises(ValueError) as e:
                vgg.VGGWeights("vgg11_bn", poisoned, "cpu", source="bad.pth")
            assert "bad.pth" in str(e.value) and key in str(e.value) and "non-finite" in str(e.value)
    with pytest.raises(ValueError, match="classifier.0.weight"):
        vgg.VGGWeights("vgg11_bn", dict(sd, **{"classifier.0.weight": torch.zeros(16, 25087)}), "cpu")
    with pytest.raises(ValueError, match="classifier.3.weight"):
        vgg.VGGWeights("vgg11_bn", dict(sd, **{"classifier.3.weight": torch.zeros(16, 17)}), "cpu")
    with pytest.raises(ValueError, match="running_var"):                         # var + eps <= 0: not a trained BatchNorm
        vgg.VGGWeights("vgg11_bn", dict(sd, **{"features.1.running_var": -torch.ones(64)}), "cpu")
    with pytest.raises(ValueError, match="features.1.weight"):                   # a plain VGG's file for a _bn arch
        vgg.VGGWeights("vgg11_bn", vgg.random_state_dict("vgg11", 3, 5, 16), "cpu")


def test_classifier0_columns_are_permuted_to_the_nhwc_flatten():
    """The packed classifier.0, unpacked and applied by a host matmul to the NHWC flatten of a random [N, 7, 7, 512] map, equals
    F.linear on torchvision's NCHW flatten; without the permutation it does not."""
    from unirestore_amd import vgg
    sd = vgg.random_state_dict("vgg11", 5, 10, 32)
    w = vgg.VGGWeights("vgg11", sd, "cpu")
    pl = w.linears["classifier.0"]
    assert tuple(pl.w.shape) == (1, 25088 // 8, 64, 4) and pl.w.is_contiguous()
    x = torch.randn(3, 512, 7, 7, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    want = F.linear(torch.flatten(x, 1), sd["classifier.0.weight"].double(), sd["classifier.0.bias"].double())
    mat = vgg.unpack_linear_weight(pl.w, 32, 25088).double()
    got = CR.nhwc(x).reshape(3, -1) @ mat.t() + pl.bias.double()
    assert float((got - want).abs().max()) < 1e-12
    assert float((torch.flatten(x, 1) @ mat.t() + pl.bias.double() - want).abs().max()) > 0.1
    assert torch.equal(vgg.unpack_linear_weight(w.linears["classifier.6"].w, 10, 32), sd["classifier.6.weight"])      # the others are not permuted


def test_linear_weight_layout():
    from unirestore_amd import vgg
    n, k = 37, 70
    w = torch.arange(n * k, dtype=torch.float32).view(n, k) + 1
    p = vgg.pack_linear_weight(w)
    assert tuple(p.shape) == (2, 16, 64, 4) and p.is_contiguous()
    for c, b, lane, j in ((0, 0, 0, 0), (0, 3, 37, 2), (1, 8, 4, 3), (1, 8, 36, 1), (1, 8, 5, 0), (0, 8, 63, 2), (1, 15, 0, 0)):
        col, kk = 32 * c + (lane & 31), 8 * b + 4 * (lane >> 5) + j
        assert float(p[c, b, lane, j]) == (float(w[col, kk]) if col < n and kk < k else 0.0), (c, b, lane, j)
    assert torch.equal(vgg.unpack_linear_weight(p, n, k), w) and float(p.sum()) == float(w.sum())


# ---- the yardstick's own constants ----------------------------------------------------------------------------------------------

def test_tolerances_follow_the_measured_fp32_error():
    """Re-measures fp32's own error against fp64 for every recorded constant (vgg_reference.py: E32_*) and holds the constants to
    the measurement by classify_reference's rule: every GPU bound (8 x the recorded e32) must be >= 4 x and <= 16 x what is
    measured here; a case fp32 gets exactly right is recorded as 0 and must measure 0."""
    pairs = [(f"linear {k}", R.LIN_TOL[k], R.measure_lin(k)) for k in R.LIN_CASES]
    pairs += [("linear, real size", R.LIN_REAL_TOL, R.measure_lin_real())]
    pairs += [(f"avgpool7 {R.avg_name(s)}", R.AVG_TOL[R.avg_name(s)], R.measure_avg(s)) for s in R.AVG_CASES]
    pairs += [(f"logits {k}", R.LOGITS_TOL[k], R.measure_logits(k)) for k in R.NET_CASES]
    pairs += [("forward", R.FORWARD_TOL, R.measure_forward())]
    assert R.GPU_FACTOR == 8 and R.LIN_REAL_TOL == 8 * R.E32_LIN_REAL and R.FORWARD_TOL == 8 * R.E32_FORWARD
    for tol, e32, cases in ((R.LIN_TOL, R.E32_LIN, R.LIN_CASES), (R.AVG_TOL, R.E32_AVG, [R.avg_name(s) for s in R.AVG_CASES]),
                            (R.LOGITS_TOL, R.E32_LOGITS, R.NET_CASES)):
        assert tol == {k: 8 * v for k, v in e32.items()} and set(e32) == set(cases)
    for name, tol, e32 in pairs:
        print(f"{name}: measured {e32:.2e}, bound {tol:.2e}")
        assert math.isfinite(e32) and e32 >= 0, name
        if tol == 0 or e32 == 0:
            assert tol == 0 and e32 == 0, (name, tol, e32)
        else:
            assert 4 * e32 <= tol <= 16 * e32, (name, tol, e32)


def test_network_cases_are_decidable():
    """What the GPU tests rely on, checked where it is chosen: finite fp64 logits and every image's top-2 gap above twice the
    absolute bound, so that the argmax can be asserted for every image of every network case - none is left out."""
    for name in R.NET_CASES:
        want = R.net_reference(name)
        bound = R.LOGITS_TOL[name] * float(want.abs().max())
        assert tuple(want.shape) == (R.NET_CASES[name][5][0], R.NET_CASES[name][2])
        assert bool(torch.isfinite(want).all()) and float(R.top2_gap(want).min()) > 2 * bound, name
        assert 0.1 < float(want.abs().max()) < 100, name                    # O(1) logits: the stand-in weights do not blow up
    want = R.forward_reference()
    assert tuple(want.shape) == (2, 1000) and bool(torch.isfinite(want).all())
    assert float(R.top2_gap(want).min()) > 2 * R.FORWARD_TOL * float(want.abs().max())


def test_cases_are_the_issues():
    assert R.LIN_MS == (1, 31, 32, 33, 65) and R.LIN_SHAPES == ((7, 5), (392, 10), (1000, 200), (4096, 1000), (25088, 64))
    assert R.LIN_REAL == (3, 25088, 4096) and R.LIN_ROWS == max(R.LIN_MS)
    assert R.POOL_CASES == ((2, 6, 6, 64), (1, 7, 5, 8), (1, 2, 2, 5), (1, 3, 3, 4))
    assert {(s[1], s[2], s[3]) for s in R.AVG_CASES} == {(h, w, c) for h, w in ((1, 1), (2, 2), (7, 7), (10, 13), (15, 8)) for c in (64, 5)}
    assert [(v[0], v[1], v[2], v[5]) for v in R.NET_CASES.values()] == [("vgg11", 64, 10, (3, 32, 32)), ("vgg16_bn", 96, 200, (2, 75, 101)),
                                                                       ("vgg19", 64, 10, (2, 64, 64))]
    assert R.FULL[:3] == ("vgg16", 4096, 1000) and R.FORWARD_SHAPE == (2, 3, 75, 101)
    x = torch.full((1, 1, 7, 7), 1.0)
    x[0, 0, 3, 3] = float("nan")
    assert int(torch.isnan(R.maxpool2(x)).sum()) == 1 and tuple(R.maxpool2(x).shape) == (1, 1, 3, 3)      # torch's pool keeps a NaN tap


# ---- the command line -------------------------------------------------------------------------------------------------------------

class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_vgg_argument(tmp_path, capsys):
    from unirestore_amd import cli
    w = str(tmp_path / "v.pth")
    open(w, "wb").close()                                          # the argument check looks for the file, it does not read it
    assert cli.check_vgg_arg(f"a=vgg16:{w},b=vgg19_bn:{w}") == {"a": ("vgg16", w), "b": ("vgg19_bn", w)}
    assert cli.check_vgg_arg({"a": ("vgg11", w)}) == {"a": ("vgg11", w)}
    assert cli.check_classifiers_arg(None, None, None, None, None) == (None, None) == cli.check_classifiers_arg(None, None)
    assert cli.check_classifiers_arg(f"r=resnet18:{w}", f"v=vit_b_16:{w}", f"s=swin_v2_b:{w}", f"t=rvt_tiny:{w}", f"g=vgg16:{w}") == (
        {"r": ("resnet18", w), "v": ("vit_b_16", w), "s": ("swin_v2_b", w), "t": ("rvt_tiny", w), "g": ("vgg16", w)}, "--classify")
    assert cli.check_classifiers_arg(None, None, None, f"t=rvt_tiny:{w}", f"g=vgg16:{w}") == ({"t": ("rvt_tiny", w), "g": ("vgg16", w)}, "--rvt")
    assert cli.check_classifiers_arg(None, None, vgg=f"g=vgg16:{w}") == ({"g": ("vgg16", w)}, "--vgg")
    assert cli.check_classifiers_arg(f"r=resnet18:{w}", None, None, f"t=rvt_tiny:{w}") == ({"r": ("resnet18", w), "t": ("rvt_tiny", w)}, "--classify")
    for kw, flag in ((dict(classify={"a": ("resnet18", w)}), "--classify"), (dict(vit={"a": ("vit_b_16", w)}), "--vit"),
                     (dict(swin={"a": ("swin_v2_b", w)}), "--swin"), (dict(rvt={"a": ("rvt_tiny", w)}), "--rvt")):
        with pytest.raises(ValueError, match=f"'a' is used by {flag} too"):
            cli.check_vgg_arg(f"a=vgg16:{w}", **kw)
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))        # its data yields no labels
    for kw, tasks, word in [
        (dict(vgg=f"a=resnet50:{w}"), ["ir", "cls"], "resnet50"),                               # an arch of another option
        (dict(classify=f"a=vgg16:{w}"), ["ir", "cls"], "vgg16"),                                # and the other way round
        (dict(vgg=f"a=vgg16:{w}.none"), ["ir", "cls"], "no such file"),
        (dict(vgg="a=vgg16"), ["ir", "cls"], "NAME=ARCH:WEIGHTS.pth"),
        (dict(vgg=f"a=vgg16:{w},a=vgg19:{w}"), ["ir", "cls"], "twice"),
        (dict(vgg=f"a=vgg16:{w}", classify=f"a=resnet18:{w}"), ["ir", "cls"], "--classify too"),      # both would write val_lq/a
        (dict(vgg=f"a=vgg16:{w}", vit=f"a=vit_b_16:{w}"), ["ir", "cls"], "--vit too"),
        (dict(vgg=f"a=vgg16:{w}", swin=f"a=swin_v2_b:{w}"), ["ir", "cls"], "--swin too"),
        (dict(vgg=f"a=vgg16:{w}", rvt=f"a=rvt_tiny:{w}"), ["ir", "cls"], "--rvt too"),
        (dict(vgg=f"a=vgg16:{w}"), None, "--vgg scores the 'cls' output"),
        (dict(vgg=f"a=vgg16:{w}"), ["ir"], "--vgg scores the 'cls' output"),
        (dict(vgg=f"a=vgg16:{w}"), ["ir", "cls"], "--vgg needs labels"),
        (dict(vgg=f"a=vgg16:{w}", rvt=f"t=rvt_tiny:{w}"), ["ir", "cls"], "--rvt needs labels"),
    ]:
        with pytest.raises(ValueError) as e:
            cli.validate(cfg, tasks=tasks, model=_NoModel(), **kw)
        assert word in str(e.value), (kw, tasks, str(e.value))
    path = os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")
    for argv, word in ((["restore", "--config", path, "--vgg", f"a=vgg16:{w}"], "--vgg belongs to validate"),
                       (["validate", "--config", path, "--vgg", f"a=vgg16:{w}"], "--vgg scores the 'cls' output"),
                       (["validate", "--config", path, "--tasks", "ir,cls", "--vgg", f"a=vgg16:{w}", "--rvt", f"a=rvt_tiny:{w}"], "--rvt too")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_litunifie_loads_a_vgg_through_its_own_module(monkeypatch):
    from unirestore_amd import classify, runner, rvt, swin, vgg, vit
    tiny = vgg.VGGWeights("vgg11", vgg.random_state_dict("vgg11", 1, 10, 16), "cpu")
    calls = []
    for name, module in (("vgg", vgg), ("rvt", rvt), ("swin", swin), ("vit", vit), ("classify", classify)):
        monkeypatch.setattr(module, "load_weights", lambda arch, path, name=name: calls.append((name, arch, path)) or tiny)
    lit = runner.LitUniFIE({}, model=object(), classifiers={"a": ("vgg16_bn", "a.pth"), "b": tiny, "c": ("resnet50", "c.pth"),
                                                            "d": ("rvt_base", "d.pth")})
    assert calls == [("vgg", "vgg16_bn", "a.pth"), ("classify", "resnet50", "c.pth"), ("rvt", "rvt_base", "d.pth")]
    assert lit.classifiers["b"] is tiny and {"cls/a", "cls_input/a", "cls/b", "cls_input/b"} <= set(lit.totals)
    assert tuple(lit.totals["cls/a"].shape) == (3, 10)


# ---- size limits: every launcher refuses one unit beyond each stated limit, before any HIP call --------------------------------

def test_launchers_refuse_sizes_beyond_their_limits():
    import ctypes
    from unirestore_amd import capi
    lib, P = capi.lib, 4096                                              # placeholder pointers: a refusal comes before any HIP call
    X, W, B, Y, WS = P, P + (1 << 40), P + (2 << 40), P + (3 << 40), P + (4 << 40)
    big = 1 << 62

    def lin(m, k, n, x=X, w=W, b=B, y=Y, ws=WS, ws_bytes=big, relu=0):
        return lib.ur_vgg_linear_f32(x, w, b, y, ws, ws_bytes, m, k, n, relu, None)
    for kw, word in ((dict(m=0, k=8, n=8), "M must be"), (dict(m=(1 << 20) + 1, k=8, n=8), "M must be"), (dict(m=1, k=0, n=8), "K and N"),
                     (dict(m=1, k=(1 << 24) + 1, n=8), "K and N"), (dict(m=1, k=8, n=(1 << 24) + 1), "K and N"), (dict(m=1, k=8, n=0), "K and N"),
                     (dict(m=1 << 20, k=8, n=2048), "M*N"), (dict(m=(1 << 20) - 1, k=8, n=2048, relu=2), "relu"),
                     (dict(m=4, k=1024, n=8, ws_bytes=4 * 2 * 4 * 8 - 1), "workspace"), (dict(m=1, k=8, n=8, x=None), "null"),
                     (dict(m=1, k=8, n=8, w=None), "null"), (dict(m=1, k=8, n=8, b=None), "null"), (dict(m=1, k=8, n=8, y=None), "null"),
                     (dict(m=1, k=8, n=8, ws=None), "null"), (dict(m=1, k=8, n=8, w=W + 4), "16-byte"), (dict(m=1, k=8, n=8, x=X + 2), "4-byte"),
                     (dict(m=1, k=8, n=8, y=X), "overlap"), (dict(m=1, k=8, n=8, ws=Y + 4), "overlap"), (dict(m=2, k=8, n=8, ws=X + 32), "overlap")):
        assert lin(**kw) == capi.UR_E_INVALID and word in lib.ur_last_error().decode(), (kw, lib.ur_last_error().decode())
    assert lib.ur_vgg_linear_ws_bytes(4, 1024, 8) == 4 * 2 * 4 * 8 and lib.ur_vgg_linear_ws_bytes(3, 25088, 4096) == 4 * 49 * 3 * 4096
    assert lib.ur_vgg_linear_ws_bytes(1 << 20, 8, 2047) == 4 * (1 << 20) * 2047               # the largest M*N the reduce launch takes
    for m, k, n in ((0, 8, 8), ((1 << 20) + 1, 8, 8), (1, (1 << 24) + 1, 8), (1, 8, (1 << 24) + 1), (1 << 20, 8, 2048)):
        assert lib.ur_vgg_linear_ws_bytes(m, k, n) == 0
    kpad, npad, s = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.ur_vgg_linear_wpack_dims(1 << 24, 1 << 24, kpad, npad, s) == 0 and (kpad.value, npad.value, s.value) == (1 << 24, 1 << 24, 1 << 15)
    for k, n in (((1 << 24) + 1, 8), (8, (1 << 24) + 1), (0, 8), (8, 0)):
        assert lib.ur_vgg_linear_wpack_dims(k, n, kpad, npad, s) == capi.UR_E_INVALID and "K and N" in lib.ur_last_error().decode()
    limit = (1 << 31) - 256
    for fn, ok_small, who in ((lib.ur_vgg_maxpool2_f32, 2, "H and W"), (lib.ur_vgg_avgpool7_f32, 1, "N, C, H and W")):
        for args, word in (((None, Y, 1, 8, 8, 4), "null"), ((X, None, 1, 8, 8, 4), "null"), ((X, X, 1, 8, 8, 4), "same buffer"),
                           ((X, Y, 0, 8, 8, 4), ">= 1"), ((X, Y, 1, 8, 8, 0), ">= 1"), ((X, Y, 1, ok_small - 1, 8, 4), who),
                           ((X, Y, 1, 8, ok_small - 1, 4), who),
                           ((X, Y, 1, 16, 16, (1 << 23) - 1), "below 2^31 - 256"),                       # N*H*W*C = 2^31 - 256 exactly
                           ((X, Y, 2, 1 << 15, 1 << 15, 1), "below 2^31 - 256")):
            assert fn(*args, None) == capi.UR_E_INVALID and word in lib.ur_last_error().decode(), (args, lib.ur_last_error().decode())
    # the average pool's own limit: the OUTPUT of a small map with very many channels: N*49*C at the limit, N*H*W*C far below it
    c = limit // 49 + 1
    assert 49 * (c - 1) < limit <= 49 * c
    assert lib.ur_vgg_avgpool7_f32(X, Y, 1, 1, 1, c, None) == capi.UR_E_INVALID and "N*49*C" in lib.ur_last_error().decode()
