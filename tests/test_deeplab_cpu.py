"""DeepLabV3+ scoring, the parts that need no GPU: the restatement against the stored vector of the reference's own network
(tests/golden/dlv3_0.npz, tools/gen_golden_dlv3.py), the plans, the half-pixel tap tables, the checkpoint loader, every --deeplab
argument error, the tolerances of deeplab_reference.py against what fp32 measures here, and the refusals of the new exports."""
import math
import os

import numpy as np
import pytest
import torch

import deeplab_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dlv3_0.npz")


def _checksum(v):
    return float((v.double().flatten() * torch.arange(1, v.numel() + 1, dtype=torch.float64)).sum())


# ---- the restatement against the reference's own network ------------------------------------------------------------------------

def test_restatement_reproduces_the_reference_network():
    from unirestore_amd import deeplab
    g = np.load(GOLDEN)
    depths = tuple(int(d) for d in g["depths"])
    sd = deeplab.random_state_dict(depths, int(g["weight_seed"]))
    sums = dict(zip(g["checksum_keys"].tolist(), g["checksums"].tolist()))
    assert set(sums) == {k for k, v in sd.items() if v.is_floating_point()}
    for k, want in sums.items():                          # first: the stand-in weights are the ones the vector was made with
        assert _checksum(sd[k]) == pytest.approx(want, rel=1e-12, abs=1e-12), \
            f"{k}: torch's random generator no longer draws the weights tests/golden/dlv3_0.npz was made with - regenerate it"
    x = torch.from_numpy(g["image"]).double() / 255
    assert tuple(x.shape) == (1, 3, 64, 320)              # the 1/16 map is 4 x 20: wider than the largest dilation
    want = torch.from_numpy(g["logits"])                  # the model's output, every row_step-th row and col_step-th column
    got = R.resize_hp(R.deeplab(R.preprocess(x), sd, depths), x.shape[2:])[:, :, ::int(g["row_step"]), ::int(g["col_step"])]
    assert got.shape == want.shape and got.shape[1] == 19
    err = float((got - want).abs().max() / want.abs().max())
    print(f"logits: max |err| / max |logit| {err:.2e}")
    assert err <= 1e-12
    pred = R.tta_logits(x, sd, depths, scales=tuple(float(s) for s in g["scales"])).argmax(dim=1)
    assert torch.equal(pred, torch.from_numpy(g["pred"]).long()) and len(set(pred.flatten().tolist())) >= R.MIN_CLASSES
    assert os.path.getsize(GOLDEN) < 256 * 1024


def test_plans_are_the_reference_modules_layout():
    """The strict=True load in tools/gen_golden_dlv3.py proves keys and shapes; here the counts and a few named entries."""
    from unirestore_amd import deeplab, f32net, segment
    assert deeplab.ARCHS == {"dlv3pr50": (3, 4, 6, 3), "dlv3pr101": (3, 4, 23, 3)}
    assert segment.ARCHS == {"rflw50": (3, 4, 6, 3), "rflw101": (3, 4, 23, 3), "rflw152": (3, 8, 36, 3)}       # untouched
    plan = {e[0]: e[2:] for e in deeplab.conv_plan("dlv3pr50")}
    base = f32net.resnet_plan("bottleneck", (3, 4, 6, 3))
    assert len(plan) == len(base) == 53 and [e[0] for e in deeplab.conv_plan("dlv3pr50")] == ["backbone." + e[0] for e in base]
    assert len(deeplab.conv_plan("dlv3pr101")) == 104 and len(deeplab.conv_plan((1, 1, 1, 1))) == 17
    # (Cout, Cin, kernel, stride, pad, dilation)
    assert plan["backbone.conv1"] == (64, 3, 7, 2, 3, 1) and plan["backbone.layer3.0.conv2"] == (256, 256, 3, 2, 1, 1)
    assert plan["backbone.layer4.0.conv2"] == (512, 512, 3, 1, 1, 1) and plan["backbone.layer4.0.downsample.0"] == (2048, 1024, 1, 1, 0, 1)
    assert plan["backbone.layer4.1.conv2"] == plan["backbone.layer4.2.conv2"] == (512, 512, 3, 1, 2, 2)
    assert plan["backbone.layer4.1.conv1"] == (512, 2048, 1, 1, 0, 1)
    for e, b in zip(deeplab.conv_plan("dlv3pr50"), base):
        if not b[0].startswith("layer4."):
            assert e[2:7] == b[2:] and e[7] == 1                     # layers 1 - 3 are f32net's plan
    head = {e[0]: e[1:] for e in deeplab.head_plan(19)}
    assert [e[0] for e in deeplab.head_plan(19)] == ["classifier." + k for k in (
        "project.0", "aspp.convs.0.0", "aspp.convs.1.0", "aspp.convs.2.0", "aspp.convs.3.0", "aspp.convs.4.1", "aspp.project.0",
        "classifier.0", "classifier.3")]
    assert head["classifier.project.0"] == ("classifier.project.1", 48, 256, 1, 1, 0, 1)
    for i, d in ((1, 6), (2, 12), (3, 18)):
        assert head[f"classifier.aspp.convs.{i}.0"] == (f"classifier.aspp.convs.{i}.1", 256, 2048, 3, 1, d, d)
    assert head["classifier.aspp.convs.4.1"] == ("classifier.aspp.convs.4.2", 256, 2048, 1, 1, 0, 1)
    assert head["classifier.aspp.project.0"] == ("classifier.aspp.project.1", 256, 1280, 1, 1, 0, 1)
    assert head["classifier.classifier.0"] == ("classifier.classifier.1", 256, 304, 3, 1, 1, 1)
    assert head["classifier.classifier.3"] == (None, 19, 256, 1, 1, 0, 1) and deeplab.head_plan(7)[-1][2] == 7
    sd = deeplab.random_state_dict((1, 1, 1, 1), 1)
    assert not any("fc." in k for k in sd) and sum(k.endswith("num_batches_tracked") for k in sd) == 17 + 8
    for bad in ("rflw50", "dlv3pr152", "resnet50", (1, 1, 1), (1, 0, 1, 1)):
        with pytest.raises(ValueError):
            deeplab.conv_plan(bad)


# ---- tables -------------------------------------------------------------------------------------------------------------------

def _axis_pairs():
    pairs = {(1, 1), (1, 5), (5, 1), (2, 2), (7, 7), (5, 9), (9, 5), (6, 16), (64, 16), (416, 1664)}
    pairs |= {(a, b) for a in range(1, 9) for b in range(1, 13)}                                   # a sweep of small ones
    for _n, _c, h, w, H, W in R.UPSAMPLE_CASES:
        pairs |= {(h, H), (w, W)}
    for _n, _c, sizes, _size in R.TTA_CASES.values():
        for (hq, wq), (hs, ws) in sizes:
            pairs |= {(hq, hs), (wq, ws)}
    for _arch, _ws, _is, _n, h, w in R.NET_CASES.values():                                          # the network's own two resizes
        for s in R.SCALES:
            hs, ws = R.scaled_hw(h, w, s)
            hq, wq = ((hs - 1) // 2 + 1 - 1) // 2 + 1, ((ws - 1) // 2 + 1 - 1) // 2 + 1
            pairs |= {(hq, hs), (wq, ws), (((hq - 1) // 2 + 1 - 1) // 2 + 1, hq), (((wq - 1) // 2 + 1 - 1) // 2 + 1, wq)}
    return sorted(pairs)


def test_half_pixel_tables_match_torch_fp64():
    from unirestore_amd import f32net
    pairs = _axis_pairs()
    assert len(pairs) > 100
    for n_in, n_out in pairs:
        idx, wt = f32net.hp_table(n_in, n_out)
        assert idx.dtype == torch.int32 and wt.dtype == torch.float64 and tuple(wt.shape) == (n_out, 2) and tuple(idx.shape) == (n_out,)
        assert int(idx.min()) >= 0 and int(idx.max()) <= n_in - 1 and float(wt.min()) >= 0 and float((wt.sum(dim=1) - 1).abs().max()) <= 1e-15
        assert float((R.table_matrix(idx, wt, n_in) - R.hp_matrix(n_in, n_out)).abs().max()) <= 1e-12, (n_in, n_out)
        if n_in == n_out:
            assert torch.equal(R.table_matrix(idx, wt, n_in), torch.eye(n_in, dtype=torch.float64))
    for bad in ((0, 4), (4, 0)):
        with pytest.raises(ValueError):
            f32net.hp_table(*bad)
    # the align_corners=True table keeps its values
    idx, wt = f32net.ac_table(3, 5)
    assert idx.tolist() == [0, 0, 1, 1, 2] and wt[:, 1].tolist() == [0.0, 0.5, 0.0, 0.5, 0.0]


# ---- weights --------------------------------------------------------------------------------------------------------------------

def test_load_weights_errors_and_the_three_checkpoint_forms(tmp_path):
    from unirestore_amd import deeplab
    arch = (1, 1, 1, 1)
    sd = deeplab.random_state_dict(arch, 4, 7)
    good = str(tmp_path / "dl.pth")
    torch.save(sd, good)
    w = deeplab.DeepLabWeights(arch, deeplab.read_state_dict(good), "cpu", source=good)
    assert w.num_classes == 7 and [len(s) for s in w.stages] == [1, 1, 1, 1] and len(w.convs) == 17 + 9 and len(w.backbone) == 17
    assert "backbone.bn1.num_batches_tracked" not in w.cpu and torch.equal(w.cpu["classifier.classifier.3.bias"], sd["classifier.classifier.3.bias"])
    c = w.convs
    assert (c["classifier.aspp.convs.3.0"].dilation, c["classifier.aspp.convs.3.0"].pad) == (18, 18)
    assert (w.backbone["layer4.0.conv2"].stride, w.backbone["layer4.0.conv2"].dilation, w.backbone["layer3.0.conv2"].stride) == (1, 1, 2)
    assert c["classifier.classifier.3"].cout == 7 and torch.equal(c["classifier.classifier.3"].bias, sd["classifier.classifier.3.bias"])
    # the BatchNorm fold is the fp64 one
    key, bn = "classifier.aspp.convs.2.0", "classifier.aspp.convs.2.1"
    scale = sd[f"{bn}.weight"].double() / torch.sqrt(sd[f"{bn}.running_var"].double() + 1e-5)
    assert torch.equal(c[key].bias, (sd[f"{bn}.bias"].double() - sd[f"{bn}.running_mean"].double() * scale).float())
    published, lightning = str(tmp_path / "best.pth"), str(tmp_path / "dl.ckpt")
    torch.save({"cur_itrs": 3, "model_state": sd, "best_score": 0.5}, published)
    torch.save({"epoch": 11, "state_dict": {**{"model.1." + k: v for k, v in sd.items()}, "model.0.mean": torch.zeros(3)}}, lightning)
    for path in (published, lightning):
        assert set(deeplab.read_state_dict(path)) == set(sd)
        w2 = deeplab.DeepLabWeights(arch, deeplab.read_state_dict(path), "cpu", source=path)
        assert torch.equal(w2.convs[key].w, c[key].w)

    def broken(change, key):
        bad = {k: v.clone() for k, v in sd.items()}
        change(bad)
        path = str(tmp_path / "bad.pth")
        torch.save(bad, path)
        with pytest.raises(ValueError) as e:
            deeplab.DeepLabWeights(arch, deeplab.read_state_dict(path), "cpu", source=path)
        assert path in str(e.value) and key in str(e.value), str(e.value)
    broken(lambda d: d.pop("backbone.layer2.0.downsample.1.running_mean"), "backbone.layer2.0.downsample.1.running_mean")
    broken(lambda d: d.pop("classifier.classifier.3.bias"), "classifier.classifier.3.bias")
    broken(lambda d: d.pop("classifier.classifier.3.weight"), "classifier.classifier.3.weight")
    broken(lambda d: d.pop("classifier.aspp.convs.4.1.weight"), "classifier.aspp.convs.4.1.weight")
    broken(lambda d: d.update({"classifier.aspp.project.0.weight": d["classifier.aspp.project.0.weight"][:, :1024]}), "classifier.aspp.project.0.weight")
    broken(lambda d: d["classifier.project.1.weight"].__setitem__(3, float("nan")), "classifier.project.1.weight")
    broken(lambda d: d["classifier.aspp.convs.1.0.weight"].__setitem__(0, float("inf")), "classifier.aspp.convs.1.0.weight")
    broken(lambda d: d["backbone.layer4.0.bn2.running_var"].__setitem__(0, -1.0), "backbone.layer4.0.bn2.running_var")
    with pytest.raises(ValueError, match="rflw50"):
        deeplab.load_weights("rflw50", good, dev="cpu")
    with pytest.raises(ValueError, match="backbone.layer1.1.conv1.weight"):           # a depth-1 file read as ResNet-50
        deeplab.load_weights("dlv3pr50", good, dev="cpu")
    notdict = str(tmp_path / "t.pth")
    torch.save(torch.zeros(3), notdict)
    with pytest.raises(ValueError, match="t.pth"):
        deeplab.load_weights("dlv3pr50", notdict, dev="cpu")


# ---- the command line -----------------------------------------------------------------------------------------------------------

def _write_pairs(folder, n=2, hw=(64, 64)):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    g = torch.Generator().manual_seed(0)
    for i in range(n):
        Image.fromarray((torch.rand(hw[0], hw[1], 3, generator=g) * 255).byte().numpy()).save(os.path.join(folder, f"im{i}.png"))
        Image.fromarray(torch.randint(0, 19, hw, generator=g).byte().numpy(), mode="L").save(os.path.join(folder, f"lab{i}.png"))
    lst = os.path.join(folder, "list.txt")
    with open(lst, "w") as f:
        f.write("".join(f"im{i}.png im{i}.png lab{i}.png\n" for i in range(n)))
    return lst


def _cfg(tmp_path, labels="map"):
    from unirestore_amd import cli
    lst = _write_pairs(str(tmp_path / "c"))
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))
    cfg["data"] = dict(class_path="unirestore_amd.data.ImageListFiles", init_args={"list_file": lst, "batch_size": 2, **({"labels": labels} if labels else {})})
    return cfg


class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_deeplab_argument_errors_come_before_the_model(tmp_path):
    from unirestore_amd import cli
    w = str(tmp_path / "dl.pth")
    torch.save({"not": torch.zeros(1)}, w)                # the checks below never open it
    assert cli.check_deeplab_arg(f"a=dlv3pr50:{w},b=dlv3pr101:{w}") == {"a": ("dlv3pr50", w), "b": ("dlv3pr101", w)}
    assert cli.check_deeplab_arg({"a": ("dlv3pr101", w)}, {"rf": ("rflw50", w)}) == {"a": ("dlv3pr101", w)}
    cfg = _cfg(tmp_path)
    plain = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))
    for arg, seg, tasks, c, word in [
        (f"a=rflw101:{w}", None, ["ir", "seg"], cfg, "rflw101"),                              # the other segmenter's arch
        (f"a=dlv3pr152:{w}", None, ["ir", "seg"], cfg, "dlv3pr152"),
        (f"a=dlv3pr50:{w}.missing", None, ["ir", "seg"], cfg, "no such file"),
        (f"a=dlv3pr50:{w},a=dlv3pr101:{w}", None, ["ir", "seg"], cfg, "twice"),
        (f"dlv3pr50:{w}", None, ["ir", "seg"], cfg, "NAME=ARCH"),
        (f"a=dlv3pr50:{w}", f"a=rflw50:{w}", ["ir", "seg"], cfg, "--segment too"),            # one name, two segmenters
        (f"a=dlv3pr50:{w}", None, None, cfg, "seg"),                                          # no --tasks
        (f"a=dlv3pr50:{w}", None, ["ir", "cls"], cfg, "--deeplab scores the 'seg' output"),
        (f"a=dlv3pr50:{w}", None, ["seg"], cfg, "'ir'"),
        (f"a=dlv3pr50:{w}", None, ["ir", "seg"], _cfg(tmp_path, labels=None), "--deeplab needs label maps"),
        (f"a=dlv3pr50:{w}", None, ["ir", "seg"], _cfg(tmp_path, labels=True), "labels: map"),
        (f"a=dlv3pr50:{w}", None, ["ir", "seg"], plain, "labels: map"),
    ]:
        with pytest.raises(ValueError) as e:
            cli.validate(c, tasks=tasks, deeplab=arg, segment=seg, model=_NoModel())
        assert word in str(e.value), (arg, tasks, str(e.value))
    # --segment keeps its own refusal of the DeepLab arch
    with pytest.raises(ValueError, match="dlv3pr50"):
        cli.check_segment_arg(f"a=dlv3pr50:{w}")


def test_deeplab_flag_belongs_to_validate(tmp_path, capsys):
    from unirestore_amd import cli
    w = str(tmp_path / "dl.pth")
    torch.save({"not": torch.zeros(1)}, w)
    cfg = os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")
    for argv, word in ((["restore", "--config", cfg, "--deeplab", f"a=dlv3pr50:{w}"], "--deeplab belongs to validate"),
                       (["print_config", "--config", cfg, "--deeplab", f"a=dlv3pr50:{w}"], "--deeplab belongs to validate"),
                       (["validate", "--config", cfg, "--deeplab", f"a=dlv3pr50:{w}"], "seg"),
                       (["validate", "--config", cfg, "--tasks", "ir,seg", "--deeplab", f"a=dlv3pr50:{w}"], "labels: map"),
                       (["validate", "--config", cfg, "--tasks", "ir,seg", "--deeplab", f"a=dlv3pr99:{w}"], "dlv3pr99"),
                       (["validate", "--config", cfg, "--tasks", "ir,seg", "--segment", f"a=rflw50:{w}", "--deeplab", f"a=dlv3pr50:{w}"],
                        "--segment too")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


# ---- the yardstick's own constants ----------------------------------------------------------------------------------------------

def test_tolerances_follow_the_measured_fp32_error():
    """Re-measures fp32's own error against fp64 for every recorded constant (deeplab_reference.py: E32_*) and fails when a
    recorded value is off by more than a factor of two, so every GPU bound (8 x the recorded e32) lies in [4, 16] x what is
    measured here."""
    pairs = [(f"conv {k}", R.CONV_TOL[k], R.measure_conv(k)) for k in R.CONV_CASES]
    pairs += [("slice", R.SLICE_TOL, R.measure_slice()),
              ("prep", R.PREP_TOL, max(R.measure_prep(c) for c in R.PREP_CASES)),
              ("upsample", R.UPSAMPLE_TOL, max(R.measure_upsample(c) for c in R.UPSAMPLE_CASES)),
              ("tta", R.TTA_TOL, max(R.measure_tta(k) for k in R.TTA_CASES))]
    for k in R.NET_CASES:
        e1, e3 = R.measure_logits(k)
        pairs += [(f"logits {k}", R.LOGITS_TOL[k], e1), (f"tta logits {k}", R.TTA_LOGITS_TOL[k], e3)]
    assert R.GPU_FACTOR == 8 and R.PREP_TOL == 8 * R.E32_PREP and R.UPSAMPLE_TOL == 8 * R.E32_UPSAMPLE and R.TTA_TOL == 8 * R.E32_TTA
    assert R.SLICE_TOL == 8 * R.E32_SLICE and R.CONV_TOL == {k: 8 * v for k, v in R.E32_CONV.items()} and set(R.E32_CONV) == set(R.CONV_CASES)
    assert R.LOGITS_TOL == {k: 8 * v for k, v in R.E32_LOGITS.items()} and R.TTA_LOGITS_TOL == {k: 8 * v for k, v in R.E32_TTA_LOGITS.items()}
    assert set(R.E32_LOGITS) == set(R.NET_CASES) == set(R.E32_TTA_LOGITS)
    for name, tol, e32 in pairs:
        print(f"{name}: measured {e32:.2e}, bound {tol:.2e}")
        assert math.isfinite(e32) and e32 > 0, name
        assert 4 * e32 <= tol <= 16 * e32, (name, tol, e32)


def test_network_cases_are_decidable_and_not_vacuous():
    """What the GPU test relies on, checked where it is chosen, IN THE REFERENCE ALONE: finite fp64 logits, at most 0.5 % of the
    pixels with a top-2 gap within twice the absolute bound, and at least five classes among the decidable pixels.  A case that
    fails here gets another seed, never another cap."""
    assert R.MAX_LEFT_OUT == 0.005 and R.MIN_CLASSES == 5
    for name in R.NET_CASES:
        want1, want3 = R.net_reference(name)
        assert bool(torch.isfinite(want1).all()) and bool(torch.isfinite(want3).all())
        ok = R.decidable(want3, R.TTA_LOGITS_TOL[name] * float(want3.abs().max()))
        left_out = 1.0 - float(ok.float().mean())
        classes = set(want3.argmax(dim=1)[ok].tolist())
        print(f"{name}: {left_out:.4%} left out, classes {sorted(classes)}, max |logit| {float(want3.abs().max()):.1f}")
        assert left_out <= R.MAX_LEFT_OUT and len(classes) >= R.MIN_CLASSES, name
    for name in R.TTA_CASES:
        maps, in_sizes, size = R.tta_case(name), [s for _q, s in R.TTA_CASES[name][2]], R.TTA_CASES[name][3]
        ok = R.decidable(R.tta_average(maps, in_sizes, size), R.TTA_TOL * max(float(m.abs().max()) for m in maps))
        assert 1.0 - float(ok.float().mean()) <= R.MAX_LEFT_OUT, name


def test_dilated_cases_exercise_what_they_claim():
    """The two ASPP-shaped cases: at dilation 6 on a 4 x 6 map every off-centre tap is padding; at 18 on 5 x 20 only horizontal
    taps are live."""
    for name, live in (("d6_all_side_taps_outside", {(1, 1)}), ("d18_horizontal_taps_only", {(1, 0), (1, 1), (1, 2)})):
        _n, h, w, _ci, _co, k, _s, pad, dil, _r, _relu = R.CONV_CASES[name]
        seen = {(kh, kw) for kh in range(k) for kw in range(k) for oh in range(h) for ow in range(w)
                if 0 <= oh - pad + kh * dil < h and 0 <= ow - pad + kw * dil < w}
        assert seen == live, (name, seen)


# ---- the new exports' argument checks (host only: every call below is refused before anything is launched) ----------------------

def test_new_exports_refuse_bad_arguments():
    from unirestore_amd import capi
    lib, P, Q, bad = capi.lib, 256, 512, capi.UR_E_INVALID   # P, Q: placeholder pointers, never dereferenced
    L = (1 << 31) - 256                                      # the 1-D launch limit
    I = (1 << 31) - 1

    def conv(x=P, w=P, b=P, res=None, y=Q, N=1, H=8, W=8, Cin=4, Cout=8, KH=3, KW=3, stride=1, pad=2, dil=2, ldy=8, relu=1):
        return lib.ur_dlv3_conv2d_f32(x, w, b, res, y, N, H, W, Cin, Cout, KH, KW, stride, pad, dil, ldy, relu, None)

    def tta(q0=P, q1=None, q2=None, nmaps=1, N=1, C=19, d=(4, 4, 16, 16, 0, 0, 0, 0, 0, 0, 0, 0), H=8, W=8, tabs=(P,) * 8, pred=Q, avg=None):
        return lib.ur_dlv3_tta_argmax(q0, q1, q2, nmaps, N, C, *d, H, W, *tabs, pred, avg, None)
    calls = [
        ("ur_dlv3_conv2d_f32", "null pointer", lambda: conv(x=None)),
        ("ur_dlv3_conv2d_f32", "null pointer", lambda: conv(y=None)),
        ("ur_dlv3_conv2d_f32", "dil must be >= 1", lambda: conv(dil=0)),
        ("ur_dlv3_conv2d_f32", "ldy >= Cout", lambda: conv(ldy=7)),
        ("ur_dlv3_conv2d_f32", "smaller than the filter", lambda: conv(dil=7, pad=2)),                # extent 15 > 8 + 4
        ("ur_dlv3_conv2d_f32", "fit an int", lambda: conv(dil=1 << 30, pad=0)),                      # dil (KH - 1) + 1 = 2^31 + 1
        ("ur_dlv3_conv2d_f32", "fit an int", lambda: conv(H=8, pad=(1 << 30) - 3)),                  # H + 2 pad = 2^31 + 2
        ("ur_dlv3_conv2d_f32", "filter too large", lambda: conv(Cin=(1 << 24) // 9 + 1)),
        ("ur_dlv3_conv2d_f32", "filter too large", lambda: conv(Cout=(1 << 24) + 1, ldy=(1 << 24) + 1)),
        ("ur_dlv3_conv2d_f32", "2^31 - 128", lambda: conv(N=(I - 128) // 64 + 1, pad=2, dil=2)),      # N*OH*OW one tile past
        ("ur_dlv3_conv2d_f32", "N*H*W below 2^31", lambda: conv(N=1 << 25, stride=8)),               # N*H*W = 2^31
        ("ur_dlv3_conv2d_f32", "16-byte aligned", lambda: conv(w=P + 4)),
        ("ur_dlv3_conv2d_f32", "same buffer", lambda: conv(res=Q)),
        ("ur_dlv3_conv2d_f32", "stride must be >= 1", lambda: conv(stride=0)),
        ("ur_dlv3_prep", "null pointer", lambda: lib.ur_dlv3_prep(P, None, 1, 3, 8, 8, 8, 8, P, P, P, P, None)),
        ("ur_dlv3_prep", "C must be 3", lambda: lib.ur_dlv3_prep(P, Q, 1, 4, 8, 8, 8, 8, P, P, P, P, None)),
        ("ur_dlv3_prep", ">= 1", lambda: lib.ur_dlv3_prep(P, Q, 1, 3, 8, 8, 0, 8, P, P, P, P, None)),
        ("ur_dlv3_prep", "below 2^31", lambda: lib.ur_dlv3_prep(P, Q, 1 << 12, 3, 512, 512, 8, 8, P, P, P, P, None)),
        ("ur_dlv3_prep", "below 2^31", lambda: lib.ur_dlv3_prep(P, Q, 1, 3, 8, 8, 1 << 15, (1 << 16) // 3 + 1, P, P, P, P, None)),
        ("ur_dlv3_broadcast_f32", "null pointer", lambda: lib.ur_dlv3_broadcast_f32(None, Q, 1, 4, 8, 8, None)),
        ("ur_dlv3_broadcast_f32", "same buffer", lambda: lib.ur_dlv3_broadcast_f32(P, P, 1, 4, 8, 8, None)),
        ("ur_dlv3_broadcast_f32", "ldy must be >= C", lambda: lib.ur_dlv3_broadcast_f32(P, Q, 1, 4, 8, 7, None)),
        ("ur_dlv3_broadcast_f32", ">= 1", lambda: lib.ur_dlv3_broadcast_f32(P, Q, 1, 0, 8, 8, None)),
        ("ur_dlv3_broadcast_f32", "2^31 - 256", lambda: lib.ur_dlv3_broadcast_f32(P, Q, L // 256, 1, 256, 256, None)),
        ("ur_dlv3_upsample_f32", "null pointer", lambda: lib.ur_dlv3_upsample_f32(P, Q, 1, 2, 2, 4, 4, 4, 4, P, None, P, P, None)),
        ("ur_dlv3_upsample_f32", "same buffer", lambda: lib.ur_dlv3_upsample_f32(P, P, 1, 2, 2, 4, 4, 4, 4, P, P, P, P, None)),
        ("ur_dlv3_upsample_f32", "ldy must be >= C", lambda: lib.ur_dlv3_upsample_f32(P, Q, 1, 2, 2, 4, 4, 4, 3, P, P, P, P, None)),
        ("ur_dlv3_upsample_f32", ">= 1", lambda: lib.ur_dlv3_upsample_f32(P, Q, 1, 0, 2, 4, 4, 4, 4, P, P, P, P, None)),
        ("ur_dlv3_upsample_f32", "2^31 - 256", lambda: lib.ur_dlv3_upsample_f32(P, Q, L // 256, 1, 1, 256, 1, 1, 256, P, P, P, P, None)),
        ("ur_dlv3_upsample_f32", "2^31 - 256", lambda: lib.ur_dlv3_upsample_f32(P, Q, 2, 8, 8, 256, 2048, 2048, 256, P, P, P, P, None)),
        ("ur_dlv3_tta_argmax", "nmaps", lambda: tta(nmaps=4)),
        ("ur_dlv3_tta_argmax", "nmaps", lambda: tta(nmaps=0)),
        ("ur_dlv3_tta_argmax", "null pointer", lambda: tta(nmaps=2)),
        ("ur_dlv3_tta_argmax", "null pointer", lambda: tta(pred=None)),
        ("ur_dlv3_tta_argmax", "null pointer", lambda: tta(tabs=(P,) * 5 + (None,) + (P,) * 2)),
        ("ur_dlv3_tta_argmax", "[1, 255]", lambda: tta(C=256)),
        ("ur_dlv3_tta_argmax", "[1, 255]", lambda: tta(C=0)),
        ("ur_dlv3_tta_argmax", "hq, wq, hs and ws", lambda: tta(d=(4, 4, 0, 16) + (0,) * 8)),
        ("ur_dlv3_tta_argmax", "hq, wq, hs and ws", lambda: tta(q1=P, nmaps=2, d=(4, 4, 16, 16, 0, 4, 8, 8) + (0,) * 4)),
        ("ur_dlv3_tta_argmax", "below 2^31 - 256", lambda: tta(N=L // 256, H=16, W=16, d=(1, 1, 16, 16) + (0,) * 8)),
        ("ur_dlv3_tta_argmax", "below 2^31 - 256", lambda: tta(N=8, H=4096, W=4096, avg=Q + 256)),
        ("ur_dlv3_tta_argmax", "below 2^31", lambda: tta(N=8, d=(4096, 4096, 16, 16) + (0,) * 8)),
        ("ur_dlv3_tta_argmax", "same buffer", lambda: tta(avg=P)),
    ]
    for export, word, call in calls:
        assert call() == bad, (export, word)
        msg = lib.ur_last_error().decode()
        assert msg.startswith(export + ":") and word in msg, (export, word, msg)
    # the old exports keep their own name in a refusal, and refuse what they refused
    assert lib.ur_conv2d_f32_res(P, P, P, None, Q, 1, 2, 2, 4, 8, 3, 3, 1, 0, 1, None) == bad
    assert lib.ur_last_error().decode().startswith("ur_conv2d_f32_res:") and "smaller than the filter" in lib.ur_last_error().decode()
