"""Classifier scoring, the parts that need no GPU: the BatchNorm fold, the resize tables, the accuracy formulas, the state-dict
loader, the labels of the file datasets, every --classify argument error, and the tolerances of classify_reference.py against
what fp32 measures here."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import classify_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- weights --------------------------------------------------------------------------------------------------------------------

def test_bn_fold_matches_the_unfused_block():
    """One Bottleneck (layer2.0: stride 2, a downsample path) with the folded fp32 weights the kernels get, evaluated in fp64,
    against the unfused fp64 restatement: the only difference is the fp32 rounding of the folded weights and biases."""
    from unirestore_amd import f32net
    sd = R.state_dict("resnet50", 3, 1000)
    x = F.relu(torch.randn(2, 256, 9, 7, generator=torch.Generator().manual_seed(1))).double()
    p = "layer2.0"
    out = F.relu(R._conv_bn(x, sd, f"{p}.conv1", f"{p}.bn1"))
    out = F.relu(R._conv_bn(out, sd, f"{p}.conv2", f"{p}.bn2", 2, 1))
    want = F.relu(R._conv_bn(out, sd, f"{p}.conv3", f"{p}.bn3") + R._conv_bn(x, sd, f"{p}.downsample.0", f"{p}.downsample.1", 2, 0))

    def folded(t, ckey, bkey, stride=1, pad=0):
        w, b = f32net.fold_bn(sd[f"{ckey}.weight"], *(sd[f"{bkey}.{n}"] for n in ("weight", "bias", "running_mean", "running_var")))
        assert w.dtype == torch.float64 and b.dtype == torch.float64
        return F.conv2d(t, w.float().double(), b.float().double(), stride=stride, padding=pad)
    got = F.relu(folded(x, f"{p}.conv1", f"{p}.bn1"))
    got = F.relu(folded(got, f"{p}.conv2", f"{p}.bn2", 2, 1))
    got = F.relu(folded(got, f"{p}.conv3", f"{p}.bn3") + folded(x, f"{p}.downsample.0", f"{p}.downsample.1", 2, 0))
    assert float(want.max()) > 0.1
    err = float((got - want).abs().max() / want.abs().max())
    print(f"fold: max |err| / max |y| {err:.2e}")
    assert err <= 4 * 2.0 ** -24                           # three layers of weights rounded to fp32 (2^-24 relative each)


def test_conv_plan_is_torchvisions_layout():
    from unirestore_amd import classify
    for arch, convs in (("resnet18", 20), ("resnet50", 53), ("resnet101", 104)):
        plan = classify.conv_plan(arch)
        assert len(plan) == convs and plan[0] == ("conv1", "bn1", 64, 3, 7, 2, 3)
        sd = classify.random_state_dict(arch, 0, 10)
        assert sd["fc.weight"].shape == (10, 512 if arch == "resnet18" else 2048)
        assert sum(k.endswith("conv1.weight") or ".conv" in k or "downsample.0" in k for k in sd) == convs
    p50 = {c[0]: c for c in classify.conv_plan("resnet50")}
    assert p50["layer2.0.conv2"][5] == 2 and p50["layer2.0.conv1"][5] == 1          # the stride sits on the 3x3 (v1.5)
    assert p50["layer2.0.downsample.0"][2:] == (512, 256, 1, 2, 0) and "layer2.1.downsample.0" not in p50
    assert "layer1.0.downsample.0" in p50 and "layer1.0.downsample.0" not in {c[0] for c in classify.conv_plan("resnet18")}
    with pytest.raises(ValueError, match="vgg16"):
        classify.conv_plan("vgg16")


def test_load_weights_errors_and_lightning_checkpoint(tmp_path):
    from unirestore_amd import classify
    sd = classify.random_state_dict("resnet18", 4, 200)
    good = str(tmp_path / "r18.pth")
    torch.save(sd, good)
    w = classify.load_weights("resnet18", good, dev="cpu")
    assert w.num_classes == 200 and w.arch == "resnet18" and len(w.blocks) == 8 and len(w.convs) == 20
    assert "bn1.num_batches_tracked" not in w.cpu and torch.equal(w.cpu["layer4.1.bn2.running_var"], sd["layer4.1.bn2.running_var"])
    assert w.convs["conv1"].stride == 2 and w.convs["conv1"].pad == 3 and w.fc.cout == 200
    # a Lightning checkpoint: ["state_dict"], keys with a leading "model."
    ckpt = str(tmp_path / "r18.ckpt")
    torch.save({"epoch": 6, "state_dict": {"model." + k: v for k, v in sd.items()}}, ckpt)
    w2 = classify.load_weights("resnet18", ckpt, dev="cpu")
    assert torch.equal(w2.convs["layer3.0.downsample.0"].w, w.convs["layer3.0.downsample.0"].w) and torch.equal(w2.fc.bias, w.fc.bias)

    def broken(change, key):
        bad = {k: v.clone() for k, v in sd.items()}
        change(bad)
        path = str(tmp_path / "bad.pth")
        torch.save(bad, path)
        with pytest.raises(ValueError) as e:
            classify.load_weights("resnet18", path, dev="cpu")
        assert path in str(e.value) and key in str(e.value), str(e.value)
    broken(lambda d: d.pop("layer2.0.downsample.1.running_mean"), "layer2.0.downsample.1.running_mean")
    broken(lambda d: d.pop("fc.bias"), "fc.bias")
    broken(lambda d: d.update({"layer1.0.conv1.weight": d["layer1.0.conv1.weight"][:, :32]}), "layer1.0.conv1.weight")
    broken(lambda d: d["layer3.1.bn1.weight"].__setitem__(3, float("nan")), "layer3.1.bn1.weight")
    broken(lambda d: d["layer4.0.bn2.running_var"].__setitem__(0, -1.0), "layer4.0.bn2.running_var")
    broken(lambda d: d.update({"fc.weight": d["fc.weight"][:, :100]}), "fc.weight")
    with pytest.raises(ValueError, match="resnet34"):
        classify.load_weights("resnet34", good, dev="cpu")
    r50 = str(tmp_path / "r50.pth")                                  # a ResNet-50 file read as ResNet-18: the stems agree, layer1 does not
    torch.save(classify.random_state_dict("resnet50", 0, 10), r50)
    with pytest.raises(ValueError, match="layer1.0.conv1.weight"):
        classify.load_weights("resnet18", r50, dev="cpu")


# ---- the preprocess tables ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.PREP_CASES, ids=["x".join(map(str, s)) for s in R.PREP_CASES])
def test_resize_tables_match_torch_fp64(shape):
    """The two tables applied in fp64 (W first, then H) against torch's fp64 interpolate(antialias=True)."""
    from unirestore_amd import classify
    x = R.images(shape, 3).double()

    def matrix(n_in):
        first, count, wt = classify.resize_table(n_in)
        assert first.dtype == torch.int32 and count.dtype == torch.int32 and wt.dtype == torch.float64 and wt.shape[0] == 224
        assert int(first.min()) >= 0 and int((first + count).max()) <= n_in and int(count.min()) >= 1 and int(count.max()) == wt.shape[1]
        a = torch.zeros(224, n_in, dtype=torch.float64)
        for i in range(224):
            a[i, first[i]:first[i] + count[i]] = wt[i, :count[i]]
            assert float(wt[i, count[i]:].abs().sum()) == 0.0
        assert float((a.sum(dim=1) - 1).abs().max()) <= 1e-15
        return a
    ah, aw = matrix(shape[2]), matrix(shape[3])
    got = torch.einsum("yh,nchw,xw->ncyx", ah, x, aw)
    want = F.interpolate(x, size=(224, 224), mode="bilinear", antialias=True, align_corners=False)
    err = float((got - want).abs().max())
    print(f"{shape}: taps {aw.shape[1]} -> {int((aw != 0).sum(dim=1).max())} x {int((ah != 0).sum(dim=1).max())}, max |err| {err:.2e}")
    assert err <= 1e-13


def test_resize_table_tap_counts():
    from unirestore_amd import classify
    assert classify.resize_table(1664)[2].shape[1] <= 16 and classify.resize_table(224)[1].max() <= 2
    up = classify.resize_table(80)                                    # growing: plain bilinear, two taps at most
    assert int(up[1].max()) == 2
    assert classify.resize_table(1)[2].tolist() == [[1.0]] * 224
    with pytest.raises(ValueError):
        classify.resize_table(0)
    with pytest.raises(ValueError, match="taps"):
        classify.resize_table(224 * 40)


# ---- accuracy -------------------------------------------------------------------------------------------------------------------

def test_accuracy_on_hand_made_counts():
    from unirestore_amd import classify
    # five classes.  0: 3 of 4 right; 1: 0 of 2 right; 2: never a target, predicted 3 times (counts as 0); 3: 1 of 1; 4: on neither
    # side (left out of the macro mean)
    tp, targets, predicted = [3, 0, 0, 1, 0], [4, 2, 0, 1, 0], [3, 0, 3, 1, 0]
    macro, micro = classify.accuracy(torch.tensor(tp), torch.tensor(targets), torch.tensor(predicted))
    assert macro == pytest.approx((0.75 + 0.0 + 0.0 + 1.0) / 4, abs=1e-15) and micro == pytest.approx(4 / 7, abs=1e-15)
    assert (macro, micro) == pytest.approx(R.accuracy(tp, targets, predicted), abs=1e-15)
    assert classify.accuracy([2, 2], [2, 2], [2, 2]) == (1.0, 1.0)
    assert classify.accuracy([0, 0], [0, 0], [0, 0]) == (0.0, 0.0)                 # no images
    # from predictions, through the bincount restatement
    pred, labels = [1, 1, 2, 0, 3, 3], [1, 2, 2, 0, 0, 3]
    c = R.counts(pred, labels, 6)
    assert c[0].tolist() == [1, 1, 1, 1, 0, 0] and c[1].tolist() == [2, 1, 2, 1, 0, 0] and c[2].tolist() == [1, 2, 1, 2, 0, 0]
    macro, micro = classify.accuracy(*(torch.from_numpy(v) for v in c))
    assert macro == pytest.approx((0.5 + 1 + 0.5 + 1) / 4) and micro == pytest.approx(4 / 6)


# ---- labels ---------------------------------------------------------------------------------------------------------------------

def _write_images(folder, n, hw=(40, 48)):
    from PIL import Image
    import numpy as np
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(7)
    names = []
    for i in range(n):
        names.append(f"img{i}.png")
        Image.fromarray(rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)).save(os.path.join(folder, names[-1]))
    return names


def test_image_list_labels(tmp_path):
    from unirestore_amd import data
    names = _write_images(str(tmp_path), 3)
    lst = tmp_path / "pairs.txt"
    lst.write_text("# lq hq label\n" + "".join(f"{n} {n} {7 * i + 1}\n" for i, n in enumerate(names)) + "\n")
    off = list(data.ImageListFiles(str(lst), batch_size=2).batches())
    on = list(data.ImageListFiles(str(lst), batch_size=2, labels=True).batches())
    assert [b[2] for b in off] == [None, None]                                     # off: exactly what it was
    assert [b[2].tolist() for b in on] == [[1, 8], [15]] and all(b[2].dtype == torch.int64 for b in on)
    for a, b in zip(off, on):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[3:] == b[3:]
    bad = tmp_path / "bad.txt"
    bad.write_text(f"{names[0]} {names[0]} 3\n{names[1]} {names[1]} cat\n")
    with pytest.raises(ValueError, match=r"bad.txt:2.*'cat'"):
        data.ImageListFiles(str(bad), labels=True)
    assert data.ImageListFiles(str(bad)).pairs                                      # without labels the column is not read
    two = tmp_path / "two.txt"
    two.write_text(f"{names[0]} {names[0]} 3\n\n{names[1]} {names[1]}\n")
    with pytest.raises(ValueError, match=r"two.txt:3"):
        data.ImageListFiles(str(two), labels=True)


@pytest.mark.parametrize("cls", ["CorruptedImageFiles", "DistortedImageFiles", "JpegImageFiles"])
def test_degraded_files_labels_are_checked_when_built(tmp_path, cls):
    from unirestore_amd import data
    names = _write_images(str(tmp_path / "imgs"), 2)
    lst = tmp_path / "imgs" / "list.txt"
    lst.write_text("".join(f"{n} {n} {i + 5}\n" for i, n in enumerate(names)))
    ds = getattr(data, cls)(str(lst), labels=True)
    assert ds.labels == [5, 6] and getattr(data, cls)(str(lst)).labels is None
    with pytest.raises(ValueError, match="folder"):
        getattr(data, cls)(str(tmp_path / "imgs"), labels=True)
    two = tmp_path / "imgs" / "two.txt"
    two.write_text("".join(f"{n} {n}\n" for n in names))
    with pytest.raises(ValueError, match=r"two.txt:1"):
        getattr(data, cls)(str(two), labels=True)
    assert getattr(data, cls)(str(two)).labels is None


# ---- the command line -----------------------------------------------------------------------------------------------------------

def _cfg(tmp_path, labels=True, data_class="ImageListFiles"):
    from unirestore_amd import cli
    names = _write_images(str(tmp_path / "d"), 2)
    lst = tmp_path / "d" / "list.txt"
    lst.write_text("".join(f"{n} {n} {i}\n" for i, n in enumerate(names)))
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))
    key = "list_file" if data_class == "ImageListFiles" else "source"
    cfg["data"] = dict(class_path=f"unirestore_amd.data.{data_class}", init_args={key: str(lst), "batch_size": 2, **({"labels": True} if labels else {})})
    return cfg


class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_classify_argument_errors_come_before_the_model(tmp_path):
    from unirestore_amd import classify, cli
    w = str(tmp_path / "r18.pth")
    torch.save(classify.random_state_dict("resnet18", 0, 10), w)
    assert cli.check_classify_arg(f"a=resnet18:{w},b=resnet18:{w}") == {"a": ("resnet18", w), "b": ("resnet18", w)}
    assert cli.check_classify_arg({"a": ("resnet18", w)}) == {"a": ("resnet18", w)}
    cfg = _cfg(tmp_path)
    for arg, tasks, c, word in [
        (f"a=vgg16:{w}", ["ir", "cls"], cfg, "vgg16"),                                        # an unknown arch
        (f"a=resnet18:{w}.missing", ["ir", "cls"], cfg, "no such file"),
        (f"a=resnet18:{w},a=resnet18:{w}", ["ir", "cls"], cfg, "twice"),
        (f"resnet18:{w}", ["ir", "cls"], cfg, "NAME=ARCH"),                                   # no name
        (f"a={w}", ["ir", "cls"], cfg, "NAME=ARCH"),                                          # no arch
        (f"a=resnet18:{w}", None, cfg, "cls"),                                                # no --tasks
        (f"a=resnet18:{w}", ["ir", "seg"], cfg, "cls"),                                       # --tasks without cls
        (f"a=resnet18:{w}", ["cls"], cfg, "'ir'"),                                            # ir stays required
        (f"a=resnet18:{w}", ["ir", "cls"], _cfg(tmp_path, labels=False), "labels: true"),
        (f"a=resnet18:{w}", ["ir", "cls"], _cfg(tmp_path, labels=False, data_class="CorruptedImageFiles"), "labels: true"),
        (f"a=resnet18:{w}", ["ir", "cls"], cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")), "labels: true"),
    ]:
        with pytest.raises(ValueError) as e:
            cli.validate(c, tasks=tasks, classify=arg, model=_NoModel())
        assert word in str(e.value), (arg, tasks, str(e.value))


def test_classify_flag_belongs_to_validate(tmp_path, capsys):
    from unirestore_amd import classify, cli
    w = str(tmp_path / "r18.pth")
    torch.save(classify.random_state_dict("resnet18", 0, 10), w)
    cfg = os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")
    for argv in (["restore", "--config", cfg, "--classify", f"a=resnet18:{w}"], ["print_config", "--config", cfg, "--classify", f"a=resnet18:{w}"],
                 ["corrupt", "--input", str(tmp_path), "--output", str(tmp_path / "o"), "--classify", f"a=resnet18:{w}"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and "--classify belongs to validate" in capsys.readouterr().err
    for argv, word in ((["validate", "--config", cfg, "--classify", f"a=resnet18:{w}"], "cls"),
                       (["validate", "--config", cfg, "--tasks", "ir,cls", "--classify", f"a=resnet18:{w}"], "labels: true"),
                       (["validate", "--config", cfg, "--tasks", "ir,cls", "--classify", f"a=resnet99:{w}"], "resnet99")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


# ---- the yardstick's own constants ----------------------------------------------------------------------------------------------

def test_tolerances_follow_the_measured_fp32_error():
    """Re-measures fp32's own error against fp64 for every recorded constant (classify_reference.py: E32_*) and holds the constants
    to the measurement by lpips_reference's rule: every GPU bound (8 x the recorded e32) must be >= 4 x and <= 16 x what is
    measured here.  The torch-fp32 preprocess figures (TORCH32_PREP) are held the same way."""
    prep = {s: R.measure_prep(s) for s in R.PREP_CASES}
    pairs = [("prep", R.PREP_TOL, max(a for a, _ in prep.values()))]
    pairs += [(f"conv {k}", R.CONV_TOL[k], R.measure_conv(k)) for k in R.CONV_CASES]
    pairs += [("avgpool", R.AVGPOOL_TOL, max(R.measure_avgpool(s) for s in R.AVGPOOL_CASES))]
    pairs += [(f"logits {k}", R.LOGITS_TOL[k], R.measure_logits(k)) for k in R.NET_CASES]
    pairs += [("forward", R.FORWARD_TOL, R.measure_forward())]
    pairs += [(f"torch32 prep {s}", 8 * R.TORCH32_PREP[s], b) for s, (_, b) in prep.items()]
    assert R.PREP_TOL == 8 * R.E32_PREP and R.AVGPOOL_TOL == 8 * R.E32_AVGPOOL and R.FORWARD_TOL == 8 * R.E32_FORWARD
    assert R.CONV_TOL == {k: 8 * v for k, v in R.E32_CONV.items()} and R.LOGITS_TOL == {k: 8 * v for k, v in R.E32_LOGITS.items()}
    assert set(R.E32_CONV) == set(R.CONV_CASES) and set(R.E32_LOGITS) == set(R.NET_CASES) and set(R.TORCH32_PREP) == set(R.PREP_CASES)
    for name, tol, e32 in pairs:
        print(f"{name}: measured {e32:.2e}, bound {tol:.2e}")
        assert math.isfinite(e32) and e32 > 0, name
        assert 4 * e32 <= tol <= 16 * e32, (name, tol, e32)
    for s, (a, b) in prep.items():
        assert a <= b + 1e-12, (s, a, b)                  # the fp32 tables are never further from fp64 than torch's own fp32 path


def test_network_cases_are_decidable():
    """What the GPU test relies on, checked where it is chosen: finite fp64 logits, every image's top-2 gap above twice the
    absolute bound, and at least two distinct predicted classes in the resnet50 64 x 64 case."""
    for name in R.NET_CASES:
        want = R.net_reference(name)
        bound = R.LOGITS_TOL[name] * float(want.abs().max())
        assert bool(torch.isfinite(want).all()) and float(R.top2_gap(want).min()) > 2 * bound, name
    assert len(set(R.net_reference("resnet50_4x64x64").argmax(dim=1).tolist())) >= 2
    want = R.forward_reference()
    assert float(R.top2_gap(want).min()) > 2 * R.FORWARD_TOL * float(want.abs().max())
