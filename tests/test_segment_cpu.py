"""Segmenter scoring, the parts that need no GPU: the restatement against the stored vector of the reference's own network
(tests/golden/rflw_0.npz, tools/gen_golden_seg.py), the scaled sizes and tap tables, the mIoU formula, the state-dict loader, the
label maps of the file datasets, every --segment / --crop argument error, and the tolerances of segment_reference.py against what
fp32 measures here."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import segment_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against the reference's own network ------------------------------------------------------------------------

def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "rflw_0.npz"))


def _checksum(v):
    return float((v.double().flatten() * torch.arange(1, v.numel() + 1, dtype=torch.float64)).sum())


def test_restatement_reproduces_the_reference_network():
    from unirestore_amd import segment
    g = _golden()
    depths = tuple(int(d) for d in g["depths"])
    sd = segment.random_state_dict(depths, int(g["weight_seed"]))
    sums = dict(zip(g["checksum_keys"].tolist(), g["checksums"].tolist()))
    assert set(sums) == {k for k, v in sd.items() if v.is_floating_point()}
    for k, want in sums.items():                          # first: the stand-in weights are the ones the vector was made with
        assert _checksum(sd[k]) == pytest.approx(want, rel=1e-12, abs=1e-12), \
            f"{k}: torch's random generator no longer draws the weights tests/golden/rflw_0.npz was made with - regenerate it"
    x = torch.from_numpy(g["image"]).double() / 255
    want = torch.from_numpy(g["logits"])
    got = R.refinenet(R.preprocess(x), sd, depths)
    assert got.shape == want.shape and got.shape[1] == 19
    err = float((got - want).abs().max() / want.abs().max())
    print(f"logits: max |err| / max |logit| {err:.2e}")
    assert err <= 1e-12
    pred = R.tta_logits(x, sd, depths, scales=tuple(float(s) for s in g["scales"])).argmax(dim=1)
    assert torch.equal(pred, torch.from_numpy(g["pred"]).long()) and len(set(pred.flatten().tolist())) >= R.MIN_CLASSES
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "rflw_0.npz")) < 256 * 1024


def test_plans_are_the_reference_modules_layout():
    from unirestore_amd import classify, segment
    assert segment.ARCHS == {"rflw50": (3, 4, 6, 3), "rflw101": (3, 4, 23, 3), "rflw152": (3, 8, 36, 3)}
    assert segment.conv_plan("rflw50") == classify.conv_plan("resnet50") and segment.conv_plan("rflw101") == classify.conv_plan("resnet101")
    assert len(segment.conv_plan((1, 1, 1, 1))) == 1 + 4 * 4 and len(segment.conv_plan("rflw152")) == 1 + 3 * 50 + 4
    head = {k: (cout, cin, ksz) for k, cout, cin, ksz in segment.head_plan(19)}
    assert len(head) == 4 + 3 + 16 + 3 + 1
    assert head["p_ims1d2_outl1_dimred"] == (512, 2048, 1) and head["p_ims1d2_outl4_dimred"] == (256, 256, 1)
    assert head["mflow_conv_g1_pool.0.4_outvar_dimred"] == (512, 512, 1) and head["mflow_conv_g1_b3_joint_varout_dimred"] == (256, 512, 1)
    assert head["adapt_stage4_b2_joint_varout_dimred"] == (256, 256, 1) and head["clf_conv"] == (19, 256, 3)
    assert "adapt_stage1_b2_joint_varout_dimred" not in head and "mflow_conv_g4_b3_joint_varout_dimred" not in head
    for bad in ("rflw18", "resnet50", (1, 1, 1), (1, 0, 1, 1)):
        with pytest.raises(ValueError):
            segment.conv_plan(bad)


# ---- sizes and tables -----------------------------------------------------------------------------------------------------------

def test_scaled_size_is_torchs_for_every_size():
    from unirestore_amd import segment
    checked = 0
    for s in (0.8, 0.6):
        for n in range(1, 2049):                          # every size, asked of torch itself (a size that scales to 0 it refuses)
            got = segment.scaled_size(n, s)
            if got == 0:
                assert n == 1
                continue
            assert F.interpolate(torch.zeros(1, 1, n, 1), scale_factor=(s, 1), mode="bilinear", align_corners=True).shape[2] == got, (n, s)
            checked += 1
    assert checked == 2 * 2047
    assert segment.scaled_size(512, 1) == 512 and segment.scaled_size(54, 0.6) == 32 and segment.scaled_size(53, 0.6) == 31


@pytest.mark.parametrize("n_in,n_out", [(1, 1), (1, 5), (5, 1), (2, 2), (16, 64), (12, 64), (9, 64), (54, 32), (97, 58), (131, 78), (7, 7), (416, 1664)])
def test_tap_tables_match_torch_fp64(n_in, n_out):
    from unirestore_amd import f32net
    idx, wt = f32net.ac_table(n_in, n_out)
    assert idx.dtype == torch.int32 and wt.dtype == torch.float64 and tuple(wt.shape) == (n_out, 2) and tuple(idx.shape) == (n_out,)
    assert int(idx.min()) >= 0 and int(idx.max()) <= n_in - 1 and float(wt.min()) >= 0 and float((wt.sum(dim=1) - 1).abs().max()) <= 1e-15
    a = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        a[o, idx[o]] += wt[o, 0]
        a[o, min(int(idx[o]) + 1, n_in - 1)] += wt[o, 1]
    assert float((a - R.ac_matrix(n_in, n_out)).abs().max()) <= 1e-12
    if n_in == n_out:
        assert torch.equal(a, torch.eye(n_in, dtype=torch.float64))      # the same size: weights (1, 0), the identity bit for bit
    with pytest.raises(ValueError):
        f32net.ac_table(0, n_out)


# ---- mIoU -----------------------------------------------------------------------------------------------------------------------

def test_miou_on_hand_made_matrices():
    from unirestore_amd import segment
    # four classes, conf[target][pred].  0: 3 right, 1 taken for class 2.  1: 2 right.  2: never a target, predicted once (IoU 0).
    # 3: on neither side (left out of the mean)
    conf = [[3, 0, 1, 0], [0, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    m, acc, ious = segment.miou(torch.tensor(conf))
    assert m == pytest.approx((3 / 4 + 1.0 + 0.0) / 3, abs=1e-15) and acc == pytest.approx(5 / 6, abs=1e-15)
    assert ious[:3] == pytest.approx([0.75, 1.0, 0.0], abs=1e-15) and math.isnan(ious[3])
    assert (m, acc) == pytest.approx(R.miou(conf), abs=1e-15)
    assert m == pytest.approx(R.miou_hist(conf), abs=1e-6)                 # the reference's own formula (a float32 histogram)
    assert segment.miou(torch.zeros(19, 19, dtype=torch.int64)) == (0.0, 0.0, [])          # all pixels ignored
    assert segment.miou(torch.eye(3, dtype=torch.int64) * 7)[:2] == (1.0, 1.0)
    # from predictions, through the bincount restatement, with ignored pixels
    g = torch.Generator().manual_seed(0)
    target = torch.randint(0, 19, (3000,), generator=g)
    target[::7] = 255
    pred = torch.where(torch.rand(3000, generator=g) < 0.7, target.clamp(max=18), torch.randint(0, 19, (3000,), generator=g))
    c = R.confusion(pred.numpy(), target.numpy())
    assert int(c.sum()) == int((target != 255).sum())
    m, acc, _ = segment.miou(torch.from_numpy(c))
    assert (m, acc) == pytest.approx(R.miou(c.tolist()), abs=1e-14) and m == pytest.approx(R.miou_hist(c), abs=1e-6) and 0.3 < m < acc < 1


# ---- weights --------------------------------------------------------------------------------------------------------------------

def test_load_weights_errors_and_lightning_checkpoint(tmp_path):
    from unirestore_amd import segment
    sd = segment.random_state_dict("rflw50", 4, 7)
    good = str(tmp_path / "rf.pth")
    torch.save(sd, good)
    w = segment.load_weights("rflw50", good, dev="cpu")
    assert w.num_classes == 7 and w.arch == "rflw50" and [len(s) for s in w.stages] == [3, 4, 6, 3] and len(w.convs) == 53 + 27
    assert "bn1.num_batches_tracked" not in w.cpu and torch.equal(w.cpu["clf_conv.bias"], sd["clf_conv.bias"])
    assert w.convs["clf_conv"].pad == 1 and w.convs["clf_conv"].cout == 7 and float(w.convs["p_ims1d2_outl1_dimred"].bias.abs().max()) == 0.0
    ckpt = str(tmp_path / "rf.ckpt")
    torch.save({"epoch": 6, "state_dict": {"model." + k: v for k, v in sd.items()}}, ckpt)
    w2 = segment.load_weights("rflw50", ckpt, dev="cpu")
    assert torch.equal(w2.convs["mflow_conv_g2_pool.0.3_outvar_dimred"].w, w.convs["mflow_conv_g2_pool.0.3_outvar_dimred"].w)

    def broken(change, key):
        bad = {k: v.clone() for k, v in sd.items()}
        change(bad)
        path = str(tmp_path / "bad.pth")
        torch.save(bad, path)
        with pytest.raises(ValueError) as e:
            segment.load_weights("rflw50", path, dev="cpu")
        assert path in str(e.value) and key in str(e.value), str(e.value)
    broken(lambda d: d.pop("layer2.0.downsample.1.running_mean"), "layer2.0.downsample.1.running_mean")
    broken(lambda d: d.pop("clf_conv.bias"), "clf_conv.bias")
    broken(lambda d: d.pop("clf_conv.weight"), "clf_conv.weight")
    broken(lambda d: d.pop("mflow_conv_g3_pool.0.2_outvar_dimred.weight"), "mflow_conv_g3_pool.0.2_outvar_dimred.weight")
    broken(lambda d: d.update({"adapt_stage2_b2_joint_varout_dimred.weight": d["adapt_stage2_b2_joint_varout_dimred.weight"][:, :32]}),
           "adapt_stage2_b2_joint_varout_dimred.weight")
    broken(lambda d: d["layer3.1.bn1.weight"].__setitem__(3, float("nan")), "layer3.1.bn1.weight")
    broken(lambda d: d["p_ims1d2_outl3_dimred.weight"].__setitem__(0, float("inf")), "p_ims1d2_outl3_dimred.weight")
    broken(lambda d: d["layer4.0.bn2.running_var"].__setitem__(0, -1.0), "layer4.0.bn2.running_var")
    with pytest.raises(ValueError, match="rflw34"):
        segment.load_weights("rflw34", good, dev="cpu")
    with pytest.raises(ValueError, match="layer3.6.conv1.weight"):           # a ResNet-50 file read as ResNet-101
        segment.load_weights("rflw101", good, dev="cpu")


# ---- label maps -----------------------------------------------------------------------------------------------------------------

def _write_pairs(folder, n=3, hw=(40, 48), label_hw=None, seed=0):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    maps = []
    for i in range(n):
        img = (torch.rand(hw[0], hw[1], 3, generator=g) * 255).byte().numpy()
        Image.fromarray(img).save(os.path.join(folder, f"im{i}.png"))
        lab = torch.randint(0, 40, label_hw or hw, generator=g).byte()
        lab[0, 0], lab[0, 1] = 255, 7
        Image.fromarray(lab.numpy(), mode="L").save(os.path.join(folder, f"lab{i}.png"))
        maps.append(lab.long())
    lst = os.path.join(folder, "list.txt")
    with open(lst, "w") as f:
        f.write("# lq hq label\n" + "".join(f"im{i}.png im{i}.png lab{i}.png\n" for i in range(n)))
    return lst, maps


def _train_id(lab):
    out = torch.full_like(lab, 255)
    for k, v in R.CITYSCAPES_TRAIN_ID.items():
        out[lab == k] = v
    return out


def test_image_list_label_maps(tmp_path):
    from unirestore_amd import data
    assert data.CITYSCAPES_TRAIN_ID == R.CITYSCAPES_TRAIN_ID and len(data.CITYSCAPES_TRAIN_ID) == 19
    lst, maps = _write_pairs(str(tmp_path / "d"))
    off = list(data.ImageListFiles(lst, batch_size=2).batches())
    city = list(data.ImageListFiles(lst, batch_size=2, labels="map").batches())
    raw = list(data.ImageListFiles(lst, batch_size=2, labels="map", label_encoding="train_id").batches())
    assert [b[2] for b in off] == [None, None] and [tuple(b[2].shape) for b in city] == [(2, 40, 48), (1, 40, 48)]
    for a, b, c in zip(off, city, raw):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[3] == b[3] == c[3]          # the images do not change
    assert all(b[2].dtype == torch.int64 for b in city + raw)
    assert torch.equal(torch.cat([b[2] for b in raw]), torch.stack(maps))
    got = torch.cat([b[2] for b in city])
    assert torch.equal(got, torch.stack([_train_id(m) for m in maps]))
    assert int(got[0, 0, 0]) == 255 and int(got[0, 0, 1]) == 0 and set(got.unique().tolist()) <= set(range(19)) | {255}
    # errors name file and line
    bad, _ = _write_pairs(str(tmp_path / "bad"), label_hw=(40, 47))
    with pytest.raises(ValueError, match=r"list.txt:2.*40 x 47"):
        list(data.ImageListFiles(bad, labels="map").batches())
    two = tmp_path / "two.txt"
    two.write_text("d/im0.png d/im0.png\n")
    with pytest.raises(ValueError, match="two.txt:1"):
        data.ImageListFiles(str(two), labels="map")
    gone = tmp_path / "gone.txt"
    gone.write_text("d/im0.png d/im0.png d/nothing.png\n")
    with pytest.raises(ValueError, match=r"gone.txt:1.*nothing.png"):
        list(data.ImageListFiles(str(gone), labels="map").batches())
    for kw in (dict(labels="maps"), dict(labels="map", label_encoding="voc")):
        with pytest.raises(ValueError):
            data.ImageListFiles(lst, **kw)
    assert data.ImageListFiles(lst, labels=False).labels is None


@pytest.mark.parametrize("cls", ["CorruptedImageFiles", "DistortedImageFiles", "JpegImageFiles"])
def test_degraded_files_label_maps_are_checked_when_built(tmp_path, cls):
    from unirestore_amd import data
    lst, _maps = _write_pairs(str(tmp_path / "d"))
    ds = getattr(data, cls)(lst, labels="map", label_encoding="train_id")
    assert [os.path.basename(p) for p, _ in ds.labels] == ["lab0.png", "lab1.png", "lab2.png"] and [ln for _, ln in ds.labels] == [2, 3, 4]
    with pytest.raises(ValueError, match="folder"):
        getattr(data, cls)(str(tmp_path / "d"), labels="map")           # a folder source carries no labels
    with pytest.raises(ValueError, match="label_encoding"):
        getattr(data, cls)(lst, labels="map", label_encoding="ade20k")
    assert getattr(data, cls)(str(tmp_path / "d")).labels is None


# ---- the command line -----------------------------------------------------------------------------------------------------------

def _cfg(tmp_path, labels="map", data_class="ImageListFiles"):
    from unirestore_amd import cli
    lst, _ = _write_pairs(str(tmp_path / "c"), n=2, hw=(64, 64))
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))
    key = "list_file" if data_class == "ImageListFiles" else "source"
    cfg["data"] = dict(class_path=f"unirestore_amd.data.{data_class}", init_args={key: lst, "batch_size": 2, **({"labels": labels} if labels else {})})
    return cfg


class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_segment_argument_errors_come_before_the_model(tmp_path):
    from unirestore_amd import cli
    w = str(tmp_path / "rf.pth")
    torch.save({"not": torch.zeros(1)}, w)                # the checks below never open it
    assert cli.check_segment_arg(f"a=rflw101:{w},b=rflw50:{w}") == {"a": ("rflw101", w), "b": ("rflw50", w)}
    assert cli.check_segment_arg({"a": ("rflw152", w)}) == {"a": ("rflw152", w)}
    assert cli.check_crop_arg("960,1664") == (960, 1664) and cli.check_crop_arg((512, 512)) == (512, 512)
    cfg = _cfg(tmp_path)
    for arg, tasks, c, word in [
        (f"a=dlv3pr50:{w}", ["ir", "seg"], cfg, "dlv3pr50"),                                  # an unknown arch
        (f"a=resnet101:{w}", ["ir", "seg"], cfg, "resnet101"),
        (f"a=rflw101:{w}.missing", ["ir", "seg"], cfg, "no such file"),
        (f"a=rflw101:{w},a=rflw50:{w}", ["ir", "seg"], cfg, "twice"),
        (f"rflw101:{w}", ["ir", "seg"], cfg, "NAME=ARCH"),                                    # no name
        (f"a={w}", ["ir", "seg"], cfg, "NAME=ARCH"),                                          # no arch
        (f"a=rflw101:{w}", None, cfg, "seg"),                                                 # no --tasks
        (f"a=rflw101:{w}", ["ir", "cls"], cfg, "seg"),                                        # --tasks without seg
        (f"a=rflw101:{w}", ["seg"], cfg, "'ir'"),                                             # ir stays required
        (f"a=rflw101:{w}", ["ir", "seg"], _cfg(tmp_path, labels=None), "labels: map"),
        (f"a=rflw101:{w}", ["ir", "seg"], _cfg(tmp_path, labels=True), "labels: map"),        # integer labels are no maps
        (f"a=rflw101:{w}", ["ir", "seg"], _cfg(tmp_path, labels=None, data_class="CorruptedImageFiles"), "labels: map"),
        (f"a=rflw101:{w}", ["ir", "seg"], cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")), "labels: map"),
    ]:
        with pytest.raises(ValueError) as e:
            cli.validate(c, tasks=tasks, segment=arg, model=_NoModel())
        assert word in str(e.value), (arg, tasks, str(e.value))
    for crop in ("960", "960,x", "0,5", (1, 2, 3), 512):
        with pytest.raises(ValueError, match="crop"):
            cli.validate(cfg, tasks=["ir"], crop=crop, model=_NoModel())


def test_segment_and_crop_flags_belong_to_validate(tmp_path, capsys):
    from unirestore_amd import cli
    w = str(tmp_path / "rf.pth")
    torch.save({"not": torch.zeros(1)}, w)
    cfg = os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")
    for argv, word in ((["restore", "--config", cfg, "--segment", f"a=rflw101:{w}"], "--segment belongs to validate"),
                       (["print_config", "--config", cfg, "--crop", "960,1664"], "--crop belongs to validate"),
                       (["validate", "--config", cfg, "--segment", f"a=rflw101:{w}"], "seg"),
                       (["validate", "--config", cfg, "--tasks", "ir,seg", "--segment", f"a=rflw101:{w}"], "labels: map"),
                       (["validate", "--config", cfg, "--tasks", "ir,seg", "--segment", f"a=rflw99:{w}"], "rflw99"),
                       (["validate", "--config", cfg, "--crop", "960x1664"], "--crop")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_crop_box_default_is_unchanged():
    from unirestore_amd import runner
    x = torch.arange(2 * 3 * 600 * 700, dtype=torch.float32).view(2, 3, 600, 700)
    assert runner.crop_tensor(x).shape == (2, 3, 512, 512) and torch.equal(runner.crop_tensor(x), x[..., 44:556, 94:606])
    assert runner.crop_tensor(x, (960, 1664)).shape == (2, 3, 600, 700) and runner.crop_tensor(x[0], (100, 64)).shape == (3, 100, 64)
    assert runner.DEFAULT_CROP == (512, 512)
    for bad in ((0, 5), (5,), "5,5", (5.0, 5)):
        with pytest.raises(ValueError):
            runner.check_crop(bad)


# ---- one segmenter path ---------------------------------------------------------------------------------------------------------

def test_both_networks_share_one_path(monkeypatch):
    import inspect
    from unirestore_amd import build, deeplab, ops, runner, segment
    assert not os.path.exists(os.path.join(ROOT, "unirestore_amd", "csrc", "deeplab.hip"))
    sources = [unit[0] for unit in build.SOURCES]
    assert "deeplab.hip" not in sources and "segment.hip" in sources and "f32_layers.hip" in sources
    # one test-time augmentation under both module names, and both public ops end in it
    assert deeplab.segment is segment.segment and deeplab.scaled_size is segment.scaled_size and deeplab.SCALES is segment.SCALES
    calls = []
    monkeypatch.setattr(ops, "_check_images", lambda *a: None)
    monkeypatch.setattr(ops, "_check_scorer", lambda who, what, obj, cls, makers: calls.append((who, cls, makers)))
    monkeypatch.setattr(segment, "segment", lambda images, weights, size, scales: calls.append((weights, size, tuple(scales))) or "pred")
    x = torch.zeros(1, 3, 64, 64)
    assert ops.segment(x, "w1") == "pred" and ops.deeplab(x, "w2", size=(5, 7), scales=(1,)) == "pred"
    assert calls == [("segment", segment.SegmenterWeights, "segment.load_weights / segment.random_weights"), ("w1", None, (1, 0.8, 0.6)),
                     ("deeplab", deeplab.DeepLabWeights, "deeplab.load_weights / deeplab.random_weights"), ("w2", (5, 7), (1,))]
    for op, word in ((ops.segment, "segment: size"), (ops.deeplab, "deeplab: size")):
        with pytest.raises(ValueError, match=word):
            op(x, "w", size=(0, 4))
    # the driver reads what differs from the weights object
    for cls, name, min_hw in ((segment.SegmenterWeights, "segment", 32), (deeplab.DeepLabWeights, "deeplab", 16)):
        assert (cls.name, cls.min_hw) == (name, min_hw) and all(callable(getattr(cls, m)) for m in ("prep", "logits", "tta_argmax"))
    # the evaluator tells the networks apart only where it loads them
    assert "isinstance(" not in inspect.getsource(runner.LitUniFIE.update_segmentation)
    assert inspect.getsource(runner).count("DeepLabWeights)") == inspect.getsource(runner.LitUniFIE.__init__).count("DeepLabWeights)") == 1


# ---- the yardstick's own constants ----------------------------------------------------------------------------------------------

def test_tolerances_follow_the_measured_fp32_error():
    """Re-measures fp32's own error against fp64 for every recorded constant (segment_reference.py: E32_*) and fails when a
    recorded value is off by more than a factor of two, so every GPU bound (8 x the recorded e32) lies in [4, 16] x what is
    measured here."""
    pairs = [("prep", R.PREP_TOL, max(R.measure_prep(c) for c in R.PREP_CASES)),
             ("upsample", R.UPSAMPLE_TOL, max(R.measure_upsample(c) for c in R.UPSAMPLE_CASES)),
             ("tta", R.TTA_TOL, max(R.measure_tta(k) for k in R.TTA_CASES))]
    for k in R.NET_CASES:
        e1, e3 = R.measure_logits(k)
        pairs += [(f"logits {k}", R.LOGITS_TOL[k], e1), (f"tta logits {k}", R.TTA_LOGITS_TOL[k], e3)]
    assert R.GPU_FACTOR == 8 and R.PREP_TOL == 8 * R.E32_PREP and R.UPSAMPLE_TOL == 8 * R.E32_UPSAMPLE and R.TTA_TOL == 8 * R.E32_TTA
    assert R.LOGITS_TOL == {k: 8 * v for k, v in R.E32_LOGITS.items()} and R.TTA_LOGITS_TOL == {k: 8 * v for k, v in R.E32_TTA_LOGITS.items()}
    assert set(R.E32_LOGITS) == set(R.NET_CASES) == set(R.E32_TTA_LOGITS)
    for name, tol, e32 in pairs:
        print(f"{name}: measured {e32:.2e}, bound {tol:.2e}")
        assert math.isfinite(e32) and e32 > 0, name
        assert 4 * e32 <= tol <= 16 * e32, (name, tol, e32)


def test_network_cases_are_decidable_and_not_vacuous():
    """What the GPU test relies on, checked where it is chosen: finite fp64 logits, at most 0.5 % of the pixels with a top-2 gap
    within twice the absolute bound, and at least five classes among the decidable pixels.  A case that fails here gets another
    seed, never another cap."""
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
        maps, size = R.tta_case(name), R.TTA_CASES[name][3]
        ok = R.decidable(R.tta_average(maps, size), R.TTA_TOL * max(float(m.abs().max()) for m in maps))
        assert float(ok.float().mean()) > 0.99, name


# ---- the launchers' argument checks (host only: every call below is refused before anything is launched) -----------------------

def test_launchers_refuse_bad_arguments():
    from unirestore_amd import capi
    lib, P, bad = capi.lib, 256, capi.UR_E_INVALID        # P: a placeholder pointer, never dereferenced
    calls = [
        ("C must be 3", lambda: lib.ur_seg_prep(P, P, 1, 4, 8, 8, 8, 8, P, P, P, P, None)),
        ("null pointer", lambda: lib.ur_seg_prep(P, None, 1, 3, 8, 8, 8, 8, P, P, P, P, None)),
        ("below 2^31", lambda: lib.ur_seg_prep(P, P, 1 << 12, 3, 512, 512, 8, 8, P, P, P, P, None)),
        ("below 2^31 - 256", lambda: lib.ur_upsample_bilinear_ac_f32(P, P + 256, 2, 8, 8, 256, 2048, 2048, P, P, P, P, None)),
        ("same buffer", lambda: lib.ur_upsample_bilinear_ac_f32(P, P, 1, 2, 2, 4, 4, 4, P, P, P, P, None)),
        (">= 1", lambda: lib.ur_upsample_bilinear_ac_f32(P, P + 256, 1, 0, 2, 4, 4, 4, P, P, P, P, None)),
        ("below 2^31 - 256", lambda: lib.ur_maxpool5_f32(P, P + 256, 4, 1024, 1024, 512, None)),
        ("below 2^31 - 256", lambda: lib.ur_maxpool5_f32(P, P + 256, 8388607, 1, 1, 256, None)),            # N*H*W*C = 2^31 - 256
        ("same buffer", lambda: lib.ur_maxpool5_f32(P, P, 1, 4, 4, 4, None)),
        ("[1, 2^31 - 256)", lambda: lib.ur_add_f32(P, P, P, 1 << 31, None)),
        ("[1, 2^31 - 256)", lambda: lib.ur_add_f32(P, P, P, (1 << 31) - 256, None)),       # the launch limit itself (csrc/launch_size.h)
        ("[1, 2^31 - 256)", lambda: lib.ur_add_f32(P, P, P, 0, None)),
        ("neither a nor b", lambda: lib.ur_add_f32(P, P + 256, P, 4, None)),
        ("neither a nor b", lambda: lib.ur_add_f32(P + 256, P, P, 4, None)),
        ("nmaps", lambda: lib.ur_seg_tta_argmax(P, P, P, 4, 1, 19, 4, 4, 4, 4, 4, 4, 8, 8, P, P, P, P, P, None, None)),
        ("null pointer", lambda: lib.ur_seg_tta_argmax(P, None, None, 2, 1, 19, 4, 4, 4, 4, 0, 0, 8, 8, P, P, P, P, P, None, None)),
        ("[1, 255]", lambda: lib.ur_seg_tta_argmax(P, None, None, 1, 1, 256, 4, 4, 0, 0, 0, 0, 8, 8, P, P, P, P, P, None, None)),
        ("[1, 255]", lambda: lib.ur_seg_tta_argmax(P, None, None, 1, 1, 0, 4, 4, 0, 0, 0, 0, 8, 8, P, P, P, P, P, None, None)),
        ("h and w", lambda: lib.ur_seg_tta_argmax(P, P, None, 2, 1, 19, 4, 4, 0, 4, 0, 0, 8, 8, P, P, P, P, P, None, None)),
        ("below 2^31 - 256", lambda: lib.ur_seg_tta_argmax(P, None, None, 1, 64, 19, 4, 4, 0, 0, 0, 0, 8192, 8192, P, P, P, P, P, None, None)),
        ("below 2^31 - 256", lambda: lib.ur_seg_tta_argmax(P, None, None, 1, 8, 19, 4, 4, 0, 0, 0, 0, 4096, 4096, P, P, P, P, P, P + 256, None)),
        ("below 2^31", lambda: lib.ur_seg_tta_argmax(P, None, None, 1, 8, 19, 4096, 4096, 0, 0, 0, 0, 8, 8, P, P, P, P, P, None, None)),
        ("[1, 255]", lambda: lib.ur_seg_confusion(P, P, 0, 100, 256, 255, P, 1 << 30, P, None)),
        ("[1, 2^31)", lambda: lib.ur_seg_confusion(P, P, 0, 1 << 31, 19, 255, P, 1 << 40, P, None)),
        ("target_i64", lambda: lib.ur_seg_confusion(P, P, 2, 100, 19, 255, P, 1 << 30, P, None)),
        ("workspace too small", lambda: lib.ur_seg_confusion(P, P, 1, 100, 19, 255, P, 19 * 19 * 4 - 1, P, None)),
        ("null pointer", lambda: lib.ur_seg_confusion(P, P, 1, 100, 19, 255, None, 1 << 30, P, None)),
    ]
    for word, call in calls:
        assert call() == bad, word
        assert word in lib.ur_last_error().decode(), (word, lib.ur_last_error().decode())
    assert lib.ur_seg_confusion_ws_bytes(100, 19) == 19 * 19 * 4 and lib.ur_seg_confusion_ws_bytes(4097, 19) == 2 * 19 * 19 * 4
    assert lib.ur_seg_confusion_ws_bytes(1 << 30, 19) == 1024 * 19 * 19 * 4          # the grid is capped; blocks stride over the chunks
    assert lib.ur_seg_confusion_ws_bytes(0, 19) == 0 and lib.ur_seg_confusion_ws_bytes(100, 256) == 0
