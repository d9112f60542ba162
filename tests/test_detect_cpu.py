"""Host-side checks of the detector scorer (unirestore_amd/detect.py): the anchors and the nearest table against restatements of
torchvision's `generate_anchors` and torch's own F.interpolate, the mean average precision against known answers and a brute-force
restatement, the annotation reader, the crop of the boxes, the --detect argument checks, and that the tolerances of the GPU tests
follow the fp32 error measured on the host."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detect_reference as R
from unirestore_amd import detect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- anchors and the nearest table ----------------------------------------------------------------------------------------------

def test_base_anchors_are_generate_anchors():
    assert detect.ANCHOR_SIZES == ((32, 40, 50), (64, 80, 101), (128, 161, 203), (256, 322, 406), (512, 645, 812))
    for level in range(detect.LEVELS):
        assert detect.base_anchors(level).tolist() == R.generate_anchors(level), level
    assert detect.base_anchors(0).tolist() == [[-23, -11, 23, 11], [-28, -14, 28, 14], [-35, -18, 35, 18], [-16, -16, 16, 16], [-20, -20, 20, 20],
                                               [-25, -25, 25, 25], [-11, -23, 11, 23], [-14, -28, 14, 28], [-18, -35, 18, 35]]


def test_sizes_and_strides():
    assert detect.resized_size(40, 56, 64, 96) == (64, 89) and detect.canvas_size(64, 89) == (64, 96)
    assert detect.resized_size(48, 48, 64, 96) == (64, 64) and detect.resized_size(512, 512, 800, 1333) == (800, 800)
    assert detect.resized_size(480, 1280, 800, 1333) == (499, 1333)                           # the long side limits
    assert detect.level_sizes(64, 96) == [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    assert detect.level_sizes(800, 800) == [(100, 100), (50, 50), (25, 25), (13, 13), (7, 7)]
    assert [(64 // h, 96 // w) for h, w in detect.level_sizes(64, 96)] == [(8, 8), (16, 16), (32, 32), (64, 48), (64, 96)]


@pytest.mark.parametrize("n_in,n_out", R.NEAREST_PAIRS)
def test_nearest_table_is_torchs(n_in, n_out):
    want = F.interpolate(torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in), size=(1, n_out), mode="nearest").view(-1)
    assert detect.nearest_table(n_in, n_out).tolist() == want.int().tolist()
    with pytest.raises(ValueError):
        detect.nearest_table(0, 4)


def test_logit_threshold():
    lt = detect.logit_threshold(0.05)
    assert lt == float(np.float32(np.log(0.05 / 0.95))) and detect.logit_threshold(0.0) == float("-inf") and detect.logit_threshold(1.0) == float("inf")


# ---- mAP ------------------------------------------------------------------------------------------------------------------------

def _det(boxes, scores, labels):
    return dict(boxes=torch.tensor(boxes, dtype=torch.float32).view(-1, 4), scores=torch.tensor(scores, dtype=torch.float32), labels=torch.tensor(labels, dtype=torch.int64))


def _gt(boxes, labels):
    return dict(boxes=torch.tensor(boxes, dtype=torch.float32).view(-1, 4), labels=torch.tensor(labels, dtype=torch.int64))


A, B, FAR = [0, 0, 10, 10], [20, 20, 30, 30], [50, 50, 60, 60]


def _map(dets, tgts, **kw):
    m = detect.MeanAP(**kw)
    m.update(dets, tgts)
    return m.compute()


def test_map_known_answers():
    # KAT 1: TP 0.9, FP 0.8, TP 0.7 on two ground truths: precision 1 up to recall 0.5 (51 points), 2/3 beyond (50 points)
    res = _map([_det([A, FAR, B], [0.9, 0.8, 0.7], [1, 1, 1])], [_gt([A, B], [1, 1])])
    assert abs(res["map"] - (51 + 50 * 2 / 3) / 101) < 1e-12 and list(res["per_class"]) == [1]
    # a class without ground truth is left out of the mean
    res = _map([_det([A, FAR, B, A], [0.9, 0.8, 0.7, 0.95], [1, 1, 1, 7])], [_gt([A, B], [1, 1])])
    assert abs(res["map"] - (51 + 50 * 2 / 3) / 101) < 1e-12 and list(res["per_class"]) == [1]
    # two detections on one ground truth: the second is an FP -> precision 1 at every recall (the FP lies behind recall 1)
    assert abs(_map([_det([A, A], [0.9, 0.8], [1, 1])], [_gt([A], [1])])["map"] - 1.0) < 1e-12
    res = _map([_det([A, A, B], [0.9, 0.8, 0.7], [1, 1, 1])], [_gt([A, B], [1, 1])])         # TP FP TP again
    assert abs(res["map"] - (51 + 50 * 2 / 3) / 101) < 1e-12
    # no ground truth at all
    assert _map([_det([A], [0.9], [1])], [_gt([], [])]) == {"map": -1.0, "per_class": {}}
    assert detect.MeanAP().compute()["map"] == -1.0
    # a class with ground truth and no detection scores 0
    assert _map([_det([], [], [])], [_gt([A], [3])]) == {"map": 0.0, "per_class": {3: 0.0}}


def test_map_equal_ious_go_to_the_later_ground_truth():
    # the detection overlaps both ground truths equally (IoU 0.5 each): it takes the second one; the next detection, which fits
    # only the second, then finds it taken and is an FP.  Were the first to win, both would be TPs.
    d, g0, g1 = [0, 0, 10, 10], [0, 0, 10, 5], [0, 5, 10, 10]
    assert detect.box_iou_np([d], [g0, g1]).tolist() == [[0.5, 0.5]]
    m = detect.MeanAP(0.5)
    m.update([_det([d, g1], [0.9, 0.8], [1, 1])], [_gt([g0, g1], [1, 1])])
    assert np.concatenate(m.tps[1]).tolist() == [True, False]
    m = detect.MeanAP(0.5)
    m.update([_det([d, g0], [0.9, 0.8], [1, 1])], [_gt([g0, g1], [1, 1])])
    assert np.concatenate(m.tps[1]).tolist() == [True, True]


def test_map_max_dets_cut():
    dets = [_det([FAR, FAR, A], [0.9, 0.8, 0.7], [1, 1, 1])]
    assert _map(dets, [_gt([A], [1])], max_dets=2)["map"] == 0.0                # the TP is the third detection of its class
    assert abs(_map(dets, [_gt([A], [1])], max_dets=3)["map"] - 1 / 3) < 1e-12
    with pytest.raises(ValueError):
        detect.MeanAP(0.0)
    with pytest.raises(ValueError):
        detect.MeanAP().update([_det([A], [0.9], [1])], [])


def test_map_merge_and_brute_force():
    dets, tgts = R.random_scene(torch.Generator().manual_seed(11))
    assert len(dets) == 50
    whole = detect.MeanAP(0.5)
    whole.update(dets, tgts)
    a, b = detect.MeanAP(0.5), detect.MeanAP(0.5)
    a.update(dets[:23], tgts[:23])
    b.update(dets[23:], tgts[23:])
    merged = a.merge(b).compute()
    res = whole.compute()
    assert merged == res
    want = R.mean_ap(dets, tgts, 0.5)
    assert sorted(res["per_class"]) == sorted(want["per_class"]) and len(want["per_class"]) >= 3
    assert abs(res["map"] - want["map"]) <= 1e-12 and 0.05 < want["map"] < 0.95
    for c, v in want["per_class"].items():
        assert abs(res["per_class"][c] - v) <= 1e-12
    for thr in (0.3, 0.75):
        m = detect.MeanAP(thr)
        m.update(dets, tgts)
        assert abs(m.compute()["map"] - R.mean_ap(dets, tgts, thr)["map"]) <= 1e-12
    from unirestore_amd import ops
    assert ops.mean_ap(dets, tgts, 0.5) == res["map"]
    with pytest.raises(ValueError):
        a.merge(detect.MeanAP(0.75))


def test_rank_states_merge_to_the_single_rank_result():
    """What `validate` does with the states it gathers from the ranks: three ranks' shares of the images, each split over two
    corruptions, give the totals, the counts and the per-corruption states one rank would hold."""
    from unirestore_amd import cli
    dets, tgts = R.random_scene(torch.Generator().manual_seed(5), n_img=30)

    def state(lo, hi):
        m = detect.MeanAP(0.5)
        m.update(dets[lo:hi], tgts[lo:hi])
        return m
    everyone = []
    for q, (lo, mid, hi) in enumerate([(0, 4, 10), (10, 17, 20), (20, 21, 30)]):
        everyone.append(({"det/rn": state(lo, hi), "det_input/rn": state(lo, mid)}, [q, 1],
                         {"fog/3": {"det/rn": state(lo, mid)}, "snow/1": {"det/rn": state(mid, hi)}}))
    totals, bad, by = cli.merge_detection_states(everyone, 0.5)
    assert bad == [3, 3] and sorted(totals) == ["det/rn", "det_input/rn"] and sorted(by) == ["fog/3", "snow/1"]
    assert totals["det/rn"].compute() == state(0, 30).compute() and 0.0 < totals["det/rn"].compute()["map"] < 1.0
    fog = [i for lo, mid, _ in [(0, 4, 10), (10, 17, 20), (20, 21, 30)] for i in range(lo, mid)]
    one = detect.MeanAP(0.5)
    one.update([dets[i] for i in fog], [tgts[i] for i in fog])
    assert by["fog/3"]["det/rn"].compute() == one.compute() == totals["det_input/rn"].compute()
    assert everyone[0][0]["det/rn"].compute() == state(0, 10).compute()          # the ranks' own states are not changed


# ---- data -----------------------------------------------------------------------------------------------------------------------

def write_pairs(folder, n=3, hw=(40, 48), seed=0, names=("person", "car", "bus")):
    """n random PNGs with annotation JSONs in the reference's shape and an `lq hq annotation` list -> (list file, targets)."""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    targets = []
    for i in range(n):
        Image.fromarray((torch.rand(hw[0], hw[1], 3, generator=g) * 255).byte().numpy()).save(os.path.join(folder, f"im{i}.png"))
        ann = {"filename": f"im{i}.png", "size": {"width": hw[1], "height": hw[0]}}
        boxes = []
        for j in range(2 + i % 2):
            x0, y0 = int(torch.randint(0, hw[1] // 2, (1,), generator=g)), int(torch.randint(0, hw[0] // 2, (1,), generator=g))
            box = [x0, y0, x0 + 6 + 3 * j, y0 + 5 + 2 * j]
            ann[f"object_{j}"] = {"name": names[(i + j) % len(names)], "bndbox": dict(zip(("xmin", "ymin", "xmax", "ymax"), box))}
            boxes.append((box, names[(i + j) % len(names)]))
        ann["object_flat"] = {"name": "person", "bndbox": {"xmin": 5, "ymin": 5, "xmax": 5, "ymax": 9}}          # degenerate: skipped
        with open(os.path.join(folder, f"ann{i}.json"), "w") as f:
            json.dump(ann, f)
        targets.append(boxes)
    lst = os.path.join(folder, "list.txt")
    with open(lst, "w") as f:
        f.write("# lq hq annotation\n" + "".join(f"im{i}.png im{i}.png ann{i}.json\n" for i in range(n)))
    return lst, targets


def test_annotation_reader_and_class_tables(tmp_path):
    from unirestore_amd import data
    assert data.RTTS_COCO_IDS == {"person": 1, "bicycle": 2, "car": 3, "motorbike": 4, "bus": 6}
    assert len(data.COCO_NAMES) == 91 and data.COCO_IDS["person"] == 1 and data.COCO_IDS["motorcycle"] == 4 and data.COCO_IDS["bus"] == 6
    assert data.COCO_IDS["toothbrush"] == 90 and data.COCO_IDS["traffic light"] == 10 and data.COCO_NAMES[12] == "N/A"
    lst, targets = write_pairs(str(tmp_path / "d"))
    batches = list(data.ImageListFiles(lst, batch_size=2, labels="boxes").batches())
    gts = [t for b in batches for t in b[2]]
    assert [len(b[2]) for b in batches] == [2, 1] and all(isinstance(b[2], list) for b in batches)
    for gt, want in zip(gts, targets):
        assert gt["boxes"].dtype == torch.float32 and gt["labels"].dtype == torch.int64 and tuple(gt["boxes"].shape) == (len(want), 4)
        assert gt["boxes"].tolist() == [[float(v) for v in b] for b, _ in want]             # the degenerate box is gone
        assert gt["labels"].tolist() == [data.RTTS_COCO_IDS[nm] for _, nm in want]
    plain = list(data.ImageListFiles(lst, batch_size=2).batches())
    assert all(torch.equal(a[0], b[0]) and a[2] is None for a, b in zip(plain, batches))
    # the COCO table: `motorbike` is no COCO name
    lst2, _ = write_pairs(str(tmp_path / "coco"), names=("person", "motorcycle", "bus"))
    gt = list(data.ImageListFiles(lst2, batch_size=8, labels="boxes", box_classes="coco").batches())[0][2]
    assert gt[0]["labels"].tolist() == [1, 4] and gt[1]["labels"].tolist() == [4, 6, 1]
    with pytest.raises(ValueError, match=r"list.txt:2.*motorcycle"):
        list(data.ImageListFiles(lst2, labels="boxes").batches())
    # an image without a valid box is an error, as in the reference; so are a missing file and a folder source
    with open(os.path.join(str(tmp_path / "d"), "ann1.json"), "w") as f:
        json.dump({"object_0": {"name": "car", "bndbox": {"xmin": 4, "ymin": 9, "xmax": 8, "ymax": 9}}}, f)
    with pytest.raises(ValueError, match=r"list.txt:3.*no valid box"):
        list(data.ImageListFiles(lst, labels="boxes").batches())
    with pytest.raises(ValueError, match="box_classes"):
        data.ImageListFiles(lst, labels="boxes", box_classes="voc")
    for cls in ("CorruptedImageFiles", "DistortedImageFiles", "JpegImageFiles"):
        ds = getattr(data, cls)(lst2, labels="boxes", box_classes="coco")
        assert [os.path.basename(p) for p, _ in ds.labels] == ["ann0.json", "ann1.json", "ann2.json"]
        with pytest.raises(ValueError, match="folder"):
            getattr(data, cls)(str(tmp_path / "coco"), labels="boxes")
    for bad in ("box", "maps", 2):
        with pytest.raises(ValueError, match=r"labels must be false, true .*\"map\" .* or \"boxes\" .*, got"):
            data.ImageListFiles(lst, labels=bad)
    os.remove(os.path.join(str(tmp_path / "coco"), "ann2.json"))
    with pytest.raises(ValueError, match=r"list.txt:4.*ann2.json"):
        list(data.ImageListFiles(lst2, batch_size=1, labels="boxes", box_classes="coco").batches())
    with open(os.path.join(str(tmp_path / "coco"), "ann0.json"), "w") as f:        # a coordinate that is no number: file and line named
        json.dump({"object_0": {"name": "bus", "bndbox": {"xmin": "left", "ymin": 1, "xmax": 8, "ymax": 9}}}, f)
    with pytest.raises(ValueError, match=r"list.txt:2.*ann0.json.*no number"):
        list(data.ImageListFiles(lst2, batch_size=1, labels="boxes", box_classes="coco").batches())


def test_crop_shifts_clips_and_drops():
    from unirestore_amd import data
    from unirestore_amd.runner import crop_box
    t, b, l, r = crop_box(100, 80, 40, 60)
    assert (t, b, l, r) == (30, 70, 10, 70)
    gt = [dict(boxes=torch.tensor([[20., 40., 50., 60.], [0., 0., 15., 90.], [0., 0., 10., 30.], [60., 65., 79., 99.], [70., 10., 75., 50.]]),
               labels=torch.tensor([1, 2, 3, 4, 6]))]
    out = data.crop_boxes(gt, t, l, b - t, r - l)[0]
    assert out["boxes"].tolist() == [[10., 10., 40., 30.], [0., 0., 5., 40.], [50., 35., 60., 40.]]
    assert out["labels"].tolist() == [1, 2, 4]                 # box 3 lies left of / above the crop, box 5 right of it
    assert gt[0]["boxes"][0].tolist() == [20., 40., 50., 60.]   # the input is not changed
    assert data.crop_boxes([dict(boxes=torch.zeros(0, 4), labels=torch.zeros(0, dtype=torch.int64))], 0, 0, 5, 5)[0]["boxes"].shape == (0, 4)


# ---- the command line -------------------------------------------------------------------------------------------------------------

def config(tmp_path, labels="boxes", det_task=True, data_class="ImageListFiles", n=2):
    from unirestore_amd import cli
    lst, _ = write_pairs(str(tmp_path / f"c_{labels}_{data_class}"), n=n, hw=(64, 64))
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))
    key = "list_file" if data_class == "ImageListFiles" else "source"
    cfg["data"] = dict(class_path=f"unirestore_amd.data.{data_class}", init_args={key: lst, "batch_size": 2, **({"labels": labels} if labels else {})})
    if det_task:
        cfg["model"]["init_args"]["model_kwargs"]["tedit"]["task"] = ["ir", "cls", "seg", "det"]
    return cfg


class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_detect_argument_errors_come_before_the_model(tmp_path):
    from unirestore_amd import cli
    w = str(tmp_path / "rn.pth")
    torch.save({"not": torch.zeros(1)}, w)                # the checks below never open it
    arch = "retinanet_resnet50_fpn_v2"
    assert cli.check_detect_arg(f"a={arch}:{w},b={arch}:{w}") == {"a": (arch, w), "b": (arch, w)}
    assert cli.check_detect_arg({"a": (arch, w)}, 0.3, 0.75) == {"a": (arch, w)}
    cfg = config(tmp_path)
    for arg, tasks, c, kw, word in [
        (f"a=fasterrcnn_resnet50_fpn:{w}", ["ir", "det"], cfg, {}, "fasterrcnn_resnet50_fpn"),         # an unknown arch
        (f"a={arch}:{w}.missing", ["ir", "det"], cfg, {}, "no such file"),
        (f"a={arch}:{w},a={arch}:{w}", ["ir", "det"], cfg, {}, "twice"),
        (f"{arch}:{w}", ["ir", "det"], cfg, {}, "NAME=ARCH"),
        (f"a={arch}:{w}", None, cfg, {}, "det"),                                                      # no --tasks
        (f"a={arch}:{w}", ["ir", "seg"], cfg, {}, "'det'"),                                           # --tasks without det
        (f"a={arch}:{w}", ["det"], cfg, {}, "'ir'"),                                                  # ir stays required
        (f"a={arch}:{w}", ["ir", "det"], config(tmp_path, det_task=False), {}, "tedit.task"),         # the model has no det prompt
        (f"a={arch}:{w}", ["ir", "det"], config(tmp_path, labels=None), {}, "labels: boxes"),
        (f"a={arch}:{w}", ["ir", "det"], config(tmp_path, labels="map"), {}, "labels: boxes"),
        (f"a={arch}:{w}", ["ir", "det"], cfg, dict(det_score=1.0), "--det-score"),
        (f"a={arch}:{w}", ["ir", "det"], cfg, dict(det_iou=0.0), "--det-iou"),
    ]:
        with pytest.raises(ValueError) as e:
            cli.validate(c, tasks=tasks, detect=arg, model=_NoModel(), **kw)
        assert word in str(e.value), (arg, tasks, str(e.value))


def test_detect_flags_belong_to_validate(tmp_path, capsys):
    from unirestore_amd import cli
    w = str(tmp_path / "rn.pth")
    torch.save({"not": torch.zeros(1)}, w)
    cfg = os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")
    arch = "retinanet_resnet50_fpn_v2"
    for argv, word in ((["restore", "--config", cfg, "--detect", f"a={arch}:{w}"], "--detect belongs to validate"),
                       (["print_config", "--config", cfg, "--det-iou", "0.5"], "--det-iou belongs to validate"),
                       (["validate", "--config", cfg, "--det-score", "0.3"], "belong to --detect"),
                       (["validate", "--config", cfg, "--detect", f"a={arch}:{w}"], "det"),
                       (["validate", "--config", cfg, "--tasks", "ir,det", "--detect", f"a={arch}:{w}"], "tedit.task"),
                       (["validate", "--config", cfg, "--tasks", "ir,det", "--detect", f"a=retinanet:{w}"], "retinanet")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


# ---- weights ----------------------------------------------------------------------------------------------------------------------

def test_state_dict_layout_and_checks(tmp_path):
    sd = detect.random_state_dict(R.ARCH, 1, num_classes=5)
    assert sd["backbone.fpn.extra_blocks.p6.weight"].shape == (256, 2048, 3, 3) and sd["backbone.fpn.inner_blocks.0.0.weight"].shape == (256, 512, 1, 1)
    assert sd["head.classification_head.cls_logits.weight"].shape == (45, 256, 3, 3) and sd["head.regression_head.bbox_reg.bias"].shape == (36,)
    assert "head.classification_head.conv.3.0.bias" not in sd and sd["head.regression_head.conv.0.1.weight"].shape == (256,)
    assert not any(k.endswith("num_batches_tracked") for k in sd)
    assert len(sd) == 53 * 5 + 8 * 2 + 2 * (4 * 3 + 2)
    lit = {"state_dict": {f"model.detector.{k}": v for k, v in sd.items()}, "epoch": 3}
    path = str(tmp_path / "lit.ckpt")
    torch.save(lit, path)
    got = detect.read_state_dict(path)
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    for key, word in (("backbone.fpn.layer_blocks.1.0.bias", "layer_blocks.1.0.bias"), ("head.regression_head.conv.2.1.weight", "conv.2.1.weight")):
        bad = dict(sd)
        del bad[key]
        with pytest.raises(ValueError, match=word):
            detect.DetectorWeights(R.ARCH, bad, dev="cpu")
    bad = dict(sd)
    bad["head.classification_head.cls_logits.weight"] = torch.zeros(44, 256, 3, 3)
    with pytest.raises(ValueError, match="cls_logits"):
        detect.DetectorWeights(R.ARCH, bad, dev="cpu")
    with pytest.raises(ValueError, match="arch"):
        detect.load_weights("retinanet_resnet50_fpn", path)
    with pytest.raises(ValueError, match="min_size"):
        detect.DetectorWeights(R.ARCH, sd, min_size=900, max_size=800, dev="cpu")


def test_tolerances_follow_the_measured_fp32_error():
    """The tolerances are 4 x the constants recorded in detect_reference.py, and the GroupNorm constant is what torch's fp32
    F.group_norm shows here too - within a factor of four either way, since its summation order is the CPU kernel's at hand, so
    the bound stays between 1 x and 16 x what any machine measures.  (The network part is re-measured by running the module.)"""
    e = 0.0
    for shape, groups in R.GN_CASES:
        x, gm, bt = R.gn_case(shape, groups)
        for relu in (False, True):
            e = max(e, float((R.group_norm(x, gm, bt, groups, relu, torch.float32).double() - R.group_norm(x, gm, bt, groups, relu)).abs().max()))
    assert R.E32_GN / 4 <= e <= R.E32_GN * 4, (e, R.E32_GN)
    assert R.GN_TOL == 4 * R.E32_GN and R.LOGITS_TOL == 4 * R.E32_LOGITS and R.REGS_TOL == 4 * R.E32_REGS


def test_reference_pipeline_is_decidable_and_cut():
    """The fp64 reference of the end-to-end GPU test, on the host: at topk_candidates = 50 a level is cut and a level is not, and
    at most 2 % of its detections sit within 1e-5 of the score threshold or within 1e-4 of the NMS threshold."""
    sd = detect.random_state_dict(R.ARCH, R.NET_SEED, 5)
    x = R.images(R.NET_IMAGES[0])
    logits, regs, geo = R.head_outputs(x, sd, R.NET_MIN, R.NET_MAX)
    lt64 = float(np.log(0.05 / 0.95))
    for n in range(2):
        res = R.postprocess(logits, regs, geo, x.shape[2:], n, 0.05, 50, 0.5, 300, lt=lt64)
        assert max(res["counts"]) == 50 and 0 < min(c for c in res["counts"] if c) < 50 and 0 in res["counts"]
        near = sum(abs(res["scores"][i] - 0.05) < 1e-5 for i in res["keep"])
        assert len(res["keep"]) >= 20 and near <= 0.02 * len(res["keep"])
        assert len(res["near"]) <= 0.02 * len(res["keep"])
