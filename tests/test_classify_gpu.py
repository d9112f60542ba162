"""Classifier scoring on the GPU (ops.classify / ops.top1, unirestore_amd/classify.py, csrc/classify.hip): every launcher
of its own against the fp64 restatement element by element (the shared fp32 layers: test_f32net_gpu.py), whole networks on tiny maps, `forward` end to end, batch-place
independence, bit-reproducibility (eager and hipGraph replay), argument checks, and the caller path (LitUniFIE, cli.validate).
Every bound is 8 x fp32's own measured error (classify_reference.py: E32_* / *_TOL, kept honest by
test_classify_cpu.py::test_tolerances_follow_the_measured_fp32_error); the weights are seeded stand-ins - no trained weights exist
where this runs, so nothing here says anything about published accuracies."""
import os

import numpy as np
import pytest
import torch

import classify_reference as R
from tiny_cfg import TINY, model_kwargs, randomise_

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_W = {}


def _weights(arch="resnet50", seed=1, classes=1000):
    """The stand-in weights of a case on the device, from the SAME state dict the fp64 restatement reads."""
    from unirestore_amd import classify
    key = (arch, seed, classes)
    if key not in _W:
        _W[key] = classify.ClassifierWeights(arch, R.state_dict(arch, seed, classes))
    return _W[key]


# ---- the launchers ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.PREP_CASES, ids=["x".join(map(str, s)) for s in R.PREP_CASES])
def test_preprocess_matches_fp64_and_writes_nhwc(shape):
    from unirestore_amd import classify
    x = R.images(shape, 3)
    y = classify.preprocess(x.cuda()).cpu()
    assert tuple(y.shape) == (shape[0], 224, 224, 3) and y.dtype == torch.float32
    err = float((R.nchw(y).double() - R.preprocess(x)).abs().max())
    print(f"preprocess {shape}: max |err| {err:.2e} (bound {R.PREP_TOL:.2e}; torch's fp32 interpolate {R.TORCH32_PREP[shape]:.2e})")
    assert err <= R.PREP_TOL
    assert err <= R.TORCH32_PREP[shape]                       # no further from fp64 than torch's own fp32 path


@pytest.mark.parametrize("classes", [1000, 200])
def test_top1_and_counts(classes):
    from unirestore_amd import ops
    g = torch.Generator().manual_seed(classes)
    n = 37
    logits = torch.randn(n, classes, generator=g)
    logits[0] = -logits[0].abs() - 1.0                       # all negative
    logits[1, [5, 17, 900 % classes]] = 9.0                  # a three-way tie: the lowest index wins
    logits[2, :] = 0.25                                      # everything ties: class 0
    logits[3, classes - 1] = 50.0                            # the last class (beyond the last full stride of 64 lanes)
    logits[4, 63], logits[4, 64] = 40.0, 40.0                # a tie across two lanes' strides
    want = logits.argmax(dim=1)
    assert want[1] == 5 and want[2] == 0 and want[3] == classes - 1 and want[4] == 63
    labels = want.clone()
    labels[::3] = (labels[::3] + 1) % classes                # a third of the predictions is wrong
    labels[5] = int(want[6])                                 # a class that is a target twice
    pred, tp, targets, predicted = ops.top1(logits.cuda(), labels.cuda())
    assert pred.dtype == torch.int64 and all(t.dtype == torch.int64 and t.shape == (classes,) and t.is_cuda for t in (tp, targets, predicted))
    assert torch.equal(pred.cpu(), want)
    for got, ref in zip((tp, targets, predicted), R.counts(want.numpy(), labels.numpy(), classes)):
        assert np.array_equal(got.cpu().numpy(), ref)
    assert 0 < int(tp.sum()) < n and int(targets.sum()) == n and int(predicted.sum()) == n
    pred2, *_ = ops.top1(logits.cuda(), labels.int())        # host labels, int32
    assert torch.equal(pred2, pred)
    for bad in (-1, classes):
        wrong = labels.clone()
        wrong[7] = bad
        with pytest.raises(ValueError, match=str(bad)):
            ops.top1(logits.cuda(), wrong.cuda())


# ---- the whole network --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.NET_CASES))
def test_logits_match_fp64_and_decide_as_fp64_does(name):
    from unirestore_amd import classify
    arch, classes, wseed, _iseed, n, _h, _w = R.NET_CASES[name]
    want = R.net_reference(name)
    scale = float(want.abs().max())
    bound = R.LOGITS_TOL[name] * scale
    gaps = R.top2_gap(want)
    assert bool(torch.isfinite(want).all()) and float(gaps.min()) > 2 * bound          # every image is decidable: none is left out
    if name == "resnet50_4x64x64":
        assert len(set(want.argmax(dim=1).tolist())) >= 2
    got = classify.logits(R.nhwc(R.net_input(name)).cuda(), _weights(arch, wseed, classes))
    assert tuple(got.shape) == (n, classes) and got.dtype == torch.float32
    err = float((got.cpu().double() - want).abs().max())
    print(f"{name}: max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.1f} (bound {R.LOGITS_TOL[name]:.2e}); "
          f"classes {want.argmax(dim=1).tolist()}, smallest top-2 gap {float(gaps.min()):.3f}")
    assert err <= bound
    assert got.argmax(dim=1).cpu().tolist() == want.argmax(dim=1).tolist()


def test_forward_end_to_end_matches_fp64():
    from unirestore_amd import ops
    arch, classes, wseed = R.FORWARD_CASE[:3]
    want = R.forward_reference()
    scale = float(want.abs().max())
    assert float(R.top2_gap(want).min()) > 2 * R.FORWARD_TOL * scale
    got = ops.classify(R.forward_images().cuda(), _weights(arch, wseed, classes))
    err = float((got.cpu().double() - want).abs().max())
    print(f"forward {R.FORWARD_CASE[4]}: max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.1f} (bound {R.FORWARD_TOL:.2e})")
    assert tuple(got.shape) == (3, classes) and err <= R.FORWARD_TOL * scale
    assert got.argmax(dim=1).cpu().tolist() == want.argmax(dim=1).tolist()


def test_logits_do_not_depend_on_the_place_in_the_batch():
    from unirestore_amd import ops
    w = _weights()
    x = R.varied_images(4, 75, 101, 12).cuda()
    whole = ops.classify(x, w)
    for i in range(4):
        assert torch.equal(ops.classify(x[i:i + 1].contiguous(), w)[0], whole[i])
        for slot in range(4):
            order = [j for j in range(4) if j != i]
            order.insert(slot, i)
            assert torch.equal(ops.classify(x[order].contiguous(), w)[slot], whole[i])


def test_deterministic_eager_and_graph_replay():
    from unirestore_amd import ops
    w = _weights()
    x = R.varied_images(3, 75, 101, 9).cuda()
    labels = torch.tensor([1, 824, 2]).cuda()
    a = ops.classify(x, w)
    b = ops.classify(x, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.classify(x, w)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = ops.classify(x, w)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a).all())
    assert all(torch.equal(p, q) for p, q in zip(ops.top1(a, labels), ops.top1(c, labels)))


def test_ops_reject_bad_inputs():
    from unirestore_amd import ops
    w = _weights("resnet18", 7, 200)
    x = R.images((2, 3, 40, 44), 1).cuda()
    for bad in (x.double(), x.half(), x.cpu(), x[0], x.transpose(2, 3), x[:, :1].contiguous(), x[:, :, :0].contiguous(), x[:0].contiguous()):
        with pytest.raises(ValueError):
            ops.classify(bad, w)
    for bad_w in (None, {"arch": "resnet18"}):
        with pytest.raises(ValueError):
            ops.classify(x, bad_w)
    logits = ops.classify(x[:, :, :1, :1].contiguous(), w)                    # a 1 x 1 image is legal
    assert logits.shape == (2, 200)
    labels = torch.tensor([3, 4]).cuda()
    for bad_l, bad_y in ((logits.double(), labels), (logits.cpu(), labels), (logits[0], labels[:1]), (logits.t(), labels), (logits, labels[:1]),
                         (logits, labels.float()), (logits, None), (logits, torch.tensor([3, 200]).cuda()), (logits, torch.tensor([-1, 0]))):
        with pytest.raises(ValueError):
            ops.top1(bad_l, bad_y)
    assert ops.top1(logits, labels)[2].sum() == 2
    # the launchers' size limits, at the first refused count (placeholder pointers: a refusal comes before any HIP call)
    from unirestore_amd import capi
    lib, P, L = capi.lib, 256, (1 << 31) - 256                                # L: the 1-D launch limit of csrc/launch_size.h
    for call in (lambda: lib.ur_maxpool2d_pad_f32(P, P + 256, L // 4, 1, 1, 4, None), lambda: lib.ur_avgpool_f32(P, P + 256, L // 4, 1, 4, None),
                 lambda: lib.ur_top1_counts(P, P, 1, L, P, P, None), lambda: lib.ur_top1_counts(P, P, L // 4, 4, P, P, None),
                 lambda: lib.ur_classify_preprocess(P, P + 256, P + 512, 10632, 3, 257, 262, P, P, P, 4, P, P, P, 4, None)):
        assert call() == capi.UR_E_INVALID and "below 2^31 - 256" in lib.ur_last_error().decode(), lib.ur_last_error().decode()


# ---- the caller ---------------------------------------------------------------------------------------------------------------

def _tiny_model():
    import unirestore_amd.modules as M
    from oracle.model import DiffUIE as ODiffUIE
    torch.manual_seed(0)
    o = randomise_(ODiffUIE(**model_kwargs(2), **TINY).eval(), 0)
    p = M.DiffUIE(**model_kwargs(2), **TINY).eval()
    p.load_state_dict(o.state_dict())
    return p


def _counts(images, labels, w):
    from unirestore_amd import ops
    pred, tp, targets, predicted = ops.top1(ops.classify(images.contiguous(), w), labels)
    return pred, torch.stack([tp, targets, predicted])


def test_litunifie_accumulates_classifier_counts_and_leaves_the_rest_alone():
    from unirestore_amd import classify, ops, runner
    model = _tiny_model()
    w = _weights("resnet18", 7, 200)
    tasks = ["ir", "cls"]
    batches = []
    for b in range(2):
        hq = R.varied_images(3, 96, 80, 100 + b).cuda()
        lq = (0.6 * hq + 0.3 * R.varied_images(3, 96, 80, 200 + b).cuda()).clamp(0, 1)
        batches.append((lq, hq))

    def run(classifiers, labels):
        lit = runner.LitUniFIE(model_kwargs(2), model=model, classifiers=classifiers)
        outs = []
        for b, (lq, hq) in enumerate(batches):
            torch.manual_seed(40 + b)                # the forward's noise draws: the same for every instance
            outs.append(lit.validation_step((lq, hq, labels[b], ["a", "b", "c"], "ir"), tasks=tasks)[-1])
        return lit, lit.metrics(), outs
    lit0, m0, o0 = run(None, [None, None])
    assert set(m0) == {"val_lq/psnr", "val_lq/ssim", "images"} and set(lit0.totals) == {"psnr", "ssim", "images"}      # today's keys
    # labels from what the classifier says about the restored images: right for some, wrong for others, on both sides
    labels = []
    for (lq, _hq), o in zip(batches, o0):
        pred = ops.classify(o["cls"].contiguous(), w).argmax(dim=1)
        pred[0] = (pred[0] + 1) % 200
        labels.append(pred.cpu())
    lit1, m1, o1 = run({"r18": w}, labels)
    for a, b in zip(o0, o1):
        assert torch.equal(a["ir"], b["ir"]) and torch.equal(a["cls"], b["cls"])          # restoring does not depend on the scoring
    assert m0["val_lq/psnr"] == m1["val_lq/psnr"] and m0["val_lq/ssim"] == m1["val_lq/ssim"] and m1["images"] == 6
    new = {"val_lq/r18", "val_lq/r18_top1", "val_input/r18", "val_input/r18_top1"}
    assert set(m1) == set(m0) | new and set(lit1.totals) == set(lit0.totals) | {"cls/r18", "cls_input/r18"}
    for key, side in (("cls/r18", [o["cls"] for o in o1]), ("cls_input/r18", [lq for lq, _ in batches])):
        tot = lit1.totals[key]
        assert tot.is_cuda and tot.dtype == torch.int64 and tuple(tot.shape) == (3, 200)
        want = sum(_counts(runner.crop_tensor(img), lab, w)[1] for img, lab in zip(side, labels))
        assert torch.equal(tot, want) and int(tot[1].sum()) == 6
        macro, micro = classify.accuracy(*want)
        prefix = "val_lq" if key == "cls/r18" else "val_input"
        assert m1[f"{prefix}/r18"] == macro and m1[f"{prefix}/r18_top1"] == micro
        assert (macro, micro) == pytest.approx(R.accuracy(*want.cpu().tolist()), abs=1e-15)
    assert m1["val_lq/r18_top1"] == pytest.approx(4 / 6) and 0 < m1["val_lq/r18"] < 1      # neither 0 nor 1
    # the classifiers need cls among the tasks and labels in the batch
    lit = runner.LitUniFIE(model_kwargs(2), model=model, classifiers={"r18": w})
    with pytest.raises(ValueError, match="cls"):
        lit.validation_step((batches[0][0], batches[0][1], labels[0], ["a", "b", "c"], "ir"), tasks=["ir"])
    with pytest.raises(ValueError, match="labels: true"):
        lit.update_classification(o1[0]["cls"], batches[0][0], None)


def _labelled_files(tmp_path, n=4, hw=(64, 64)):
    from PIL import Image
    imgs = (R.varied_images(n, hw[0], hw[1], 31) * 255).round().byte().permute(0, 2, 3, 1).numpy()
    lines = []
    for i in range(n):
        Image.fromarray(imgs[i]).save(str(tmp_path / f"im{i}.png"))
        lines.append(f"im{i}.png im{i}.png {i % 3}\n")
    lst = tmp_path / "list.txt"
    lst.write_text("".join(lines))
    return str(lst)


def _tiny_cli_cfg(data):
    return dict(seed_everything=3, trainer=dict(accelerator="gpu", devices=1, precision="bf16-mixed"),
                model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=model_kwargs(2))), data=data)


def test_cli_validate_classify(tmp_path):
    from unirestore_amd import classify, cli
    lst = _labelled_files(tmp_path)
    wpath = str(tmp_path / "r18.pth")
    torch.save(classify.random_state_dict("resnet18", 7, 3), wpath)
    model = _tiny_model()
    keys = {"val_lq/r18", "val_lq/r18_top1", "val_input/r18", "val_input/r18_top1"}
    cfg = _tiny_cli_cfg(dict(class_path="unirestore_amd.data.ImageListFiles", init_args=dict(list_file=lst, batch_size=2, labels=True)))
    r0 = cli.validate(cfg, tasks=["ir", "cls"], model=model)
    r1 = cli.validate(cfg, tasks=["ir", "cls"], model=model, classify=f"r18=resnet18:{wpath}")
    print({k: r1[k] for k in sorted(keys)})
    assert set(r1) == set(r0) | keys and r1["images"] == r0["images"] == 4
    assert r1["val_lq/psnr"] == r0["val_lq/psnr"] and r1["val_lq/ssim"] == r0["val_lq/ssim"]
    assert all(0.0 <= r1[k] <= 1.0 for k in keys)
    # clean files corrupted on the GPU: two corruptions, every entry of the table carries the new keys
    cfg = _tiny_cli_cfg(dict(class_path="unirestore_amd.data.CorruptedImageFiles",
                             init_args=dict(source=lst, corruptions="fog,contrast", severity=3, batch_size=2, seed=2, labels=True)))
    r2 = cli.validate(cfg, tasks=["ir", "cls"], model=model, classify={"r18": ("resnet18", wpath)})
    table = r2["by_corruption"]
    print(table)
    assert len(table) == 2 and sum(v["images"] for v in table.values()) == r2["images"] == 4
    for v in table.values():
        assert {"r18", "r18_top1", "input/r18", "input/r18_top1", "psnr", "ssim", "images"} <= set(v)
    for side, key in (("", "val_lq/r18_top1"), ("input/", "val_input/r18_top1")):              # micro recombines by image count
        assert sum(v[f"{side}r18_top1"] * v["images"] for v in table.values()) / 4 == pytest.approx(r2[key], abs=1e-12)
