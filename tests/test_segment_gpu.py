"""Segmenter scoring on the GPU (ops.segment / ops.confusion, unirestore_amd/segment.py, csrc/segment.hip): every launcher of
its own against the fp64 restatement element by element (the shared fp32 layers: test_f32net_gpu.py), whole networks on tiny maps, `ops.segment` end to end, batch-place independence,
bit-reproducibility (eager and hipGraph replay), argument checks, and the caller path (LitUniFIE, cli.validate).  Every bound
is 8 x fp32's own measured error (segment_reference.py: E32_* / *_TOL, kept honest by
test_segment_cpu.py::test_tolerances_follow_the_measured_fp32_error); confusion and argmax on exact inputs are
compared for equality.  The weights are seeded stand-ins - no trained weights exist where this runs, so nothing here says
anything about any published mIoU."""
import numpy as np
import pytest
import torch

import segment_reference as R
from tiny_cfg import TINY, model_kwargs, randomise_

pytestmark = pytest.mark.gpu

_W = {}


def _weights(arch=R.TINY, seed=3):
    """The stand-in weights of a case on the device, from the SAME state dict the fp64 restatement reads."""
    from unirestore_amd import segment
    if (arch, seed) not in _W:
        _W[(arch, seed)] = segment.SegmenterWeights(arch, R.state_dict(arch, seed))
    return _W[(arch, seed)]


# ---- the launchers ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.PREP_CASES, ids=[f"{'x'.join(map(str, c[0]))}@{c[1]}" for c in R.PREP_CASES])
def test_prep_matches_fp64_and_writes_nhwc_bgr(case):
    from unirestore_amd import segment
    shape, s = case
    x = R.images(shape, sum(shape))
    size = (segment.scaled_size(shape[2], s), segment.scaled_size(shape[3], s))
    assert size == R.scaled_hw(shape[2], shape[3], s) and (shape != (1, 3, 54, 54) or size == (32, 32))
    y = segment.prep(x.cuda(), size).cpu()
    assert tuple(y.shape) == (shape[0], size[0], size[1], 3) and y.dtype == torch.float32
    err = float((R.nchw(y).double() - R.prep(x, size)).abs().max())
    print(f"prep {shape} @ {s}: max |err| {err:.2e} (bound {R.PREP_TOL:.2e})")
    assert err <= R.PREP_TOL


def test_prep_at_scale_1_is_bit_exact():
    from unirestore_amd import segment
    x = R.images((2, 3, 37, 53), 5)
    y = segment.prep(x.cuda()).cpu()
    assert torch.equal(R.nchw(y), R.preprocess(x, torch.float32))


@pytest.mark.parametrize("name", sorted(R.TTA_CASES))
def test_tta_argmax_matches_fp64(name):
    from unirestore_amd import segment
    n, c, _sizes, size = R.TTA_CASES[name]
    maps = R.tta_case(name)
    want = R.tta_average(maps, size)
    scale = max(float(m.abs().max()) for m in maps)
    pred, avg = segment.tta_argmax([R.nhwc(m).cuda() for m in maps], size, want_avg=True)
    assert tuple(pred.shape) == (n, *size) and pred.dtype == torch.uint8 and tuple(avg.shape) == (n, *size, c)
    err = float((R.nchw(avg.cpu()).double() - want).abs().max())
    print(f"tta {name}: max |err| {err:.2e} = {err / scale:.2e} of max |logit| (bound {R.TTA_TOL:.2e})")
    assert err <= R.TTA_TOL * scale
    ok = R.decidable(want, R.TTA_TOL * scale)
    assert float(ok.float().mean()) > 0.99
    assert torch.equal(pred.cpu().long()[ok], want.argmax(dim=1)[ok])
    # the prediction is the argmax of the kernel's own averaged logits everywhere, and the same without the optional output
    assert torch.equal(pred.cpu().long(), avg.cpu().argmax(dim=3))
    assert torch.equal(segment.tta_argmax([R.nhwc(m).cuda() for m in maps], size), pred)


def test_tta_argmax_ties_and_nan():
    from unirestore_amd import segment
    c = 19
    m = torch.zeros(1, 6, 7, c)                              # same size as the target: the resize is the identity
    m[0, 0, 0, [4, 9, 17]] = 2.0                             # a three-way tie: the lowest index wins
    m[0, 0, 1, :] = 0.25                                     # everything ties: class 0
    m[0, 0, 2, c - 1] = 5.0                                  # the last class
    m[0, 0, 3, :] = -torch.arange(1, c + 1).float()          # all negative: class 0
    # a non-finite value also reaches the pixels to its left and above (0 x NaN, as in torch's own resize): those are not checked
    m[0, 5, 6, 7], m[0, 5, 6, 12], m[0, 5, 6, 3] = float("nan"), float("nan"), 9.0      # the first NaN is the maximum
    m[0, 3, 6, 0], m[0, 3, 6, 5] = float("nan"), 3.0         # NaN in class 0
    m[0, 3, 2, [2, 3]] = float("inf")                        # tied infinities
    checked = {(0, 0): 4, (0, 1): 0, (0, 2): c - 1, (0, 3): 0, (5, 6): 7, (3, 6): 0, (3, 2): 2, (5, 0): 0}
    for (y, x), k in checked.items():
        assert int(m[0, y, x].argmax()) == k
    for maps in ([m], [m, m], [m, m, m]):                    # equal maps average to themselves
        pred = segment.tta_argmax([t.cuda() for t in maps], (6, 7)).cpu()
        assert {yx: int(pred[0, yx[0], yx[1]]) for yx in checked} == checked


CONF_CASES = {"u8_4096": (4096, torch.uint8, 19), "i64_5000": (5000, torch.int64, 19), "u8_1": (1, torch.uint8, 19), "i64_9001_c5": (9001, torch.int64, 5),
              "u8_20000_c21": (20000, torch.uint8, 21)}


@pytest.mark.parametrize("name", sorted(CONF_CASES))
def test_confusion_equals_numpy_bincount(name):
    from unirestore_amd import ops
    p, dtype, c = CONF_CASES[name]
    g = torch.Generator().manual_seed(p)
    target = torch.randint(0, c - 1, (p,), generator=g)      # class c - 1 is never a target: an absent row
    target[torch.rand(p, generator=g) < 0.2] = 255
    pred = torch.randint(0, c, (p,), generator=g).to(torch.uint8)
    conf = ops.confusion(pred.cuda(), target.to(dtype).cuda(), classes=c)
    assert conf.dtype == torch.int64 and tuple(conf.shape) == (c, c) and conf.is_cuda
    want = R.confusion(pred.numpy(), target.numpy(), c)
    assert np.array_equal(conf.cpu().numpy(), want)
    assert int(conf.sum()) == int((target != 255).sum()) and int(conf[c - 1].sum()) == 0
    assert torch.equal(ops.confusion(pred.cuda(), target.to(dtype), classes=c), conf)             # host targets


def test_confusion_all_ignored_and_shapes():
    from unirestore_amd import ops
    pred = torch.randint(0, 19, (2, 33, 47), generator=torch.Generator().manual_seed(1)).to(torch.uint8).cuda()
    assert int(ops.confusion(pred, torch.full((2, 33, 47), 255, dtype=torch.uint8).cuda()).sum()) == 0
    target = pred.clone().long()
    target[0, :5] = 255
    conf = ops.confusion(pred, target)
    assert int(conf.sum()) == 2 * 33 * 47 - 5 * 47 and torch.equal(conf, torch.diag(torch.diag(conf)))


# ---- the whole network --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.NET_CASES))
def test_logits_and_prediction_match_fp64(name):
    from unirestore_amd import ops, segment
    arch, wseed, _iseed, n, h, w_ = R.NET_CASES[name]
    want1, want3 = R.net_reference(name)
    x = R.net_images(name)
    wts = _weights(arch, wseed)
    got = segment.logits(segment.prep(x.cuda()), wts)
    assert tuple(got.shape) == (n, h // 4, w_ // 4, 19) and got.dtype == torch.float32
    scale = float(want1.abs().max())
    err = float((R.nchw(got.cpu()).double() - want1).abs().max())
    print(f"{name}: scale-1 logits max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.1f} (bound {R.LOGITS_TOL[name]:.2e})")
    assert err <= R.LOGITS_TOL[name] * scale
    scale3 = float(want3.abs().max())
    ok = R.decidable(want3, R.TTA_LOGITS_TOL[name] * scale3)
    left_out = 1.0 - float(ok.float().mean())
    classes = sorted(set(want3.argmax(dim=1)[ok].tolist()))
    pred = ops.segment(x.cuda(), wts)
    assert tuple(pred.shape) == (n, h, w_) and pred.dtype == torch.uint8
    flips = int((pred.cpu().long()[ok] != want3.argmax(dim=1)[ok]).sum())
    print(f"{name}: {left_out:.4%} of the pixels left out, classes {classes}, {flips} argmax flips on the decidable ones")
    assert left_out <= R.MAX_LEFT_OUT and len(classes) >= R.MIN_CLASSES
    assert flips == 0
    # the mIoU of the prediction against the fp64 one, through the confusion kernel: every present class scores, none is lost
    conf = ops.confusion(pred, want3.argmax(dim=1).to(torch.uint8).cuda())
    miou, acc, _ = segment.miou(conf)
    assert acc >= 1.0 - R.MAX_LEFT_OUT and miou > 0.9


def test_prediction_does_not_depend_on_the_place_in_the_batch():
    from unirestore_amd import ops
    w = _weights()
    x = R.varied_images(3, 64, 80, 12).cuda()
    whole = ops.segment(x, w)
    for i in range(3):
        assert torch.equal(ops.segment(x[i:i + 1].contiguous(), w)[0], whole[i])
        for slot in range(3):
            order = [j for j in range(3) if j != i]
            order.insert(slot, i)
            assert torch.equal(ops.segment(x[order].contiguous(), w)[slot], whole[i])


def test_deterministic_eager_and_graph_replay():
    from unirestore_amd import ops
    w = _weights()
    x = R.varied_images(2, 64, 80, 9).cuda()
    target = torch.randint(0, 19, (2, 64, 80), generator=torch.Generator().manual_seed(4)).to(torch.uint8).cuda()
    a = ops.segment(x, w)
    b = ops.segment(x, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.segment(x, w)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = ops.segment(x, w)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and len(set(a.flatten().tolist())) >= 2
    assert torch.equal(ops.confusion(a, target), ops.confusion(c, target))


def test_ops_reject_bad_inputs():
    from unirestore_amd import ops
    w = _weights()
    x = R.images((2, 3, 64, 72), 1).cuda()
    for bad in (x.double(), x.half(), x.cpu(), x[0], x.transpose(2, 3), x[:, :1].contiguous(), x[:, :, :0].contiguous(), x[:0].contiguous()):
        with pytest.raises(ValueError):
            ops.segment(bad, w)
    for bad_w in (None, {"arch": "rflw50"}):
        with pytest.raises(ValueError):
            ops.segment(x, bad_w)
    with pytest.raises(ValueError, match="32"):
        ops.segment(x[:, :, :53].contiguous(), w)            # 53 * 0.6 = 31.8: below the network's smallest input
    for kw in (dict(size=(0, 4)), dict(size=5), dict(scales=()), dict(scales=(1, 0.8, 0.6, 0.4)), dict(scales=(0,))):
        with pytest.raises(ValueError):
            ops.segment(x, w, **kw)
    assert ops.segment(x, w, size=(5, 7), scales=(1,)).shape == (2, 5, 7)
    pred = torch.zeros(2, 4, 4, dtype=torch.uint8).cuda()
    tgt = torch.zeros(2, 4, 4, dtype=torch.int64).cuda()
    for bad_p, bad_t in ((pred.long(), tgt), (pred.cpu(), tgt), (pred, tgt[:1]), (pred, tgt.float()), (pred, None), (pred, tgt + 19), (pred, tgt - 1),
                         (pred + 19, tgt), (pred.transpose(1, 2)[:, :, :2], tgt.transpose(1, 2)[:, :, :2]), (pred[:0], tgt[:0])):
        with pytest.raises(ValueError):
            ops.confusion(bad_p, bad_t)
    for kw in (dict(classes=0), dict(classes=256), dict(classes=19.0)):
        with pytest.raises(ValueError):
            ops.confusion(pred, tgt, **kw)
    assert int(ops.confusion(pred, tgt)[0, 0]) == 32
    # the launchers' size limits, at the first refused count (placeholder pointers: a refusal comes before any HIP call)
    from unirestore_amd import capi
    lib, P, L = capi.lib, 256, (1 << 31) - 256                                # L: the 1-D launch limit of csrc/launch_size.h
    for call in (lambda: lib.ur_add_f32(P, P + 256, P + 512, L, None), lambda: lib.ur_maxpool5_f32(P, P + 256, L // 256, 1, 1, 256, None),
                 lambda: lib.ur_upsample_bilinear_ac_f32(P, P + 256, L // 256, 1, 1, 256, 1, 1, P, P, P, P, None),
                 lambda: lib.ur_seg_tta_argmax(P, None, None, 1, L // 256, 19, 1, 1, 0, 0, 0, 0, 16, 16, P, P, P, P, P + 256, None, None)):
        assert call() == capi.UR_E_INVALID and "2^31 - 256" in lib.ur_last_error().decode(), lib.ur_last_error().decode()


# ---- the caller ---------------------------------------------------------------------------------------------------------------

def _tiny_model():
    import unirestore_amd.modules as M
    from oracle.model import DiffUIE as ODiffUIE
    torch.manual_seed(0)
    o = randomise_(ODiffUIE(**model_kwargs(2), **TINY).eval(), 0)
    p = M.DiffUIE(**model_kwargs(2), **TINY).eval()
    p.load_state_dict(o.state_dict())
    return p


def _label_maps(n, h, w, seed):
    """int64 [n,h,w] trainId maps: coarse blobs of 19 classes with some ignored pixels."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, 19, (n, 1, h // 16, w // 16), generator=g).float()
    maps = torch.nn.functional.interpolate(coarse, size=(h, w), mode="nearest")[:, 0].long()
    maps[torch.rand(n, h, w, generator=g) < 0.1] = 255
    return maps


def test_litunifie_accumulates_confusion_matrices_and_leaves_the_rest_alone():
    from unirestore_amd import ops, runner, segment
    model = _tiny_model()
    w = _weights()
    tasks = ["ir", "cls", "seg"]
    batches = []
    for b in range(2):
        hq = R.varied_images(2, 96, 80, 100 + b).cuda()
        lq = (0.6 * hq + 0.3 * R.varied_images(2, 96, 80, 200 + b).cuda()).clamp(0, 1)
        batches.append((lq, hq, _label_maps(2, 96, 80, 300 + b)))

    def run(segmenters, with_maps, **kw):
        lit = runner.LitUniFIE(model_kwargs(2), model=model, segmenters=segmenters, **kw)
        outs = []
        for b, (lq, hq, maps) in enumerate(batches):
            torch.manual_seed(40 + b)                # the forward's noise draws: the same for every instance
            outs.append(lit.validation_step((lq, hq, maps if with_maps else None, ["a", "b"], "ir"), tasks=tasks)[-1])
        return lit, lit.metrics(), outs
    lit0, m0, o0 = run(None, False)
    assert set(m0) == {"val_lq/psnr", "val_lq/ssim", "images"} and set(lit0.totals) == {"psnr", "ssim", "images"}      # today's keys
    lit1, m1, o1 = run({"rf": w}, True)
    for a, b in zip(o0, o1):
        assert all(torch.equal(a[t], b[t]) for t in tasks)                        # restoring does not depend on the scoring
    assert m0["val_lq/psnr"] == m1["val_lq/psnr"] and m0["val_lq/ssim"] == m1["val_lq/ssim"] and m1["images"] == 4
    new = {"val_lq/rf", "val_lq/rf_acc", "val_input/rf", "val_input/rf_acc"}
    assert set(m1) == set(m0) | new and set(lit1.totals) == set(lit0.totals) | {"seg/rf", "seg_input/rf"}
    assert lit1.segmenter_keys("rf") == ("seg/rf", "seg_input/rf")
    for key, side in (("seg/rf", [o["seg"] for o in o1]), ("seg_input/rf", [lq for lq, _, _ in batches])):
        tot = lit1.totals[key]
        assert tot.is_cuda and tot.dtype == torch.int64 and tuple(tot.shape) == (19, 19)
        want = sum(ops.confusion(ops.segment(runner.crop_tensor(img).contiguous(), w), runner.crop_tensor(maps).contiguous().cuda())
                   for img, (_, _, maps) in zip(side, batches))
        assert torch.equal(tot, want) and int(tot.sum()) == sum(int((maps != 255).sum()) for _, _, maps in batches)
        miou, acc, _ = segment.miou(want)
        prefix = "val_lq" if key == "seg/rf" else "val_input"
        assert m1[f"{prefix}/rf"] == miou and m1[f"{prefix}/rf_acc"] == acc and 0.0 <= miou <= 1.0
        assert (miou, acc) == pytest.approx(R.miou(want.cpu().tolist()), abs=1e-15)
    # a smaller crop: inputs and label maps are cut with the restoration's own box
    lit2, m2, o2 = run({"rf": w}, True, crop=(64, 64))
    assert o2[0]["seg"].shape[-2:] == (64, 64) and int(lit2.totals["seg/rf"].sum()) == sum(int((m[:, 16:80, 8:72] != 255).sum()) for _, _, m in batches)
    lq, _hq, maps = batches[0]
    box = (slice(None), slice(16, 80), slice(8, 72))
    assert torch.equal(lit2.totals["seg_input/rf"], sum(ops.confusion(ops.segment(q[:, :, 16:80, 8:72].contiguous(), w), m[box].contiguous().cuda())
                                                        for q, _, m in batches))
    # the segmenters need seg among the tasks and label maps in the batch
    lit = runner.LitUniFIE(model_kwargs(2), model=model, segmenters={"rf": w})
    with pytest.raises(ValueError, match="seg"):
        lit.validation_step((lq, _hq, maps, ["a", "b"], "ir"), tasks=["ir", "cls"])
    with pytest.raises(ValueError, match="labels: map"):
        lit.update_segmentation(o1[0]["seg"], lq, None)
    with pytest.raises(ValueError, match="labels: map"):
        lit.update_segmentation(o1[0]["seg"], lq, torch.tensor([1, 2]))          # integer labels are no maps
    with pytest.raises(ValueError, match="19"):
        lit.update_segmentation(o1[0]["seg"], lq, maps.clamp(max=19))            # a trainId outside [0, 19) that is not 255
    assert int(lit.totals["seg/rf"].sum()) == 0                                  # refused before anything was counted


def _labelled_files(tmp_path, n=4, hw=(64, 64)):
    from PIL import Image
    imgs = (R.varied_images(n, hw[0], hw[1], 31) * 255).round().byte().permute(0, 2, 3, 1).numpy()
    maps = _label_maps(n, hw[0], hw[1], 7).to(torch.uint8).numpy()
    lines = []
    for i in range(n):
        Image.fromarray(imgs[i]).save(str(tmp_path / f"im{i}.png"))
        Image.fromarray(maps[i], mode="L").save(str(tmp_path / f"lab{i}.png"))
        lines.append(f"im{i}.png im{i}.png lab{i}.png\n")
    lst = tmp_path / "list.txt"
    lst.write_text("".join(lines))
    return str(lst), int((maps != 255).sum())


def _tiny_cli_cfg(data):
    return dict(seed_everything=3, trainer=dict(accelerator="gpu", devices=1, precision="bf16-mixed"),
                model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=model_kwargs(2))), data=data)


def test_cli_validate_segment(tmp_path):
    from unirestore_amd import cli, segment
    lst, _labelled = _labelled_files(tmp_path)
    wpath = str(tmp_path / "rf.pth")
    torch.save(segment.random_state_dict("rflw50", 7), wpath)
    model = _tiny_model()
    keys = {"val_lq/rf", "val_lq/rf_acc", "val_input/rf", "val_input/rf_acc"}
    labels = dict(labels="map", label_encoding="train_id")
    cfg = _tiny_cli_cfg(dict(class_path="unirestore_amd.data.ImageListFiles", init_args=dict(list_file=lst, batch_size=2, **labels)))
    r0 = cli.validate(cfg, tasks=["ir", "seg"], model=model)
    r1 = cli.validate(cfg, tasks=["ir", "seg"], model=model, segment=f"rf=rflw50:{wpath}")
    print({k: r1[k] for k in sorted(keys)})
    assert set(r1) == set(r0) | keys and r1["images"] == r0["images"] == 4
    assert r1["val_lq/psnr"] == r0["val_lq/psnr"] and r1["val_lq/ssim"] == r0["val_lq/ssim"]
    assert all(0.0 <= r1[k] <= 1.0 for k in keys)
    r3 = cli.validate(cfg, tasks=["ir", "seg"], model=model, segment={"rf": ("rflw50", wpath)}, crop="64,64")     # the images' own size
    assert {k: r3[k] for k in keys} == {k: r1[k] for k in keys}
    # clean files corrupted on the GPU: two corruptions, every entry of the table carries the new keys
    cfg = _tiny_cli_cfg(dict(class_path="unirestore_amd.data.CorruptedImageFiles",
                             init_args=dict(source=lst, corruptions="fog,contrast", severity=3, batch_size=2, seed=2, **labels)))
    r2 = cli.validate(cfg, tasks=["ir", "seg"], model=model, segment={"rf": ("rflw50", wpath)})
    table = r2["by_corruption"]
    print(table)
    assert len(table) == 2 and sum(v["images"] for v in table.values()) == r2["images"] == 4
    for v in table.values():
        assert {"rf", "rf_acc", "input/rf", "input/rf_acc", "psnr", "ssim", "images"} <= set(v)
    # pixel accuracy recombines by labelled-pixel counts: the label maps, read again, give each entry's count
    from unirestore_amd import data as D
    ds = D.CorruptedImageFiles(lst, "fog,contrast", 3, batch_size=2, seed=2, **labels)
    pixels = {}
    for batch in ds.batches(device="cuda"):
        key = "%s/%d" % ds.last
        pixels[key] = pixels.get(key, 0) + int((batch[2] != 255).sum())
    assert set(pixels) == set(table) and sum(pixels.values()) == _labelled
    for side, key in (("", "val_lq/rf_acc"), ("input/", "val_input/rf_acc")):
        assert sum(table[k][f"{side}rf_acc"] * pixels[k] for k in table) / _labelled == pytest.approx(r2[key], abs=1e-12)
