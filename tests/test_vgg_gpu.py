"""VGG scoring on the GPU (ops.vgg, unirestore_amd/vgg.py, csrc/vgg.hip): the split-K Linear, the 2 x 2 max-pool and the adaptive
average pool against the fp64 restatement element by element, whole networks against it, `ops.vgg` end to end at torchvision's own
sizes, batch-place independence, bit-reproducibility (eager and hipGraph replay), non-finite values, argument checks, and the caller
path (LitUniFIE, cli.validate).  Every bound is 8 x fp32's own measured error (vgg_reference.py: E32_* / *_TOL, kept honest by
test_vgg_cpu.py); the weights are seeded stand-ins - no trained weights exist where this runs, so nothing here says anything about
published accuracies."""
import pytest
import torch

import classify_reference as CR
import vgg_reference as R

pytestmark = pytest.mark.gpu

_W = {}


def _weights(arch, hidden, classes, seed):
    """The stand-in weights of a case on the device, from the SAME state dict the fp64 restatement reads."""
    from unirestore_amd import vgg
    key = (arch, hidden, classes, seed)
    if key not in _W:
        _W[key] = vgg.VGGWeights(arch, R.state_dict(arch, seed, classes, hidden))
    return _W[key]


def _small():
    return _weights(*R.NET_CASES[R.SMALL][:4])


def _packed(k, n):
    from unirestore_amd import vgg
    key = ("linear", k, n)
    if key not in _W:
        _x, w, b = R.lin_case(k, n)
        _W[key] = vgg.PackedLinearF32(w, b, "cuda")
    return _W[key]


# ---- the Linear -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.LIN_CASES))
def test_linear_matches_fp64(name):
    from unirestore_amd import vgg
    k, n, relu = R.LIN_CASES[name]
    want, scale = R.lin_reference(name)
    x = R.lin_case(k, n)[0].cuda()
    pl = _packed(k, n)
    assert pl.splits == -(-k // 512)
    full = None
    for m in R.LIN_MS:
        got = vgg.linear(x[:m].contiguous(), pl, relu)
        err = float(((got.cpu().double() - want[:m]).abs() / scale[:m]).max())
        print(f"linear {name} M={m}: max |err| / (sum |a b| + |bias|) {err:.2e} (bound {R.LIN_TOL[name]:.2e})")
        assert got.dtype == torch.float32 and tuple(got.shape) == (m, n) and err <= R.LIN_TOL[name]
        full = got if m == R.LIN_ROWS else full
        if relu:
            assert float(got.min()) >= 0
    shifted = torch.zeros(x.numel() + 1, device="cuda")[1:].view(x.shape).copy_(x)          # an unaligned x: the scalar loads, the same bits
    assert shifted.data_ptr() % 16 == 4 and torch.equal(vgg.linear(shifted, pl, relu), full)


def test_linear_at_classifier0s_real_size():
    from unirestore_amd import vgg
    x, w, b = R.lin_real_case()
    want, scale = R.lin_real_reference()
    got = vgg.linear(x.cuda(), vgg.PackedLinearF32(w, b, "cuda"), relu=True)
    err = float(((got.cpu().double() - want).abs() / scale).max())
    print(f"linear 25088 -> 4096, M=3: max |err| / (sum |a b| + |bias|) {err:.2e} (bound {R.LIN_REAL_TOL:.2e})")
    assert tuple(got.shape) == (3, 4096) and err <= R.LIN_REAL_TOL


@pytest.mark.parametrize("k,n", [(1000, 200), (25088, 64)])
def test_linear_rows_do_not_depend_on_the_batch(k, n):
    """Row i of M = 33 has the bits it has alone and at another position, two runs are bit-equal, and a NaN and a +inf in one
    input row reach that row only."""
    from unirestore_amd import vgg
    pl = _packed(k, n)
    x = R.lin_case(k, n)[0][:33].contiguous().cuda()
    whole = vgg.linear(x, pl, True)
    assert torch.equal(whole, vgg.linear(x, pl, True))
    for i in (0, 5, 31, 32):
        assert torch.equal(vgg.linear(x[i:i + 1].contiguous(), pl, True)[0], whole[i])
        order = [j for j in range(33) if j != i]
        at = (i + 17) % 33
        order.insert(at, i)
        assert torch.equal(vgg.linear(x[order].contiguous(), pl, True)[at], whole[i])
    raw = vgg.linear(x, pl, False)
    for value, col in ((float("nan"), 3), (float("inf"), k - 1)):
        bad = x.clone()
        bad[7, col] = value
        got = vgg.linear(bad, pl, False)
        want = R.linear(bad.cpu(), *R.lin_case(k, n)[1:], False)
        keep = [j for j in range(33) if j != 7]
        assert not bool(torch.isfinite(want[7]).any()) and torch.equal(torch.isnan(got[7]).cpu(), torch.isnan(want[7]))
        assert torch.equal((got[7] == float("inf")).cpu(), want[7] == float("inf")) and torch.equal(got[keep], raw[keep])


def test_linear_relu_keeps_nan_and_inf_and_turns_minus_inf_into_zero():
    from unirestore_amd import vgg
    g = torch.Generator().manual_seed(5)
    w, b = torch.rand(40, 600, generator=g) + 0.1, torch.randn(40, generator=g)              # positive weights: the sign of an infinite input stays
    pl = vgg.PackedLinearF32(w, b, "cuda")
    x = torch.rand(4, 600, generator=g)
    x[0, 599], x[1, 0], x[2, 300] = float("-inf"), float("inf"), float("nan")
    raw, got = vgg.linear(x.cuda(), pl, False).cpu(), vgg.linear(x.cuda(), pl, True).cpu()
    assert bool((raw[0] == float("-inf")).all()) and bool((got[0] == 0).all())
    assert bool((got[1] == float("inf")).all()) and bool(torch.isnan(got[2]).all()) and bool(torch.isfinite(got[3]).all())
    assert torch.equal(got[3], torch.relu(raw[3]))


# ---- the pools ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.POOL_CASES, ids=R.avg_name)
def test_maxpool2_is_torchs_bit_for_bit(shape):
    from unirestore_amd import vgg
    x = R.pool_case(shape)
    want = CR.nhwc(R.maxpool2(x))
    got = vgg.maxpool2(CR.nhwc(x).cuda())
    assert tuple(got.shape) == (shape[0], shape[1] // 2, shape[2] // 2, shape[3]) and torch.equal(got.cpu(), want)
    bad = x.clone()
    bad[0, 1, 1, 0] = float("nan")                                  # a NaN tap is its window's maximum
    bad[0, 2, :2, :2] = float("-inf")                               # a window of -inf gives -inf
    bad[0, 3, 0, 1] = float("-inf")
    want = CR.nhwc(R.maxpool2(bad))
    got = vgg.maxpool2(CR.nhwc(bad).cuda()).cpu()
    assert bool(torch.isnan(want[0, 0, 0, 1])) and float(want[0, 0, 0, 2]) == float("-inf") and int(torch.isnan(want).sum()) == 1
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~torch.isnan(want)], want[~torch.isnan(want)])
    if shape[3] % 4 == 0:                                           # an unaligned view: the scalar path, the same bits
        xd = CR.nhwc(x)
        shifted = torch.zeros(xd.numel() + 1, device="cuda")[1:].view(xd.shape).copy_(xd)
        assert shifted.data_ptr() % 16 == 4 and torch.equal(vgg.maxpool2(shifted).cpu(), CR.nhwc(R.maxpool2(x)))


@pytest.mark.parametrize("shape", R.AVG_CASES, ids=R.avg_name)
def test_avgpool7_matches_fp64(shape):
    from unirestore_amd import capi, vgg
    x = R.avg_case(shape)
    want = CR.nhwc(R.avgpool7(x))
    xd = CR.nhwc(x).cuda()
    got = vgg.avgpool7(xd)
    err = R.rel_err(got.cpu(), want)
    print(f"avgpool7 {R.avg_name(shape)}: max |err| {err:.2e} of max |fp64| (bound {R.AVG_TOL[R.avg_name(shape)]:.2e})")
    assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0], 7, 7, shape[3]) and err <= R.AVG_TOL[R.avg_name(shape)]
    if shape[1:3] == (7, 7):                                        # the Python path skips the launch; the kernel returns the input's bits
        assert got is xd
        y = torch.empty_like(xd)
        capi.check(capi.lib.ur_vgg_avgpool7_f32(xd.data_ptr(), y.data_ptr(), *shape, torch.cuda.current_stream().cuda_stream))
        assert torch.equal(y, xd)


# ---- the whole network --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.NET_CASES))
def test_logits_match_fp64_and_decide_as_fp64_does(name):
    from unirestore_amd import vgg
    arch, hidden, classes, wseed, _iseed, (n, _h, _w) = R.NET_CASES[name]
    want = R.net_reference(name)
    scale = float(want.abs().max())
    bound = R.LOGITS_TOL[name] * scale
    gaps = R.top2_gap(want)
    assert bool(torch.isfinite(want).all()) and float(gaps.min()) > 2 * bound          # every image is decidable: none is left out
    wts = _weights(arch, hidden, classes, wseed)
    assert (wts.hidden, wts.num_classes) == (hidden, classes)
    got = vgg.logits(CR.nhwc(R.net_input(name)).contiguous().cuda(), wts)
    assert tuple(got.shape) == (n, classes) and got.dtype == torch.float32
    err = float((got.cpu().double() - want).abs().max())
    print(f"{name}: max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.2f} (bound {R.LOGITS_TOL[name]:.2e}); "
          f"classes {want.argmax(dim=1).tolist()}, smallest top-2 gap {float(gaps.min()):.4f}")
    assert err <= bound
    assert got.argmax(dim=1).cpu().tolist() == want.argmax(dim=1).tolist()
    one = vgg.logits(CR.nhwc(R.net_input(name))[:1].contiguous().cuda(), wts)
    assert tuple(one.shape) == (1, classes) and torch.equal(one[0], got[0])


def test_full_size_vgg16_end_to_end_matches_fp64():
    """torchvision's own sizes (hidden 4096, 1000 classes, 138 M parameters) through ops.vgg from two 75 x 101 images."""
    from unirestore_amd import ops
    want = R.forward_reference()
    scale = float(want.abs().max())
    assert float(R.top2_gap(want).min()) > 2 * R.FORWARD_TOL * scale
    wts = _weights(*R.FULL)
    assert (wts.hidden, wts.num_classes, wts.linears["classifier.0"].splits) == (4096, 1000, 49)
    got = ops.vgg(R.forward_images().cuda(), wts)
    err = float((got.cpu().double() - want).abs().max())
    print(f"forward vgg16: max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.2f} (bound {R.FORWARD_TOL:.2e})")
    assert tuple(got.shape) == (2, 1000) and err <= R.FORWARD_TOL * scale
    assert got.argmax(dim=1).cpu().tolist() == want.argmax(dim=1).tolist()
    pred, tp, targets, predicted = ops.top1(got, want.argmax(dim=1))      # ops.top1 serves the VGG's logits as the ResNet's
    assert pred.cpu().tolist() == want.argmax(dim=1).tolist() and int(tp.sum()) == 2 == int(targets.sum()) == int(predicted.sum())
    del _W[R.FULL]                                                        # 550 MB of device memory the later tests do not need


def test_logits_do_not_depend_on_the_place_in_the_batch():
    from unirestore_amd import ops
    w = _small()
    x = R.property_images().cuda()
    whole = ops.vgg(x, w)
    for i in range(4):
        assert torch.equal(ops.vgg(x[i:i + 1].contiguous(), w)[0], whole[i])
        order = [j for j in range(4) if j != i]
        order.insert((i + 2) % 4, i)
        assert torch.equal(ops.vgg(x[order].contiguous(), w)[(i + 2) % 4], whole[i])


def test_deterministic_eager_and_graph_replay():
    from unirestore_amd import ops
    w = _small()
    x = R.property_images(9)[:3].contiguous().cuda()
    a = ops.vgg(x, w)
    b = ops.vgg(x, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.vgg(x, w)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = ops.vgg(x, w)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a).all())


def test_a_nan_pixel_makes_its_image_nan_and_leaves_the_others_alone():
    from unirestore_amd import ops
    w = _small()
    x = R.property_images(21)[:3].contiguous()
    clean = ops.vgg(x.cuda(), w)
    bad = x.clone()
    bad[1, 2, 20, 26] = float("nan")
    want = R.vgg(CR.preprocess(bad), R.net_state_dict(R.SMALL))
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isfinite(want[[0, 2]]).all())      # the restatement, on the host first
    got = ops.vgg(bad.cuda(), w)
    assert bool(torch.isnan(got[1]).all())
    assert torch.equal(got[[0, 2]], clean[[0, 2]])


# ---- the interface ----------------------------------------------------------------------------------------------------------------

def test_ops_vgg_rejects_bad_inputs():
    from unirestore_amd import classify, ops, vgg
    w = _small()
    x = CR.images((2, 3, 40, 44), 1).cuda()
    for bad in (x.double(), x.half(), x.cpu(), x[0], x.transpose(2, 3), x[:, :1].contiguous(), x[:, :, :0].contiguous(), x[:0].contiguous()):
        with pytest.raises(ValueError):
            ops.vgg(bad, w)
    for bad_w in (None, {"arch": "vgg16"}, classify.random_weights("resnet18", 7, 10)):
        with pytest.raises(ValueError, match="vgg.load_weights"):
            ops.vgg(x, bad_w)
    with pytest.raises(ValueError, match="classify.load_weights"):
        ops.classify(x, w)                                               # each operator takes its own weights class
    with pytest.raises(ValueError, match="rvt.load_weights"):
        ops.rvt(x, w)
    assert ops.vgg(x[:, :, :1, :1].contiguous(), w).shape == (2, 10)     # a 1 x 1 image is legal: the preprocess resizes it
    with pytest.raises(ValueError, match="vgg.logits"):
        vgg.logits(torch.zeros(1, 31, 64, 3, device="cuda"), w)          # five pools need 32 x 32
    with pytest.raises(ValueError, match="vgg.logits"):
        vgg.logits(torch.zeros(1, 64, 64, 4, device="cuda"), w)
    f = torch.zeros(2, 25088, device="cuda")
    for bad in (f.cpu(), f.double(), f[:, :25087], f[0], f[:0], f[:, :100].contiguous()):
        with pytest.raises(ValueError, match="vgg.linear"):
            vgg.linear(bad, w.linears["classifier.0"])
    m = torch.zeros(1, 4, 4, 8, device="cuda")
    for bad in (m.cpu(), m.double(), m[0], m[:0], m[..., :6], m[:, :1]):
        with pytest.raises(ValueError, match="vgg.maxpool2"):
            vgg.maxpool2(bad)
    for bad in (m.cpu(), m.double(), m[0], m[:0], m[..., :6]):
        with pytest.raises(ValueError, match="vgg.avgpool7"):
            vgg.avgpool7(bad)


def _tiny_model():
    import unirestore_amd.modules as M
    from oracle.model import DiffUIE as ODiffUIE
    from tiny_cfg import TINY, model_kwargs, randomise_
    torch.manual_seed(0)
    o = randomise_(ODiffUIE(**model_kwargs(2), **TINY).eval(), 0)
    p = M.DiffUIE(**model_kwargs(2), **TINY).eval()
    p.load_state_dict(o.state_dict())
    return p


def test_litunifie_and_cli_validate_score_a_vgg_from_a_checkpoint(tmp_path):
    """The caller path with an architecture loaded from a file: LitUniFIE(classifiers={"vgg": ("vgg11", path)}) next to a ResNet in
    the same dict, and cli.validate(vgg=...) on a tiny labelled list."""
    from PIL import Image
    from tiny_cfg import model_kwargs
    from unirestore_amd import classify, cli, ops, runner, vgg
    path = str(tmp_path / "vgg11.pth")
    torch.save(vgg.random_state_dict(R.CALLER_ARCH, 5, 3, 64), path)
    model = _tiny_model()
    resnet = classify.random_weights("resnet18", 7, 3)
    lit = runner.LitUniFIE(model_kwargs(2), model=model, classifiers={"vgg": (R.CALLER_ARCH, path), "r18": resnet})
    ws = lit.classifiers["vgg"]
    assert isinstance(ws, vgg.VGGWeights) and ws.arch == R.CALLER_ARCH and (ws.num_classes, ws.hidden) == (3, 64) and lit.classifiers["r18"] is resnet
    hq = CR.varied_images(3, 96, 80, 100).cuda()
    lq = (0.6 * hq + 0.3 * CR.varied_images(3, 96, 80, 200).cuda()).clamp(0, 1)
    labels = torch.tensor([0, 1, 2])
    torch.manual_seed(40)
    out = lit.validation_step((lq, hq, labels, ["a", "b", "c"], "ir"), tasks=["ir", "cls"])[-1]
    m = lit.metrics()
    keys = {"val_lq/vgg", "val_lq/vgg_top1", "val_input/vgg", "val_input/vgg_top1", "val_lq/r18", "val_input/r18_top1"}
    assert keys <= set(m) and {"cls/vgg", "cls_input/vgg", "cls/r18", "cls_input/r18"} <= set(lit.totals)
    for name, predict, w in (("vgg", ops.vgg, ws), ("r18", ops.classify, resnet)):
        for key, img in ((f"cls/{name}", out["cls"]), (f"cls_input/{name}", lq)):
            want = torch.stack(ops.top1(predict(runner.crop_tensor(img).contiguous(), w), labels)[1:])
            assert torch.equal(lit.totals[key], want) and int(want[1].sum()) == 3
            prefix = "val_lq" if key.startswith("cls/") else "val_input"
            assert (m[f"{prefix}/{name}"], m[f"{prefix}/{name}_top1"]) == classify.accuracy(*want)

    imgs = (CR.varied_images(4, 64, 64, 31) * 255).round().byte().permute(0, 2, 3, 1).numpy()
    for i in range(4):
        Image.fromarray(imgs[i]).save(str(tmp_path / f"im{i}.png"))
    lst = tmp_path / "list.txt"
    lst.write_text("".join(f"im{i}.png im{i}.png {i % 3}\n" for i in range(4)))

    def cfg(data):
        return dict(seed_everything=3, trainer=dict(accelerator="gpu", devices=1, precision="bf16-mixed"),
                    model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=model_kwargs(2))), data=data)
    keys = {"val_lq/t", "val_lq/t_top1", "val_input/t", "val_input/t_top1"}
    files = cfg(dict(class_path="unirestore_amd.data.ImageListFiles", init_args=dict(list_file=str(lst), batch_size=2, labels=True)))
    r0 = cli.validate(files, tasks=["ir", "cls"], model=model)
    r1 = cli.validate(files, tasks=["ir", "cls"], model=model, vgg=f"t={R.CALLER_ARCH}:{path}")
    print({k: r1[k] for k in sorted(keys)})
    assert set(r1) == set(r0) | keys and r1["images"] == r0["images"] == 4
    assert all(r1[k] == r0[k] for k in r0 if k != "images_per_s")            # without --vgg the result is what it was
    assert all(0.0 <= r1[k] <= 1.0 for k in keys)
    corrupted = cfg(dict(class_path="unirestore_amd.data.CorruptedImageFiles",
                         init_args=dict(source=str(lst), corruptions="fog,contrast", severity=3, batch_size=2, seed=2, labels=True)))
    table = cli.validate(corrupted, tasks=["ir", "cls"], model=model, vgg={"t": ws})["by_corruption"]
    assert len(table) == 2 and all({"t", "t_top1", "input/t", "input/t_top1", "psnr", "ssim", "images"} <= set(v) for v in table.values())
