"""Non-finite pixels must reach the scores: NaN, +inf and -inf through every fp32 scoring kernel (csrc/f32_layers.hip and the
metrics' own kernels) and through the four scorers, on the GPU.  The contract (nonfinite_cases.py): every output element is
finite, +inf, -inf or NaN exactly where the fp64 restatement is on the same input; the finite ones stay within the bound their
case already has; an image without a non-finite value gives the bits it gives in a clean batch.  One function,
`assert_same_classes`, carries out every comparison.  test_nonfinite_cpu.py keeps the restatements honest against torch's own
operators and shows on the reference alone that every case reaches (or does not reach) an output, so nothing here passes
vacuously.

Before the ReLU epilogue and the three max-pools kept NaN (maximum(v, 0) for fmaxf(v, 0); (t > v || t != t) ? t : v for
fmaxf(v, t)) the NaN cases of the convolution with relu=True (10 of them: all but the never-read pixel) and of the three pools
(15) failed here, with a finite output where the reference has NaN; the other 94 convolution and pool cases passed on that
library too (the infinities, relu=False, the never-read pixel, the windows of -inf)."""
import functools
import importlib

import numpy as np
import pytest
import torch

import classify_reference as CR
import deeplab_reference as DR
import lpips_reference as LR
import nonfinite_cases as NF
import segment_reference as SR
from tiny_cfg import model_kwargs

pytestmark = pytest.mark.gpu


def assert_same_classes(got, want, bound=None, what=""):
    """got (any float dtype, any device) against the fp64 reference `want` of the same shape: the same class (finite / +inf /
    -inf / NaN) in every element, and the finite ones within `bound` - None: equal; a number or a tensor of want's shape:
    |got - want| <= bound, absolute (elements whose bound is not finite belong to non-finite outputs and are not looked at)."""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    kg, kw = NF.classes(got), NF.classes(want)
    wrong = kg != kw
    if bool(wrong.any()):
        i = tuple(int(v) for v in wrong.nonzero()[0])
        raise AssertionError(f"{what}: {int(wrong.sum())} of {wrong.numel()} elements are of another class than the reference "
                             f"({int((kw != NF.FINITE).sum())} non-finite in the reference, {int((kg != NF.FINITE).sum())} in the result); "
                             f"first at {i}: got {float(got[i])}, want {float(want[i])}")
    ok = kw == NF.FINITE
    if bound is None:
        assert torch.equal(got[ok].double(), want[ok].double()), f"{what}: finite values differ"
        return
    err = (got.double() - want.double())[ok].abs()
    lim = bound[ok] if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    assert bool(torch.isfinite(lim).all()), f"{what}: a finite output has no finite bound"
    worst = float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: {int((~ok).sum())} non-finite outputs of {ok.numel()}; finite ones at most {worst:.2f} of their bound")
    assert bool((err <= lim).all()), f"{what}: a finite output is {worst:.2f} x its bound away"


def same_bits(a, b):
    """Bit-identical fp32 / fp64 / integer tensors (NaN payloads included)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype.is_floating_point:
        view = torch.int32 if a.dtype == torch.float32 else torch.int64
        a, b = a.view(view), b.view(view)
    return a.shape == b.shape and torch.equal(a, b)


# ---- the convolution ----------------------------------------------------------------------------------------------------------

def _run_conv(case, relu, entry):
    """The case through one entry point -> NHWC result on the device."""
    from unirestore_amd import capi, f32net
    pc = f32net.PackedConvF32(case["w"], case["b"], case["stride"], case["pad"], "cuda", dilation=case["dil"])
    x = LR.nhwc(case["x"]).cuda()
    res = None if case["res"] is None else LR.nhwc(case["res"]).cuda()
    if entry == "res":                                                   # ur_conv2d_f32_res (ur_dlv3_conv2d_f32 when dilated)
        return f32net.conv2d_f32(x, pc, res, relu=relu)
    n, h, w_, cin = x.shape
    oh, ow = (h + 2 * pc.pad - pc.dilation * (pc.kh - 1) - 1) // pc.stride + 1, (w_ + 2 * pc.pad - pc.dilation * (pc.kw - 1) - 1) // pc.stride + 1
    if entry == "plain":                                                 # ur_conv2d_f32: no residual argument
        assert res is None and pc.dilation == 1
        y = torch.empty(n, oh, ow, pc.cout, device="cuda")
        capi.check(capi.lib.ur_conv2d_f32(x.data_ptr(), pc.w.data_ptr(), pc.bias.data_ptr(), y.data_ptr(), n, h, w_, cin, pc.cout, pc.kh, pc.kw,
                                          pc.stride, pc.pad, int(relu), f32net.stream()))
        return y
    assert entry == "dlv3"                                               # ur_dlv3_conv2d_f32, dense, whatever the dilation
    y = torch.empty(n, oh, ow, pc.cout, device="cuda")
    assert f32net.conv2d_f32(x, pc, res, relu=relu, out=(y, 0)) is y
    return y


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "no_relu"])
@pytest.mark.parametrize("value", NF.VALUE_NAMES)
@pytest.mark.parametrize("name", sorted(NF.CONV_NONFINITE))
def test_conv2d_f32_classifies_as_fp64(name, value, relu):
    """conv2d_f32 through ur_conv2d_f32 / ur_conv2d_f32_res / ur_dlv3_conv2d_f32: the class pattern of the fp64 restatement, the
    finite outputs within the case's own bound, the clean images' outputs with the clean run's bits, and the same bits through
    ur_dlv3_conv2d_f32.  relu=True with NaN is what `fmaxf(v, 0)` got wrong."""
    from unirestore_amd import f32net
    _maker, _where, _pos, reach, clean_images, entry = NF.CONV_NONFINITE[name]
    case, clean, want, bound = NF.conv_case(name, value, relu)
    if entry == "slice":
        channels, off = NF.CONV_SLICE
        pc = f32net.PackedConvF32(case["w"], case["b"], case["stride"], case["pad"], "cuda", dilation=case["dil"])
        x = LR.nhwc(case["x"]).cuda()
        y = f32net.conv2d_f32(x, pc, relu=relu)                          # dense
        buf = torch.full((*y.shape[:3], channels), NF.SENTINEL, device="cuda")
        assert f32net.conv2d_f32(x, pc, relu=relu, out=(buf, off)) is buf
        assert same_bits(buf[..., off:off + pc.cout], y)                 # the slice is the dense result bit for bit
        rest = torch.cat([buf[..., :off], buf[..., off + pc.cout:]], dim=3)
        assert rest.numel() == y.numel() // pc.cout * (channels - pc.cout) and bool((rest == NF.SENTINEL).all())
        y_clean = f32net.conv2d_f32(LR.nhwc(clean["x"]).cuda(), pc, relu=relu)
    else:
        y = _run_conv(case, relu, entry)
        assert same_bits(_run_conv(case, relu, "dlv3"), y)
        y_clean = _run_conv(clean, relu, entry)
    assert_same_classes(LR.nchw(y.cpu()), want, bound, f"{name} {value} relu={relu}")
    for i in clean_images:
        assert same_bits(y[i], y_clean[i]), f"image {i} holds no non-finite value but differs from the clean run"
    if not reach:
        assert same_bits(y, y_clean)                                     # the value is never read
    if relu:
        assert not bool((y < 0).any())


# ---- the pools ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", NF.pool_runs(), ids=[r[0] for r in NF.pool_runs()])
def test_maxpools_classify_as_fp64_and_are_exact(run):
    """The three max-pools: NaN wins a window wherever it sits (first tap, last tap, shared by windows), a dropped row is not
    read, a window of -inf gives -inf, +inf beats -inf; the finite outputs are the reference's, exactly."""
    from unirestore_amd import f32net
    _id, name, value = run
    kind, x, clean, want = NF.pool_case(name, value)
    f = getattr(f32net, f"{kind}_f32")
    y = f(LR.nhwc(x).cuda())
    assert_same_classes(LR.nchw(y.cpu()), want, None, run[0])
    if not NF.POOL_NONFINITE[name][3]:
        assert same_bits(y, f(LR.nhwc(clean).cuda()))                    # the value is never read
    # the other images keep the clean run's bits
    poisoned = {index[0] for index, _v in NF.POOL_NONFINITE[name][2]}
    y_clean = f(LR.nhwc(clean).cuda())
    for i in set(range(x.shape[0])) - poisoned:
        assert same_bits(y[i], y_clean[i])


@pytest.mark.parametrize("run", NF.avgpool_runs(), ids=[r[0] for r in NF.avgpool_runs()])
def test_avgpool_f32_classifies_as_fp64(run):
    """One poisoned (image, channel) turns exactly that output non-finite; +inf and -inf in one map average to NaN."""
    from unirestore_amd import f32net
    _id, name, value = run
    x, clean, want = NF.avgpool_case(name, value)
    y = f32net.avgpool_f32(CR.nhwc(x).cuda())
    assert_same_classes(y, want, CR.AVGPOOL_TOL * clean.double().abs().mean(dim=(2, 3)), run[0])
    y_clean = f32net.avgpool_f32(CR.nhwc(clean).cuda())
    ok = NF.classes(want) == NF.FINITE
    assert int((~ok).sum()) == 1 and same_bits(y.cpu()[ok], y_clean.cpu()[ok])      # every other (image, channel) keeps its bits


@pytest.mark.parametrize("value", NF.VALUE_NAMES)
@pytest.mark.parametrize("shape", NF.ADD_SHAPES, ids=["x".join(map(str, s)) for s in NF.ADD_SHAPES])
def test_add_f32_classifies_as_fp64(shape, value):
    from unirestore_amd import f32net
    a, b, want = NF.add_case(shape, value)
    y = f32net.add_f32(a.cuda(), b.cuda())
    assert_same_classes(y, want, want.abs() * 2.0 ** -24, f"add {shape} {value}")      # one fp32 rounding of the exact sum
    ok = NF.classes(want) == NF.FINITE
    assert torch.equal(y.cpu()[ok], (a + b)[ok])                         # one fp32 rounding, as torch's


@pytest.mark.parametrize("value", NF.VALUE_NAMES)
def test_broadcast_f32_classifies_as_fp64(value):
    """The pooled vector into channels 5..23 of a sentinel-filled 30-channel map: each value on every pixel of its image."""
    from unirestore_amd import f32net
    v = NF.poison(torch.randn(3, 19, generator=torch.Generator().manual_seed(19)), [((1, 7), value)])
    buf = torch.full((3, 4, 5, 30), NF.SENTINEL, device="cuda")
    assert f32net.broadcast_f32(v.cuda(), buf, 5) is buf
    want = v.double().view(3, 1, 1, 19).expand(3, 4, 5, 19)
    NF.reach_conditions(want, True)
    assert_same_classes(buf[..., 5:24], want, None, f"broadcast {value}")
    assert bool((buf[..., :5] == NF.SENTINEL).all()) and bool((buf[..., 24:] == NF.SENTINEL).all())


# ---- the table-driven resizes -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", NF.VALUE_NAMES)
@pytest.mark.parametrize("name", sorted(NF.RESIZE_NONFINITE))
def test_bilinear_resizes_classify_as_fp64(name, value):
    """Both tables, dense and into a channel slice, against `resize_tables` (the tables applied as `bilerp` documents, fp64; on
    these cases torch's own pattern but for the half-pixel resize of a 1 x 1 map: test_nonfinite_cpu.py)."""
    from unirestore_amd import capi, f32net
    table, size, x, clean, want, bound = NF.resize_case(name, value)
    xg = LR.nhwc(x).cuda()
    n, h, w_, c = xg.shape
    if table == "align_corners":
        dense = f32net.upsample_bilinear_ac_f32(xg, size)
        tabs = f32net._device_tables((h,), size[0], xg.device.index), f32net._device_tables((w_,), size[1], xg.device.index)
    else:
        dense = f32net.upsample_bilinear_hp_f32(xg, size)
        tabs = f32net._device_tables_hp(((h, size[0]),), xg.device.index), f32net._device_tables_hp(((w_, size[1]),), xg.device.index)
    assert_same_classes(LR.nchw(dense.cpu()), want, bound, f"{name} {value}")
    for channels, off in ((c + 52, 48), (c + 3, 3)):                     # float4 stores where C allows, and a misaligned slice
        buf = torch.full((n, *size, channels), NF.SENTINEL, device="cuda")
        assert f32net._upsample_bilinear("test", xg, size, *tabs, (buf, off), capi.lib.ur_dlv3_upsample_f32) is buf
        assert same_bits(buf[..., off:off + c], dense)
        assert bool((buf[..., :off] == NF.SENTINEL).all()) and bool((buf[..., off + c:] == NF.SENTINEL).all())
    # the other image keeps the clean run's bits
    dense_clean = (f32net.upsample_bilinear_ac_f32 if table == "align_corners" else f32net.upsample_bilinear_hp_f32)(LR.nhwc(clean).cuda(), size)
    for i in set(range(n)) - {NF.RESIZE_NONFINITE[name][2][0]}:
        assert same_bits(dense[i], dense_clean[i])


# ---- the metrics' own kernels -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", NF.VALUE_NAMES)
def test_lpips_prep_classifies_as_fp64(value):
    from unirestore_amd import lpips
    x = NF.poison(LR.images(NF.LPIPS_PREP_SHAPE, 3)[0], [(NF.IMAGE_POSITION, value)])
    want = LR.scale_input(x)
    NF.reach_conditions(want, True)
    assert_same_classes(LR.nchw(lpips.prep(x.cuda()).cpu()), want, LR.PREP_TOL, f"lpips prep {value}")


@pytest.mark.parametrize("name", sorted(NF.LPIPS_LAYER_CASES))
def test_lpips_layer_keeps_a_nan_in_its_own_image(name):
    """One NaN feature at one pixel of prediction 1 of 3: only image 1's row of partial sums is non-finite, the others keep the
    clean run's bits, and the tap's distance has the reference's pattern."""
    from unirestore_amd import lpips
    n, c, h, w_ = NF.LPIPS_LAYER_CASES[name]
    g = torch.Generator().manual_seed(len(name) + c)
    fp, ft = torch.relu(torch.randn(n, c, h, w_, generator=g)), torch.relu(torch.randn(n, c, h, w_, generator=g))
    lin = torch.rand(c, generator=g) / c
    bad = NF.poison(fp, [((1, c - 3, h // 2, w_ - 1), "nan")])
    want = LR.layer(bad, ft, lin)
    assert NF.classes(want).tolist() == [NF.FINITE, NF.NAN, NF.FINITE]
    part = lpips.layer(LR.nhwc(torch.cat([bad, ft])).cuda(), lin.cuda())
    part_clean = lpips.layer(LR.nhwc(torch.cat([fp, ft])).cuda(), lin.cuda())
    assert bool(torch.isfinite(part_clean).all())
    assert_same_classes(part.cpu().sum(dim=1) / (h * w_), want, LR.LAYER_TOL * LR.layer_abs(fp, ft, lin), f"lpips layer {name}")
    assert bool(torch.isnan(part[1]).any()) and same_bits(part[[0, 2]], part_clean[[0, 2]])


@pytest.mark.parametrize("value", NF.VALUE_NAMES)
def test_classify_preprocess_classifies_as_fp64(value):
    from unirestore_amd import classify
    x = NF.poison(CR.images(NF.CLASSIFY_PREP_SHAPE, 5), [(NF.IMAGE_POSITION, value)])
    want = CR.preprocess(x)
    y = classify.preprocess(x.cuda())
    assert_same_classes(CR.nchw(y.cpu()), want, CR.PREP_TOL, f"classify preprocess {value}")
    assert same_bits(y[0], classify.preprocess(CR.images(NF.CLASSIFY_PREP_SHAPE, 5).cuda())[0])


@pytest.mark.parametrize("value", NF.VALUE_NAMES)
@pytest.mark.parametrize("net", ["segment", "deeplab"])
def test_segmenter_preps_classify_as_fp64(net, value):
    """The smallest PREP_CASES entry of each network: the align_corners=True resize and the network's own arithmetic."""
    mod = importlib.import_module(f"unirestore_amd.{net}")
    R = SR if net == "segment" else DR
    shape, s = R.PREP_CASES[0]
    size = R.scaled_hw(shape[2], shape[3], s)
    x = NF.poison(R.images(shape, sum(shape)), [((0, 1, 9, 13), value)])
    want = R.prep(x, size)
    NF.reach_conditions(want, True)
    assert_same_classes(R.nchw(mod.prep(x.cuda(), size).cpu()), want, R.PREP_TOL, f"{net} prep {value}")


# ---- the whole scorers: N = 3, one NaN pixel in image 1 -----------------------------------------------------------------------

_W = {}


def _lpips_weights():
    from unirestore_amd import lpips
    if "lpips" not in _W:
        _W["lpips"] = lpips.random_weights(LR.WEIGHT_SEED)
    return _W["lpips"]


CLS = ("resnet18", 7, 200)                   # arch, weight seed, classes of CR.NET_CASES["resnet18_200_2x64x64"]


def _classifier():
    from unirestore_amd import classify
    if "cls" not in _W:
        _W["cls"] = classify.ClassifierWeights(CLS[0], CR.state_dict(*CLS[:2], CLS[2]))
    return _W["cls"]


def _segmenter(net):
    from unirestore_amd import deeplab, segment
    if net not in _W:
        _W[net] = (segment.SegmenterWeights(SR.TINY, SR.state_dict(SR.TINY, 3)) if net == "segment" else
                   deeplab.DeepLabWeights(DR.TINY, DR.state_dict(DR.TINY, 3)))
    return _W[net]


def _spliced(reference, x, bad):
    """reference(batch) of the clean batch x and of `bad`, which differs from x in image 1 only: the restatements treat every
    image on its own, so the poisoned batch's reference is the clean one with image 1 replaced."""
    clean = reference(x)
    return clean, torch.cat([clean[:1], reference(bad[1:2]), clean[2:]])


@functools.lru_cache(maxsize=None)
def _scorer_images(h, w_):
    """(clean [3,3,h,w], the same with a NaN in one pixel of image 1), on the 8-bit grid.  Callers must not modify them."""
    x = CR.varied_images(3, h, w_, 21 + w_)
    return x, NF.poison(x, [(NF.IMAGE_POSITION, "nan")])


@functools.lru_cache(maxsize=None)
def _classifier_reference(h, w_):
    """fp64 logits (clean, poisoned) of _scorer_images(h, w): preprocess + ResNet-18."""
    sd = CR.state_dict(*CLS[:2], CLS[2])
    return _spliced(lambda t: CR.resnet(CR.preprocess(t), sd, CLS[0]), *_scorer_images(h, w_))


@functools.lru_cache(maxsize=None)
def _segmenter_reference(net):
    """fp64 three-scale averaged logits (clean, poisoned) of _scorer_images(64, 96)."""
    R = SR if net == "segment" else DR
    sd = R.state_dict(R.TINY, 3)
    return _spliced(lambda t: R.tta_logits(t, sd, R.depths(R.TINY)), *_scorer_images(64, 96))


def test_lpips_of_a_poisoned_image_is_nan():
    from unirestore_amd import ops
    shape = (3, 3, 33, 47)
    pred, tgt = LR.images(shape, LR.E2E_CASES[shape])
    bad = NF.poison(pred, [(NF.IMAGE_POSITION, "nan")])
    want = LR.lpips(bad, tgt, LR.weights_cpu())
    assert NF.classes(want).tolist() == [NF.FINITE, NF.NAN, NF.FINITE] and torch.equal(want[[0, 2]], LR.e2e_reference(shape)[[0, 2]])
    out, clean = ops.lpips(bad.cuda(), tgt.cuda(), _lpips_weights()), ops.lpips(pred.cuda(), tgt.cuda(), _lpips_weights())
    assert_same_classes(out, want, LR.METRIC_TOL, "ops.lpips")
    assert bool(torch.isnan(out[1])) and same_bits(out[[0, 2]], clean[[0, 2]]) and bool(torch.isfinite(clean).all())


def test_classify_of_a_poisoned_image_is_nan():
    from unirestore_amd import ops
    x, bad = _scorer_images(64, 64)
    want_clean, want = _classifier_reference(64, 64)
    assert int((NF.classes(want[1]) == NF.NAN).sum()) >= 1 and int((NF.classes(want[[0, 2]]) != NF.FINITE).sum()) == 0
    w = _classifier()
    logits, clean = ops.classify(bad.cuda(), w), ops.classify(x.cuda(), w)
    bound = CR.LOGITS_TOL["resnet18_200_2x64x64"] * float(want_clean.abs().max())
    assert_same_classes(logits, want, bound, "ops.classify")
    assert same_bits(logits[[0, 2]], clean[[0, 2]])
    labels = torch.tensor([3, 0, 5])
    pred = ops.top1(logits, labels)[0].cpu()
    theirs = torch.argmax(want, dim=1)                                   # NaN is the maximum: the first NaN's index
    assert int(pred[1]) == int(theirs[1]) == int(torch.isnan(want[1]).nonzero()[0])
    decidable = CR.top2_gap(want_clean) > 2 * bound
    assert torch.equal(pred[[0, 2]][decidable[[0, 2]]], theirs[[0, 2]][decidable[[0, 2]]])


@pytest.mark.parametrize("net", ["segment", "deeplab"])
def test_segmenters_of_a_poisoned_image(net):
    """The three-scale averaged logits have the reference's pattern; where the reference's class vector holds a NaN the prediction
    is the index of its first NaN (torch.argmax); images 0 and 2 are byte-identical to the clean batch."""
    from unirestore_amd import ops, segment
    R = SR if net == "segment" else DR
    x, bad = _scorer_images(64, 96)
    want_clean, want = _segmenter_reference(net)
    assert int((NF.classes(want[1]) == NF.NAN).sum()) >= 1 and int((NF.classes(want[[0, 2]]) != NF.FINITE).sum()) == 0
    w = _segmenter(net)
    sizes = [(segment.scaled_size(64, s), segment.scaled_size(96, s)) for s in R.SCALES]
    maps = [w.logits(w.prep(bad.cuda(), sz)) for sz in sizes]
    pred, avg = w.tta_argmax(maps, sizes, (64, 96), want_avg=True)
    bound = R.TTA_LOGITS_TOL["tiny_2x64x96"] * float(want_clean.abs().max())
    assert_same_classes(R.nchw(avg.cpu()), want, bound, f"{net} averaged logits")
    scorer = getattr(ops, net)
    assert same_bits(scorer(bad.cuda(), w), pred)                        # the scorer is this pipeline
    has_nan = torch.isnan(want).any(dim=1)
    first_nan = torch.isnan(want).int().argmax(dim=1)
    assert int(has_nan.sum()) >= 1
    assert torch.equal(pred.cpu().long()[has_nan], first_nan[has_nan]) and torch.equal(first_nan[has_nan], want.argmax(dim=1)[has_nan])
    clean = scorer(x.cuda(), w)
    assert same_bits(pred[[0, 2]], clean[[0, 2]]) and len(set(clean.flatten().tolist())) >= 2


def test_image_metrics_of_a_poisoned_image():
    """PSNR and SSIM of image 1 have the class runner.psnr_per_image / runner.ssim give (NaN); the others keep their bits."""
    from unirestore_amd import ops, runner
    pred, tgt = LR.images((3, 3, 20, 24), 8)
    bad = NF.poison(pred, [(NF.IMAGE_POSITION, "nan")])
    want_p = runner.psnr_per_image(bad, tgt)
    want_s = torch.tensor([runner.ssim(bad[i:i + 1], tgt[i:i + 1]) for i in range(3)], dtype=torch.float64)
    assert NF.classes(want_p).tolist() == NF.classes(want_s).tolist() == [NF.FINITE, NF.NAN, NF.FINITE]
    ps, ss = ops.image_metrics(bad.cuda(), tgt.cuda())
    ps_clean, ss_clean = ops.image_metrics(pred.cuda(), tgt.cuda())
    assert_same_classes(ps, want_p, 1e-9, "psnr")                        # fp64 on both sides (test_metrics_gpu.py holds the values)
    assert_same_classes(ss, want_s, 1e-9, "ssim")
    assert same_bits(ps[[0, 2]], ps_clean[[0, 2]]) and same_bits(ss[[0, 2]], ss_clean[[0, 2]])


# ---- the evaluator ------------------------------------------------------------------------------------------------------------

class _StubModel:
    """A restoration that returns a fixed batch for every task: what the evaluator sees when the model emits a NaN."""

    def __init__(self, restored):
        self.restored = restored

    def forward_tasks(self, imgs, tasks, quantize=False):
        assert tuple(imgs.shape) == tuple(self.restored.shape)
        return {t: self.restored for t in tasks}


def test_litunifie_does_not_hide_a_nan_pixel():
    """One NaN pixel in the restored batch: val_lq/lpips is NaN, not a finite number, and the classifier's and the segmenter's
    totals are those of the fp64 reference's decisions (a NaN class vector is its first NaN's class) - on the restored side and
    on the clean input side.  The label maps ignore the pixels whose fp64 decision is within the fp32 bound of a tie."""
    from unirestore_amd import runner
    x, bad = _scorer_images(64, 96)
    stub = _StubModel(bad.cuda())
    hq = LR.images((3, 3, 64, 96), 4)[1]
    cls_clean, cls_bad = _classifier_reference(64, 96)
    cls_bound = CR.LOGITS_TOL["resnet18_200_2x64x64"] * float(cls_clean.abs().max())
    assert bool((CR.top2_gap(cls_clean) > 2 * cls_bound).all()), "choose other images: a clean image's fp64 class is within the bound of a tie"
    # image 0 is right on both sides, image 1 (all NaN: class 0) on the restored side, image 2 on neither
    labels = torch.tensor([int(cls_clean[0].argmax()), 0, (int(cls_clean[2].argmax()) + 1) % CLS[2]])
    lit = runner.LitUniFIE(model_kwargs(2), model=stub, need_crop=False, lpips_weights=_lpips_weights(), classifiers={"r18": _classifier()})
    lit.validation_step((x.cuda(), hq.cuda(), labels, ["a", "b", "c"], "ir"), tasks=["ir", "cls"])
    m = lit.metrics()
    assert m["images"] == 3 and m["val_lq/lpips"] != m["val_lq/lpips"] and m["val_lq/psnr"] != m["val_lq/psnr"] and m["val_lq/ssim"] != m["val_lq/ssim"]
    for key, ref in (("cls/r18", cls_bad), ("cls_input/r18", cls_clean)):
        want = CR.counts(torch.argmax(ref, dim=1).numpy(), labels.numpy(), CLS[2])
        assert np.array_equal(lit.totals[key].cpu().numpy(), np.stack(want)), key
    assert int(lit.totals["cls/r18"][0].sum()) == 2 and int(torch.argmax(cls_bad, dim=1)[1]) == 0

    seg_clean, seg_bad = _segmenter_reference("segment")
    seg_bound = SR.TTA_LOGITS_TOL["tiny_2x64x96"] * float(seg_clean.abs().max())
    maps = seg_clean.argmax(dim=1)                                        # the clean fp64 decision as the target ...
    maps[2] = (maps[2] + 1) % 19                                          # ... (image 2: every pixel wrong)
    maps[~SR.decidable(seg_clean, seg_bound)] = 255
    maps[~(SR.decidable(seg_bad, seg_bound) | torch.isnan(seg_bad).any(dim=1))] = 255      # (a NaN decides its pixel exactly)
    assert float((maps == 255).float().mean()) <= SR.MAX_LEFT_OUT
    lit = runner.LitUniFIE(model_kwargs(2), model=stub, need_crop=False, segmenters={"rf": _segmenter("segment")})
    lit.validation_step((x.cuda(), hq.cuda(), maps, ["a", "b", "c"], "ir"), tasks=["ir", "seg"])
    for key, ref in (("seg/rf", seg_bad), ("seg_input/rf", seg_clean)):
        want = SR.confusion(ref.argmax(dim=1).numpy(), maps.numpy())
        assert np.array_equal(lit.totals[key].cpu().numpy(), want), key
    # image 1's NaN pixels count as class 0 on the restored side: its score drops, and nothing else moves
    assert int(lit.totals["seg/rf"].trace()) < int(lit.totals["seg_input/rf"].trace()) == int((maps[:2] != 255).sum())
