"""DeepLabV3+ scoring on the GPU (ops.deeplab, unirestore_amd/deeplab.py, csrc/segment.hip and the dilated, strided-output
convolution of csrc/f32_layers.hip): every new launcher against the fp64 restatement element by element, whole networks on tiny
maps, `ops.deeplab` end to end, batch-place independence, bit-reproducibility (eager and hipGraph replay), argument checks, and
the caller path (LitUniFIE, cli.validate).  Every bound is 8 x fp32's own measured error (deeplab_reference.py: E32_* / *_TOL,
kept honest by test_deeplab_cpu.py::test_tolerances_follow_the_measured_fp32_error); copies and argmax on exact inputs are
compared for equality.  The weights are seeded stand-ins - no trained weights exist where this runs, so nothing here says
anything about any published mIoU."""
import pytest
import torch

import deeplab_reference as R
import segment_reference as SR
from tiny_cfg import TINY, model_kwargs, randomise_

pytestmark = pytest.mark.gpu

_W = {}


def _weights(arch=R.TINY, seed=3):
    """The stand-in weights of a case on the device, from the SAME state dict the fp64 restatement reads."""
    from unirestore_amd import deeplab
    if (arch, seed) not in _W:
        _W[(arch, seed)] = deeplab.DeepLabWeights(arch, R.state_dict(arch, seed))
    return _W[(arch, seed)]


# ---- the dilated convolution --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.CONV_CASES))
def test_dilated_conv_matches_fp64_elementwise(name):
    from unirestore_amd import f32net
    n, _h, _w, _cin, cout, _k, stride, pad, dil, has_res, relu = R.CONV_CASES[name]
    x, wt, b, res = R.conv_case(name)
    pc = f32net.PackedConvF32(wt, b, stride, pad, "cuda", dilation=dil)
    y = f32net.conv2d_f32(R.nhwc(x).cuda(), pc, None if res is None else R.nhwc(res).cuda(), relu=relu)
    want = R.conv(x, wt, b, stride, pad, dil, res, relu)
    assert tuple(y.shape) == (n, want.shape[2], want.shape[3], cout) and (res is not None) == has_res
    ratio = float(((R.nchw(y.cpu()).double() - want).abs() / R.conv_abs(x, wt, b, stride, pad, dil, res)).max())
    print(f"{name}: max |err| / (sum|ab| + |bias| + |res|) {ratio:.2e} (bound {R.CONV_TOL[name]:.2e})")
    assert ratio <= R.CONV_TOL[name]
    assert (float(y.min()) >= 0.0) if relu else (float(y.min()) < 0.0)


def test_conv_writes_a_channel_slice_and_nothing_else():
    """Channels 48..303 of a 304-channel buffer: the slice is the convolution, the other channels keep their bits."""
    from unirestore_amd import f32net
    n, h, w_, _cin, cout, _k, stride, pad, dil = R.SLICE_CASE
    x, wt, b = R.slice_case()
    pc = f32net.PackedConvF32(wt, b, stride, pad, "cuda", dilation=dil)
    before = torch.randn(n, h, w_, 304, generator=torch.Generator().manual_seed(3)).cuda()
    buf = before.clone()
    assert f32net.conv2d_f32(R.nhwc(x).cuda(), pc, out=(buf, 48)) is buf
    assert torch.equal(buf[..., :48], before[..., :48]) and cout == 256
    want = R.conv(x, wt, b, stride, pad, dil)
    ratio = float(((R.nchw(buf[..., 48:].cpu()).double() - want).abs() / R.conv_abs(x, wt, b, stride, pad, dil)).max())
    print(f"slice: max |err| / (sum|ab| + |bias|) {ratio:.2e} (bound {R.SLICE_TOL:.2e})")
    assert ratio <= R.SLICE_TOL
    assert torch.equal(buf[..., 48:].contiguous(), f32net.conv2d_f32(R.nhwc(x).cuda(), pc))       # the dense launch: the same bits
    # a slice in the middle leaves both sides alone
    mid = before[..., :300].contiguous()
    pc8 = f32net.PackedConvF32(wt[:8], b[:8], stride, pad, "cuda", dilation=dil)
    f32net.conv2d_f32(R.nhwc(x).cuda(), pc8, out=(mid, 7))
    assert torch.equal(mid[..., :7], before[..., :7]) and torch.equal(mid[..., 15:], before[..., 15:300])
    assert torch.equal(mid[..., 7:15], buf[..., 48:56])
    for bad in ((buf, 49), (buf, -1), (buf[:, :-1], 48), (buf.double(), 48), (buf.cpu(), 48)):
        with pytest.raises(ValueError):
            f32net.conv2d_f32(R.nhwc(x).cuda(), pc, out=bad)


@pytest.mark.parametrize("name", ["1x1_64_256_res_relu", "3x3_s2_128_128", "7x7_s2_3_64", "fc_2048_1000"])
def test_dilation_1_dense_is_conv2d_f32_res_bit_for_bit(name):
    """At the C entry points: ur_dlv3_conv2d_f32 with dil = 1 and ldy = Cout gives the bits of ur_conv2d_f32_res."""
    import classify_reference as CR
    from unirestore_amd import capi, f32net
    _n, _h, _w, _cin, _cout, _k, stride, pad, _r, relu = CR.CONV_CASES[name]
    x, wt, b, res = CR.conv_case(name)
    pc = f32net.PackedConvF32(wt, b, stride, pad, "cuda")
    xg = CR.nhwc(x).cuda()
    rg = None if res is None else CR.nhwc(res).cuda()
    n, h, w_, cin = xg.shape
    old = f32net.conv2d_f32(xg, pc, rg, relu=relu)
    new = torch.empty_like(old)
    capi.check(capi.lib.ur_dlv3_conv2d_f32(xg.data_ptr(), pc.w.data_ptr(), pc.bias.data_ptr(), None if rg is None else rg.data_ptr(),
                                           new.data_ptr(), n, h, w_, cin, pc.cout, pc.kh, pc.kw, stride, pad, 1, pc.cout, int(relu),
                                           f32net.stream()))
    assert torch.equal(old, new)


# ---- the other launchers ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.PREP_CASES, ids=[f"{'x'.join(map(str, c[0]))}@{c[1]}" for c in R.PREP_CASES])
def test_prep_matches_fp64_and_writes_nhwc_rgb(case):
    from unirestore_amd import deeplab
    shape, s = case
    x = R.images(shape, sum(shape))
    size = (deeplab.scaled_size(shape[2], s), deeplab.scaled_size(shape[3], s))
    assert size == R.scaled_hw(shape[2], shape[3], s) and (shape != (1, 3, 27, 27) or size == (16, 16))
    y = deeplab.prep(x.cuda(), size).cpu()
    assert tuple(y.shape) == (shape[0], size[0], size[1], 3) and y.dtype == torch.float32
    err = float((R.nchw(y).double() - R.prep(x, size)).abs().max())
    print(f"prep {shape} @ {s}: max |err| {err:.2e} (bound {R.PREP_TOL:.2e})")
    assert err <= R.PREP_TOL


def test_prep_at_scale_1_is_bit_exact():
    from unirestore_amd import deeplab
    x = R.images((2, 3, 37, 53), 5)
    y = deeplab.prep(x.cuda()).cpu()
    assert torch.equal(R.nchw(y), R.preprocess(x, torch.float32))


def test_broadcast_is_bit_exact():
    from unirestore_amd import deeplab
    for n, h, w_, c, call, off in ((2, 3, 5, 256, 1280, 1024), (1, 1, 1, 19, 19, 0), (3, 7, 2, 5, 12, 4)):
        g = torch.Generator().manual_seed(n + c)
        v = torch.randn(n, c, generator=g).cuda()
        before = torch.randn(n, h, w_, call, generator=g).cuda()
        buf = before.clone()
        assert deeplab.broadcast_f32(v, buf, off) is buf
        assert torch.equal(buf[..., off:off + c], v.view(n, 1, 1, c).expand(n, h, w_, c))
        assert torch.equal(buf[..., :off], before[..., :off]) and torch.equal(buf[..., off + c:], before[..., off + c:])
        # what it stands for: the half-pixel resize of a 1 x 1 map, whose two weights (they sum to 1) both fall on the one source -
        # the value itself in exact arithmetic, within a rounding of it in torch's and in the table-driven kernel
        up = deeplab.upsample_bilinear_hp_f32(v.view(n, 1, 1, c), (h, w_))
        assert float((up - buf[..., off:off + c]).abs().max() / v.abs().max()) <= R.UPSAMPLE_TOL
    with pytest.raises(ValueError):
        deeplab.broadcast_f32(v, buf, 8)


@pytest.mark.parametrize("case", R.UPSAMPLE_CASES, ids=["x".join(map(str, c)) for c in R.UPSAMPLE_CASES])
def test_half_pixel_upsample_matches_fp64(case):
    from unirestore_amd import deeplab
    n, c, _h, _w, H, W = case
    x = R.upsample_case(case)
    y = deeplab.upsample_bilinear_hp_f32(R.nhwc(x).cuda(), (H, W))
    assert tuple(y.shape) == (n, H, W, c)
    want = R.resize_hp(x, (H, W))
    err = float((R.nchw(y.cpu()).double() - want).abs().max() / x.abs().max())
    print(f"upsample {case}: max |err| / max |x| {err:.2e} (bound {R.UPSAMPLE_TOL:.2e})")
    assert err <= R.UPSAMPLE_TOL
    # into channels 48.. of a wider buffer: the same bits, the rest untouched
    before = torch.randn(n, H, W, 48 + c + 4, generator=torch.Generator().manual_seed(1)).cuda()      # C = 48: the float4 path
    buf = before.clone()
    deeplab.upsample_bilinear_hp_f32(R.nhwc(x).cuda(), (H, W), out=(buf, 48))
    assert torch.equal(buf[..., 48:48 + c], y) and torch.equal(buf[..., :48], before[..., :48]) and torch.equal(buf[..., 48 + c:], before[..., 48 + c:])


def test_half_pixel_upsample_to_the_same_size_is_the_identity():
    from unirestore_amd import deeplab
    for c in (19, 48):
        x = torch.randn(2, 5, 7, c, generator=torch.Generator().manual_seed(c)).cuda()
        assert torch.equal(deeplab.upsample_bilinear_hp_f32(x, (5, 7)), x)


@pytest.mark.parametrize("name", sorted(R.TTA_CASES))
def test_tta_argmax_matches_fp64(name):
    from unirestore_amd import deeplab
    n, c, sizes, size = R.TTA_CASES[name]
    maps, in_sizes = R.tta_case(name), [s for _q, s in sizes]
    want = R.tta_average(maps, in_sizes, size)
    scale = max(float(m.abs().max()) for m in maps)
    pred, avg = deeplab.tta_argmax([R.nhwc(m).cuda() for m in maps], in_sizes, size, want_avg=True)
    assert tuple(pred.shape) == (n, *size) and pred.dtype == torch.uint8 and tuple(avg.shape) == (n, *size, c)
    err = float((R.nchw(avg.cpu()).double() - want).abs().max())
    print(f"tta {name}: max |err| {err:.2e} = {err / scale:.2e} of max |logit| (bound {R.TTA_TOL:.2e})")
    assert err <= R.TTA_TOL * scale
    ok = R.decidable(want, R.TTA_TOL * scale)
    assert 1.0 - float(ok.float().mean()) <= R.MAX_LEFT_OUT
    assert torch.equal(pred.cpu().long()[ok], want.argmax(dim=1)[ok])
    # the prediction is the argmax of the kernel's own averaged logits everywhere, and the same without the optional output
    assert torch.equal(pred.cpu().long(), avg.cpu().argmax(dim=3))
    assert torch.equal(deeplab.tta_argmax([R.nhwc(m).cuda() for m in maps], in_sizes, size), pred)


def test_tta_argmax_ties_and_nan():
    from unirestore_amd import deeplab
    c = 19
    m = torch.zeros(1, 6, 7, c)                              # map = input = target size: both resizes are the identity
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
        pred = deeplab.tta_argmax([t.cuda() for t in maps], [(6, 7)] * len(maps), (6, 7)).cpu()
        assert {yx: int(pred[0, yx[0], yx[1]]) for yx in checked} == checked


# ---- the whole network --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.NET_CASES))
def test_logits_and_prediction_match_fp64(name):
    from unirestore_amd import deeplab, ops, segment
    arch, wseed, _iseed, n, h, w_ = R.NET_CASES[name]
    want1, want3 = R.net_reference(name)
    x = R.net_images(name)
    wts = _weights(arch, wseed)
    got = deeplab.logits(deeplab.prep(x.cuda()), wts)
    assert tuple(got.shape) == (n, h // 4, w_ // 4, 19) and got.dtype == torch.float32
    scale = float(want1.abs().max())
    err = float((R.nchw(got.cpu()).double() - want1).abs().max())
    print(f"{name}: scale-1 logits max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.1f} (bound {R.LOGITS_TOL[name]:.2e})")
    assert err <= R.LOGITS_TOL[name] * scale
    scale3 = float(want3.abs().max())
    ok = R.decidable(want3, R.TTA_LOGITS_TOL[name] * scale3)
    left_out = 1.0 - float(ok.float().mean())
    classes = sorted(set(want3.argmax(dim=1)[ok].tolist()))
    pred = ops.deeplab(x.cuda(), wts)
    assert tuple(pred.shape) == (n, h, w_) and pred.dtype == torch.uint8
    flips = int((pred.cpu().long()[ok] != want3.argmax(dim=1)[ok]).sum())
    print(f"{name}: {left_out:.4%} of the pixels left out, classes {classes}, {flips} argmax flips on the decidable ones")
    assert left_out <= R.MAX_LEFT_OUT and len(classes) >= R.MIN_CLASSES
    assert flips == 0
    # the three-scale averaged logits themselves, from the same maps the prediction was made of
    sizes = [(deeplab.scaled_size(h, s), deeplab.scaled_size(w_, s)) for s in R.SCALES]
    maps = [deeplab.logits(deeplab.prep(x.cuda(), sz), wts) for sz in sizes]
    pred2, avg = deeplab.tta_argmax(maps, sizes, (h, w_), want_avg=True)
    err3 = float((R.nchw(avg.cpu()).double() - want3).abs().max())
    print(f"{name}: averaged logits max |err| {err3 / scale3:.2e} of max |logit| {scale3:.1f} (bound {R.TTA_LOGITS_TOL[name]:.2e})")
    assert err3 <= R.TTA_LOGITS_TOL[name] * scale3 and torch.equal(pred2, pred)
    # the mIoU of the prediction against the fp64 one, through the shared confusion kernel
    conf = ops.confusion(pred, want3.argmax(dim=1).to(torch.uint8).cuda())
    miou, acc, _ = segment.miou(conf)
    assert acc >= 1.0 - R.MAX_LEFT_OUT and miou > 0.9


def test_prediction_does_not_depend_on_the_place_in_the_batch():
    from unirestore_amd import ops
    w = _weights()
    x = R.varied_images(3, 64, 80, 12).cuda()
    whole = ops.deeplab(x, w)
    assert len({bytes(whole[i].cpu().numpy().tobytes()) for i in range(3)}) == 3          # different images, different maps
    for i in range(3):
        assert torch.equal(ops.deeplab(x[i:i + 1].contiguous(), w)[0], whole[i])
        for slot in range(3):
            order = [j for j in range(3) if j != i]
            order.insert(slot, i)
            assert torch.equal(ops.deeplab(x[order].contiguous(), w)[slot], whole[i])


def test_deterministic_eager_and_graph_replay():
    from unirestore_amd import ops
    w = _weights()
    x = R.varied_images(2, 64, 80, 9).cuda()
    target = torch.randint(0, 19, (2, 64, 80), generator=torch.Generator().manual_seed(4)).to(torch.uint8).cuda()
    a = ops.deeplab(x, w)
    b = ops.deeplab(x, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.deeplab(x, w)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = ops.deeplab(x, w)
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
            ops.deeplab(bad, w)
    from unirestore_amd import segment
    rf = segment.SegmenterWeights(SR.TINY, SR.state_dict(SR.TINY, 3))
    for bad_w in (None, {"arch": "dlv3pr50"}, rf):                               # the other segmenter's weights are not these
        with pytest.raises(ValueError):
            ops.deeplab(x, bad_w)
    with pytest.raises(ValueError):
        ops.segment(x, w)                                                        # and the other way round
    with pytest.raises(ValueError, match="16"):
        ops.deeplab(x[:, :, :26].contiguous(), w)                                # 26 * 0.6 = 15.6: below the network's smallest input
    assert ops.deeplab(x[:, :, :27].contiguous(), w).shape == (2, 27, 72)
    for kw in (dict(size=(0, 4)), dict(size=5), dict(scales=()), dict(scales=(1, 0.8, 0.6, 0.4)), dict(scales=(0,))):
        with pytest.raises(ValueError):
            ops.deeplab(x, w, **kw)
    assert ops.deeplab(x, w, size=(5, 7), scales=(1,)).shape == (2, 5, 7)


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


def test_litunifie_scores_both_segmenters_and_leaves_the_rest_alone():
    from unirestore_amd import ops, runner, segment
    model = _tiny_model()
    dl = _weights()
    rf = segment.SegmenterWeights(SR.TINY, SR.state_dict(SR.TINY, 3))
    tasks = ["ir", "cls", "seg"]
    batches = []
    for b in range(2):
        hq = R.varied_images(2, 96, 80, 100 + b).cuda()
        lq = (0.6 * hq + 0.3 * R.varied_images(2, 96, 80, 200 + b).cuda()).clamp(0, 1)
        batches.append((lq, hq, _label_maps(2, 96, 80, 300 + b)))

    def run(segmenters, with_maps):
        lit = runner.LitUniFIE(model_kwargs(2), model=model, segmenters=segmenters)
        outs = []
        for b, (lq, hq, maps) in enumerate(batches):
            torch.manual_seed(40 + b)                # the forward's noise draws: the same for every instance
            outs.append(lit.validation_step((lq, hq, maps if with_maps else None, ["a", "b"], "ir"), tasks=tasks)[-1])
        return lit, lit.metrics(), outs
    lit0, m0, o0 = run(None, False)
    lit1, m1, o1 = run({"rf": rf}, True)
    lit2, m2, o2 = run({"dl": dl, "rf": rf}, True)
    for a, b in zip(o0, o2):
        assert all(torch.equal(a[t], b[t]) for t in tasks)                        # restoring does not depend on the scoring
    new = {"val_lq/dl", "val_lq/dl_acc", "val_input/dl", "val_input/dl_acc"}
    assert set(m2) == set(m1) | new and set(lit2.totals) == set(lit1.totals) | {"seg/dl", "seg_input/dl"}
    assert all(m2[k] == m1[k] for k in m1) and all(m1[k] == m0[k] for k in m0)    # every other result key is unchanged
    assert torch.equal(lit2.totals["seg/rf"], lit1.totals["seg/rf"]) and torch.equal(lit2.totals["seg_input/rf"], lit1.totals["seg_input/rf"])
    for key, side in (("seg/dl", [o["seg"] for o in o2]), ("seg_input/dl", [lq for lq, _, _ in batches])):
        tot = lit2.totals[key]
        assert tot.is_cuda and tot.dtype == torch.int64 and tuple(tot.shape) == (19, 19)
        want = sum(ops.confusion(ops.deeplab(runner.crop_tensor(img).contiguous(), dl), runner.crop_tensor(maps).contiguous().cuda())
                   for img, (_, _, maps) in zip(side, batches))
        assert torch.equal(tot, want) and int(tot.sum()) == sum(int((maps != 255).sum()) for _, _, maps in batches)
        assert not torch.equal(tot, lit2.totals[key.replace("dl", "rf")])         # two networks, two matrices
        miou, acc, _ = segment.miou(want)
        prefix = "val_lq" if key == "seg/dl" else "val_input"
        assert m2[f"{prefix}/dl"] == miou and m2[f"{prefix}/dl_acc"] == acc and 0.0 <= miou <= 1.0


def _labelled_files(tmp_path, n=2, hw=(64, 64)):
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
    return str(lst)


def test_cli_validate_deeplab(tmp_path):
    from unirestore_amd import cli, deeplab
    lst = _labelled_files(tmp_path)
    wpath = str(tmp_path / "dl.pth")
    torch.save({"model_state": deeplab.random_state_dict("dlv3pr50", 7)}, wpath)      # the published checkpoints' form
    model = _tiny_model()
    keys = {"val_lq/dl", "val_lq/dl_acc", "val_input/dl", "val_input/dl_acc"}
    cfg = dict(seed_everything=3, trainer=dict(accelerator="gpu", devices=1, precision="bf16-mixed"),
               model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=model_kwargs(2))),
               data=dict(class_path="unirestore_amd.data.ImageListFiles",
                         init_args=dict(list_file=lst, batch_size=2, labels="map", label_encoding="train_id")))
    r0 = cli.validate(cfg, tasks=["ir", "seg"], model=model)
    r1 = cli.validate(cfg, tasks=["ir", "seg"], model=model, deeplab=f"dl=dlv3pr50:{wpath}")
    print({k: r1[k] for k in sorted(keys)})
    assert set(r1) == set(r0) | keys and r1["images"] == r0["images"] == 2
    assert r1["val_lq/psnr"] == r0["val_lq/psnr"] and r1["val_lq/ssim"] == r0["val_lq/ssim"]
    assert all(0.0 <= r1[k] <= 1.0 for k in keys)
    r2 = cli.validate(cfg, tasks=["ir", "seg"], model=model, deeplab={"dl": ("dlv3pr50", wpath)}, crop="64,64")     # the images' own size
    assert {k: r2[k] for k in keys} == {k: r1[k] for k in keys}
