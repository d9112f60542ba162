"""Swin-V2 scoring on the GPU (ops.swin, unirestore_amd/swin.py, csrc/swin.hip): the fused shifted-window attention and the
residual LayerNorm against the fp64 restatement element by element, whole networks, `ops.swin` end to end, batch-place independence,
bit-reproducibility (eager and hipGraph replay), non-finite values, argument checks, and the caller path (LitUniFIE, cli.validate).
Every bound is 8 x fp32's own measured error, relative to the case's max |fp64 result| (swin_reference.py: E32_* / *_TOL, kept honest
by test_swin_cpu.py); the weights are seeded stand-ins - no trained weights exist where this runs, so nothing here says anything
about published accuracies."""
import pytest
import torch

import classify_reference as CR
import swin_reference as R

pytestmark = pytest.mark.gpu

_W = {}


def _weights(spec, seed, classes):
    """The stand-in weights of a case on the device, from the SAME state dict the fp64 restatement reads."""
    from unirestore_amd import swin
    key = (spec, seed, classes)
    if key not in _W:
        _W[key] = swin.SwinWeights(R.net_config(spec), R.state_dict(spec, seed, classes))
    return _W[key]


def _check(name, got, want, tol):
    err = R.rel_err(got.cpu(), want)
    print(f"{name}: max |err| {err:.2e} of max |fp64| {float(want.abs().max()):.3g} (bound {tol:.2e})")
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and err <= tol


def _attend(name, qkv=None):
    from unirestore_amd import swin
    case_qkv, qkv_bias, _logit_scale, bias = R.attn_case(name)
    qkv = case_qkv if qkv is None else qkv
    return swin.window_attention(qkv.cuda(), qkv_bias.cuda(), R.attn_scale(name).cuda(), bias.cuda(), R.ATTN_CASES[name][4])


# ---- the kernels ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_window_attention_matches_fp64(name):
    got = _attend(name)
    assert bool(torch.isfinite(got).all())
    _check(f"window attention {name}", got, R.attn_reference(name), R.ATTN_TOL[name])


def test_window_attention_ignores_a_checkpoints_k_bias():
    """The block of KBIAS_CASE through the loader (which zeroes the k third of qkv.bias once), the qkv Linear and the kernel."""
    from unirestore_amd import f32net, swin
    spec, wseed, pre = R.KBIAS_CASE[:3]
    x, sd, _pre, _heads = R.kbias_case()
    w = _weights(spec, wseed, 10)
    assert bool(sd[f"{pre}.attn.qkv.bias"][64:128].any())
    got = swin.window_attention(f32net.conv2d_f32(x.cuda(), w.linears[f"{pre}.attn.qkv"], relu=False), *w.attn[pre], R.KBIAS_SHIFT)
    _check("window attention, k bias in the checkpoint", got, R.kbias_reference(), R.KBIAS_TOL)
    kb = sd[f"{pre}.attn.qkv.bias"].clone()
    kb[64:128] += 1.0                                                    # another k bias in the checkpoint ...
    w2 = swin.SwinWeights(R.net_config(spec), dict(sd, **{f"{pre}.attn.qkv.bias": kb}))
    again = swin.window_attention(f32net.conv2d_f32(x.cuda(), w2.linears[f"{pre}.attn.qkv"], relu=False), *w2.attn[pre], R.KBIAS_SHIFT)
    assert torch.equal(again, got)                                       # ... the same bits


@pytest.mark.parametrize("name", list(R.LNRES_CASES))
def test_layernorm_res_matches_fp64(name):
    from unirestore_amd import f32net, swin
    x, res, gamma, beta = R.lnres_case(name)
    got = swin.layernorm_res(x.cuda(), res.cuda(), gamma.cuda(), beta.cuda())
    _check(f"layernorm_res {name}", got, R.layer_norm_res(x, res, gamma, beta), R.LNRES_TOL[name])
    ln = f32net.layernorm_f32(x.cuda(), gamma.cuda(), beta.cuda(), R.LN_EPS)
    assert torch.equal(got, res.cuda() + ln)                              # the same LayerNorm bits, then one fp32 addition
    if name == "3x7":                                                    # an unaligned view takes the scalar path: the same bits
        shifted = torch.zeros(x.numel() + 1, device="cuda")[1:].view(x.shape).copy_(x)
        assert shifted.data_ptr() % 16 == 4 and torch.equal(swin.layernorm_res(shifted, res.cuda(), gamma.cuda(), beta.cuda()), got)


def test_refusals_come_before_any_launch():
    from unirestore_amd import capi, swin
    lib, P = capi.lib, 256                                               # placeholder pointers: a refusal comes before any HIP call
    Q = P + 4096
    for args, word in (((None, P, P, P, Q, 1, 8, 8, 1, 0), "null"), ((P, None, P, P, Q, 1, 8, 8, 1, 0), "null"), ((P, P, None, P, Q, 1, 8, 8, 1, 0), "null"),
                       ((P, P, P, None, Q, 1, 8, 8, 1, 0), "null"), ((P, P, P, P, None, 1, 8, 8, 1, 0), "null"), ((P, P, P, P, P, 1, 8, 8, 1, 0), "same buffer"),
                       ((P, P, P, P, Q, 0, 8, 8, 1, 0), ">= 1"), ((P, P, P, P, Q, 1, 0, 8, 1, 0), ">= 1"), ((P, P, P, P, Q, 1, 8, -1, 1, 0), ">= 1"),
                       ((P, P, P, P, Q, 1, 8, 8, 0, 0), ">= 1"), ((P, P, P, P, Q, 1, 8, 8, 1, 2), "shift"), ((P, P, P, P, Q, 1, 8, 8, 1, 8), "shift"),
                       ((P, P, P, P, Q, 1, 8, 8, 1, -4), "shift"), ((P + 4, P, P, P, Q, 1, 8, 8, 1, 0), "aligned"), ((P, P + 4, P, P, Q, 1, 8, 8, 1, 0), "aligned"),
                       ((P, P, P, P + 8, Q, 1, 8, 8, 1, 4), "aligned"), ((P, P, P, P, Q, 1 << 16, 1 << 8, 1 << 8, 1, 0), "N*H*W"),
                       ((P, P, P, P, Q, 1 << 14, 1 << 8, 1 << 8, 1 << 12, 4), "N*windows*heads")):
        assert lib.ur_swin_attention_f32(*args, None) == capi.UR_E_INVALID and word in lib.ur_last_error().decode(), (args, lib.ur_last_error().decode())
    L = (1 << 31) - 256
    for args, word in (((None, P, P, P, Q, 1, 4, 1e-5), "null"), ((P, None, P, P, Q, 1, 4, 1e-5), "null"), ((P, P, P, P, None, 1, 4, 1e-5), "null"),
                       ((P, Q, P, P, P, 1, 4, 1e-5), "same buffer"), ((P, Q, P, P, Q, 1, 4, 1e-5), "same buffer"), ((P, P, P, P, Q, 0, 4, 1e-5), ">= 1"),
                       ((P, P, P, P, Q, 1, 0, 1e-5), ">= 1"), ((P, P, P, P, Q, L, 1, 1e-5), "below 2^31 - 256"), ((P, P, P, P, Q, 1, 4, -1.0), "eps")):
        assert lib.ur_layernorm_res_f32(*args, None) == capi.UR_E_INVALID and word in lib.ur_last_error().decode(), (args, lib.ur_last_error().decode())
    qkv, qkv_bias, _ls, bias = R.attn_case("1x8x8x1_s0")
    scale = R.attn_scale("1x8x8x1_s0")
    with pytest.raises(ValueError, match="shift"):
        swin.window_attention(qkv.cuda(), qkv_bias.cuda(), scale.cuda(), bias.cuda(), 3)
    for bad in (qkv, qkv.cuda().double(), qkv.cuda()[..., :64], qkv.cuda()[0], qkv.cuda()[:0]):
        with pytest.raises(ValueError, match="window_attention"):
            swin.window_attention(bad, qkv_bias.cuda(), scale.cuda(), bias.cuda(), 0)
    with pytest.raises(ValueError, match="bias must be"):
        swin.window_attention(qkv.cuda(), qkv_bias.cuda(), scale.cuda(), bias.cuda()[:, :32], 0)
    with pytest.raises(ValueError, match="scale must be"):
        swin.window_attention(qkv.cuda(), qkv_bias.cuda(), torch.ones(2, device="cuda"), bias.cuda(), 0)
    with pytest.raises(ValueError, match="res must be"):
        swin.layernorm_res(torch.zeros(2, 8, device="cuda"), torch.zeros(2, 4, device="cuda"), torch.ones(8, device="cuda"), torch.zeros(8, device="cuda"))


# ---- the whole network --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.NET_CASES))
def test_logits_match_fp64_and_decide_as_fp64_does(name):
    from unirestore_amd import swin
    spec, classes, wseed, _iseed, n = R.NET_CASES[name]
    want = R.net_reference(name)
    scale = float(want.abs().max())
    bound = R.LOGITS_TOL[name] * scale
    gaps = R.top2_gap(want)
    assert bool(torch.isfinite(want).all()) and float(gaps.min()) > 2 * bound          # every image is decidable: none is left out
    got = swin.logits(CR.nhwc(R.net_input(name)).cuda(), _weights(spec, wseed, classes))
    assert tuple(got.shape) == (n, classes) and got.dtype == torch.float32
    err = float((got.cpu().double() - want).abs().max())
    print(f"{name}: max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.2f} (bound {R.LOGITS_TOL[name]:.2e}); "
          f"classes {want.argmax(dim=1).tolist()}, smallest top-2 gap {float(gaps.min()):.4f}")
    assert err <= bound
    assert got.argmax(dim=1).cpu().tolist() == want.argmax(dim=1).tolist()


def test_forward_end_to_end_matches_fp64():
    """swin_v2_b, the reference's, from non-square images on the 8-bit grid."""
    from unirestore_amd import ops
    spec, classes, wseed = R.FORWARD_CASE[:3]
    want = R.forward_reference()
    n = R.FORWARD_CASE[4][0]
    scale = float(want.abs().max())
    assert float(R.top2_gap(want).min()) > 2 * R.FORWARD_TOL * scale
    got = ops.swin(R.forward_images().cuda(), _weights(spec, wseed, classes))
    err = float((got.cpu().double() - want).abs().max())
    print(f"forward {R.FORWARD_CASE[4]}: max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.2f} (bound {R.FORWARD_TOL:.2e})")
    assert tuple(got.shape) == (n, classes) and err <= R.FORWARD_TOL * scale
    assert got.argmax(dim=1).cpu().tolist() == want.argmax(dim=1).tolist()
    pred, tp, targets, predicted = ops.top1(got, want.argmax(dim=1))      # ops.top1 serves the Swin's logits as the ResNet's
    assert pred.cpu().tolist() == want.argmax(dim=1).tolist() and int(tp.sum()) == n == int(targets.sum()) == int(predicted.sum())


def _small():
    """The four-stage, 32-channel network of NET_CASES at 224 (10 classes): what the tests that need no particular network run."""
    spec, classes, wseed = R.NET_CASES["224px_e32"][:3]
    return _weights(spec, wseed, classes)


def test_logits_do_not_depend_on_the_place_in_the_batch():
    from unirestore_amd import ops
    w = _small()
    x = CR.varied_images(4, 75, 101, 12).cuda()
    whole = ops.swin(x, w)
    for i in range(4):
        assert torch.equal(ops.swin(x[i:i + 1].contiguous(), w)[0], whole[i])
        order = [j for j in range(4) if j != i]
        order.insert((i + 2) % 4, i)
        assert torch.equal(ops.swin(x[order].contiguous(), w)[(i + 2) % 4], whole[i])


def test_deterministic_eager_and_graph_replay():
    from unirestore_amd import ops
    w = _small()
    x = CR.varied_images(3, 75, 101, 9).cuda()
    a = ops.swin(x, w)
    b = ops.swin(x, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.swin(x, w)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = ops.swin(x, w)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a).all())


# ---- non-finite values ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_kernels_place_nonfinite_values_where_fp64_does(value):
    from unirestore_amd import swin
    # the residual LayerNorm: one element of row 1 of x
    x, res, gamma, beta = R.lnres_case("5x96")
    clean = swin.layernorm_res(x.cuda(), res.cuda(), gamma.cuda(), beta.cuda())
    bad = x.clone()
    bad[1, 7] = value
    got = swin.layernorm_res(bad.cuda(), res.cuda(), gamma.cuda(), beta.cuda())
    want = R.classes_of(R.layer_norm_res(bad, res, gamma, beta))
    assert bool((want[1] == 3).all()) and int((want != 0).sum()) == 96
    assert torch.equal(R.classes_of(got.cpu()), want) and torch.equal(got[[0, 2, 3, 4]], clean[[0, 2, 3, 4]])
    # window attention: one element of one query, of one key, of one V row of image 0, head 1; image 1 stays clean
    name = "2x12x12x3_s4"
    _n, _h, _w, heads, shift, _ = R.ATTN_CASES[name]
    qkv, qkv_bias, logit_scale, bias = R.attn_case(name)
    c = heads * 32
    clean = _attend(name)
    # q, k: token (9, 2), which the roll moves across the map's edge into a masked window.  v: token (6, 7), whose window has one
    # region - behind the mask a weight exp(-100 - ...) is 0 in fp32 and tiny in fp64, and 0 * inf is not tiny * inf.
    for where, col, (ty, tx) in (("q", 32 + 5, (9, 2)), ("k", c + 32 + 5, (9, 2)), ("v", 2 * c + 32 + 5, (6, 7))):
        bad = qkv.clone()
        bad[0, ty, tx, col] = value
        got = _attend(name, bad)
        want = R.classes_of(R.attention_from_qkv(bad, qkv_bias, logit_scale, bias, heads, shift))
        print(f"{where} = {value}: {int((want != 0).sum())} non-finite outputs in fp64")
        assert int((want != 0).sum()) > 0 and bool((want[1] == 0).all()) and bool((want[0, :, :, :32] == 0).all())
        assert torch.equal(R.classes_of(got.cpu()), want), where
        assert torch.equal(got[1], clean[1]) and torch.equal(got[0, :, :, :32], clean[0, :, :, :32]) and torch.equal(got[0, :, :, 64:], clean[0, :, :, 64:])


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_a_nonfinite_pixel_makes_its_image_nan_and_leaves_the_others_alone(value):
    from unirestore_amd import ops
    spec, classes, wseed = R.NET_CASES["224px_e32"][:3]
    w = _small()
    x = CR.varied_images(3, 75, 101, 21)
    clean = ops.swin(x.cuda(), w)
    bad = x.clone()
    bad[1, 2, 40, 60] = value
    want = R.swin(CR.preprocess(bad), R.state_dict(spec, wseed, classes), R.net_config(spec))
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isfinite(want[[0, 2]]).all())      # the restatement, on the host first
    got = ops.swin(bad.cuda(), w)
    assert bool(torch.isnan(got[1]).all())
    assert torch.equal(got[[0, 2]], clean[[0, 2]])


# ---- the interface ----------------------------------------------------------------------------------------------------------------

def test_ops_swin_rejects_bad_inputs():
    from unirestore_amd import classify, ops, swin
    w = _small()
    x = CR.images((2, 3, 40, 44), 1).cuda()
    for bad in (x.double(), x.half(), x.cpu(), x[0], x.transpose(2, 3), x[:, :1].contiguous(), x[:, :, :0].contiguous(), x[:0].contiguous()):
        with pytest.raises(ValueError):
            ops.swin(bad, w)
    for bad_w in (None, {"arch": "swin_v2_b"}, classify.random_weights("resnet18", 7, 10)):
        with pytest.raises(ValueError, match="swin.load_weights"):
            ops.swin(x, bad_w)
    with pytest.raises(ValueError, match="classify.load_weights"):
        ops.classify(x, w)                                               # each operator takes its own weights class
    with pytest.raises(ValueError, match="vit.load_weights"):
        ops.vit(x, w)
    assert ops.swin(x[:, :, :1, :1].contiguous(), w).shape == (2, 10)    # a 1 x 1 image is legal: the preprocess resizes it
    spec, classes, wseed = R.NET_CASES["32px_8_4"][:3]
    small = _weights(spec, wseed, classes)
    with pytest.raises(ValueError, match="configured for 32 x 32"):
        ops.swin(x, small)                                               # a 32 x 32 network behind the 224 x 224 preprocess
    with pytest.raises(ValueError, match="NHWC"):
        swin.logits(torch.zeros(1, 64, 64, 3, device="cuda"), small)


def _tiny_model():
    import unirestore_amd.modules as M
    from oracle.model import DiffUIE as ODiffUIE
    from tiny_cfg import TINY, model_kwargs, randomise_
    torch.manual_seed(0)
    o = randomise_(ODiffUIE(**model_kwargs(2), **TINY).eval(), 0)
    p = M.DiffUIE(**model_kwargs(2), **TINY).eval()
    p.load_state_dict(o.state_dict())
    return p


def test_litunifie_scores_a_resnet_a_vit_and_a_swin_side_by_side():
    import vit_reference as VR
    from tiny_cfg import model_kwargs
    from unirestore_amd import classify, ops, runner, swin, vit
    model = _tiny_model()
    wr = classify.ClassifierWeights("resnet18", CR.state_dict("resnet18", 7, 200))
    wv = vit.ViTWeights(vit.ViTConfig(*VR.TINY_224), VR.state_dict(VR.TINY_224, 5, 200))
    ws = swin.SwinWeights(swin.SwinConfig(*R.TINY_224), R.state_dict(R.TINY_224, 5, 200))
    tasks = ["ir", "cls"]
    batches = []
    for b in range(2):
        hq = CR.varied_images(3, 96, 80, 100 + b).cuda()
        batches.append(((0.6 * hq + 0.3 * CR.varied_images(3, 96, 80, 200 + b).cuda()).clamp(0, 1), hq))

    def run(classifiers, labels):
        lit = runner.LitUniFIE(model_kwargs(2), model=model, classifiers=classifiers)
        outs = []
        for b, (lq, hq) in enumerate(batches):
            torch.manual_seed(40 + b)                # the forward's noise draws: the same for every instance
            outs.append(lit.validation_step((lq, hq, labels[b], ["a", "b", "c"], "ir"), tasks=tasks)[-1])
        return lit, outs
    _lit, o0 = run(None, [None, None])
    labels = []                                      # from what the Swin says about the restored images, one of three made wrong
    for o in o0:
        pred = ops.swin(o["cls"].contiguous(), ws).argmax(dim=1)
        pred[0] = (pred[0] + 1) % 200
        labels.append(pred.cpu())
    lit1, o1 = run({"r18": wr, "vit": wv}, labels)
    lit2, o2 = run({"r18": wr, "vit": wv, "swin": ws}, labels)
    m1, m2 = lit1.metrics(), lit2.metrics()
    new = {"val_lq/swin", "val_lq/swin_top1", "val_input/swin", "val_input/swin_top1"}
    assert set(m2) == set(m1) | new and set(lit2.totals) == set(lit1.totals) | {"cls/swin", "cls_input/swin"}
    assert all(m1[k] == m2[k] for k in m1)                                   # the ResNet's and the ViT's figures do not change
    for key in ("cls/r18", "cls_input/r18", "cls/vit", "cls_input/vit"):
        assert torch.equal(lit1.totals[key], lit2.totals[key])               # nor their counts
    for key, side in (("cls/swin", [o["cls"] for o in o2]), ("cls_input/swin", [lq for lq, _ in batches])):
        tot = lit2.totals[key]
        assert tot.is_cuda and tot.dtype == torch.int64 and tuple(tot.shape) == (3, 200)
        want = sum(torch.stack(ops.top1(ops.swin(runner.crop_tensor(img).contiguous(), ws), lab)[1:]) for img, lab in zip(side, labels))
        assert torch.equal(tot, want) and int(tot[1].sum()) == 6
        prefix = "val_lq" if key == "cls/swin" else "val_input"
        assert (m2[f"{prefix}/swin"], m2[f"{prefix}/swin_top1"]) == classify.accuracy(*want)
    assert m2["val_lq/swin_top1"] == pytest.approx(4 / 6) and 0 < m2["val_lq/swin"] < 1


def test_cli_validate_swin(tmp_path):
    from PIL import Image
    from tiny_cfg import model_kwargs
    from unirestore_amd import cli, swin
    imgs = (CR.varied_images(4, 64, 64, 31) * 255).round().byte().permute(0, 2, 3, 1).numpy()
    for i in range(4):
        Image.fromarray(imgs[i]).save(str(tmp_path / f"im{i}.png"))
    lst = tmp_path / "list.txt"
    lst.write_text("".join(f"im{i}.png im{i}.png {i % 3}\n" for i in range(4)))
    ws = swin.SwinWeights(swin.SwinConfig(*R.TINY_224), R.state_dict(R.TINY_224, 5, 3))
    model = _tiny_model()

    def cfg(data):
        return dict(seed_everything=3, trainer=dict(accelerator="gpu", devices=1, precision="bf16-mixed"),
                    model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=model_kwargs(2))), data=data)
    keys = {"val_lq/s", "val_lq/s_top1", "val_input/s", "val_input/s_top1"}
    files = cfg(dict(class_path="unirestore_amd.data.ImageListFiles", init_args=dict(list_file=str(lst), batch_size=2, labels=True)))
    r0 = cli.validate(files, tasks=["ir", "cls"], model=model)
    r1 = cli.validate(files, tasks=["ir", "cls"], model=model, swin={"s": ws})
    print({k: r1[k] for k in sorted(keys)})
    assert set(r1) == set(r0) | keys and r1["images"] == r0["images"] == 4
    assert all(r1[k] == r0[k] for k in r0 if k != "images_per_s")            # without --swin the result is what it was
    assert all(0.0 <= r1[k] <= 1.0 for k in keys)
    corrupted = cfg(dict(class_path="unirestore_amd.data.CorruptedImageFiles",
                         init_args=dict(source=str(lst), corruptions="fog,contrast", severity=3, batch_size=2, seed=2, labels=True)))
    table = cli.validate(corrupted, tasks=["ir", "cls"], model=model, swin={"s": ws})["by_corruption"]
    assert len(table) == 2 and all({"s", "s_top1", "input/s", "input/s_top1", "psnr", "ssim", "images"} <= set(v) for v in table.values())
