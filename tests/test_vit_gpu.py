"""ViT scoring on the GPU (ops.vit, unirestore_amd/vit.py, csrc/vit.hip): every kernel against the fp64 restatement element by
element, whole networks, `ops.vit` end to end, batch-place independence, bit-reproducibility (eager and hipGraph replay), non-finite
values, argument checks, and the caller path (LitUniFIE, cli.validate).  Every bound is 8 x fp32's own measured error, relative to
the case's max |fp64 result| (vit_reference.py: E32_* / *_TOL, kept honest by test_vit_cpu.py); the weights are seeded stand-ins - no
trained weights exist where this runs, so nothing here says anything about published accuracies."""
import pytest
import torch

import classify_reference as CR
import vit_reference as R

pytestmark = pytest.mark.gpu

_W = {}


def _weights(spec, seed, classes):
    """The stand-in weights of a case on the device, from the SAME state dict the fp64 restatement reads."""
    from unirestore_amd import vit
    key = (spec, seed, classes)
    if key not in _W:
        _W[key] = vit.ViTWeights(R.net_config(spec), R.state_dict(spec, seed, classes))
    return _W[key]


def _check(name, got, want, tol):
    err = R.rel_err(got.cpu(), want)
    print(f"{name}: max |err| {err:.2e} of max |fp64| {float(want.abs().max()):.3g} (bound {tol:.2e})")
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and err <= tol


# ---- the kernels ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.LN_CASES))
def test_layernorm_matches_fp64(name):
    from unirestore_amd import f32net
    x, gamma, beta, eps = R.ln_case(name)
    got = f32net.layernorm_f32(x.cuda(), gamma.cuda(), beta.cuda(), eps)
    _check(f"layernorm {name}", got, R.layer_norm(x, gamma, beta, eps), R.LN_TOL[name])
    if name == "1x1":
        assert torch.equal(got.cpu(), beta.view(1, 1))                  # variance 0: the result is beta


def test_layernorm_of_the_class_token_rows():
    from unirestore_amd import f32net
    x, gamma, beta, eps = R.ln_strided_case()
    n, s, d = R.LN_STRIDED
    got = f32net.layernorm_f32(x.cuda(), gamma.cuda(), beta.cuda(), eps, first_row_of=s)
    _check("layernorm strided", got, R.layer_norm(x[:, 0], gamma, beta, eps), R.LN_STRIDED_TOL)
    assert torch.equal(got, f32net.layernorm_f32(x.cuda(), gamma.cuda(), beta.cuda(), eps)[:, 0])       # the rows the dense call gives
    # an unaligned view takes the scalar path (other partial sums in fp64: the same bound, not the same bits)
    shifted = torch.zeros(n * s * d + 1, device="cuda")[1:].view(n, s, d).copy_(x)
    assert shifted.data_ptr() % 16 == 4
    _check("layernorm strided, scalar", f32net.layernorm_f32(shifted, gamma.cuda(), beta.cuda(), eps, first_row_of=s),
           R.layer_norm(x[:, 0], gamma, beta, eps), R.LN_STRIDED_TOL)


@pytest.mark.parametrize("n", R.GELU_SIZES)
def test_gelu_matches_fp64_and_runs_in_place(n):
    from unirestore_amd import f32net
    x = R.gelu_case(n)
    want = R.gelu(x)
    dev = x.cuda()
    got = f32net.gelu_f32(dev)
    _check(f"gelu n={n}", got, want, R.GELU_TOL)
    assert torch.equal(dev.cpu(), x)                                      # the input is left alone
    same = f32net.gelu_f32(dev, inplace=True)
    assert same.data_ptr() == dev.data_ptr() and torch.equal(same, got)
    if n == 4097:                                                        # the grid, +-0 and the subnormals are all in it
        zeros = (x == 0)
        assert int(zeros.sum()) >= 2 and bool((got.cpu()[zeros] == 0).all())
        shifted = torch.zeros(n + 1, device="cuda")[1:].copy_(x)         # an unaligned pointer: the scalar path
        assert torch.equal(f32net.gelu_f32(shifted), got)


@pytest.mark.parametrize("shape", R.EMBED_CASES, ids=["x".join(map(str, s)) for s in R.EMBED_CASES])
def test_embed_is_the_fp64_sum_rounded_once(shape):
    from unirestore_amd import vit
    patches, cls, pos = R.embed_case(shape)
    got = vit.embed(patches.cuda(), cls.cuda(), pos.cuda())
    assert torch.equal(got.cpu(), R.embed(patches, cls, pos).float())      # one addition per element: exact


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attention_matches_fp64(name):
    from unirestore_amd import vit
    n, s, h, kind = R.ATTN_CASES[name]
    qkv = R.attn_case(name)
    got = vit.attention(qkv.cuda(), h)
    assert bool(torch.isfinite(got).all())
    _check(f"attention {name}", got, R.attn_reference(name), R.ATTN_TOL[name])
    if kind == "constv":                                                  # a padded key leaking into the sum would show here
        v = qkv[:, :, 2 * h * 64:]
        err = float((got.cpu().double() - v.double()).abs().max())
        print(f"constant V: max |out - v| {err:.2e}")
        assert err <= R.ATTN_TOL[name] * float(v.abs().max())


def test_attention_refusals_come_before_any_launch():
    from unirestore_amd import capi, vit
    lib, P = capi.lib, 256                                               # placeholder pointers: a refusal comes before any HIP call
    assert vit.S_MAX == R.S_MAX == lib.ur_vit_attention_s_max()
    for args, word in (((P, P + 256, 1, R.S_MAX + 1, 1, 64, 64), "S must be"), ((P, P + 256, 1, 0, 1, 64, 64), "S must be"),
                       ((P, P + 256, 1, 5, 2, 32, 64), "must be 64"), ((P, P + 256, 1, 5, 2, 64, 192), "H * d"),
                       ((None, P, 1, 5, 1, 64, 64), "null"), ((P, None, 1, 5, 1, 64, 64), "null"), ((P, P, 1, 5, 1, 64, 64), "same buffer"),
                       ((P + 4, P + 256, 1, 5, 1, 64, 64), "aligned"), ((P, P + 256, 0, 5, 1, 64, 64), ">= 1")):
        assert lib.ur_vit_attention_f32(*args, None) == capi.UR_E_INVALID and word in lib.ur_last_error().decode(), (args, lib.ur_last_error().decode())
    L = (1 << 31) - 256
    for call, word in ((lambda: lib.ur_layernorm_f32(None, P, P, P, 1, 1, 1e-6, 1, None), "null"),
                       (lambda: lib.ur_layernorm_f32(P, P, P, P + 256, 1, 8, 1e-6, 4, None), "ldx"),
                       (lambda: lib.ur_layernorm_f32(P, P, P, P + 256, L, 1, 1e-6, 1, None), "below 2^31 - 256"),
                       (lambda: lib.ur_layernorm_f32(P, P, P, P + 256, 0, 1, 1e-6, 1, None), ">= 1"),
                       (lambda: lib.ur_gelu_f32(P, P, L, None), "2^31 - 256"), (lambda: lib.ur_gelu_f32(P, None, 4, None), "null"),
                       (lambda: lib.ur_vit_embed_f32(P, P, P, P + 256, L // 8, 1, 4, None), "below 2^31 - 256"),
                       (lambda: lib.ur_vit_embed_f32(P, P, None, P + 256, 1, 1, 4, None), "null")):
        assert call() == capi.UR_E_INVALID and word in lib.ur_last_error().decode(), lib.ur_last_error().decode()
    with pytest.raises(ValueError, match="S must be"):
        vit.attention(torch.zeros(1, R.S_MAX + 1, 192, device="cuda"), 1)
    with pytest.raises(ValueError, match="H \\* d"):
        vit.attention(torch.zeros(1, 4, 192, device="cuda"), 2)


# ---- the whole network --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.NET_CASES))
def test_logits_match_fp64_and_decide_as_fp64_does(name):
    from unirestore_amd import vit
    spec, classes, wseed, _iseed, n = R.NET_CASES[name]
    want = R.net_reference(name)
    scale = float(want.abs().max())
    bound = R.LOGITS_TOL[name] * scale
    gaps = R.top2_gap(want)
    assert bool(torch.isfinite(want).all()) and float(gaps.min()) > 2 * bound          # every image is decidable: none is left out
    got = vit.logits(CR.nhwc(R.net_input(name)).cuda(), _weights(spec, wseed, classes))
    assert tuple(got.shape) == (n, classes) and got.dtype == torch.float32
    err = float((got.cpu().double() - want).abs().max())
    print(f"{name}: max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.2f} (bound {R.LOGITS_TOL[name]:.2e}); "
          f"classes {want.argmax(dim=1).tolist()}, smallest top-2 gap {float(gaps.min()):.4f}")
    assert err <= bound
    assert got.argmax(dim=1).cpu().tolist() == want.argmax(dim=1).tolist()


def test_forward_end_to_end_matches_fp64():
    from unirestore_amd import ops
    spec, classes, wseed = R.FORWARD_CASE[:3]
    want = R.forward_reference()
    scale = float(want.abs().max())
    assert float(R.top2_gap(want).min()) > 2 * R.FORWARD_TOL * scale
    got = ops.vit(R.forward_images().cuda(), _weights(spec, wseed, classes))
    err = float((got.cpu().double() - want).abs().max())
    print(f"forward {R.FORWARD_CASE[4]}: max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.2f} (bound {R.FORWARD_TOL:.2e})")
    assert tuple(got.shape) == (3, classes) and err <= R.FORWARD_TOL * scale
    assert got.argmax(dim=1).cpu().tolist() == want.argmax(dim=1).tolist()
    pred, tp, targets, predicted = ops.top1(got, want.argmax(dim=1))      # ops.top1 serves the ViT's logits as the ResNet's
    assert pred.cpu().tolist() == want.argmax(dim=1).tolist() and int(tp.sum()) == 3 == int(targets.sum()) == int(predicted.sum())


def _small():
    """The two-layer, 197-token network of NET_CASES (10 classes): what the tests that need no particular network run."""
    spec, classes, wseed = R.NET_CASES["2layer_p16_s197"][:3]
    return _weights(spec, wseed, classes)


def test_logits_do_not_depend_on_the_place_in_the_batch():
    from unirestore_amd import ops
    w = _small()
    x = CR.varied_images(4, 75, 101, 12).cuda()
    whole = ops.vit(x, w)
    for i in range(4):
        assert torch.equal(ops.vit(x[i:i + 1].contiguous(), w)[0], whole[i])
        order = [j for j in range(4) if j != i]
        order.insert((i + 2) % 4, i)
        assert torch.equal(ops.vit(x[order].contiguous(), w)[(i + 2) % 4], whole[i])


def test_deterministic_eager_and_graph_replay():
    from unirestore_amd import ops
    w = _small()
    x = CR.varied_images(3, 75, 101, 9).cuda()
    a = ops.vit(x, w)
    b = ops.vit(x, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.vit(x, w)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = ops.vit(x, w)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a).all())


# ---- non-finite values ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_kernels_place_nonfinite_values_where_fp64_does(value):
    from unirestore_amd import f32net, vit
    # LayerNorm: one element of row 1
    x, gamma, beta, eps = R.ln_case("5x64")
    clean = f32net.layernorm_f32(x.cuda(), gamma.cuda(), beta.cuda(), eps)
    bad = x.clone()
    bad[1, 7] = value
    got = f32net.layernorm_f32(bad.cuda(), gamma.cuda(), beta.cuda(), eps)
    want = R.classes_of(R.layer_norm(bad, gamma, beta, eps))
    assert bool((want[1] == 3).all()) and int((want != 0).sum()) == 64           # the row is all NaN, as F.layer_norm
    assert torch.equal(R.classes_of(got.cpu()), want) and torch.equal(got[[0, 2, 3, 4]], clean[[0, 2, 3, 4]])
    # GELU
    x = torch.tensor([1.5, value, -0.25, 2.0, -3.0])
    want = R.classes_of(R.gelu(x))
    assert int(want[1]) == (1 if value == float("inf") else 3)                   # NaN -> NaN, +inf -> +inf, -inf -> NaN
    assert torch.equal(R.classes_of(f32net.gelu_f32(x.cuda()).cpu()), want)
    # attention: one element of one query, of one key, of one V row; image 1 stays clean
    qkv = R.attn_case("2x33x3")
    h, d = 3, 192
    clean = vit.attention(qkv.cuda(), h)
    for where, col in (("q", 64 + 5), ("k", d + 64 + 5), ("v", 2 * d + 64 + 5)):      # head 1, dimension 5
        bad = qkv.clone()
        bad[0, 32, col] = value                                                  # the last token: the second key tile's only real key
        got = vit.attention(bad.cuda(), h)
        want = R.classes_of(R.attention(bad, h))
        print(f"{where} = {value}: {int((want != 0).sum())} non-finite outputs in fp64")
        assert int((want != 0).sum()) > 0 and bool((want[1] == 0).all()) and bool((want[0, :, :64] == 0).all())
        assert torch.equal(R.classes_of(got.cpu()), want), where
        assert torch.equal(got[1], clean[1]) and torch.equal(got[0, :, :64], clean[0, :, :64]) and torch.equal(got[0, :, 128:], clean[0, :, 128:])
        if where == "v" and value != value:
            assert bool((want[0, :, 64 + 5] == 3).all())                         # a NaN in V reaches every query of the head


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_a_nonfinite_pixel_makes_its_image_nan_and_leaves_the_others_alone(value):
    from unirestore_amd import ops
    spec, classes, wseed = R.NET_CASES["2layer_p16_s197"][:3]
    w = _small()
    x = CR.varied_images(3, 75, 101, 21)
    clean = ops.vit(x.cuda(), w)
    bad = x.clone()
    bad[1, 2, 40, 60] = value
    want = R.vit(CR.preprocess(bad), R.state_dict(spec, wseed, classes), R.net_config(spec))
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isfinite(want[[0, 2]]).all())      # the restatement, on the host first
    got = ops.vit(bad.cuda(), w)
    assert bool(torch.isnan(got[1]).all())
    assert torch.equal(got[[0, 2]], clean[[0, 2]])


# ---- the interface ----------------------------------------------------------------------------------------------------------------

def test_ops_vit_rejects_bad_inputs():
    from unirestore_amd import classify, ops, vit
    w = _small()
    x = CR.images((2, 3, 40, 44), 1).cuda()
    for bad in (x.double(), x.half(), x.cpu(), x[0], x.transpose(2, 3), x[:, :1].contiguous(), x[:, :, :0].contiguous(), x[:0].contiguous()):
        with pytest.raises(ValueError):
            ops.vit(bad, w)
    for bad_w in (None, {"arch": "vit_b_16"}, classify.random_weights("resnet18", 7, 10)):
        with pytest.raises(ValueError, match="vit.load_weights"):
            ops.vit(x, bad_w)
    with pytest.raises(ValueError, match="classify.load_weights"):
        ops.classify(x, w)                                               # each operator takes its own weights class
    assert ops.vit(x[:, :, :1, :1].contiguous(), w).shape == (2, 10)     # a 1 x 1 image is legal: the preprocess resizes it
    spec, classes, wseed = R.NET_CASES["1layer_32px_s5"][:3]
    small = _weights(spec, wseed, classes)
    with pytest.raises(ValueError, match="interpolat"):
        ops.vit(x, small)                                                # a 32 x 32 network behind the 224 x 224 preprocess
    with pytest.raises(ValueError, match="interpolat"):
        vit.logits(torch.zeros(1, 64, 64, 3, device="cuda"), small)


def _tiny_model():
    import unirestore_amd.modules as M
    from oracle.model import DiffUIE as ODiffUIE
    from tiny_cfg import TINY, model_kwargs, randomise_
    torch.manual_seed(0)
    o = randomise_(ODiffUIE(**model_kwargs(2), **TINY).eval(), 0)
    p = M.DiffUIE(**model_kwargs(2), **TINY).eval()
    p.load_state_dict(o.state_dict())
    return p


def test_litunifie_scores_a_resnet_and_a_vit_side_by_side():
    from tiny_cfg import model_kwargs
    from unirestore_amd import classify, ops, runner, vit
    model = _tiny_model()
    wr = classify.ClassifierWeights("resnet18", CR.state_dict("resnet18", 7, 200))
    wv = vit.ViTWeights(vit.ViTConfig(*R.TINY_224), R.state_dict(R.TINY_224, 5, 200))
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
    labels = []                                      # from what the ViT says about the restored images, one of three made wrong
    for o in o0:
        pred = ops.vit(o["cls"].contiguous(), wv).argmax(dim=1)
        pred[0] = (pred[0] + 1) % 200
        labels.append(pred.cpu())
    lit1, o1 = run({"r18": wr}, labels)
    lit2, o2 = run({"r18": wr, "vit": wv}, labels)
    m1, m2 = lit1.metrics(), lit2.metrics()
    new = {"val_lq/vit", "val_lq/vit_top1", "val_input/vit", "val_input/vit_top1"}
    assert set(m2) == set(m1) | new and set(lit2.totals) == set(lit1.totals) | {"cls/vit", "cls_input/vit"}
    assert all(m1[k] == m2[k] for k in m1)                                   # the ResNet's figures do not change
    for key in ("cls/r18", "cls_input/r18"):
        assert torch.equal(lit1.totals[key], lit2.totals[key])               # nor its counts
    for key, side in (("cls/vit", [o["cls"] for o in o2]), ("cls_input/vit", [lq for lq, _ in batches])):
        tot = lit2.totals[key]
        assert tot.is_cuda and tot.dtype == torch.int64 and tuple(tot.shape) == (3, 200)
        want = sum(torch.stack(ops.top1(ops.vit(runner.crop_tensor(img).contiguous(), wv), lab)[1:]) for img, lab in zip(side, labels))
        assert torch.equal(tot, want) and int(tot[1].sum()) == 6
        prefix = "val_lq" if key == "cls/vit" else "val_input"
        assert (m2[f"{prefix}/vit"], m2[f"{prefix}/vit_top1"]) == classify.accuracy(*want)
    assert m2["val_lq/vit_top1"] == pytest.approx(4 / 6) and 0 < m2["val_lq/vit"] < 1


def test_cli_validate_vit(tmp_path):
    from PIL import Image
    from tiny_cfg import model_kwargs
    from unirestore_amd import cli, vit
    imgs = (CR.varied_images(4, 64, 64, 31) * 255).round().byte().permute(0, 2, 3, 1).numpy()
    for i in range(4):
        Image.fromarray(imgs[i]).save(str(tmp_path / f"im{i}.png"))
    lst = tmp_path / "list.txt"
    lst.write_text("".join(f"im{i}.png im{i}.png {i % 3}\n" for i in range(4)))
    wv = vit.ViTWeights(vit.ViTConfig(*R.TINY_224), R.state_dict(R.TINY_224, 5, 3))
    model = _tiny_model()

    def cfg(data):
        return dict(seed_everything=3, trainer=dict(accelerator="gpu", devices=1, precision="bf16-mixed"),
                    model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=model_kwargs(2))), data=data)
    keys = {"val_lq/v", "val_lq/v_top1", "val_input/v", "val_input/v_top1"}
    files = cfg(dict(class_path="unirestore_amd.data.ImageListFiles", init_args=dict(list_file=str(lst), batch_size=2, labels=True)))
    r0 = cli.validate(files, tasks=["ir", "cls"], model=model)
    r1 = cli.validate(files, tasks=["ir", "cls"], model=model, vit={"v": wv})
    print({k: r1[k] for k in sorted(keys)})
    assert set(r1) == set(r0) | keys and r1["images"] == r0["images"] == 4
    assert all(r1[k] == r0[k] for k in r0 if k != "images_per_s")            # without --vit the result is what it was
    assert all(0.0 <= r1[k] <= 1.0 for k in keys)
    corrupted = cfg(dict(class_path="unirestore_amd.data.CorruptedImageFiles",
                         init_args=dict(source=str(lst), corruptions="fog,contrast", severity=3, batch_size=2, seed=2, labels=True)))
    table = cli.validate(corrupted, tasks=["ir", "cls"], model=model, vit={"v": wv})["by_corruption"]
    assert len(table) == 2 and all({"v", "v_top1", "input/v", "input/v_top1", "psnr", "ssim", "images"} <= set(v) for v in table.values())
