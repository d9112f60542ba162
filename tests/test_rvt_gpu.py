"""RVT scoring on the GPU (ops.rvt, unirestore_amd/rvt.py, csrc/rvt.hip): the gated attention and the depthwise convolution against
the fp64 restatement element by element, whole networks against the reference module's own stored logits, `ops.rvt` end to end,
batch-place independence, bit-reproducibility (eager and hipGraph replay), non-finite values, argument checks, and the caller path
(LitUniFIE, cli.validate).  Every bound is 8 x fp32's own measured error, relative to the case's max |fp64 result|
(rvt_reference.py: E32_* / *_TOL, kept honest by test_rvt_cpu.py); the weights are seeded stand-ins - no trained weights exist
where this runs, so nothing here says anything about published accuracies."""
import pytest
import torch

import classify_reference as CR
import rvt_reference as R

pytestmark = pytest.mark.gpu

_W = {}


def _weights(spec, seed, classes):
    """The stand-in weights of a case on the device, from the SAME state dict the fp64 restatement reads."""
    from unirestore_amd import rvt
    key = (spec, seed, classes)
    if key not in _W:
        _W[key] = rvt.RVTWeights(R.net_config(spec), R.state_dict(spec, seed, classes))
    return _W[key]


def _small():
    spec, classes, wseed = R.NET_CASES[R.SMALL][:3]
    return _weights(spec, wseed, classes)


def _check(name, got, want, tol):
    err = R.rel_err(got.cpu(), want)
    print(f"{name}: max |err| {err:.2e} of max |fp64| {float(want.abs().max()):.3g} (bound {tol:.2e})")
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and err <= tol


# ---- the kernels ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attention_matches_fp64(name):
    from unirestore_amd import rvt
    qkv, gate = R.attn_case(name)
    got = rvt.attention(qkv.cuda(), R.ATTN_CASES[name][1], None if gate is None else gate.cuda())
    assert bool(torch.isfinite(got).all())
    _check(f"attention {name}", got, R.attn_reference(name), R.ATTN_TOL[name])


def test_attention_with_a_gate_of_zeros_and_ones():
    from unirestore_amd import rvt
    qkv, gate = R.gate01_case()
    heads = R.ATTN_CASES[R.GATE01_CASE][1]
    got = rvt.attention(qkv.cuda(), heads, gate.cuda())
    _check("attention, 0 / 1 gate", got, R.gate01_reference(), R.GATE01_TOL)
    ones = rvt.attention(qkv.cuda(), heads, torch.ones_like(gate).cuda())      # a gate of ones is one exact multiplication by 1
    assert torch.equal(ones, rvt.attention(qkv.cuda(), heads))
    unaligned = torch.zeros(gate.numel() + 1, device="cuda")[1:].view(gate.shape).copy_(gate)      # the scalar gate path: the same bits
    assert unaligned.data_ptr() % 16 == 4 and torch.equal(rvt.attention(qkv.cuda(), heads, unaligned), got)


@pytest.mark.parametrize("s,heads", R.VIT_EQUAL_CASES)
def test_ungated_attention_at_d64_is_the_vit_kernels_bit_for_bit(s, heads):
    from unirestore_amd import rvt, vit
    qkv = torch.randn(2, s, 3 * heads * 64, generator=torch.Generator().manual_seed(s)).cuda()
    assert torch.equal(rvt.attention(qkv, heads, None), vit.attention(qkv, heads))


def _dw(name, x=None, act=None):
    from unirestore_amd import rvt
    cx, w, b = R.dw_case(name)
    _h, _w, _c, mult, stride, case_act = R.DW_CASES[name]
    x = CR.nhwc(cx).contiguous().cuda() if x is None else x
    return rvt.dwconv3x3(x, rvt.pack_dw_weight(w).cuda(), b.cuda(), mult, stride, gelu=bool(case_act if act is None else act))


@pytest.mark.parametrize("name", list(R.DW_CASES))
def test_dwconv_matches_fp64(name):
    from unirestore_amd import f32net
    got = _dw(name)
    _check(f"dwconv {name}", got, R.dw_reference(name), R.DW_TOL[name])
    if R.DW_CASES[name][5]:                                                # the fused GELU: the bits of the convolution, then gelu_f32
        assert torch.equal(got, f32net.gelu_f32(_dw(name, act=0)))
    x = CR.nhwc(R.dw_case(name)[0]).contiguous()
    shifted = torch.zeros(x.numel() + 1, device="cuda")[1:].view(x.shape).copy_(x)      # an unaligned view: the scalar path, the same bits
    assert shifted.data_ptr() % 16 == 4 and torch.equal(_dw(name, shifted), got)


def test_refusals_come_before_any_launch():
    from unirestore_amd import capi, rvt
    lib, P = capi.lib, 4096                                              # placeholder pointers: a refusal comes before any HIP call
    Q, G = P + (1 << 20), P + (1 << 21)
    for args, word in (((None, G, Q, 1, 8, 1, 32), "null"), ((P, G, None, 1, 8, 1, 32), "null"), ((P, G, P, 1, 8, 1, 32), "overlap qkv"),
                       ((P, G, P + 64, 1, 8, 1, 32), "overlap qkv"), ((P, Q, Q, 1, 8, 1, 32), "overlap gate"), ((P, Q - 4, Q, 1, 8, 1, 32), "overlap gate"),
                       ((P, G, Q, 1, 8, 1, 16), "32 or 64"), ((P, G, Q, 1, 8, 1, 48), "32 or 64"), ((P, G, Q, 1, 8, 1, 0), "32 or 64"),
                       ((P, G, Q, 0, 8, 1, 32), ">= 1"), ((P, G, Q, 1, 8, 0, 64), ">= 1"), ((P, G, Q, 1, 0, 1, 32), "S must be"),
                       ((P, G, Q, 1, 257, 1, 64), "S must be"), ((P, G, Q, 1, -3, 1, 64), "S must be"), ((P + 4, G, Q, 1, 8, 1, 32), "16-byte"),
                       ((P, G + 2, Q, 1, 8, 1, 32), "4-byte"), ((P, G, Q + 1, 1, 8, 1, 32), "4-byte"), ((P, None, Q, 1 << 12, 8, 1 << 11, 64), "N*H")):
        assert lib.ur_rvt_attention_f32(*args, None) == capi.UR_E_INVALID and word in lib.ur_last_error().decode(), (args, lib.ur_last_error().decode())
    X, W, B, Y = P, P + (1 << 24), P + (1 << 25), P + (1 << 26)
    for args, word in (((None, W, B, Y, 1, 4, 4, 8, 1, 1, 0), "null"), ((X, None, B, Y, 1, 4, 4, 8, 1, 1, 0), "null"), ((X, W, None, Y, 1, 4, 4, 8, 1, 1, 0), "null"),
                       ((X, W, B, None, 1, 4, 4, 8, 1, 1, 0), "null"), ((X, W, B, X, 1, 4, 4, 8, 1, 1, 0), "overlap"), ((X, W, B, X + 64, 1, 4, 4, 8, 1, 1, 0), "overlap"),
                       ((X, W, B, W + 32, 1, 4, 4, 8, 1, 1, 0), "overlap"), ((X, W, B, B, 1, 4, 4, 8, 1, 1, 0), "overlap"),
                       ((X, W, B, Y, 0, 4, 4, 8, 1, 1, 0), ">= 1"), ((X, W, B, Y, 1, 0, 4, 8, 1, 1, 0), ">= 1"), ((X, W, B, Y, 1, 4, -1, 8, 1, 1, 0), ">= 1"),
                       ((X, W, B, Y, 1, 4, 4, 0, 1, 1, 0), ">= 1"), ((X, W, B, Y, 1, 4, 4, 8, 0, 1, 0), "mult"), ((X, W, B, Y, 1, 4, 4, 8, -2, 1, 0), "mult"),
                       ((X, W, B, Y, 1, 4, 4, 8, 1, 0, 0), "stride"), ((X, W, B, Y, 1, 4, 4, 8, 1, 3, 0), "stride"), ((X, W, B, Y, 1, 4, 4, 8, 1, 1, 2), "act"),
                       ((X + 2, W, B, Y, 1, 4, 4, 8, 1, 1, 0), "4-byte"), ((X, W, B, Y + 1, 1, 4, 4, 8, 1, 1, 0), "4-byte"),
                       ((X, W, B, Y, 1 << 10, 1 << 10, 1 << 10, 2, 1, 2, 0), "below 2^31 - 256"),            # the input alone is too large
                       ((X, W, B, Y, 1, 1 << 10, 1 << 10, 1 << 10, 4, 1, 0), "below 2^31 - 256")):           # the output alone
        assert lib.ur_dwconv3x3_f32(*args, None) == capi.UR_E_INVALID and word in lib.ur_last_error().decode(), (args, lib.ur_last_error().decode())
    qkv, gate = (t.cuda() for t in R.attn_case("S33_H3_d32_g"))
    for bad in (qkv.cpu(), qkv.double(), qkv[..., :90], qkv[0], qkv[:0], qkv[:, :, :96].contiguous()):      # (the last: D = 32 is no multiple of 3 heads)
        with pytest.raises(ValueError, match="rvt.attention"):
            rvt.attention(bad, 3, None)
    with pytest.raises(ValueError, match="32 or 64"):
        rvt.attention(qkv, 2, None)                                      # d = 48
    for bad in (gate[:2], gate.double(), gate.cpu(), gate.transpose(1, 2), gate[:, :, :32]):
        with pytest.raises(ValueError, match="gate must be"):
            rvt.attention(qkv, 3, bad)
    x = torch.zeros(1, 4, 4, 8, device="cuda")
    w, b = torch.zeros(9, 8, device="cuda"), torch.zeros(8, device="cuda")
    for bad in (x.cpu(), x.double(), x[0], x[:0], x[..., :6]):
        with pytest.raises(ValueError, match="rvt.dwconv3x3"):
            rvt.dwconv3x3(bad, w, b)
    for kw in (dict(mult=0), dict(mult=1.5), dict(stride=3), dict(mult=2)):                  # (mult = 2 needs w (9, 16))
        with pytest.raises(ValueError, match="rvt.dwconv3x3"):
            rvt.dwconv3x3(x, w, b, **kw)
    with pytest.raises(ValueError, match="rvt.dwconv3x3"):
        rvt.dwconv3x3(x, w.t().contiguous(), b)


# ---- the whole network --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.NET_CASES))
def test_logits_match_fp64_and_decide_as_fp64_does(name):
    """The golden networks against the logits the reference's own PoolingTransformer computed (tests/golden/rvt_0.npz), the others
    against the restatement."""
    from unirestore_amd import rvt
    spec, classes, wseed, _iseed, n = R.NET_CASES[name]
    want = R.golden_logits(name) if name in R.GOLDEN_CASES else R.net_reference(name)
    scale = float(want.abs().max())
    bound = R.LOGITS_TOL[name] * scale
    gaps = R.top2_gap(want)
    assert bool(torch.isfinite(want).all()) and float(gaps.min()) > 2 * bound          # every image is decidable: none is left out
    got = rvt.logits(CR.nhwc(R.net_input(name)).contiguous().cuda(), _weights(spec, wseed, classes))
    assert tuple(got.shape) == (n, classes) and got.dtype == torch.float32
    err = float((got.cpu().double() - want).abs().max())
    print(f"{name}: max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.2f} (bound {R.LOGITS_TOL[name]:.2e}); "
          f"classes {want.argmax(dim=1).tolist()}, smallest top-2 gap {float(gaps.min()):.4f}")
    assert err <= bound
    assert got.argmax(dim=1).cpu().tolist() == want.argmax(dim=1).tolist()
    one = rvt.logits(CR.nhwc(R.net_input(name))[:1].contiguous().cuda(), _weights(spec, wseed, classes))
    assert tuple(one.shape) == (1, classes) and torch.equal(one[0], got[0])            # the batch axis stays at N = 1


@pytest.mark.parametrize("shape", R.FORWARD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_end_to_end_matches_fp64(shape):
    from unirestore_amd import ops
    want = R.forward_reference(shape)
    scale = float(want.abs().max())
    tol = R.FORWARD_TOL[shape]
    assert float(R.top2_gap(want).min()) > 2 * tol * scale
    got = ops.rvt(R.forward_images(shape).cuda(), _small())
    err = float((got.cpu().double() - want).abs().max())
    print(f"forward {shape}: max |err| {err:.2e} = {err / scale:.2e} of max |logit| {scale:.2f} (bound {tol:.2e})")
    assert tuple(got.shape) == (shape[0], 10) and err <= tol * scale
    assert got.argmax(dim=1).cpu().tolist() == want.argmax(dim=1).tolist()
    pred, tp, targets, predicted = ops.top1(got, want.argmax(dim=1))      # ops.top1 serves the RVT's logits as the ResNet's
    assert pred.cpu().tolist() == want.argmax(dim=1).tolist() and int(tp.sum()) == shape[0] == int(targets.sum()) == int(predicted.sum())


@pytest.mark.parametrize("shape", R.FORWARD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_logits_do_not_depend_on_the_place_in_the_batch(shape):
    from unirestore_amd import ops
    w = _small()
    x = CR.varied_images(4, shape[2], shape[3], 12).cuda()
    whole = ops.rvt(x, w)
    for i in range(4):
        assert torch.equal(ops.rvt(x[i:i + 1].contiguous(), w)[0], whole[i])
        order = [j for j in range(4) if j != i]
        order.insert((i + 2) % 4, i)
        assert torch.equal(ops.rvt(x[order].contiguous(), w)[(i + 2) % 4], whole[i])


@pytest.mark.parametrize("shape", R.FORWARD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_deterministic_eager_and_graph_replay(shape):
    from unirestore_amd import ops
    w = _small()
    x = CR.varied_images(3, shape[2], shape[3], 9).cuda()
    a = ops.rvt(x, w)
    b = ops.rvt(x, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.rvt(x, w)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = ops.rvt(x, w)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a).all())


# ---- non-finite values ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_kernels_place_nonfinite_values_where_fp64_does(value):
    from unirestore_amd import rvt
    # attention: one element of one query, of one key, of one V row of image 0, head 1; image 1 and the other heads stay clean
    name = "S49_H3_d32_g"
    _s, heads, d, _g = R.ATTN_CASES[name]
    qkv, gate = R.attn_case(name)
    c = heads * d
    clean = rvt.attention(qkv.cuda(), heads, gate.cuda())
    for where, col in (("q", d + 5), ("k", c + d + 5), ("v", 2 * c + d + 5)):
        bad = qkv.clone()
        bad[0, 17, col] = value
        got = rvt.attention(bad.cuda(), heads, gate.cuda())
        want = R.classes_of(R.attention(bad, heads, gate))
        print(f"{where} = {value}: {int((want != 0).sum())} non-finite outputs in fp64")
        assert int((want != 0).sum()) > 0 and bool((want[1] == 0).all()) and bool((want[0, :, :d] == 0).all())
        assert torch.equal(R.classes_of(got.cpu()), want), where
        assert torch.equal(got[1], clean[1]) and torch.equal(got[0, :, :d], clean[0, :, :d]) and torch.equal(got[0, :, 2 * d:], clean[0, :, 2 * d:])
    # a gate of exactly 0 against an infinite score is NaN, as in torch (not a masked key)
    bad, zero = qkv.clone(), gate.clone()
    bad[0, 17, c + d + 5] = value
    zero[1, :, 17] = 0
    got = rvt.attention(bad.cuda(), heads, zero.cuda())
    want = R.classes_of(R.attention(bad, heads, zero))
    assert int((want == 3).sum()) > 0 and torch.equal(R.classes_of(got.cpu()), want)
    # the depthwise convolution: the value reaches exactly the outputs whose window holds it, of its own channel's outputs
    for dname in ("7x7_C6_m2s2_gelu", "7x7_C64_m1s1", "14x14_C64_m1s2_gelu"):
        x, w, b = R.dw_case(dname)
        stride, act = R.DW_CASES[dname][4:]
        clean = _dw(dname)
        bad = x.clone()
        bad[1, 3, 0, 2] = value                                          # on the top border: the padded taps above it must not spread it
        got = _dw(dname, CR.nhwc(bad).contiguous().cuda())
        want = R.classes_of(CR.nhwc(R.dwconv(bad, w, b, stride, act)))
        hit = want != 0
        assert 0 < int(hit.sum()) <= 6 * R.DW_CASES[dname][3] and not bool(hit[0].any())
        assert torch.equal(R.classes_of(got.cpu()), want) and torch.equal(got[~hit.cuda()], clean[~hit.cuda()])


@pytest.mark.parametrize("shape", R.FORWARD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_a_nonfinite_pixel_makes_its_image_nan_and_leaves_the_others_alone(value, shape):
    from unirestore_amd import ops
    spec, classes, wseed = R.NET_CASES[R.SMALL][:3]
    w = _small()
    x = CR.varied_images(3, shape[2], shape[3], 21)
    clean = ops.rvt(x.cuda(), w)
    bad = x.clone()
    bad[1, 2, shape[2] // 2, shape[3] // 2] = value
    want = R.rvt(CR.preprocess(bad), R.state_dict(spec, wseed, classes), spec)
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isfinite(want[[0, 2]]).all())      # the restatement, on the host first
    got = ops.rvt(bad.cuda(), w)
    assert bool(torch.isnan(got[1]).all())
    assert torch.equal(got[[0, 2]], clean[[0, 2]])


# ---- the interface ----------------------------------------------------------------------------------------------------------------

def test_ops_rvt_rejects_bad_inputs():
    from unirestore_amd import classify, ops, rvt
    w = _small()
    x = CR.images((2, 3, 40, 44), 1).cuda()
    for bad in (x.double(), x.half(), x.cpu(), x[0], x.transpose(2, 3), x[:, :1].contiguous(), x[:, :, :0].contiguous(), x[:0].contiguous()):
        with pytest.raises(ValueError):
            ops.rvt(bad, w)
    for bad_w in (None, {"arch": "rvt_tiny"}, classify.random_weights("resnet18", 7, 10)):
        with pytest.raises(ValueError, match="rvt.load_weights"):
            ops.rvt(x, bad_w)
    with pytest.raises(ValueError, match="classify.load_weights"):
        ops.classify(x, w)                                               # each operator takes its own weights class
    with pytest.raises(ValueError, match="swin.load_weights"):
        ops.swin(x, w)
    assert ops.rvt(x[:, :, :1, :1].contiguous(), w).shape == (2, 10)     # a 1 x 1 image is legal: the preprocess resizes it
    other = rvt.random_weights(rvt.RVTConfig(96, (32,), (1,), (2,), 4, False, None), 1, 10)
    with pytest.raises(ValueError, match="configured for 96 x 96"):
        ops.rvt(x, other)                                                # a 96 x 96 network behind the 224 x 224 preprocess
    with pytest.raises(ValueError, match="NHWC"):
        rvt.logits(torch.zeros(1, 64, 64, 3, device="cuda"), other)
    assert rvt.logits(torch.zeros(1, 96, 96, 3, device="cuda"), other).shape == (1, 10)      # 6 x 6 = 36 tokens, ungated


def _tiny_model():
    import unirestore_amd.modules as M
    from oracle.model import DiffUIE as ODiffUIE
    from tiny_cfg import TINY, model_kwargs, randomise_
    torch.manual_seed(0)
    o = randomise_(ODiffUIE(**model_kwargs(2), **TINY).eval(), 0)
    p = M.DiffUIE(**model_kwargs(2), **TINY).eval()
    p.load_state_dict(o.state_dict())
    return p


def test_litunifie_and_cli_validate_score_an_rvt_from_a_checkpoint(tmp_path):
    """The caller path with a full architecture loaded from a file in the published wrapping: LitUniFIE(classifiers={"rvt":
    ("rvt_tiny_plus", path)}) and cli.validate(rvt=...) on a tiny labelled list."""
    from PIL import Image
    from tiny_cfg import model_kwargs
    from unirestore_amd import classify, cli, ops, runner, rvt
    path = str(tmp_path / "rvt_ti_plus.pth")
    torch.save({"model": rvt.random_state_dict(R.CALLER_ARCH, 5, 3)}, path)
    model = _tiny_model()
    lit = runner.LitUniFIE(model_kwargs(2), model=model, classifiers={"rvt": (R.CALLER_ARCH, path)})
    ws = lit.classifiers["rvt"]
    assert isinstance(ws, rvt.RVTWeights) and ws.arch == R.CALLER_ARCH and ws.num_classes == 3 and len(ws.gates) == 10 and len(ws.blocks) == 12
    hq = CR.varied_images(3, 96, 80, 100).cuda()
    lq = (0.6 * hq + 0.3 * CR.varied_images(3, 96, 80, 200).cuda()).clamp(0, 1)
    labels = torch.tensor([0, 1, 2])
    torch.manual_seed(40)
    out = lit.validation_step((lq, hq, labels, ["a", "b", "c"], "ir"), tasks=["ir", "cls"])[-1]
    m = lit.metrics()
    keys = {"val_lq/rvt", "val_lq/rvt_top1", "val_input/rvt", "val_input/rvt_top1"}
    assert keys <= set(m) and {"cls/rvt", "cls_input/rvt"} <= set(lit.totals)
    for key, img in (("cls/rvt", out["cls"]), ("cls_input/rvt", lq)):
        want = torch.stack(ops.top1(ops.rvt(runner.crop_tensor(img).contiguous(), ws), labels)[1:])
        assert torch.equal(lit.totals[key], want) and int(want[1].sum()) == 3
        prefix = "val_lq" if key == "cls/rvt" else "val_input"
        assert (m[f"{prefix}/rvt"], m[f"{prefix}/rvt_top1"]) == classify.accuracy(*want)

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
    r1 = cli.validate(files, tasks=["ir", "cls"], model=model, rvt=f"t={R.CALLER_ARCH}:{path}")
    print({k: r1[k] for k in sorted(keys)})
    assert set(r1) == set(r0) | keys and r1["images"] == r0["images"] == 4
    assert all(r1[k] == r0[k] for k in r0 if k != "images_per_s")            # without --rvt the result is what it was
    assert all(0.0 <= r1[k] <= 1.0 for k in keys)
    corrupted = cfg(dict(class_path="unirestore_amd.data.CorruptedImageFiles",
                         init_args=dict(source=str(lst), corruptions="fog,contrast", severity=3, batch_size=2, seed=2, labels=True)))
    table = cli.validate(corrupted, tasks=["ir", "cls"], model=model, rvt={"t": ws})["by_corruption"]
    assert len(table) == 2 and all({"t", "t_top1", "input/t", "input/t_top1", "psnr", "ssim", "images"} <= set(v) for v in table.values())
