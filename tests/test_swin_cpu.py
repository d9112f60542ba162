"""Host-only checks of the Swin-V2 scorer (unirestore_amd/swin.py, tests/swin_reference.py): the yardstick's recorded constants are
current, its network cases are decidable, its shifted-window attention is plain per-window attention where nothing is shifted or
padded, its two views of a padded token agree, the relative-position bias and the patch-merging repack, the configuration's and
the weight loader's refusals, and the --swin argument."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import swin_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = R.TINY_224


# ---- the yardstick's own constants ----------------------------------------------------------------------------------------------

def test_tolerances_follow_the_measured_fp32_error():
    """Re-measures fp32's own error against fp64 for every recorded constant (swin_reference.py: E32_*) and holds the constants to
    the measurement by classify_reference's rule: every GPU bound (8 x the recorded e32) must be >= 4 x and <= 16 x what is
    measured here - a recorded value below half of what is measured fails; a case fp32 gets exactly right is recorded as 0 and
    must measure 0."""
    pairs = [(f"attention {k}", R.ATTN_TOL[k], R.measure_attn(k)) for k in R.ATTN_CASES]
    pairs += [("attention k bias", R.KBIAS_TOL, R.measure_kbias())]
    pairs += [(f"layernorm_res {k}", R.LNRES_TOL[k], R.measure_lnres(k)) for k in R.LNRES_CASES]
    pairs += [(f"logits {k}", R.LOGITS_TOL[k], R.measure_logits(k)) for k in R.NET_CASES]
    pairs += [("forward", R.FORWARD_TOL, R.measure_forward())]
    assert R.GPU_FACTOR == 8 and R.KBIAS_TOL == 8 * R.E32_KBIAS and R.FORWARD_TOL == 8 * R.E32_FORWARD
    for tol, e32, cases in ((R.ATTN_TOL, R.E32_ATTN, R.ATTN_CASES), (R.LNRES_TOL, R.E32_LNRES, R.LNRES_CASES), (R.LOGITS_TOL, R.E32_LOGITS, R.NET_CASES)):
        assert tol == {k: 8 * v for k, v in e32.items()} and set(e32) == set(cases)
    for name, tol, e32 in pairs:
        print(f"{name}: measured {e32:.2e}, bound {tol:.2e}")
        assert math.isfinite(e32) and e32 >= 0, name
        if tol == 0 or e32 == 0:
            assert tol == 0 and e32 == 0, (name, tol, e32)
        else:
            assert 4 * e32 <= tol <= 16 * e32, (name, tol, e32)


def test_network_cases_are_decidable():
    """What the GPU tests rely on, checked where it is chosen: finite fp64 logits and every image's top-2 gap above twice the
    absolute bound, so that the argmax can be asserted for every image of every network case."""
    for name in R.NET_CASES:
        want = R.net_reference(name)
        bound = R.LOGITS_TOL[name] * float(want.abs().max())
        assert bool(torch.isfinite(want).all()) and float(R.top2_gap(want).min()) > 2 * bound, name
        assert 0.1 < float(want.abs().max()) < 100, name                    # O(1) logits: the stand-in weights do not blow up
    want = R.forward_reference()
    assert bool(torch.isfinite(want).all()) and float(R.top2_gap(want).min()) > 2 * R.FORWARD_TOL * float(want.abs().max())


def test_attention_cases_are_the_issues_and_what_they_claim():
    shapes = {v[:5] for v in R.ATTN_CASES.values() if v[5] == ""}
    assert shapes == {(1, 8, 8, 1, 0), (1, 8, 8, 1, 4), (1, 16, 16, 2, 4), (2, 12, 12, 3, 4), (1, 7, 7, 4, 4), (1, 8, 20, 1, 4),
                      (2, 28, 28, 8, 4), (1, 56, 56, 4, 4)}
    assert {v[5] for v in R.ATTN_CASES.values()} == {"", "clamp", "zero"}
    # the clamp binds and scores reach +-100
    qkv, _b, logit_scale, _bias = R.attn_case("clamp_1x16x16x2_s4")
    c = qkv.shape[3] // 3
    assert float(logit_scale.min()) == 10.0 > math.log(100.0) and torch.equal(R.attn_scale("clamp_1x16x16x2_s4"), torch.tensor([100.0, 100.0]))
    q, k = qkv[0, :, :, :32].double().reshape(-1, 32), qkv[0, :, :, c:c + 32].double().reshape(-1, 32)
    cos = 100 * (F.normalize(q, dim=-1) * F.normalize(k, dim=-1)).sum(-1)      # a token's own key: +-100
    assert float(cos.max()) > 99.999 and float(cos.min()) < -99.999
    # rows of zeros in q and in k
    qkv = R.attn_case("zero_2x12x12x3_s4")[0]
    c = qkv.shape[3] // 3
    for third in (qkv[..., :c], qkv[..., c:2 * c]):
        zero = (third == 0).all(dim=-1)
        assert 10 < int(zero.sum()) < zero.numel() // 2
    assert bool(torch.isfinite(R.attn_reference("zero_2x12x12x3_s4")).all())
    for name in R.ATTN_CASES:                                                 # the k third of the kernel's bias input is zero
        qkv, qkv_bias, _s, bias = R.attn_case(name)
        c = qkv.shape[3] // 3
        assert not bool(qkv_bias[c:2 * c].any()) and bool(qkv_bias[:c].all()) and 0 < float(bias.min()) and float(bias.max()) < 16


# ---- the restatement against plainer ones -------------------------------------------------------------------------------------------

def test_unshifted_attention_on_whole_windows_is_plain_per_window_attention():
    """shift 0 on a map that is a multiple of 8: no padding, no roll, no mask - every 8 x 8 tile attends within itself."""
    heads = 2
    c = heads * R.HEAD_DIM
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(2, 16, 24, 3 * c, generator=g, dtype=torch.float64)
    qkv_bias = torch.randn(3 * c, generator=g, dtype=torch.float64)             # never read: there is no padded token
    logit_scale = math.log(10.0) + 0.3 * torch.randn(heads, generator=g, dtype=torch.float64)
    bias = 16 * torch.rand(heads, 64, 64, generator=g, dtype=torch.float64)
    got = R.attention_from_qkv(qkv, qkv_bias, logit_scale, bias, heads, 0)
    want = torch.empty(2, 16, 24, c, dtype=torch.float64)
    for n in range(2):
        for wy in range(2):
            for wx in range(3):
                tile = qkv[n, 8 * wy:8 * wy + 8, 8 * wx:8 * wx + 8].reshape(64, 3 * c)
                for h in range(heads):
                    q, k, v = (tile[:, i * c + 32 * h:i * c + 32 * h + 32] for i in range(3))
                    qn, kn = q / q.norm(dim=1, keepdim=True), k / k.norm(dim=1, keepdim=True)
                    p = torch.softmax(qn @ kn.t() * torch.exp(logit_scale[h]) + bias[h], dim=1)
                    want[n, 8 * wy:8 * wy + 8, 8 * wx:8 * wx + 8, 32 * h:32 * h + 32] = (p @ v).view(8, 8, 32)
    assert float((got - want).abs().max()) < 1e-13


def test_a_padded_tokens_qkv_is_the_bias_and_the_k_bias_has_no_effect():
    """The two restatements agree: the padded map through the qkv Linear (torchvision's way) and the real tokens' qkv with qkv_bias
    in the padded places (what the kernel is given).  And the checkpoint's k bias changes nothing, though keeping it would."""
    x, sd, pre, heads = R.kbias_case()
    c = x.shape[3]
    qkv_b = sd[f"{pre}.attn.qkv.bias"].double().clone()
    assert float(qkv_b[c:2 * c].abs().max()) > 0.01                             # the checkpoint does hold a k bias
    qkv_b[c:2 * c] = 0
    bias = R.position_bias(sd[f"{pre}.attn.cpb_mlp.0.weight"], sd[f"{pre}.attn.cpb_mlp.0.bias"], sd[f"{pre}.attn.cpb_mlp.2.weight"])
    qkv = F.linear(x.double(), sd[f"{pre}.attn.qkv.weight"].double(), qkv_b)
    via_qkv = R.attention_from_qkv(qkv, qkv_b, sd[f"{pre}.attn.logit_scale"].view(-1), bias, heads, R.KBIAS_SHIFT)
    assert float((via_qkv - R.kbias_reference()).abs().max()) < 1e-12
    assert float((R.kbias_attention(keep_k_bias=True) - R.kbias_reference()).abs().max()) > 1e-3


def test_position_bias_and_index():
    from unirestore_amd import swin
    index = R.relative_position_index().view(64, 64)
    s = torch.arange(64)
    y, x = s // 8, s % 8
    assert torch.equal(index, (y.view(-1, 1) - y.view(1, -1) + 7) * 15 + (x.view(-1, 1) - x.view(1, -1) + 7))
    assert torch.equal(swin.relative_position_index(), index)
    table = R.relative_coords_table()[0]
    f = lambda t: math.copysign(math.log2(abs(t) + 1) / 3, t) if t else 0.0      # noqa: E731
    for dy, dx in ((-7, -7), (0, 0), (3, -5), (7, 1)):
        assert table[dy + 7, dx + 7].tolist() == pytest.approx([f(8 * dy / 7), f(8 * dx / 7)], abs=1e-15)
    assert float((swin.relative_coords_table() - table).abs().max()) < 1e-15
    sd = swin.random_state_dict(swin.SwinConfig(*TINY), 3, 5)
    pre = "features.3.0"
    args = [sd[f"{pre}.attn.cpb_mlp.{k}"] for k in ("0.weight", "0.bias", "2.weight")]
    bias = R.position_bias(*args)
    assert tuple(bias.shape) == (2, 64, 64) and 0 < float(bias.min()) and float(bias.max()) < 16
    assert float(bias.max() - bias.min()) > 6                                   # the stand-in spans a good part of (0, 16)
    dy, dx = (y.view(-1, 1) - y.view(1, -1)), (x.view(-1, 1) - x.view(1, -1))
    for ddy, ddx in ((0, 0), (2, -3), (-7, 7)):                                # it depends on (dy, dx) alone
        same = bias[:, (dy == ddy) & (dx == ddx)]
        assert same.shape[1] >= 1 and bool((same == same[:, :1]).all())
    assert float((swin.position_bias(*args) - bias).abs().max()) < 1e-12     # the loader's table is the restatement's


def test_patch_merging_is_a_2x2_stride_2_convolution():
    from unirestore_amd import swin
    g = torch.Generator().manual_seed(2)
    c = 6
    x = torch.randn(2, 4, 6, c, generator=g, dtype=torch.float64)
    red = torch.randn(2 * c, 4 * c, generator=g, dtype=torch.float64)
    cat = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    want = F.linear(cat, red)
    got = F.conv2d(x.permute(0, 3, 1, 2), swin.merge_conv_weight(red), stride=2).permute(0, 2, 3, 1)
    assert tuple(got.shape) == (2, 2, 3, 2 * c) and float((got - want).abs().max()) < 1e-13
    swapped = F.conv2d(x.permute(0, 3, 1, 2), swin.merge_conv_weight(red).transpose(2, 3), stride=2).permute(0, 2, 3, 1)
    assert float((swapped - want).abs().max()) > 1e-2                          # blocks 1 and 2 the other way round are far away


# ---- the weights ------------------------------------------------------------------------------------------------------------------

def test_archs_and_config_checks():
    from unirestore_amd import swin
    assert swin.ARCHS == {"swin_v2_t": (224, 4, 96, (2, 2, 6, 2), (3, 6, 12, 24)), "swin_v2_s": (224, 4, 96, (2, 2, 18, 2), (3, 6, 12, 24)),
                          "swin_v2_b": (224, 4, 128, (2, 2, 18, 2), (4, 8, 16, 32))}
    assert swin.maps(swin.ARCHS["swin_v2_b"]) == (56, 28, 14, 7) and swin.WINDOW == 8 and swin.HEAD_DIM == 32
    for spec in list(R.NET_CASES.values()) + [(TINY,), (R.KBIAS_CASE[0],)]:
        R.net_config(spec[0])
    C = swin.SwinConfig
    for bad, word in (("swin_b", "swin_b"), (C(224, 4, 96, (2, 2), (3, 5)), "32"), (C(224, 4, 64, (2,), (1,)), "32"),
                      (C(222, 4, 32, (2,), (1,)), "multiple"), (C(40, 4, 32, (2, 2, 2), (1, 2, 4)), "odd"),      # maps 10 -> 5 -> merge
                      (C(28, 4, 32, (2, 2), (1, 2)), "odd"), (C(224, 4, 32, (2, 0), (1, 2)), ">= 1"), (C(224, 4, 32, (2, 2), (1,)), "same stages"),
                      (C(224, 4, 32, (), ()), ">= 1"), ((224, 4, 32, (2,), (1,)), "SwinConfig")):
        with pytest.raises(ValueError, match=word):
            swin.config(bad)
        with pytest.raises(ValueError, match=word):
            swin.SwinWeights(bad, {}, "cpu")
    assert swin.config(C(28, 4, 32, (2,), (1,))).depths == (2,)                 # an odd map is fine where no merge follows


def _expected_keys(cfg):
    e = cfg.embed_dim
    keys = {"features.0.0.weight": (e, 3, cfg.patch_size, cfg.patch_size), "features.0.0.bias": (e,), "features.0.2.weight": (e,), "features.0.2.bias": (e,)}
    for i, depth in enumerate(cfg.depths):
        c, heads = e * 2 ** i, cfg.num_heads[i]
        for j in range(depth):
            pre = f"features.{2 * i + 1}.{j}"
            keys.update({f"{pre}.norm1.weight": (c,), f"{pre}.norm1.bias": (c,), f"{pre}.norm2.weight": (c,), f"{pre}.norm2.bias": (c,),
                         f"{pre}.attn.qkv.weight": (3 * c, c), f"{pre}.attn.qkv.bias": (3 * c,), f"{pre}.attn.proj.weight": (c, c),
                         f"{pre}.attn.proj.bias": (c,), f"{pre}.attn.logit_scale": (heads, 1, 1), f"{pre}.attn.cpb_mlp.0.weight": (512, 2),
                         f"{pre}.attn.cpb_mlp.0.bias": (512,), f"{pre}.attn.cpb_mlp.2.weight": (heads, 512),
                         f"{pre}.mlp.0.weight": (4 * c, c), f"{pre}.mlp.0.bias": (4 * c,), f"{pre}.mlp.3.weight": (c, 4 * c), f"{pre}.mlp.3.bias": (c,)})
        if i < len(cfg.depths) - 1:
            pre = f"features.{2 * i + 2}"
            keys.update({f"{pre}.reduction.weight": (2 * c, 4 * c), f"{pre}.norm.weight": (2 * c,), f"{pre}.norm.bias": (2 * c,)})
    c = e * 2 ** (len(cfg.depths) - 1)
    keys.update({"norm.weight": (c,), "norm.bias": (c,), "head.weight": (7, c), "head.bias": (7,)})
    return keys


def test_random_state_dict_has_torchvisions_keys_and_shapes():
    from unirestore_amd import swin
    for cfg in (swin.SwinConfig(*TINY), swin.ARCHS["swin_v2_t"]):
        sd = swin.random_state_dict(cfg, 0, 7)
        want = _expected_keys(cfg)
        assert set(sd) == set(want) and all(tuple(sd[k].shape) == want[k] for k in want)
        scales = torch.cat([v.view(-1) for k, v in sd.items() if k.endswith("logit_scale")])
        assert abs(float(scales.mean()) - math.log(10.0)) < 0.3 and float(scales.max()) < math.log(100.0)
    assert len(swin.random_state_dict("swin_v2_b", 0, 7)) == 4 + 24 * 16 + 3 * 3 + 4


def test_weights_refuse_bad_state_dicts_before_any_upload():
    from unirestore_amd import swin
    cfg = swin.SwinConfig(*TINY)
    good = swin.random_state_dict(cfg, 0, 7)
    w = swin.SwinWeights(cfg, good, "cpu", source="good.pth")
    assert w.num_classes == 7 and w.device == torch.device("cpu") and set(w.cpu) == set(good)
    assert all(torch.equal(w.cpu[k], good[k]) for k in good)                    # the k bias too: `cpu` is the file's
    pre = "features.3.0"
    qkv_bias, scale, bias = w.attn[pre]
    assert not bool(qkv_bias[64:128].any()) and torch.equal(qkv_bias[:64], good[f"{pre}.attn.qkv.bias"][:64])
    assert not bool(w.linears[f"{pre}.attn.qkv"].bias[64:128].any()) and bool(good[f"{pre}.attn.qkv.bias"][64:128].any())
    assert torch.equal(scale, torch.exp(good[f"{pre}.attn.logit_scale"].double().clamp(max=math.log(100.0))).view(2).float())
    assert tuple(bias.shape) == (2, 64, 64) and bias.dtype == torch.float32
    # buffers a real state dict also holds are ignored (recomputed), and a clamped logit_scale gives exactly 100
    more = dict(good, **{f"{pre}.attn.relative_coords_table": torch.zeros(1, 15, 15, 2), f"{pre}.attn.relative_position_index": torch.zeros(4096, dtype=torch.long),
                         f"{pre}.attn.logit_scale": torch.full((2, 1, 1), 10.0)})
    w2 = swin.SwinWeights(cfg, more, "cpu")
    assert torch.equal(w2.attn[pre][2], bias) and w2.attn[pre][1].tolist() == [100.0, 100.0]
    for key in ("features.0.0.weight", "features.0.2.bias", "features.1.0.norm1.weight", f"{pre}.attn.qkv.weight", f"{pre}.attn.qkv.bias",
                f"{pre}.attn.proj.bias", f"{pre}.attn.logit_scale", f"{pre}.attn.cpb_mlp.0.weight", f"{pre}.attn.cpb_mlp.0.bias",
                f"{pre}.attn.cpb_mlp.2.weight", f"{pre}.norm2.bias", f"{pre}.mlp.0.weight", f"{pre}.mlp.3.bias", "features.2.reduction.weight",
                "features.2.norm.weight", "norm.weight", "head.weight", "head.bias"):
        missing = {k: v for k, v in good.items() if k != key}
        with pytest.raises(ValueError) as e:
            swin.SwinWeights(cfg, missing, "cpu", source="bad.pth")
        assert "bad.pth" in str(e.value) and key in str(e.value)
        if key == "head.weight":
            continue                                               # its first axis is the class count: any [classes, C] matrix is taken
        shaped = dict(good, **{key: torch.zeros(*good[key].shape, 2)})
        with pytest.raises(ValueError) as e:
            swin.SwinWeights(cfg, shaped, "cpu", source="bad.pth")
        assert "bad.pth" in str(e.value) and key in str(e.value) and "shape" in str(e.value)
        for value in (float("nan"), float("inf")):
            poisoned = dict(good, **{key: good[key].clone()})
            poisoned[key].view(-1)[-1] = value
            with pytest.raises(ValueError) as e:
                swin.SwinWeights(cfg, poisoned, "cpu", source="bad.pth")
            assert "bad.pth" in str(e.value) and key in str(e.value) and "non-finite" in str(e.value)
    with pytest.raises(ValueError, match="head.weight"):
        swin.SwinWeights(cfg, dict(good, **{"head.weight": torch.zeros(7, 65)}), "cpu")


def test_load_weights_reads_plain_and_lightning_files(tmp_path):
    from unirestore_amd import swin
    cfg = swin.SwinConfig(*TINY)
    sd = swin.random_state_dict(cfg, 3, 5)
    a = swin.SwinWeights(cfg, sd, "cpu")
    plain, lit = tmp_path / "plain.pth", tmp_path / "lit.ckpt"
    torch.save(sd, str(plain))
    torch.save({"state_dict": {f"model.{k}": v for k, v in sd.items()}}, str(lit))
    for path in (plain, lit):
        b = swin.load_weights(cfg, str(path), "cpu")
        assert all(torch.equal(a.cpu[k], b.cpu[k]) for k in sd)
        assert all(torch.equal(a.linears[k].w, b.linears[k].w) and torch.equal(a.linears[k].bias, b.linears[k].bias) for k in a.linears)
    torch.save({k: v for k, v in sd.items() if k != "norm.bias"}, str(plain))
    with pytest.raises(ValueError) as e:
        swin.load_weights(cfg, str(plain), "cpu")
    assert "plain.pth" in str(e.value) and "norm.bias" in str(e.value)
    with pytest.raises(ValueError, match="swin_x"):
        swin.load_weights("swin_x", str(lit), "cpu")


def test_litunifie_loads_an_arch_path_pair_through_the_module_its_arch_names(monkeypatch):
    from unirestore_amd import classify, runner, swin, vit
    tiny = swin.SwinWeights(swin.SwinConfig(*TINY), swin.random_state_dict(swin.SwinConfig(*TINY), 0, 7), "cpu")
    calls = []
    monkeypatch.setattr(swin, "load_weights", lambda arch, path: calls.append(("swin", arch, path)) or tiny)
    monkeypatch.setattr(vit, "load_weights", lambda arch, path: calls.append(("vit", arch, path)) or tiny)
    monkeypatch.setattr(classify, "load_weights", lambda arch, path: calls.append(("classify", arch, path)) or tiny)
    lit = runner.LitUniFIE({}, model=object(), classifiers={"a": ("swin_v2_b", "a.pth"), "b": tiny, "c": ("resnet50", "c.pth"), "d": ("vit_b_16", "d.pth")})
    assert calls == [("swin", "swin_v2_b", "a.pth"), ("classify", "resnet50", "c.pth"), ("vit", "vit_b_16", "d.pth")] and lit.classifiers["b"] is tiny
    assert {"cls/a", "cls_input/a", "cls/b", "cls_input/b"} <= set(lit.totals) and tuple(lit.totals["cls/a"].shape) == (3, 7)


# ---- the command line -------------------------------------------------------------------------------------------------------------

class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_swin_argument(tmp_path, capsys):
    from unirestore_amd import cli
    w = str(tmp_path / "s.pth")
    open(w, "wb").close()                                          # the argument check looks for the file, it does not read it
    assert cli.check_swin_arg(f"a=swin_v2_b:{w},b=swin_v2_t:{w}") == {"a": ("swin_v2_b", w), "b": ("swin_v2_t", w)}
    assert cli.check_swin_arg({"a": ("swin_v2_s", w)}) == {"a": ("swin_v2_s", w)}
    assert cli.check_classifiers_arg(None, None) == (None, None) == cli.check_classifiers_arg(None, None, None)
    assert cli.check_classifiers_arg(f"r=resnet18:{w}", f"v=vit_b_16:{w}", f"s=swin_v2_b:{w}") == (
        {"r": ("resnet18", w), "v": ("vit_b_16", w), "s": ("swin_v2_b", w)}, "--classify")
    assert cli.check_classifiers_arg(None, f"v=vit_b_16:{w}", f"s=swin_v2_b:{w}") == ({"v": ("vit_b_16", w), "s": ("swin_v2_b", w)}, "--vit")
    assert cli.check_classifiers_arg(None, None, f"s=swin_v2_b:{w}") == ({"s": ("swin_v2_b", w)}, "--swin")
    assert cli.check_classifiers_arg(f"r=resnet18:{w}", f"v=vit_b_16:{w}") == ({"r": ("resnet18", w), "v": ("vit_b_16", w)}, "--classify")
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))        # its data yields no labels
    for kw, tasks, word in [
        (dict(swin=f"a=vit_b_16:{w}"), ["ir", "cls"], "vit_b_16"),                             # an arch of another option
        (dict(swin=f"a=swin_v2_b:{w}.none"), ["ir", "cls"], "no such file"),
        (dict(swin="a=swin_v2_b"), ["ir", "cls"], "NAME=ARCH:WEIGHTS.pth"),
        (dict(swin=f"a=swin_v2_b:{w},a=swin_v2_t:{w}"), ["ir", "cls"], "twice"),
        (dict(swin=f"a=swin_v2_b:{w}", classify=f"a=resnet18:{w}"), ["ir", "cls"], "--classify too"),   # both would write val_lq/a
        (dict(swin=f"a=swin_v2_b:{w}", vit=f"a=vit_b_16:{w}"), ["ir", "cls"], "--vit too"),
        (dict(swin=f"a=swin_v2_b:{w}"), None, "--swin scores the 'cls' output"),
        (dict(swin=f"a=swin_v2_b:{w}"), ["ir"], "--swin scores the 'cls' output"),
        (dict(swin=f"a=swin_v2_b:{w}"), ["ir", "cls"], "--swin needs labels"),
        (dict(swin=f"a=swin_v2_b:{w}", vit=f"v=vit_b_16:{w}"), ["ir", "cls"], "--vit needs labels"),
        (dict(swin=f"a=swin_v2_b:{w}", classify=f"r=resnet18:{w}"), ["ir", "cls"], "--classify needs labels"),
    ]:
        with pytest.raises(ValueError) as e:
            cli.validate(cfg, tasks=tasks, model=_NoModel(), **kw)
        assert word in str(e.value), (kw, tasks, str(e.value))
    path = os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")
    for argv, word in ((["restore", "--config", path, "--swin", f"a=swin_v2_b:{w}"], "--swin belongs to validate"),
                       (["validate", "--config", path, "--swin", f"a=swin_v2_b:{w}"], "--swin scores the 'cls' output"),
                       (["validate", "--config", path, "--tasks", "ir,cls", "--swin", f"a=swin_v2_b:{w}", "--vit", f"a=vit_b_16:{w}"], "--vit too")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
