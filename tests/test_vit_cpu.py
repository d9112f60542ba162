"""Host-only checks of the ViT scorer (unirestore_amd/vit.py, tests/vit_reference.py): the yardstick's recorded constants are
current, its network cases are decidable, its encoder block is torch's own nn.MultiheadAttention + nn.LayerNorm + nn.GELU (the
independent check of in_proj's q | k | v layout - torchvision itself is not installed where this runs), the weight loader's
refusals, and the --vit argument."""
import math
import os

import pytest
import torch

import vit_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = R.TINY_224


# ---- the yardstick's own constants ----------------------------------------------------------------------------------------------

def test_tolerances_follow_the_measured_fp32_error():
    """Re-measures fp32's own error against fp64 for every recorded constant (vit_reference.py: E32_*) and holds the constants to
    the measurement by classify_reference's rule: every GPU bound (8 x the recorded e32) must be >= 4 x and <= 16 x what is
    measured here; a case fp32 gets exactly right is recorded as 0 and must measure 0."""
    pairs = [(f"ln {k}", R.LN_TOL[k], R.measure_ln(k)) for k in R.LN_CASES]
    pairs += [("ln strided", R.LN_STRIDED_TOL, R.measure_ln_strided()), ("gelu", R.GELU_TOL, R.measure_gelu())]
    pairs += [(f"attention {k}", R.ATTN_TOL[k], R.measure_attn(k)) for k in R.ATTN_CASES]
    pairs += [(f"logits {k}", R.LOGITS_TOL[k], R.measure_logits(k)) for k in R.NET_CASES]
    pairs += [("forward", R.FORWARD_TOL, R.measure_forward())]
    assert R.GPU_FACTOR == 8 and R.LN_STRIDED_TOL == 8 * R.E32_LN_STRIDED and R.GELU_TOL == 8 * R.E32_GELU and R.FORWARD_TOL == 8 * R.E32_FORWARD
    for tol, e32, cases in ((R.LN_TOL, R.E32_LN, R.LN_CASES), (R.ATTN_TOL, R.E32_ATTN, R.ATTN_CASES), (R.LOGITS_TOL, R.E32_LOGITS, R.NET_CASES)):
        assert tol == {k: 8 * v for k, v in e32.items()} and set(e32) == set(cases)
    for name, tol, e32 in pairs:
        print(f"{name}: measured {e32:.2e}, bound {tol:.2e}")
        assert math.isfinite(e32) and e32 >= 0, name
        if tol == 0 or e32 == 0:
            assert tol == 0 and e32 == 0, (name, tol, e32)
        else:
            assert 4 * e32 <= tol <= 16 * e32, (name, tol, e32)
    assert [k for k, v in R.E32_LN.items() if v == 0] == ["1x1"] and [k for k, v in R.E32_ATTN.items() if v == 0] == ["1x1x1"]


def test_network_cases_are_decidable():
    """What the GPU tests rely on, checked where it is chosen: finite fp64 logits and every image's top-2 gap above twice the
    absolute bound, so that the argmax can be asserted for every image of every network case."""
    for name in R.NET_CASES:
        want = R.net_reference(name)
        bound = R.LOGITS_TOL[name] * float(want.abs().max())
        assert bool(torch.isfinite(want).all()) and float(R.top2_gap(want).min()) > 2 * bound, name
        assert 0.1 < float(want.abs().max()) < 100, name                    # O(1) logits: the stand-in weights do not blow up
    assert len(set(R.net_reference("vit_b_16").argmax(dim=1).tolist())) == 2
    want = R.forward_reference()
    assert float(R.top2_gap(want).min()) > 2 * R.FORWARD_TOL * float(want.abs().max())


def test_kernel_cases_are_what_they_claim():
    assert float(R.scores(R.attn_case("big_2x50x2"), 2).abs().max()) > 100          # exp overflows fp32 without the row maximum
    n, s, h, _ = R.ATTN_CASES["constv_2x197x2"]
    v = R.attn_case("constv_2x197x2")[:, :, 2 * h * 64:].reshape(n, s, h, 64)
    assert bool((v == v[:, :1, :, :1]).all()) and len(set(v[:, 0, :, 0].flatten().tolist())) == n * h
    assert float((R.attn_reference("constv_2x197x2").reshape(n, s, h, 64) - v.double()).abs().max()) < 1e-14
    x, _g, _b, _eps = R.ln_case("mean1e4_4x768")
    assert abs(float(x.mean()) - 1e4) < 1 and 0.9 < float(x.double().std()) < 1.1
    naive = (x * x).mean(dim=1) - x.mean(dim=1) ** 2                              # E[x^2] - mean^2 in fp32: no digit of the variance
    assert float((naive - x.double().var(dim=1, unbiased=False)).abs().max()) > 0.5
    assert R.S_MAX >= 197 and R.ATTN_CASES["1xSMAXx1"][1] == R.S_MAX
    assert [R.gelu_case(n).numel() for n in R.GELU_SIZES] == list(R.GELU_SIZES) and float(R.gelu_case(1)[0]) == 10.0


# ---- the restatement against torch's own modules ----------------------------------------------------------------------------------

def test_block_is_torchs_multihead_attention_layernorm_and_gelu():
    """The restated encoder block (F.multi_head_attention_forward on in_proj's packed weight) equals nn.MultiheadAttention +
    nn.LayerNorm + nn.GELU + nn.Linear modules loaded with the same tensors, and the stand-alone attention restatement - the
    layout the kernel is tested against - equals the same module between its two projections."""
    from unirestore_amd import vit
    cfg = vit.ViTConfig(32, 16, 1, 3, 192, 384)
    sd = vit.random_state_dict(cfg, 5, 10)
    pre = "encoder.layers.encoder_layer_0"
    d, heads = cfg.hidden_dim, cfg.num_heads
    x = torch.randn(2, 5, d, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    ln1, ln2 = torch.nn.LayerNorm(d, eps=1e-6).double(), torch.nn.LayerNorm(d, eps=1e-6).double()
    mha = torch.nn.MultiheadAttention(d, heads, dropout=0.0, batch_first=True).double().eval()
    fc1, fc2, act = torch.nn.Linear(d, cfg.mlp_dim).double(), torch.nn.Linear(cfg.mlp_dim, d).double(), torch.nn.GELU()
    for mod, key in ((ln1, "ln_1"), (ln2, "ln_2"), (mha, "self_attention"), (fc1, "mlp.0"), (fc2, "mlp.3")):
        missing = mod.load_state_dict({k[len(f"{pre}.{key}."):]: v.double() for k, v in sd.items() if k.startswith(f"{pre}.{key}.")})
        assert not missing.missing_keys and not missing.unexpected_keys
    with torch.no_grad():
        y = ln1(x)
        attn = mha(y, y, y, need_weights=False)[0]
        h = x + attn
        want = h + fc2(act(fc1(ln2(h))))
        got = R.block(x, sd, pre, heads, torch.float64)
        assert float((got - want).abs().max()) < 1e-12
        qkv = torch.nn.functional.linear(y, mha.in_proj_weight, mha.in_proj_bias)
        alone = torch.nn.functional.linear(R.attention(qkv, heads), mha.out_proj.weight, mha.out_proj.bias)
        assert float((alone - attn).abs().max()) < 1e-12
        # a wrong split (heads interleaved instead of q | k | v) is far away
        wrong = R.attention(qkv.reshape(2, 5, heads, 3 * 64).transpose(2, 3).reshape(2, 5, 3 * d), heads)
        assert float((torch.nn.functional.linear(wrong, mha.out_proj.weight, mha.out_proj.bias) - attn).abs().max()) > 1e-3


# ---- the weights ------------------------------------------------------------------------------------------------------------------

def test_archs_and_config_checks():
    from unirestore_amd import vit
    assert vit.ARCHS == {"vit_b_16": (224, 16, 12, 12, 768, 3072), "vit_b_32": (224, 32, 12, 12, 768, 3072),
                         "vit_l_16": (224, 16, 24, 16, 1024, 4096), "vit_l_32": (224, 32, 24, 16, 1024, 4096)}
    assert vit.seq_len(vit.ARCHS["vit_b_16"]) == 197 and vit.seq_len(vit.ARCHS["vit_l_32"]) == 50 and vit.S_MAX == R.S_MAX
    for bad, word in (("vit_h_14", "vit_h_14"), (vit.ViTConfig(224, 16, 1, 2, 64, 128), "64"), (vit.ViTConfig(224, 15, 1, 1, 64, 128), "multiple"),
                      (vit.ViTConfig(224, 14, 1, 20, 1280, 5120), "tokens"),                # 257 tokens
                      (vit.ViTConfig(256, 8, 1, 1, 64, 128), "tokens"), (vit.ViTConfig(224, 16, 0, 1, 64, 128), ">= 1"), ((224, 16, 1, 1, 64, 128), "ViTConfig")):
        with pytest.raises(ValueError, match=word):
            vit.config(bad)
        with pytest.raises(ValueError, match=word):
            vit.ViTWeights(bad, {}, "cpu")


def test_weights_refuse_bad_state_dicts_before_any_upload():
    from unirestore_amd import vit
    cfg = vit.ViTConfig(*TINY)
    good = vit.random_state_dict(cfg, 0, 7)
    w = vit.ViTWeights(cfg, good, "cpu", source="good.pth")
    assert w.num_classes == 7 and w.seq_len == 50 and w.device == torch.device("cpu") and set(w.cpu) == set(good)
    assert all(torch.equal(w.cpu[k], good[k]) for k in good) and w.pos.shape == (50, 64) and w.class_token.shape == (64,)
    pre = "encoder.layers.encoder_layer_0"
    for key in ("conv_proj.weight", "class_token", "encoder.pos_embedding", f"{pre}.ln_1.weight", f"{pre}.self_attention.in_proj_weight",
                f"{pre}.self_attention.out_proj.bias", f"{pre}.ln_2.bias", f"{pre}.mlp.0.weight", f"{pre}.mlp.3.bias", "encoder.ln.weight",
                "heads.head.weight", "heads.head.bias"):
        missing = {k: v for k, v in good.items() if k != key}
        with pytest.raises(ValueError) as e:
            vit.ViTWeights(cfg, missing, "cpu", source="bad.pth")
        assert "bad.pth" in str(e.value) and key in str(e.value)
        if key == "heads.head.weight":
            continue                                               # its first axis is the class count: any [classes, D] matrix is taken
        shaped = dict(good, **{key: torch.zeros(*good[key].shape, 2)})
        with pytest.raises(ValueError) as e:
            vit.ViTWeights(cfg, shaped, "cpu", source="bad.pth")
        assert "bad.pth" in str(e.value) and key in str(e.value) and "shape" in str(e.value)
        for value in (float("nan"), float("inf")):
            poisoned = dict(good, **{key: good[key].clone()})
            poisoned[key].view(-1)[-1] = value
            with pytest.raises(ValueError) as e:
                vit.ViTWeights(cfg, poisoned, "cpu", source="bad.pth")
            assert "bad.pth" in str(e.value) and key in str(e.value) and "non-finite" in str(e.value)
    with pytest.raises(ValueError, match="heads.head.weight"):
        vit.ViTWeights(cfg, dict(good, **{"heads.head.weight": torch.zeros(7, 65)}), "cpu")
    # a state dict of another network (a wider one): the first key says so
    with pytest.raises(ValueError, match="conv_proj.weight"):
        vit.ViTWeights(cfg, vit.random_state_dict(vit.ViTConfig(224, 32, 1, 2, 128, 128), 0, 7), "cpu")


def test_both_mlp_spellings_load_to_identical_tensors(tmp_path):
    from unirestore_amd import vit
    cfg = vit.ViTConfig(*TINY)
    new = vit.random_state_dict(cfg, 3, 5)
    old = {k.replace(".mlp.0.", ".mlp.linear_1.").replace(".mlp.3.", ".mlp.linear_2."): v for k, v in new.items()}
    assert set(old) != set(new) and any(".mlp.linear_1." in k for k in old)
    a, b = vit.ViTWeights(cfg, new, "cpu"), vit.ViTWeights(cfg, old, "cpu")
    assert set(a.cpu) == set(b.cpu) == set(new) and all(torch.equal(a.cpu[k], b.cpu[k]) for k in new)
    assert set(a.linears) == set(b.linears)
    for k in a.linears:
        assert torch.equal(a.linears[k].w, b.linears[k].w) and torch.equal(a.linears[k].bias, b.linears[k].bias)
    # a Lightning checkpoint of the same weights, through load_weights
    path = tmp_path / "lit.ckpt"
    torch.save({"state_dict": {f"model.{k}": v for k, v in old.items()}}, str(path))
    c = vit.load_weights(cfg, str(path), "cpu")
    assert all(torch.equal(a.cpu[k], c.cpu[k]) for k in new)
    with pytest.raises(ValueError, match="vit_x"):
        vit.load_weights("vit_x", str(path), "cpu")


def test_litunifie_loads_an_arch_path_pair_through_the_module_its_arch_names(monkeypatch):
    from unirestore_amd import classify, runner, vit
    tiny = vit.ViTWeights(vit.ViTConfig(*TINY), vit.random_state_dict(vit.ViTConfig(*TINY), 0, 7), "cpu")
    calls = []
    monkeypatch.setattr(vit, "load_weights", lambda arch, path: calls.append(("vit", arch, path)) or tiny)
    monkeypatch.setattr(classify, "load_weights", lambda arch, path: calls.append(("classify", arch, path)) or tiny)
    lit = runner.LitUniFIE({}, model=object(), classifiers={"a": ("vit_l_32", "a.pth"), "b": tiny, "c": ("resnet50", "c.pth")})
    assert calls == [("vit", "vit_l_32", "a.pth"), ("classify", "resnet50", "c.pth")] and lit.classifiers["b"] is tiny
    assert {"cls/a", "cls_input/a", "cls/b", "cls_input/b"} <= set(lit.totals) and tuple(lit.totals["cls/a"].shape) == (3, 7)


# ---- the command line -------------------------------------------------------------------------------------------------------------

class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_vit_argument(tmp_path, capsys):
    from unirestore_amd import cli
    w = str(tmp_path / "v.pth")
    open(w, "wb").close()                                          # the argument check looks for the file, it does not read it
    assert cli.check_vit_arg(f"a=vit_b_16:{w},b=vit_l_32:{w}") == {"a": ("vit_b_16", w), "b": ("vit_l_32", w)}
    assert cli.check_vit_arg({"a": ("vit_b_32", w)}) == {"a": ("vit_b_32", w)}
    assert cli.check_classifiers_arg(None, None) == (None, None)
    assert cli.check_classifiers_arg(f"r=resnet18:{w}", f"v=vit_b_16:{w}") == ({"r": ("resnet18", w), "v": ("vit_b_16", w)}, "--classify")
    assert cli.check_classifiers_arg(None, f"v=vit_b_16:{w}") == ({"v": ("vit_b_16", w)}, "--vit")
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))        # its data yields no labels
    for kw, tasks, word in [
        (dict(vit=f"a=resnet18:{w}"), ["ir", "cls"], "resnet18"),                              # an arch of the other option
        (dict(vit=f"a=vit_b_16:{w}.none"), ["ir", "cls"], "no such file"),
        (dict(vit="a=vit_b_16"), ["ir", "cls"], "NAME=ARCH:WEIGHTS.pth"),
        (dict(vit=f"a=vit_b_16:{w},a=vit_b_32:{w}"), ["ir", "cls"], "twice"),
        (dict(vit=f"a=vit_b_16:{w}", classify=f"a=resnet18:{w}"), ["ir", "cls"], "--classify too"),     # both would write val_lq/a
        (dict(vit=f"a=vit_b_16:{w}"), None, "--vit scores the 'cls' output"),
        (dict(vit=f"a=vit_b_16:{w}"), ["ir"], "--vit scores the 'cls' output"),
        (dict(vit=f"a=vit_b_16:{w}"), ["ir", "cls"], "--vit needs labels"),
        (dict(vit=f"a=vit_b_16:{w}", classify=f"r=resnet18:{w}"), ["ir", "cls"], "--classify needs labels"),
    ]:
        with pytest.raises(ValueError) as e:
            cli.validate(cfg, tasks=tasks, model=_NoModel(), **kw)
        assert word in str(e.value), (kw, tasks, str(e.value))
    path = os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")
    for argv, word in ((["restore", "--config", path, "--vit", f"a=vit_b_16:{w}"], "--vit belongs to validate"),
                       (["validate", "--config", path, "--vit", f"a=vit_b_16:{w}"], "--vit scores the 'cls' output"),
                       (["validate", "--config", path, "--tasks", "ir,cls", "--vit", f"a=vit_b_16:{w}", "--classify", f"a=resnet18:{w}"], "--classify too")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
