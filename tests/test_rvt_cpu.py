"""Host-only checks of the RVT scorer (unirestore_amd/rvt.py, tests/rvt_reference.py): the restatement against what the reference's
own PoolingTransformer computed (tests/golden/rvt_0.npz, tools/gen_golden_rvt.py), the yardstick's recorded constants are current,
its network cases are decidable, the cases are the issue's, the BatchNorm-with-bias fold and the depthwise repack, the
configuration's and the weight loader's refusals, the three checkpoint wrappings, and the --rvt argument."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import rvt_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_STAGE = R.NET_CASES["golden_two_stage"][0]
BASE_WIDTH = R.NET_CASES["golden_base_width"][0]


# ---- the restatement against the reference's own network ------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_restatement_reproduces_the_reference_network(name):
    g = R.golden()
    assert tuple(g["cases"]) == R.GOLDEN_CASES
    spec, classes, wseed, iseed, n = R.NET_CASES[name]
    stored = (int(g[f"{name}/image_size"]), tuple(int(v) for v in g[f"{name}/base_dims"]), tuple(int(v) for v in g[f"{name}/depth"]),
              tuple(int(v) for v in g[f"{name}/heads"]), int(g[f"{name}/mlp_ratio"]), bool(g[f"{name}/use_mask"]), int(g[f"{name}/masked_block"]))
    assert stored == spec and (int(g[f"{name}/classes"]), int(g[f"{name}/weight_seed"]), int(g[f"{name}/image_seed"]), int(g[f"{name}/n"])) == (
        classes, wseed, iseed, n)
    sd = R.state_dict(spec, wseed, classes)
    keys = [str(k) for k in g[f"{name}/checksum_keys"]]
    assert keys == sorted(k for k, v in sd.items() if v.is_floating_point())      # strict=True loaded exactly these into the module
    for k, want in zip(keys, g[f"{name}/checksums"]):
        assert R.checksum(sd[k]) == pytest.approx(float(want), rel=1e-12, abs=1e-12), \
            f"{k}: torch's random generator no longer draws the weights tests/golden/rvt_0.npz was made with - regenerate it"
    assert R.checksum(R.net_input(name)) == pytest.approx(float(g[f"{name}/input_checksum"]), rel=1e-12)
    want = R.golden_logits(name)
    got = R.net_reference(name)
    assert got.shape == want.shape == (n, classes) and want.dtype == torch.float64
    err = float((got - want).abs().max() / want.abs().max())
    print(f"{name}: max |err| / max |logit| {err:.2e}")
    assert err <= 1e-12
    assert os.path.getsize(R.GOLDEN) < 256 * 1024


def test_golden_networks_cover_what_they_claim():
    from unirestore_amd import rvt
    cfg = rvt.config(rvt.RVTConfig(*TWO_STAGE))
    assert rvt.maps(cfg) == (14, 7) and rvt.dims(cfg) == (64, 128) and cfg.base_dims == (32, 32)
    assert [g for _p, _s, g in rvt.block_keys(cfg)] == [True, False, False]      # a gated and a plain block at 196 tokens, one at 49
    sd = R.state_dict(TWO_STAGE, 41, 10)
    assert tuple(sd["transformers.0.blocks.0.mlp.fc1.weight"].shape) == (256, 64, 1, 1) and "transformers.0.blocks.0.mlp.dwconv.weight" in sd
    assert tuple(sd["pools.0.conv.weight"].shape) == (128, 1, 3, 3) and "transformers.0.blocks.1.attn.att_mask" not in sd
    cfg = rvt.config(rvt.RVTConfig(*BASE_WIDTH))
    assert rvt.dims(cfg) == (768,) and cfg.base_dims == (64,)
    sd = R.state_dict(BASE_WIDTH, 43, 10)
    assert tuple(sd["transformers.0.blocks.0.mlp.fc1.weight"].shape) == (3072, 768) and not any("dwconv" in k or "pools" in k for k in sd)
    assert tuple(sd["transformers.0.blocks.0.attn.att_mask"].shape) == (12, 196, 196)


# ---- the yardstick's own constants ----------------------------------------------------------------------------------------------

def test_tolerances_follow_the_measured_fp32_error():
    """Re-measures fp32's own error against fp64 for every recorded constant (rvt_reference.py: E32_*) and holds the constants to
    the measurement by classify_reference's rule: every GPU bound (8 x the recorded e32) must be >= 4 x and <= 16 x what is
    measured here; a case fp32 gets exactly right is recorded as 0 and must measure 0."""
    pairs = [(f"attention {k}", R.ATTN_TOL[k], R.measure_attn(k)) for k in R.ATTN_CASES]
    pairs += [("attention, 0 / 1 gate", R.GATE01_TOL, R.measure_gate01())]
    pairs += [(f"dwconv {k}", R.DW_TOL[k], R.measure_dw(k)) for k in R.DW_CASES]
    pairs += [(f"logits {k}", R.LOGITS_TOL[k], R.measure_logits(k)) for k in R.NET_CASES]
    pairs += [(f"forward {k}", R.FORWARD_TOL[k], R.measure_forward(k)) for k in R.FORWARD_SHAPES]
    assert R.GPU_FACTOR == 8 and R.GATE01_TOL == 8 * R.E32_GATE01
    for tol, e32, cases in ((R.ATTN_TOL, R.E32_ATTN, R.ATTN_CASES), (R.DW_TOL, R.E32_DW, R.DW_CASES), (R.LOGITS_TOL, R.E32_LOGITS, R.NET_CASES),
                            (R.FORWARD_TOL, R.E32_FORWARD, R.FORWARD_SHAPES)):
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
    absolute bound, so that the argmax can be asserted for every image of every network case - for the golden networks with the
    reference module's own logits."""
    for name in R.NET_CASES:
        want = R.golden_logits(name) if name in R.GOLDEN_CASES else R.net_reference(name)
        bound = R.LOGITS_TOL[name] * float(want.abs().max())
        assert bool(torch.isfinite(want).all()) and float(R.top2_gap(want).min()) > 2 * bound, name
        assert 0.1 < float(want.abs().max()) < 100, name                    # O(1) logits: the stand-in weights do not blow up
    for shape in R.FORWARD_SHAPES:
        want = R.forward_reference(shape)
        assert bool(torch.isfinite(want).all()) and float(R.top2_gap(want).min()) > 2 * R.FORWARD_TOL[shape] * float(want.abs().max())


def test_cases_are_the_issues():
    assert {v for v in R.ATTN_CASES.values()} == {(s, h, d, g) for s in (1, 31, 33, 49, 196, 256) for h in (1, 3) for d in (32, 64)
                                                  for g in (False, True)} and R.ATTN_N == 2
    assert {v for v in R.DW_CASES.values()} == {(h, w, c, m, st, act) for h, w in ((1, 1), (2, 3), (7, 7), (14, 14)) for c in (6, 64)
                                                for m, st in ((1, 1), (2, 2), (1, 2)) for act in (0, 1)}
    assert R.VIT_EQUAL_CASES == ((49, 3), (197, 2))
    gate = R.gate01_case()[1]
    assert set(gate.unique().tolist()) == {0.0, 1.0} and 0.3 < float(gate.mean()) < 0.7
    for name in ("S196_H3_d32_g", "S33_H1_d64_g"):                             # the gate is a sigmoid: inside (0, 1), and it matters
        qkv, g = R.attn_case(name)
        assert 0 < float(g.min()) and float(g.max()) < 1
        assert R.rel_err(R.attention(qkv, R.ATTN_CASES[name][1], None), R.attn_reference(name)) > 1e-2
    assert R.attn_case("S33_H1_d64")[1] is None
    assert R.NET_CASES["small_plus_trimmed"][4] == R.NET_CASES["base_plus_trimmed"][4] == 3


def test_attention_restatement_is_plain_softmax_attention():
    qkv, gate = R.attn_case("S33_H3_d32_g")
    got = R.attn_reference("S33_H3_d32_g")
    n, h, d = 1, 2, 32
    q, k, v = (qkv[n, :, i * 96 + h * d:i * 96 + (h + 1) * d].double() for i in range(3))
    p = torch.softmax(q @ k.t() / math.sqrt(d) * gate[h].double(), dim=1)
    assert float((got[n, :, h * d:(h + 1) * d] - p @ v).abs().max()) < 1e-13


# ---- the loader's arithmetic ------------------------------------------------------------------------------------------------------

def test_bn_fold_with_a_conv_bias_equals_conv_then_batch_norm():
    from unirestore_amd import rvt
    g = torch.Generator().manual_seed(3)
    for cout, cin, k, groups in ((8, 5, 3, 1), (12, 1, 3, 12), (6, 4, 1, 1)):
        w = torch.randn(cout, cin, k, k, generator=g)
        b = torch.randn(cout, generator=g)                                      # a bias far from 0: dropping it would show
        gamma, beta, mean = (torch.randn(cout, generator=g) for _ in range(3))
        var = 0.5 + torch.rand(cout, generator=g)
        x = torch.randn(2, cin * groups, 6, 7, generator=g, dtype=torch.float64)
        want = F.batch_norm(F.conv2d(x, w.double(), b.double(), padding=k // 2, groups=groups), mean.double(), var.double(), gamma.double(),
                            beta.double(), False, 0.1, rvt.BN_EPS)
        fw, fb = rvt.fold_bn_bias(w, b, gamma, beta, mean, var)
        assert fw.dtype == fb.dtype == torch.float64 and fw.shape == w.shape
        got = F.conv2d(x, fw, fb, padding=k // 2, groups=groups)
        assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())
        no_bias = F.conv2d(x, fw, fb - b.double() * gamma.double() / torch.sqrt(var.double() + rvt.BN_EPS), padding=k // 2, groups=groups)
        assert float((no_bias - want).abs().max()) > 1e-2
    w = torch.arange(2 * 9, dtype=torch.float32).view(2, 1, 3, 3)
    packed = rvt.pack_dw_weight(w)
    assert tuple(packed.shape) == (9, 2) and packed.is_contiguous() and packed[3 * 1 + 2].tolist() == [float(w[0, 0, 1, 2]), float(w[1, 0, 1, 2])]


def test_weights_hold_the_folds_the_gate_and_the_repack():
    from unirestore_amd import f32net, rvt
    cfg = rvt.RVTConfig(*TWO_STAGE)
    sd = R.state_dict(TWO_STAGE, 41, 10)
    w = rvt.RVTWeights(cfg, sd, "cpu", source="good.pth")
    assert w.num_classes == 10 and w.device == torch.device("cpu") and w.maps == (14, 7) and w.dims == (64, 128)
    assert set(w.cpu) == {k for k, v in sd.items() if v.is_floating_point()} and all(torch.equal(w.cpu[k], sd[k]) for k in w.cpu)
    pre = "transformers.0.blocks.0"
    assert set(w.gates) == {pre} and torch.equal(w.gates[pre], torch.sigmoid(sd[f"{pre}.attn.att_mask"].double()).float())
    assert set(w.dwconvs) == {f"transformers.{s}.blocks.{i}.mlp.dwconv" for s, i in ((0, 0), (0, 1), (1, 0))} | {"pools.0.conv"}
    pw, pb, mult, stride = w.dwconvs["pools.0.conv"]
    assert (mult, stride) == (2, 2) and torch.equal(pw, sd["pools.0.conv.weight"].view(128, 9).t()) and torch.equal(pb, sd["pools.0.conv.bias"])
    dw, db, mult, stride = w.dwconvs[f"{pre}.mlp.dwconv"]
    bn = [sd[f"{pre}.mlp.bn2.{n}"] for n in ("weight", "bias", "running_mean", "running_var")]
    fw, fb = rvt.fold_bn_bias(sd[f"{pre}.mlp.dwconv.weight"], sd[f"{pre}.mlp.dwconv.bias"], *bn)
    assert (mult, stride) == (1, 1) and torch.equal(dw, fw.float().view(256, 9).t()) and torch.equal(db, fb.float())
    stem = w.linears["patch_embed.proj.0"]
    bn = [sd[f"patch_embed.proj.1.{n}"] for n in ("weight", "bias", "running_mean", "running_var")]
    fw, fb = rvt.fold_bn_bias(sd["patch_embed.proj.0.weight"], sd["patch_embed.proj.0.bias"], *bn)
    assert (stem.kh, stem.stride, stem.pad) == (7, 2, 2) and torch.equal(stem.w, f32net.pack_conv_weight(fw.float())) and torch.equal(stem.bias, fb.float())
    p3 = w.linears["patch_embed.proj.3"]
    assert (p3.kh, p3.stride, p3.pad, p3.cout) == (4, 4, 0, 64)


def _some_keys(sd):
    pre = "transformers.0.blocks.0"
    return ("patch_embed.proj.0.weight", "patch_embed.proj.0.bias", "patch_embed.proj.1.running_var", "patch_embed.proj.3.bias", f"{pre}.norm1.weight",
            f"{pre}.attn.qkv.weight", f"{pre}.attn.proj.bias", f"{pre}.attn.att_mask", f"{pre}.norm2.bias", f"{pre}.mlp.fc1.weight",
            f"{pre}.mlp.bn1.running_mean", f"{pre}.mlp.dwconv.weight", f"{pre}.mlp.dwconv.bias", f"{pre}.mlp.bn2.weight", f"{pre}.mlp.fc2.bias",
            f"{pre}.mlp.bn3.bias", "transformers.1.blocks.0.attn.qkv.bias", "pools.0.conv.weight", "pools.0.conv.bias", "norm.weight", "head.weight",
            "head.bias")


def test_weights_refuse_bad_state_dicts_before_any_upload(monkeypatch):
    from unirestore_amd import rvt
    monkeypatch.setattr(rvt, "PackedConvF32", lambda *a, **k: pytest.fail("a convolution was packed for a bad state dict"))
    cfg = rvt.RVTConfig(*TWO_STAGE)
    good = R.state_dict(TWO_STAGE, 41, 10)
    for key in _some_keys(good):
        missing = {k: v for k, v in good.items() if k != key}
        with pytest.raises(ValueError) as e:
            rvt.RVTWeights(cfg, missing, "cpu", source="bad.pth")
        assert "bad.pth" in str(e.value) and key in str(e.value)
        if key == "head.weight":
            continue                                               # its first axis is the class count: any [classes, C] matrix is taken
        shaped = dict(good, **{key: torch.zeros(*good[key].shape, 2)})
        with pytest.raises(ValueError) as e:
            rvt.RVTWeights(cfg, shaped, "cpu", source="bad.pth")
        assert "bad.pth" in str(e.value) and key in str(e.value) and "shape" in str(e.value)
        for value in (float("nan"), float("inf")):
            poisoned = dict(good, **{key: good[key].clone()})
            poisoned[key].view(-1)[-1] = value
            with pytest.raises(ValueError) as e:
                rvt.RVTWeights(cfg, poisoned, "cpu", source="bad.pth")
            assert "bad.pth" in str(e.value) and key in str(e.value) and "non-finite" in str(e.value)
    with pytest.raises(ValueError, match="head.weight"):
        rvt.RVTWeights(cfg, dict(good, **{"head.weight": torch.zeros(10, 65)}), "cpu")
    with pytest.raises(ValueError, match="running_var"):                         # var + eps <= 0: not a trained BatchNorm
        rvt.RVTWeights(cfg, dict(good, **{"patch_embed.proj.1.running_var": -torch.ones(32)}), "cpu")
    linear_fc1 = dict(good, **{"transformers.0.blocks.0.mlp.fc1.weight": torch.zeros(256, 64)})      # the Linear branch's shape in a conv-branch net
    with pytest.raises(ValueError, match="shape"):
        rvt.RVTWeights(cfg, linear_fc1, "cpu")


def test_config_refusals():
    from unirestore_amd import rvt
    assert set(rvt.ARCHS) == {"rvt_tiny", "rvt_tiny_plus", "rvt_small", "rvt_small_plus", "rvt_base", "rvt_base_plus"}
    assert rvt.ARCHS["rvt_tiny_plus"] == (224, (32, 32), (10, 2), (6, 12), 4, True, 10) and rvt.ARCHS["rvt_small_plus"][5:] == (True, 5)
    assert rvt.ARCHS["rvt_base"] == (224, (64,), (12,), (12,), 4, False, None) and rvt.ARCHS["rvt_base_plus"][5:] == (True, 5)
    assert all(rvt.config(rvt.RVTConfig(*rvt.ARCHS[a])) == rvt.ARCHS[a] == rvt.config(a) for a in rvt.ARCHS)     # the table passes its own checks
    assert rvt.S_MAX == 256 and rvt.stem_side(224) == 14 and rvt.stem_side(15) == 1 and rvt.stem_side(256) == 16
    assert rvt.config(rvt.RVTConfig(256, [64], [1], [2], 4, False, None)).base_dims == (64,)       # lists are taken; 256 tokens fit
    ok = dict(image_size=224, base_dims=(32, 32), depth=(2, 1), heads=(2, 4), mlp_ratio=4, use_mask=True, masked_block=1)
    for change, word in ((dict(base_dims=(48, 32)), "head dimension"), (dict(base_dims=(32,)), "same one or two stages"),
                         (dict(base_dims=(32, 32, 32), depth=(1, 1, 1), heads=(1, 2, 4)), "same one or two stages"),
                         (dict(depth=(2, 0)), ">= 1"), (dict(heads=(2, 3)), "no multiple"), (dict(image_size=272, use_mask=False), "tokens per image"),
                         (dict(image_size=14, use_mask=False), "at least 15"), (dict(image_size=192), "14 x 14"), (dict(masked_block=3), "masked_block"),
                         (dict(masked_block=None), "masked_block"), (dict(mlp_ratio=4.0), ">= 1"), (dict(use_mask=1), "use_mask")):
        with pytest.raises(ValueError) as e:
            rvt.config(rvt.RVTConfig(**dict(ok, **change)))
        assert word in str(e.value), (change, str(e.value))
    assert rvt.config(rvt.RVTConfig(**dict(ok, image_size=192, use_mask=False, masked_block=None))).image_size == 192      # unmasked: any size that fits
    for bad, word in (("rvt_huge", "unknown RVT arch"), ((224, (32,), (1,), (1,), 4, False, None), "rvt.RVTConfig"), (None, "rvt.RVTConfig")):
        with pytest.raises(ValueError, match=word):
            rvt.config(bad)
    with pytest.raises(ValueError, match="rvt_huge"):
        rvt.random_weights("rvt_huge", 0, 10, "cpu")


def test_random_state_dict_is_the_layout_of_every_arch():
    from unirestore_amd import rvt
    counts = {"rvt_tiny": 9 + 12 * 29 + 2 + 4, "rvt_tiny_plus": 9 + 12 * 29 + 10 + 2 + 4, "rvt_small_plus": 9 + 12 * 29 + 5 + 4,
              "rvt_base": 9 + 12 * 12 + 4, "rvt_base_plus": 9 + 12 * 12 + 5 + 4}
    for arch, count in counts.items():
        sd = rvt.random_state_dict(arch, 0, 7)
        assert len(sd) == count, arch
    sd = rvt.random_state_dict("rvt_tiny_plus", 1, 7)
    assert tuple(sd["transformers.0.blocks.9.attn.att_mask"].shape) == (6, 196, 196) and "transformers.1.blocks.0.attn.att_mask" not in sd
    assert tuple(sd["pools.0.conv.weight"].shape) == (384, 1, 3, 3) and tuple(sd["transformers.1.blocks.1.mlp.dwconv.weight"].shape) == (1536, 1, 3, 3)
    assert 0.9 < float(sd["transformers.0.blocks.3.attn.att_mask"].std()) < 1.1
    mean, var = sd["transformers.0.blocks.0.mlp.bn2.running_mean"], sd["transformers.0.blocks.0.mlp.bn2.running_var"]
    assert float(mean.abs().max()) > 0.1 and 0.5 <= float(var.min()) and float(var.max()) <= 1.5 and float(var.std()) > 0.2      # non-trivial statistics
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), rvt.random_state_dict("rvt_tiny_plus", 1, 7).values()))


def test_load_weights_reads_the_three_wrappings(tmp_path):
    from unirestore_amd import rvt
    cfg = rvt.RVTConfig(*TWO_STAGE)
    sd = rvt.random_state_dict(cfg, 3, 5)
    a = rvt.RVTWeights(cfg, sd, "cpu")
    published, plain, lit = tmp_path / "rvt.pth", tmp_path / "plain.pth", tmp_path / "lit.ckpt"
    torch.save({"model": sd}, str(published))
    torch.save(sd, str(plain))
    torch.save({"state_dict": {f"model.{k}": v for k, v in sd.items()}}, str(lit))
    for path in (published, plain, lit):
        b = rvt.load_weights(cfg, str(path), "cpu")
        assert set(a.cpu) == set(b.cpu) and all(torch.equal(a.cpu[k], b.cpu[k]) for k in a.cpu)
        assert all(torch.equal(a.linears[k].w, b.linears[k].w) and torch.equal(a.linears[k].bias, b.linears[k].bias) for k in a.linears)
        assert all(torch.equal(a.dwconvs[k][0], b.dwconvs[k][0]) and torch.equal(a.dwconvs[k][1], b.dwconvs[k][1]) for k in a.dwconvs)
        assert all(torch.equal(a.gates[k], b.gates[k]) for k in a.gates) and b.num_classes == 5
    torch.save({"model": {k: v for k, v in sd.items() if k != "norm.bias"}}, str(published))
    with pytest.raises(ValueError) as e:
        rvt.load_weights(cfg, str(published), "cpu")
    assert "rvt.pth" in str(e.value) and "norm.bias" in str(e.value)
    with pytest.raises(ValueError, match="rvt_x"):
        rvt.load_weights("rvt_x", str(lit), "cpu")


def test_litunifie_loads_an_arch_path_pair_through_the_module_its_arch_names(monkeypatch):
    from unirestore_amd import classify, runner, rvt, swin, vit
    tiny = rvt.RVTWeights(rvt.RVTConfig(*TWO_STAGE), R.state_dict(TWO_STAGE, 41, 10), "cpu")
    calls = []
    for name, module in (("rvt", rvt), ("swin", swin), ("vit", vit), ("classify", classify)):
        monkeypatch.setattr(module, "load_weights", lambda arch, path, name=name: calls.append((name, arch, path)) or tiny)
    lit = runner.LitUniFIE({}, model=object(), classifiers={"a": ("rvt_tiny_plus", "a.pth"), "b": tiny, "c": ("resnet50", "c.pth"),
                                                            "d": ("swin_v2_b", "d.pth"), "e": ("rvt_base", "e.pth")})
    assert calls == [("rvt", "rvt_tiny_plus", "a.pth"), ("classify", "resnet50", "c.pth"), ("swin", "swin_v2_b", "d.pth"), ("rvt", "rvt_base", "e.pth")]
    assert lit.classifiers["b"] is tiny and {"cls/a", "cls_input/a", "cls/b", "cls_input/b"} <= set(lit.totals)
    assert tuple(lit.totals["cls/a"].shape) == (3, 10)


# ---- the command line -------------------------------------------------------------------------------------------------------------

class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def test_rvt_argument(tmp_path, capsys):
    from unirestore_amd import cli
    w = str(tmp_path / "r.pth")
    open(w, "wb").close()                                          # the argument check looks for the file, it does not read it
    assert cli.check_rvt_arg(f"a=rvt_tiny_plus:{w},b=rvt_base:{w}") == {"a": ("rvt_tiny_plus", w), "b": ("rvt_base", w)}
    assert cli.check_rvt_arg({"a": ("rvt_small", w)}) == {"a": ("rvt_small", w)}
    assert cli.check_classifiers_arg(None, None, None, None) == (None, None)
    assert cli.check_classifiers_arg(f"r=resnet18:{w}", f"v=vit_b_16:{w}", f"s=swin_v2_b:{w}", f"t=rvt_tiny:{w}") == (
        {"r": ("resnet18", w), "v": ("vit_b_16", w), "s": ("swin_v2_b", w), "t": ("rvt_tiny", w)}, "--classify")
    assert cli.check_classifiers_arg(None, None, f"s=swin_v2_b:{w}", f"t=rvt_tiny:{w}") == ({"s": ("swin_v2_b", w), "t": ("rvt_tiny", w)}, "--swin")
    assert cli.check_classifiers_arg(None, None, None, f"t=rvt_tiny:{w}") == ({"t": ("rvt_tiny", w)}, "--rvt")
    for kw, flag in ((dict(classify={"a": ("resnet18", w)}), "--classify"), (dict(vit={"a": ("vit_b_16", w)}), "--vit"),
                     (dict(swin={"a": ("swin_v2_b", w)}), "--swin")):
        with pytest.raises(ValueError, match=f"'a' is used by {flag} too"):
            cli.check_rvt_arg(f"a=rvt_tiny:{w}", **kw)
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))        # its data yields no labels
    for kw, tasks, word in [
        (dict(rvt=f"a=swin_v2_b:{w}"), ["ir", "cls"], "swin_v2_b"),                             # an arch of another option
        (dict(rvt=f"a=rvt_tiny:{w}.none"), ["ir", "cls"], "no such file"),
        (dict(rvt="a=rvt_tiny"), ["ir", "cls"], "NAME=ARCH:WEIGHTS.pth"),
        (dict(rvt=f"a=rvt_tiny:{w},a=rvt_base:{w}"), ["ir", "cls"], "twice"),
        (dict(rvt=f"a=rvt_tiny:{w}", classify=f"a=resnet18:{w}"), ["ir", "cls"], "--classify too"),   # both would write val_lq/a
        (dict(rvt=f"a=rvt_tiny:{w}", vit=f"a=vit_b_16:{w}"), ["ir", "cls"], "--vit too"),
        (dict(rvt=f"a=rvt_tiny:{w}", swin=f"a=swin_v2_b:{w}"), ["ir", "cls"], "--swin too"),
        (dict(rvt=f"a=rvt_tiny:{w}"), None, "--rvt scores the 'cls' output"),
        (dict(rvt=f"a=rvt_tiny:{w}"), ["ir"], "--rvt scores the 'cls' output"),
        (dict(rvt=f"a=rvt_tiny:{w}"), ["ir", "cls"], "--rvt needs labels"),
        (dict(rvt=f"a=rvt_tiny:{w}", swin=f"s=swin_v2_b:{w}"), ["ir", "cls"], "--swin needs labels"),
    ]:
        with pytest.raises(ValueError) as e:
            cli.validate(cfg, tasks=tasks, model=_NoModel(), **kw)
        assert word in str(e.value), (kw, tasks, str(e.value))
    path = os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")
    for argv, word in ((["restore", "--config", path, "--rvt", f"a=rvt_tiny:{w}"], "--rvt belongs to validate"),
                       (["validate", "--config", path, "--rvt", f"a=rvt_tiny:{w}"], "--rvt scores the 'cls' output"),
                       (["validate", "--config", path, "--tasks", "ir,cls", "--rvt", f"a=rvt_tiny:{w}", "--swin", f"a=swin_v2_b:{w}"], "--swin too")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
