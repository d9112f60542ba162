"""Host restatement of the ViT scoring (torchvision's VisionTransformer: patch embedding, class token, positional embedding, encoder
blocks, final LayerNorm, head) and of each of its kernels, built from torch's own operators on the CPU and nothing of the
project's: F.layer_norm, F.multi_head_attention_forward (what torchvision's encoder block calls through nn.MultiheadAttention),
F.gelu, F.linear, F.conv2d; the stand-alone attention is torch.softmax(q k^T / 8) v.  dtype=torch.float64 is the yardstick;
torch.float32 is what an fp32 host evaluation of the same restatement computes - its distance from fp64 is the source of every GPU
tolerance.  Images are NCHW here, tokens [N,S,D] on both sides.  The weights are seeded stand-ins (vit.random_state_dict): nothing
here says anything about published accuracies.  torchvision is not installed where this is developed; the block's layout is
checked against torch's own nn.MultiheadAttention instead (test_vit_cpu.py)."""
import functools

import torch
import torch.nn.functional as F

import classify_reference as CR

GPU_FACTOR = 8                               # the rule of classify_reference.py: a GPU bound is 8 x fp32's own measured error
LN_EPS = 1e-6
HEAD_DIM = 64
S_MAX = 256                                  # ur_vit_attention_f32's limit (UR_VIT_S_MAX); the GPU test checks it is the library's

# ---- the cases ----------------------------------------------------------------------------------------------------------------
# name -> (rows, D, eps, mean of the inputs)
LN_CASES = {"1x1": (1, 1, 1e-6, 0.0), "3x7": (3, 7, 1e-6, 0.0), "5x64": (5, 64, 1e-6, 0.0), "5x64_eps1e-5": (5, 64, 1e-5, 0.0),
            "2x1000": (2, 1000, 1e-6, 0.0), "394x768": (394, 768, 1e-6, 0.0), "4x1024": (4, 1024, 1e-6, 0.0),
            "3x1300": (3, 1300, 1e-6, 0.0),                       # longer than the rows the kernel keeps in registers
            "mean1e4_4x768": (4, 768, 1e-6, 1e4)}                 # mean 1e4, std 1: E[x^2] - mean^2 has no digit left in fp32
LN_STRIDED = (3, 5, 64)                                           # [N,S,D]: row 0 of every image, rows S * D apart
GELU_SIZES = (1, 3, 4096, 4097)
EMBED_CASES = ((2, 1, 4), (1, 9, 6), (1, 9, 128), (2, 196, 768))  # (N, P, D)
# name -> (N, S, H, kind): "" plain; "big": q scaled until max |score| > 100; "constv": V constant per head
ATTN_CASES = {"1x1x1": (1, 1, 1, ""), "2x2x2": (2, 2, 2, ""), "1x31x1": (1, 31, 1, ""), "1x32x1": (1, 32, 1, ""), "2x33x3": (2, 33, 3, ""),
              "2x50x12": (2, 50, 12, ""), "1x64x2": (1, 64, 2, ""), "1x65x2": (1, 65, 2, ""), "2x197x12": (2, 197, 12, ""),
              "1xSMAXx1": (1, S_MAX, 1, ""), "big_2x50x2": (2, 50, 2, "big"), "constv_2x197x2": (2, 197, 2, "constv")}
BIG_Q = 40.0
# name -> ((image_size, patch_size, num_layers, num_heads, hidden_dim, mlp_dim) or an arch name, classes, weight seed, image seed, N)
NET_CASES = {"1layer_32px_s5": ((32, 16, 1, 1, 64, 128), 10, 1, 1, 3), "2layer_p16_s197": ((224, 16, 2, 2, 128, 256), 10, 2, 2, 2),
             "2layer_p32_s50": ((224, 32, 2, 3, 192, 384), 10, 3, 3, 2), "vit_b_16": ("vit_b_16", 1000, 4, 4, 2)}
FORWARD_CASE = ("vit_b_16", 1000, 4, 6, (3, 3, 75, 101))         # arch, classes, weight seed, image seed, image shape
TINY_224 = (224, 32, 1, 1, 64, 128)                               # the smallest network the evaluator's 224 x 224 preprocess feeds

# ---- the tolerances: fp32's OWN error against fp64 on these cases, measured with the restatement below on the CPU (measure_*),
# each relative to the case's max |fp64 result|, and GPU_FACTOR x that for the GPU.  A case torch's fp32 gets exactly right (a
# one-element row, a single key) has the bound 0: the kernel must be exact there too.
E32_LN = {"1x1": 0.0, "3x7": 6.39e-08, "5x64": 1.06e-07, "5x64_eps1e-5": 1.22e-07, "2x1000": 6.59e-08, "394x768": 1.49e-07,
          "4x1024": 1.50e-07, "3x1300": 8.44e-08, "mean1e4_4x768": 2.93e-04}      # (mean 1e4: fp32's mean is ~1e-3 off, of a std of 1)
E32_LN_STRIDED = 1.01e-07
E32_GELU = 6.96e-08                          # of 10, the largest result on the grid
E32_ATTN = {"1x1x1": 0.0, "2x2x2": 9.78e-08, "1x31x1": 2.54e-07, "1x32x1": 4.09e-07, "2x33x3": 3.32e-07, "2x50x12": 6.33e-07,
            "1x64x2": 4.69e-07, "1x65x2": 6.60e-07, "2x197x12": 6.61e-07, "1xSMAXx1": 9.54e-07, "big_2x50x2": 4.85e-06,
            "constv_2x197x2": 7.37e-07}
# per NET_CASES entry, max |logits32 - logits64| / max |logits64| (the stand-in logits reach |max| 1.1 .. 2.4)
E32_LOGITS = {"1layer_32px_s5": 2.33e-07, "2layer_p16_s197": 2.73e-07, "2layer_p32_s50": 3.04e-07, "vit_b_16": 4.74e-07}
E32_FORWARD = 6.26e-07                       # the same for FORWARD_CASE (preprocess + network; |max| 2.0)
LN_TOL = {k: GPU_FACTOR * v for k, v in E32_LN.items()}
LN_STRIDED_TOL = GPU_FACTOR * E32_LN_STRIDED
GELU_TOL = GPU_FACTOR * E32_GELU
ATTN_TOL = {k: GPU_FACTOR * v for k, v in E32_ATTN.items()}
LOGITS_TOL = {k: GPU_FACTOR * v for k, v in E32_LOGITS.items()}
FORWARD_TOL = GPU_FACTOR * E32_FORWARD


def _gen(*key):
    """A generator seeded by a tuple of integers."""
    seed = 0
    for k in key:
        seed = (seed * 1000003 + k + 1) % ((1 << 31) - 1)
    return torch.Generator().manual_seed(seed)


def rel_err(got, want):
    """max |got - want| / max |want| in fp64 (0 / 0 = 0: a case whose result is all zeros)."""
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    return err / scale if scale > 0 else err


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------

def layer_norm(x, gamma, beta, eps, dtype=torch.float64):
    return F.layer_norm(x.to(dtype), (x.shape[-1],), gamma.to(dtype), beta.to(dtype), eps)


def ln_case(name):
    """(x [rows, D], gamma, beta, eps) of an LN_CASES entry, fp32."""
    rows, d, eps, mean = LN_CASES[name]
    g = _gen(11, sorted(LN_CASES).index(name))
    return torch.randn(rows, d, generator=g) + mean, 0.5 + torch.rand(d, generator=g), 0.1 * torch.randn(d, generator=g), eps


def ln_strided_case():
    n, s, d = LN_STRIDED
    g = _gen(12, 0)
    return torch.randn(n, s, d, generator=g), 0.5 + torch.rand(d, generator=g), 0.1 * torch.randn(d, generator=g), LN_EPS


def measure_ln(name):
    x, gamma, beta, eps = ln_case(name)
    return rel_err(layer_norm(x, gamma, beta, eps, torch.float32), layer_norm(x, gamma, beta, eps))


def measure_ln_strided():
    x, gamma, beta, eps = ln_strided_case()
    return rel_err(layer_norm(x[:, 0], gamma, beta, eps, torch.float32), layer_norm(x[:, 0], gamma, beta, eps))


# ---- GELU ---------------------------------------------------------------------------------------------------------------------

def gelu(x, dtype=torch.float64):
    return F.gelu(x.to(dtype))                                    # approximate="none": 0.5 x (1 + erf(x / sqrt 2))


def gelu_values():
    """The grid [-10, 10] from the top down (every prefix holds 10, the largest result), then +-0 and subnormals."""
    grid = torch.linspace(-10, 10, 4001).flip(0)
    return torch.cat([grid, torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45])]).float()


def gelu_case(n):
    """n values: gelu_values(), repeated as often as needed."""
    v = gelu_values()
    return v.repeat((n + v.numel() - 1) // v.numel())[:n].clone()


def measure_gelu():
    x = gelu_values()
    return rel_err(gelu(x, torch.float32), gelu(x))


# ---- the class token and the positional embedding -----------------------------------------------------------------------------

def embed(patches, class_token, pos, dtype=torch.float64):
    """patches [N,P,D], class_token [D], pos [P+1,D] -> [N,P+1,D]."""
    n = patches.shape[0]
    return torch.cat([class_token.to(dtype).expand(n, 1, -1), patches.to(dtype)], dim=1) + pos.to(dtype)


def embed_case(shape):
    n, p, d = shape
    g = _gen(13, n, p, d)
    return torch.randn(n, p, d, generator=g), torch.randn(d, generator=g), torch.randn(p + 1, d, generator=g)


# ---- attention ----------------------------------------------------------------------------------------------------------------

def scores(qkv, heads, dtype=torch.float64):
    """[N, H, S, S]: q k^T / sqrt(64) per head, from qkv [N,S,3D] laid out q | k | v with head h in columns 64 h .. 64 h + 63."""
    n, s, d3 = qkv.shape
    q, k, _v = (t.reshape(n, s, heads, HEAD_DIM).transpose(1, 2) for t in qkv.to(dtype).split(d3 // 3, dim=2))
    return (q * 0.125) @ k.transpose(2, 3)


def attention(qkv, heads, dtype=torch.float64):
    """softmax(q k^T / 8) v per (image, head), heads concatenated: [N,S,D]."""
    n, s, d3 = qkv.shape
    v = qkv.to(dtype)[:, :, 2 * d3 // 3:].reshape(n, s, heads, HEAD_DIM).transpose(1, 2)
    return (torch.softmax(scores(qkv, heads, dtype), dim=-1) @ v).transpose(1, 2).reshape(n, s, d3 // 3)


@functools.lru_cache(maxsize=None)
def attn_case(name):
    """qkv fp32 [N,S,3D] of an ATTN_CASES entry (callers must not modify it)."""
    n, s, h, kind = ATTN_CASES[name]
    d = h * HEAD_DIM
    g = _gen(14, sorted(ATTN_CASES).index(name))
    qkv = torch.randn(n, s, 3 * d, generator=g)
    if kind == "big":
        qkv[:, :, :d] *= BIG_Q
    if kind == "constv":
        qkv[:, :, 2 * d:] = (1.0 + torch.rand(n, 1, h, 1, generator=g)).expand(n, s, h, HEAD_DIM).reshape(n, s, d)
    return qkv


@functools.lru_cache(maxsize=None)
def attn_reference(name):
    return attention(attn_case(name), ATTN_CASES[name][2])


def measure_attn(name):
    return rel_err(attention(attn_case(name), ATTN_CASES[name][2], torch.float32), attn_reference(name))


# ---- the network (torchvision.models.vision_transformer: EncoderBlock, Encoder, VisionTransformer) ----------------------------

def block(x, sd, pre, heads, dtype):
    """One EncoderBlock on tokens [N,S,D]: x + attn(ln_1(x)), then + mlp(ln_2(.)).  nn.MultiheadAttention(batch_first=True) is
    F.multi_head_attention_forward on the sequence-first transpose."""
    p = lambda k: sd[f"{pre}.{k}"].to(dtype)                      # noqa: E731
    d = x.shape[2]
    y = F.layer_norm(x, (d,), p("ln_1.weight"), p("ln_1.bias"), LN_EPS).transpose(0, 1)
    y, _ = F.multi_head_attention_forward(y, y, y, d, heads, p("self_attention.in_proj_weight"), p("self_attention.in_proj_bias"), None, None,
                                          False, 0.0, p("self_attention.out_proj.weight"), p("self_attention.out_proj.bias"),
                                          training=False, need_weights=False)
    x = x + y.transpose(0, 1)
    y = F.layer_norm(x, (d,), p("ln_2.weight"), p("ln_2.bias"), LN_EPS)
    y = F.linear(F.gelu(F.linear(y, p("mlp.0.weight"), p("mlp.0.bias"))), p("mlp.3.weight"), p("mlp.3.bias"))
    return x + y


def vit(x, sd, cfg, dtype=torch.float64):
    """x: the network's NCHW input (already preprocessed), sd: a torchvision state dict, cfg: (image_size, patch_size, num_layers,
    num_heads, hidden_dim, mlp_dim) -> logits [N, classes] of dtype."""
    _size, patch, layers, heads, d, _mlp = cfg
    n = x.shape[0]
    t = F.conv2d(x.to(dtype), sd["conv_proj.weight"].to(dtype), sd["conv_proj.bias"].to(dtype), stride=patch)
    t = t.reshape(n, d, -1).permute(0, 2, 1)
    t = torch.cat([sd["class_token"].to(dtype).expand(n, -1, -1), t], dim=1) + sd["encoder.pos_embedding"].to(dtype)
    for i in range(layers):
        t = block(t, sd, f"encoder.layers.encoder_layer_{i}", heads, dtype)
    t = F.layer_norm(t, (d,), sd["encoder.ln.weight"].to(dtype), sd["encoder.ln.bias"].to(dtype), LN_EPS)[:, 0]
    return F.linear(t, sd["heads.head.weight"].to(dtype), sd["heads.head.bias"].to(dtype))


def net_config(spec):
    """A NET_CASES / FORWARD_CASE network as a vit.ViTConfig."""
    from unirestore_amd import vit as V
    return V.config(spec) if isinstance(spec, str) else V.ViTConfig(*spec)


@functools.lru_cache(maxsize=None)
def state_dict(spec, seed, classes):
    """The seeded stand-in weights of a case (host only; callers must not modify them)."""
    from unirestore_amd import vit as V
    return V.random_state_dict(spec if isinstance(spec, str) else V.ViTConfig(*spec), seed, classes)


def net_input(name):
    """The already-preprocessed NCHW fp32 input of a NET_CASES entry: varied images of the network's size, normalised."""
    spec, _classes, _wseed, iseed, n = NET_CASES[name]
    size = net_config(spec).image_size
    return CR.normalise(CR.varied_images(n, size, size, iseed), torch.float32)


@functools.lru_cache(maxsize=None)
def net_reference(name):
    """fp64 logits of a NET_CASES entry (computed once per process; callers must not modify them)."""
    spec, classes, wseed = NET_CASES[name][:3]
    return vit(net_input(name), state_dict(spec, wseed, classes), net_config(spec))


def measure_logits(name):
    spec, classes, wseed = NET_CASES[name][:3]
    return rel_err(vit(net_input(name), state_dict(spec, wseed, classes), net_config(spec), torch.float32), net_reference(name))


def forward_images():
    return CR.varied_images(FORWARD_CASE[4][0], FORWARD_CASE[4][2], FORWARD_CASE[4][3], FORWARD_CASE[3])


@functools.lru_cache(maxsize=None)
def forward_reference():
    spec, classes, wseed = FORWARD_CASE[:3]
    return vit(CR.preprocess(forward_images()), state_dict(spec, wseed, classes), net_config(spec))


def measure_forward():
    spec, classes, wseed = FORWARD_CASE[:3]
    got = vit(CR.preprocess_einsum32(forward_images()), state_dict(spec, wseed, classes), net_config(spec), torch.float32)
    return rel_err(got, forward_reference())


top2_gap = CR.top2_gap


def classes_of(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, per element."""
    return torch.where(torch.isnan(t), 3, torch.where(t == float("inf"), 1, torch.where(t == float("-inf"), 2, 0)))
