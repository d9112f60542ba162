"""Host restatement of the Swin-V2 scoring (torchvision's SwinTransformer with SwinTransformerBlockV2 and PatchMergingV2: patch
embedding, post-norm blocks of shifted-window cosine attention and an MLP, patch merging, final LayerNorm, mean, head) and of its two
new kernels, built from torch's own operators on the CPU and nothing of the project's: F.pad, torch.roll, view / permute,
F.normalize, F.linear, masked_fill, F.softmax, F.layer_norm, F.gelu, F.conv2d.  It is written the way torchvision writes it - an
explicit padded tensor, an explicit mask tensor filled by slice assignment of region counts, the relative-position index built from
a meshgrid - so it shares nothing with the kernel's index arithmetic.  dtype=torch.float64 is the yardstick; torch.float32 is what an
fp32 host evaluation of the same restatement computes - its distance from fp64 is the source of every GPU tolerance.  Images are
NCHW here, token maps [N,H,W,C] on both sides.  The weights are seeded stand-ins (swin.random_state_dict): nothing here says
anything about published accuracies.  torchvision is not installed where this is developed: the forward is restated from its
source (models/swin_transformer.py) as recalled, unchecked against the package."""
import functools
import math

import torch
import torch.nn.functional as F

import classify_reference as CR

GPU_FACTOR = 8                               # the rule of classify_reference.py: a GPU bound is 8 x fp32's own measured error
LN_EPS = 1e-5
WINDOW = 8
HEAD_DIM = 32

# ---- the cases ----------------------------------------------------------------------------------------------------------------
# name -> (N, H, W, heads, shift, kind): "" plain; "clamp": logit_scale = 10 (the clamp at log 100 binds) and k = +-q per token, so
# scores reach +-100; "zero": a quarter of the q rows and a quarter of the k rows are zero (the 1e-12 floor of F.normalize)
ATTN_CASES = {"1x8x8x1_s0": (1, 8, 8, 1, 0, ""),             # one window
              "1x8x8x1_s4": (1, 8, 8, 1, 4, ""),             # shift forced to 0 on both axes
              "1x16x16x2_s4": (1, 16, 16, 2, 4, ""),         # 2 x 2 windows, all nine mask regions
              "2x12x12x3_s4": (2, 12, 12, 3, 4, ""),         # pad to 16: pad tokens are rolled into windows
              "1x7x7x4_s4": (1, 7, 7, 4, 4, ""),             # the last stage: pad to 8, no shift
              "1x8x20x1_s4": (1, 8, 20, 1, 4, ""),           # shift 0 on H and 4 on W, W padded to 24
              "2x28x28x8_s4": (2, 28, 28, 8, 4, ""),         # stage 2 of the real net
              "1x56x56x4_s4": (1, 56, 56, 4, 4, ""),         # stage 1, N = 1
              "clamp_1x16x16x2_s4": (1, 16, 16, 2, 4, "clamp"), "zero_2x12x12x3_s4": (2, 12, 12, 3, 4, "zero")}
# the case with a non-zero k bias in the checkpoint, through the loader and the qkv Linear: (config, weight seed, block, N, H, W)
KBIAS_CASE = ((48, 4, 64, (2,), (2,)), 21, "features.1.1", 2, 12, 12)
LNRES_CASES = {"1x1": (1, 1), "3x7": (3, 7), "5x96": (5, 96), "64x128": (64, 128), "9x1024": (9, 1024), "3x1300": (3, 1300)}   # (rows, D)
# name -> ((image_size, patch_size, embed_dim, depths, num_heads) or an arch name, classes, weight seed, image seed, N)
NET_CASES = {"32px_8_4": ((32, 4, 32, (2, 2), (1, 2)), 10, 1, 1, 3),                        # maps 8 -> 4
             "48px_12_6_3": ((48, 4, 32, (2, 2, 2), (1, 2, 4)), 10, 2, 2, 2),               # padding, shift and mask all active
             "224px_e32": ((224, 4, 32, (2, 2, 2, 2), (1, 2, 4, 8)), 10, 3, 3, 2),
             "swin_v2_t": ("swin_v2_t", 1000, 4, 4, 2)}
FORWARD_CASE = ("swin_v2_b", 1000, 5, 6, (2, 3, 75, 101))         # arch, classes, weight seed, image seed, image shape
TINY_224 = (224, 4, 32, (1, 1), (1, 2))                           # the smallest network the evaluator's 224 x 224 preprocess feeds

# ---- the tolerances: fp32's OWN error against fp64 on these cases, measured with the restatement below on the CPU (measure_*),
# each relative to the case's max |fp64 result|, and GPU_FACTOR x that for the GPU.  A case torch's fp32 gets exactly right would
# have the bound 0.
E32_ATTN = {"1x8x8x1_s0": 5.36e-07, "1x8x8x1_s4": 4.00e-07, "1x16x16x2_s4": 5.78e-07, "2x12x12x3_s4": 5.96e-07, "1x7x7x4_s4": 3.67e-07,
            "1x8x20x1_s4": 5.31e-07, "2x28x28x8_s4": 6.02e-07, "1x56x56x4_s4": 7.41e-07, "clamp_1x16x16x2_s4": 2.42e-06,
            "zero_2x12x12x3_s4": 4.61e-07}      # (clamp: scores of +-100 carry an absolute error of 100 x 2^-24 into exp)
E32_KBIAS = 8.82e-07                         # (the qkv Linear in fp32 is part of this case)
E32_LNRES = {"1x1": 0.0, "3x7": 9.01e-08, "5x96": 7.60e-08, "64x128": 1.35e-07, "9x1024": 1.03e-07, "3x1300": 1.25e-07}   # (1x1: res + beta, exact here)
# per NET_CASES entry, max |logits32 - logits64| / max |logits64| (the stand-in logits reach |max| 1.1 .. 2.2)
E32_LOGITS = {"32px_8_4": 1.77e-07, "48px_12_6_3": 6.70e-07, "224px_e32": 2.89e-07, "swin_v2_t": 3.29e-07}
E32_FORWARD = 3.59e-07                       # the same for FORWARD_CASE (preprocess + network; |max| 2.0)
ATTN_TOL = {k: GPU_FACTOR * v for k, v in E32_ATTN.items()}
KBIAS_TOL = GPU_FACTOR * E32_KBIAS
LNRES_TOL = {k: GPU_FACTOR * v for k, v in E32_LNRES.items()}
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


top2_gap = CR.top2_gap


def classes_of(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, per element."""
    return torch.where(torch.isnan(t), 3, torch.where(t == float("inf"), 1, torch.where(t == float("-inf"), 2, 0)))


# ---- the residual LayerNorm ---------------------------------------------------------------------------------------------------

def layer_norm_res(x, res, gamma, beta, eps=LN_EPS, dtype=torch.float64):
    return res.to(dtype) + F.layer_norm(x.to(dtype), (x.shape[-1],), gamma.to(dtype), beta.to(dtype), eps)


def lnres_case(name):
    """(x [rows, D], res, gamma, beta) of an LNRES_CASES entry, fp32."""
    rows, d = LNRES_CASES[name]
    g = _gen(31, sorted(LNRES_CASES).index(name))
    return torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g), 0.5 + torch.rand(d, generator=g), 0.1 * torch.randn(d, generator=g)


def measure_lnres(name):
    case = lnres_case(name)
    return rel_err(layer_norm_res(*case, dtype=torch.float32), layer_norm_res(*case))


# ---- shifted-window attention, as torchvision.models.swin_transformer.shifted_window_attention --------------------------------

def relative_position_index():
    """[4096] int64, as SwinTransformerBlock's ShiftedWindowAttention.define_relative_position_index builds it."""
    coords = torch.stack(torch.meshgrid(torch.arange(WINDOW), torch.arange(WINDOW), indexing="ij"))      # 2, 8, 8
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()                            # 64, 64, 2
    rel[:, :, 0] += WINDOW - 1
    rel[:, :, 1] += WINDOW - 1
    rel[:, :, 0] *= 2 * WINDOW - 1
    return rel.sum(-1).flatten()


def relative_coords_table(dtype=torch.float64):
    """[1, 15, 15, 2], as ShiftedWindowAttentionV2.define_relative_coords_table builds it."""
    r = torch.arange(-(WINDOW - 1), WINDOW, dtype=dtype)
    table = torch.stack(torch.meshgrid([r, r], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
    table[:, :, :, 0] /= WINDOW - 1
    table[:, :, :, 1] /= WINDOW - 1
    table *= 8
    return torch.sign(table) * torch.log2(torch.abs(table) + 1.0) / 3.0


def position_bias(w0, b0, w2, dtype=torch.float64):
    """[heads, 64, 64]: 16 sigmoid(cpb_mlp(table))[index], cpb_mlp = Linear(2, 512) -> ReLU -> Linear(512, heads, bias=False)."""
    heads = w2.shape[0]
    table = F.linear(F.relu(F.linear(relative_coords_table(dtype), w0.to(dtype), b0.to(dtype))), w2.to(dtype)).view(-1, heads)
    bias = table[relative_position_index()].view(WINDOW * WINDOW, WINDOW * WINDOW, -1).permute(2, 0, 1).contiguous()
    return 16 * torch.sigmoid(bias)


def pad_roll_partition(x, shift):
    """x [N,H,W,D] -> (windows [N * nW, 64, D], (pH, pW), (shift_y, shift_x)): zero padding on the bottom and right to multiples of
    8, per axis no shift when the window covers the padded axis, torch.roll by the negative shifts, row-major 8 x 8 windows."""
    n, h, w, d = x.shape
    pad_r, pad_b = (WINDOW - w % WINDOW) % WINDOW, (WINDOW - h % WINDOW) % WINDOW
    x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
    _, ph, pw, _ = x.shape
    shifts = [shift, shift]
    if WINDOW >= ph:
        shifts[0] = 0
    if WINDOW >= pw:
        shifts[1] = 0
    if sum(shifts) > 0:
        x = torch.roll(x, shifts=(-shifts[0], -shifts[1]), dims=(1, 2))
    x = x.view(n, ph // WINDOW, WINDOW, pw // WINDOW, WINDOW, d).permute(0, 1, 3, 2, 4, 5).reshape(-1, WINDOW * WINDOW, d)
    return x, (ph, pw), shifts


def reverse_unroll_crop(x, n, h, w, padded, shifts):
    """The inverse: windows [N * nW, 64, C] -> [N,H,W,C]."""
    ph, pw = padded
    c = x.shape[-1]
    x = x.view(n, ph // WINDOW, pw // WINDOW, WINDOW, WINDOW, c).permute(0, 1, 3, 2, 4, 5).reshape(n, ph, pw, c)
    if sum(shifts) > 0:
        x = torch.roll(x, shifts=(shifts[0], shifts[1]), dims=(1, 2))
    return x[:, :h, :w, :].contiguous()


def region_mask(padded, shifts, dtype):
    """[nW, 64, 64]: 0 where two slots of a window lie in one region of the rolled map, -100 where they do not (not -inf)."""
    ph, pw = padded
    mask = torch.zeros((ph, pw), dtype=dtype)
    h_slices = ((0, -WINDOW), (-WINDOW, -shifts[0]), (-shifts[0], None))
    w_slices = ((0, -WINDOW), (-WINDOW, -shifts[1]), (-shifts[1], None))
    count = 0
    for hs in h_slices:
        for ws in w_slices:
            mask[hs[0]:hs[1], ws[0]:ws[1]] = count
            count += 1
    mask = mask.view(ph // WINDOW, WINDOW, pw // WINDOW, WINDOW).permute(0, 2, 1, 3).reshape(-1, WINDOW * WINDOW)
    mask = mask.unsqueeze(1) - mask.unsqueeze(2)
    return mask.masked_fill(mask != 0, -100.0).masked_fill(mask == 0, 0.0)


def window_core(qkv, heads, logit_scale, bias, padded, shifts):
    """qkv windows [B_, 64, 3C] -> [B_, 64, C]: cosine scores, temperature, relative-position bias, region mask, softmax, @ v."""
    b_, t, c3 = qkv.shape
    c = c3 // 3
    q, k, v = qkv.reshape(b_, t, 3, heads, c // heads).permute(2, 0, 3, 1, 4)
    attn = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
    attn = attn * torch.clamp(logit_scale.to(qkv.dtype).view(heads, 1, 1), max=math.log(100.0)).exp()
    attn = attn + bias.to(qkv.dtype).unsqueeze(0)
    if sum(shifts) > 0:
        mask = region_mask(padded, shifts, qkv.dtype)
        nw = mask.shape[0]
        attn = attn.view(b_ // nw, nw, heads, t, t) + mask.unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, heads, t, t)
    attn = F.softmax(attn, dim=-1)
    return attn.matmul(v).transpose(1, 2).reshape(b_, t, c)


def attention_from_x(x, qkv_w, qkv_b, logit_scale, bias, heads, shift, dtype=torch.float64):
    """torchvision's shifted_window_attention up to (not including) proj, from the block's input x [N,H,W,C]: the padded map goes
    through the qkv Linear, with the k third of its bias zeroed."""
    n, h, w, c = x.shape
    xw, padded, shifts = pad_roll_partition(x.to(dtype), shift)
    qkv_b = qkv_b.to(dtype).clone()
    qkv_b[c:2 * c].zero_()
    out = window_core(F.linear(xw, qkv_w.to(dtype), qkv_b), heads, logit_scale, bias, padded, shifts)
    return reverse_unroll_crop(out, n, h, w, padded, shifts)


def attention_from_qkv(qkv, qkv_bias, logit_scale, bias, heads, shift, dtype=torch.float64):
    """What ur_swin_attention_f32 is given: qkv [N,H,W,3C] of the real tokens and qkv_bias [3C], a zero-padded token's q | k | v
    (the Linear of a zero row).  The explicit padded tensor: qkv and an all-ones map are zero-padded alike, and the padded
    positions take qkv_bias."""
    n, h, w, c3 = qkv.shape
    qw, padded, shifts = pad_roll_partition(qkv.to(dtype), shift)
    real, _, _ = pad_roll_partition(torch.ones(n, h, w, 1, dtype=dtype), shift)
    qw = torch.where(real != 0, qw, qkv_bias.to(dtype).view(1, 1, c3))
    out = window_core(qw, heads, logit_scale, bias, padded, shifts)
    return reverse_unroll_crop(out, n, h, w, padded, shifts)


@functools.lru_cache(maxsize=None)
def attn_case(name):
    """(qkv [N,H,W,3C], qkv_bias [3C] with its k third zero, logit_scale [heads], bias [heads,64,64]) of an ATTN_CASES entry, fp32
    (callers must not modify them).  The bias is random per (head, query slot, key slot) in (0, 16) - no relative structure, so a
    transposed or shifted table lookup shows."""
    n, h, w, heads, _shift, kind = ATTN_CASES[name]
    c = heads * HEAD_DIM
    g = _gen(32, sorted(ATTN_CASES).index(name))
    qkv = torch.randn(n, h, w, 3 * c, generator=g)
    qkv_bias = 0.5 * torch.randn(3 * c, generator=g)
    qkv_bias[c:2 * c] = 0
    logit_scale = math.log(10.0) + 0.3 * torch.randn(heads, generator=g)
    bias = 16 * torch.sigmoid(1.5 * torch.randn(heads, WINDOW ** 2, WINDOW ** 2, generator=g))
    if kind == "clamp":
        logit_scale = torch.full((heads,), 10.0)
        sign = (torch.rand(n, h, w, 1, generator=g) > 0.5).float() * 2 - 1
        qkv[..., c:2 * c] = qkv[..., :c] * sign
    if kind == "zero":
        qkv[..., :c] *= (torch.rand(n, h, w, 1, generator=g) > 0.25).float()
        qkv[..., c:2 * c] *= (torch.rand(n, h, w, 1, generator=g) > 0.25).float()
    return qkv, qkv_bias, logit_scale, bias


def attn_scale(name):
    """scale [heads] fp32 as the loader computes it: exp(min(logit_scale, log 100)) in fp64, rounded once."""
    return torch.exp(attn_case(name)[2].double().clamp(max=math.log(100.0))).float()


@functools.lru_cache(maxsize=None)
def attn_reference(name):
    _n, _h, _w, heads, shift, _kind = ATTN_CASES[name]
    return attention_from_qkv(*attn_case(name), heads, shift)


def measure_attn(name):
    _n, _h, _w, heads, shift, _kind = ATTN_CASES[name]
    return rel_err(attention_from_qkv(*attn_case(name), heads, shift, torch.float32), attn_reference(name))


def kbias_case():
    """(x [N,H,W,C] fp32, state dict, block prefix, heads) of KBIAS_CASE: a block whose checkpoint holds a non-zero k bias."""
    spec, wseed, pre, n, h, w = KBIAS_CASE
    sd = state_dict(spec, wseed, 10)
    return torch.randn(n, h, w, spec[2], generator=_gen(33, 0)), sd, pre, spec[4][0]


def kbias_attention(dtype=torch.float64, keep_k_bias=False):
    x, sd, pre, heads = kbias_case()
    bias = position_bias(sd[f"{pre}.attn.cpb_mlp.0.weight"], sd[f"{pre}.attn.cpb_mlp.0.bias"], sd[f"{pre}.attn.cpb_mlp.2.weight"], dtype)
    qkv_w, qkv_b = sd[f"{pre}.attn.qkv.weight"], sd[f"{pre}.attn.qkv.bias"]
    if keep_k_bias:                                              # what a forward that did NOT zero it would compute: for the CPU test
        n, h, w, _ = x.shape
        xw, padded, shifts = pad_roll_partition(x.to(dtype), KBIAS_SHIFT)
        out = window_core(F.linear(xw, qkv_w.to(dtype), qkv_b.to(dtype)), heads, sd[f"{pre}.attn.logit_scale"], bias, padded, shifts)
        return reverse_unroll_crop(out, n, h, w, padded, shifts)
    return attention_from_x(x, qkv_w, qkv_b, sd[f"{pre}.attn.logit_scale"], bias, heads, KBIAS_SHIFT, dtype)


KBIAS_SHIFT = 4                                                   # features.1.1 is an odd block


@functools.lru_cache(maxsize=None)
def kbias_reference():
    return kbias_attention()


def measure_kbias():
    return rel_err(kbias_attention(torch.float32), kbias_reference())


# ---- the network (torchvision.models.swin_transformer: SwinTransformerBlockV2, PatchMergingV2, SwinTransformer) ---------------

def block(x, sd, pre, heads, shift, dtype):
    """One SwinTransformerBlockV2 on [N,H,W,C]: x + norm1(attn(x)), then + norm2(mlp(.)) - post-norm."""
    p = lambda k: sd[f"{pre}.{k}"].to(dtype)                      # noqa: E731
    c = x.shape[3]
    bias = position_bias(p("attn.cpb_mlp.0.weight"), p("attn.cpb_mlp.0.bias"), p("attn.cpb_mlp.2.weight"), dtype)
    a = attention_from_x(x, p("attn.qkv.weight"), p("attn.qkv.bias"), p("attn.logit_scale"), bias, heads, shift, dtype)
    a = F.linear(a, p("attn.proj.weight"), p("attn.proj.bias"))
    x = x + F.layer_norm(a, (c,), p("norm1.weight"), p("norm1.bias"), LN_EPS)
    y = F.linear(F.gelu(F.linear(x, p("mlp.0.weight"), p("mlp.0.bias"))), p("mlp.3.weight"), p("mlp.3.bias"))
    return x + F.layer_norm(y, (c,), p("norm2.weight"), p("norm2.bias"), LN_EPS)


def patch_merging(x, sd, pre, dtype):
    """PatchMergingV2 on [N,H,W,C] (H, W even): norm(reduction(cat of the four 2 x 2 taps)) -> [N,H/2,W/2,2C]."""
    x = torch.cat([x[..., 0::2, 0::2, :], x[..., 1::2, 0::2, :], x[..., 0::2, 1::2, :], x[..., 1::2, 1::2, :]], -1)
    x = F.linear(x, sd[f"{pre}.reduction.weight"].to(dtype))
    return F.layer_norm(x, (x.shape[-1],), sd[f"{pre}.norm.weight"].to(dtype), sd[f"{pre}.norm.bias"].to(dtype), LN_EPS)


def swin(x, sd, cfg, dtype=torch.float64):
    """x: the network's NCHW input (already preprocessed), sd: a torchvision state dict, cfg: (image_size, patch_size, embed_dim,
    depths, num_heads) -> logits [N, classes] of dtype."""
    _size, patch, e, depths, num_heads = cfg
    t = F.conv2d(x.to(dtype), sd["features.0.0.weight"].to(dtype), sd["features.0.0.bias"].to(dtype), stride=patch).permute(0, 2, 3, 1)
    t = F.layer_norm(t, (e,), sd["features.0.2.weight"].to(dtype), sd["features.0.2.bias"].to(dtype), LN_EPS)
    for i, depth in enumerate(depths):
        for j in range(depth):
            t = block(t, sd, f"features.{2 * i + 1}.{j}", num_heads[i], 0 if j % 2 == 0 else WINDOW // 2, dtype)
        if i < len(depths) - 1:
            t = patch_merging(t, sd, f"features.{2 * i + 2}", dtype)
    t = F.layer_norm(t, (t.shape[-1],), sd["norm.weight"].to(dtype), sd["norm.bias"].to(dtype), LN_EPS)
    t = t.permute(0, 3, 1, 2).mean(dim=(2, 3))                    # AdaptiveAvgPool2d(1) + flatten
    return F.linear(t, sd["head.weight"].to(dtype), sd["head.bias"].to(dtype))


def net_config(spec):
    """A NET_CASES / FORWARD_CASE network as a swin.SwinConfig."""
    from unirestore_amd import swin as S
    return S.config(spec) if isinstance(spec, str) else S.SwinConfig(*spec)


@functools.lru_cache(maxsize=None)
def state_dict(spec, seed, classes):
    """The seeded stand-in weights of a case (host only; callers must not modify them)."""
    from unirestore_amd import swin as S
    return S.random_state_dict(spec if isinstance(spec, str) else S.SwinConfig(*spec), seed, classes)


def net_input(name):
    """The already-preprocessed NCHW fp32 input of a NET_CASES entry: varied images of the network's size, normalised."""
    spec, _classes, _wseed, iseed, n = NET_CASES[name]
    size = net_config(spec).image_size
    return CR.normalise(CR.varied_images(n, size, size, iseed), torch.float32)


@functools.lru_cache(maxsize=None)
def net_reference(name):
    """fp64 logits of a NET_CASES entry (computed once per process; callers must not modify them)."""
    spec, classes, wseed = NET_CASES[name][:3]
    return swin(net_input(name), state_dict(spec, wseed, classes), net_config(spec))


def measure_logits(name):
    spec, classes, wseed = NET_CASES[name][:3]
    return rel_err(swin(net_input(name), state_dict(spec, wseed, classes), net_config(spec), torch.float32), net_reference(name))


def forward_images():
    return CR.varied_images(FORWARD_CASE[4][0], FORWARD_CASE[4][2], FORWARD_CASE[4][3], FORWARD_CASE[3])


@functools.lru_cache(maxsize=None)
def forward_reference():
    spec, classes, wseed = FORWARD_CASE[:3]
    return swin(CR.preprocess(forward_images()), state_dict(spec, wseed, classes), net_config(spec))


def measure_forward():
    spec, classes, wseed = FORWARD_CASE[:3]
    got = swin(CR.preprocess_einsum32(forward_images()), state_dict(spec, wseed, classes), net_config(spec), torch.float32)
    return rel_err(got, forward_reference())
