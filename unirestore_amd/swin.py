"""Swin-V2 scoring of the `cls` output on the GPU in exact fp32: torchvision-layout SwinTransformers with SwinTransformerBlockV2 and
PatchMergingV2 (swin_v2_t / swin_v2_s / swin_v2_b) on the fp32 convolution of f32net.py - every Linear is that convolution on the
NHWC token map [N,H,W,C], the 4 x 4 patch embedding and the patch-merging reduction (a 2 x 2 / stride 2 convolution) included - the
LayerNorm and GELU of csrc/vit.hip, and the fused shifted-window cosine attention of csrc/swin.hip.  What the reference's
`ClassificationMetric` builds for its `swin` entry (eval_classification.py: torchvision.models.swin_v2_b): quantised image ->
Resize((224, 224)) -> ImageNet Normalize -> Swin -> MulticlassAccuracy(top_k=1); the preprocess and the accuracy are classify.py's.

The project ships NO weights.  `load_weights` reads the torchvision state dict (or Lightning checkpoint) a user of the metric
already has; `random_weights` makes seeded stand-ins for tests and timing, which say nothing about published accuracies.
torchvision is not installed where this project is developed: the key layout and the forward are taken from its source
(models/swin_transformer.py) as recalled and have NOT been checked against the package or against published accuracies.  V1 Swin,
timm-layout checkpoints, windows other than 8 and head dimensions other than 32 are not supported.
"""
import collections
import math

import torch

from . import classify, f32net
from .capi import check, lib
from .f32net import PackedConvF32, stream, take

SwinConfig = collections.namedtuple("SwinConfig", "image_size patch_size embed_dim depths num_heads")

ARCHS = {"swin_v2_t": SwinConfig(224, 4, 96, (2, 2, 6, 2), (3, 6, 12, 24)), "swin_v2_s": SwinConfig(224, 4, 96, (2, 2, 18, 2), (3, 6, 12, 24)),
         "swin_v2_b": SwinConfig(224, 4, 128, (2, 2, 18, 2), (4, 8, 16, 32))}
WINDOW = 8                                               # ur_swin_attention_f32's only window
HEAD_DIM = 32                                            # and its only head dimension
SHIFT = WINDOW // 2                                      # of the odd blocks
LN_EPS = 1e-5                                            # torchvision's SwinTransformer: partial(nn.LayerNorm, eps=1e-5)
LOGIT_MAX = math.log(100.0)                              # the clamp of logit_scale
CPB_HIDDEN = 512


def config(arch_or_config) -> SwinConfig:
    """The checked SwinConfig of an ARCHS name or of a SwinConfig: ValueError for an unknown name, sizes below 1, depths and
    num_heads of different lengths, embed_dim * 2**i != 32 * num_heads[i], an image that is no whole number of patches, or a map
    that is odd in H or W where a patch merging follows."""
    if isinstance(arch_or_config, str):
        if arch_or_config not in ARCHS:
            raise ValueError(f"unknown Swin arch {arch_or_config!r}: choose from {sorted(ARCHS)}")
        return ARCHS[arch_or_config]
    if not isinstance(arch_or_config, SwinConfig):
        raise ValueError(f"a Swin is named by one of {sorted(ARCHS)} or a swin.SwinConfig, got {type(arch_or_config).__name__}")
    cfg = SwinConfig(*arch_or_config[:3], *(tuple(v) if isinstance(v, (tuple, list)) else v for v in arch_or_config[3:]))
    ints = lambda vs: all(isinstance(v, int) and not isinstance(v, bool) and v >= 1 for v in vs)      # noqa: E731
    if not ints(cfg[:3]) or not all(isinstance(v, tuple) and v and ints(v) for v in cfg[3:]):
        raise ValueError(f"{cfg}: image_size, patch_size, embed_dim and every depth and head count must be an integer >= 1")
    if len(cfg.depths) != len(cfg.num_heads):
        raise ValueError(f"{cfg}: depths and num_heads must name the same stages")
    for i, heads in enumerate(cfg.num_heads):
        if cfg.embed_dim * 2 ** i != HEAD_DIM * heads:
            raise ValueError(f"{cfg}: stage {i} has {cfg.embed_dim * 2 ** i} channels and {heads} heads; channels / heads must be "
                             f"{HEAD_DIM}, the attention kernel's head dimension")
    if cfg.image_size % cfg.patch_size:
        raise ValueError(f"{cfg}: image_size must be a multiple of patch_size")
    side = cfg.image_size // cfg.patch_size
    for i in range(len(cfg.depths) - 1):
        if side % 2:
            raise ValueError(f"{cfg}: the map of stage {i} is {side} x {side}, odd where a patch merging follows (its padding is not "
                             "supported)")
        side //= 2
    return cfg


def maps(cfg: SwinConfig):
    """The side of every stage's (square) token map."""
    side = cfg.image_size // cfg.patch_size
    return tuple(side >> i for i in range(len(cfg.depths)))


def block_keys(cfg: SwinConfig):
    """[(key prefix, stage, shift)] of every block in forward order: features.{1,3,5,7}.{j}, shift 0 for even j, 4 for odd."""
    return [(f"features.{2 * i + 1}.{j}", i, SHIFT if j % 2 else 0) for i, depth in enumerate(cfg.depths) for j in range(depth)]


def relative_coords_table() -> torch.Tensor:
    """[15, 15, 2] fp64: table[dy + 7, dx + 7] = (f(8 dy / 7), f(8 dx / 7)), f(t) = sign(t) log2(|t| + 1) / 3."""
    r = torch.arange(-(WINDOW - 1), WINDOW, dtype=torch.float64) * 8 / (WINDOW - 1)
    f = torch.sign(r) * torch.log2(r.abs() + 1) / 3
    return torch.stack([f.view(-1, 1).expand(-1, f.numel()), f.view(1, -1).expand(f.numel(), -1)], dim=2)


def relative_position_index() -> torch.Tensor:
    """[64, 64] int64: index[i, j] = (y_i - y_j + 7) * 15 + (x_i - x_j + 7) of window slots i, j (row-major)."""
    s = torch.arange(WINDOW * WINDOW)
    y, x = s // WINDOW, s % WINDOW
    return (y.view(-1, 1) - y.view(1, -1) + WINDOW - 1) * (2 * WINDOW - 1) + (x.view(-1, 1) - x.view(1, -1) + WINDOW - 1)


def position_bias(w0: torch.Tensor, b0: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """[heads, 64, 64] fp64: 16 sigmoid(cpb_mlp(table))[index] - Linear(2, 512) -> ReLU -> Linear(512, heads, no bias) on the
    fixed coordinate table, gathered per slot pair.  It does not depend on the image: computed once, in fp64."""
    hidden = torch.relu(relative_coords_table().view(-1, 2) @ w0.double().t() + b0.double())
    table = 16 * torch.sigmoid(hidden @ w2.double().t())                     # [225, heads]
    return table[relative_position_index().view(-1)].view(WINDOW * WINDOW, WINDOW * WINDOW, -1).permute(2, 0, 1).contiguous()


def merge_conv_weight(reduction: torch.Tensor) -> torch.Tensor:
    """PatchMergingV2's reduction.weight [2C, 4C] on cat(x[0::2,0::2], x[1::2,0::2], x[0::2,1::2], x[1::2,1::2]) as the OIHW filter
    [2C, C, 2, 2] of a 2 x 2 / stride 2 convolution: tap (dy, dx) holds the columns of concat block 0 = (0,0), 1 = (1,0),
    2 = (0,1), 3 = (1,1)."""
    c = reduction.shape[1] // 4
    w = torch.empty(reduction.shape[0], c, 2, 2, dtype=reduction.dtype)
    for blk, (dy, dx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        w[:, :, dy, dx] = reduction[:, blk * c:(blk + 1) * c]
    return w


class SwinWeights:
    """One Swin-V2 ready for the fp32 kernels: every Linear, the patch embedding and the patch mergings as repacked convolutions on
    the device, the LayerNorm vectors, and per block what the attention kernel takes besides qkv - the qkv bias with its k third
    zeroed (torchvision zeroes it in every forward: a checkpoint's values there have no effect), scale = exp(min(logit_scale,
    log 100)) and the [heads, 64, 64] relative-position bias, both computed here once in fp64 and rounded to fp32.  The state
    dict's relative_coords_table / relative_position_index buffers are recomputed, not read.  `cpu` keeps the state dict's
    parameters (fp32 tensors under torchvision's keys, as given): what a host restatement of the network needs."""

    def __init__(self, arch_or_config, sd: dict, dev=None, source: str = "state dict"):
        cfg = config(arch_or_config)                                         # every check first: nothing is uploaded for a bad file
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        self.arch = arch_or_config if isinstance(arch_or_config, str) else None
        self.config, self.device = cfg, dev
        e, p = cfg.embed_dim, cfg.patch_size
        cpu = {}
        get = lambda key, shape: take(sd, source, key, shape, keep=cpu)      # noqa: E731
        host = {"features.0.0": (get("features.0.0.weight", (e, 3, p, p)), get("features.0.0.bias", (e,)), p)}
        norms = {"features.0.2": [get(f"features.0.2.{n}", (e,)) for n in ("weight", "bias")]}
        attn = {}
        for pre, stage, _shift in block_keys(cfg):
            c, heads = e * 2 ** stage, cfg.num_heads[stage]
            for ln in ("norm1", "norm2"):
                norms[f"{pre}.{ln}"] = [get(f"{pre}.{ln}.{n}", (c,)) for n in ("weight", "bias")]
            qkv_bias = get(f"{pre}.attn.qkv.bias", (3 * c,)).clone()
            qkv_bias[c:2 * c] = 0                                            # the k bias: zeroed once here instead of in every forward
            host[f"{pre}.attn.qkv"] = (get(f"{pre}.attn.qkv.weight", (3 * c, c)), qkv_bias, 1)
            host[f"{pre}.attn.proj"] = (get(f"{pre}.attn.proj.weight", (c, c)), get(f"{pre}.attn.proj.bias", (c,)), 1)
            host[f"{pre}.mlp.0"] = (get(f"{pre}.mlp.0.weight", (4 * c, c)), get(f"{pre}.mlp.0.bias", (4 * c,)), 1)
            host[f"{pre}.mlp.3"] = (get(f"{pre}.mlp.3.weight", (c, 4 * c)), get(f"{pre}.mlp.3.bias", (c,)), 1)
            scale = torch.exp(get(f"{pre}.attn.logit_scale", (heads, 1, 1)).double().clamp(max=LOGIT_MAX)).view(heads)
            bias = position_bias(get(f"{pre}.attn.cpb_mlp.0.weight", (CPB_HIDDEN, 2)), get(f"{pre}.attn.cpb_mlp.0.bias", (CPB_HIDDEN,)),
                                 get(f"{pre}.attn.cpb_mlp.2.weight", (heads, CPB_HIDDEN)))
            attn[pre] = (qkv_bias, scale.float(), bias.float())
        for i in range(len(cfg.depths) - 1):
            pre, c = f"features.{2 * i + 2}", e * 2 ** i
            host[f"{pre}.reduction"] = (merge_conv_weight(get(f"{pre}.reduction.weight", (2 * c, 4 * c))), torch.zeros(2 * c), 2)
            norms[f"{pre}.norm"] = [get(f"{pre}.norm.{n}", (2 * c,)) for n in ("weight", "bias")]
        c = e * 2 ** (len(cfg.depths) - 1)
        norms["norm"] = [get(f"norm.{n}", (c,)) for n in ("weight", "bias")]
        hw = sd.get("head.weight")
        if not torch.is_tensor(hw) or hw.ndim != 2:
            raise ValueError(f"{source}: key 'head.weight' is missing or is no [classes, features] matrix")
        self.num_classes = int(hw.shape[0])
        host["head"] = (get("head.weight", (self.num_classes, c)), get("head.bias", (self.num_classes,)), 1)
        self.cpu = cpu
        self.linears = {k: PackedConvF32(w if w.ndim == 4 else w.view(*w.shape, 1, 1), b, s, 0, dev) for k, (w, b, s) in host.items()}
        self.norms = {k: tuple(t.contiguous().to(dev) for t in v) for k, v in norms.items()}
        self.attn = {k: tuple(t.contiguous().to(dev) for t in v) for k, v in attn.items()}
        self.blocks = block_keys(cfg)


def load_weights(arch, path, dev=None) -> SwinWeights:
    """arch: one of ARCHS (or a SwinConfig); path: the user's torchvision state dict (`features.0.{0,2}.*`, per block
    `features.{1,3,5,7}.{j}.{norm1,norm2}.*`, `.attn.{qkv,proj}.*`, `.attn.logit_scale`, `.attn.cpb_mlp.0.*`, `.attn.cpb_mlp.2.weight`,
    `.mlp.{0,3}.*`, per merging `features.{2,4,6}.reduction.weight` and `.norm.*`, `norm.*`, `head.*`) or a Lightning checkpoint of
    one.  The number of classes is head.weight's.  ValueError (file and key named) for a missing key, a wrong shape or a non-finite
    value."""
    config(arch)                                                     # an unknown arch, before the file is read
    return SwinWeights(arch, f32net.read_state_dict(path), dev, source=str(path))


def random_state_dict(arch_or_config, seed: int, num_classes: int = 1000) -> dict:
    """A seeded stand-in in torchvision's key layout (parameters only), for tests and timing ONLY: Linears with std 1 / sqrt(fan_in)
    (proj and mlp.3 at half gain), small biases - the k third of qkv.bias too, which the forward must ignore - LayerNorm gamma in
    [0.5, 1.5] with a small beta, logit_scale around log 10, a cpb_mlp small enough that the relative-position bias spans a good
    part of (0, 16), a uniform(+-1/sqrt(fan_in)) head: fp32 logits stay finite and O(1).  NOT trained weights - its predictions
    say nothing about any published accuracy."""
    cfg = config(arch_or_config)
    g = torch.Generator().manual_seed(seed)
    e, p = cfg.embed_dim, cfg.patch_size
    sd = {}

    def linear(prefix, cout, cin, gain=1.0):
        sd[f"{prefix}.weight"] = torch.randn(cout, cin, generator=g) * (gain / math.sqrt(cin))
        sd[f"{prefix}.bias"] = 0.05 * torch.randn(cout, generator=g)

    def norm(prefix, d):
        sd[f"{prefix}.weight"] = 0.5 + torch.rand(d, generator=g)
        sd[f"{prefix}.bias"] = 0.1 * torch.randn(d, generator=g)
    sd["features.0.0.weight"] = torch.randn(e, 3, p, p, generator=g) / math.sqrt(3 * p * p)
    sd["features.0.0.bias"] = 0.05 * torch.randn(e, generator=g)
    norm("features.0.2", e)
    for i, depth in enumerate(cfg.depths):
        c, heads = e * 2 ** i, cfg.num_heads[i]
        for j in range(depth):
            pre = f"features.{2 * i + 1}.{j}"
            norm(f"{pre}.norm1", c)
            linear(f"{pre}.attn.qkv", 3 * c, c)
            linear(f"{pre}.attn.proj", c, c, 0.5)
            sd[f"{pre}.attn.logit_scale"] = math.log(10.0) + 0.3 * torch.randn(heads, 1, 1, generator=g)
            sd[f"{pre}.attn.cpb_mlp.0.weight"] = torch.randn(CPB_HIDDEN, 2, generator=g)
            sd[f"{pre}.attn.cpb_mlp.0.bias"] = 0.5 * torch.randn(CPB_HIDDEN, generator=g)
            sd[f"{pre}.attn.cpb_mlp.2.weight"] = torch.randn(heads, CPB_HIDDEN, generator=g) * (2.0 / math.sqrt(CPB_HIDDEN))
            norm(f"{pre}.norm2", c)
            linear(f"{pre}.mlp.0", 4 * c, c)
            linear(f"{pre}.mlp.3", c, 4 * c, 0.5)
        if i < len(cfg.depths) - 1:
            sd[f"features.{2 * i + 2}.reduction.weight"] = torch.randn(2 * c, 4 * c, generator=g) / math.sqrt(4 * c)
            norm(f"features.{2 * i + 2}.norm", 2 * c)
    c = e * 2 ** (len(cfg.depths) - 1)
    norm("norm", c)
    sd["head.weight"] = (2 * torch.rand(num_classes, c, generator=g) - 1) / math.sqrt(c)
    sd["head.bias"] = (2 * torch.rand(num_classes, generator=g) - 1) / math.sqrt(c)
    return sd


def random_weights(arch_or_config, seed: int = 0, num_classes: int = 1000, dev=None) -> SwinWeights:
    """The structure `load_weights` returns, with `random_state_dict`'s values.  For tests and timing ONLY: no trained weights
    exist where this project is developed, so no parity with any published accuracy is claimed."""
    return SwinWeights(arch_or_config, random_state_dict(arch_or_config, seed, num_classes), dev,
                       source=f"random_state_dict({arch_or_config!r}, {seed})")


# ---- launch wrappers (fp32 device tensors, NHWC token maps) ---------------------------------------------------------------------

def window_attention(qkv: torch.Tensor, qkv_bias: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, shift: int) -> torch.Tensor:
    """qkv [N,H,W,3C] as the block's qkv Linear writes it for the real tokens (q | k | v, head h in columns 32 h .. 32 h + 31 of
    each), qkv_bias [3C] (what a zero-padded token's q, k, v are; its k third zeroed), scale [heads], bias [heads,64,64] ->
    [N,H,W,C]: torchvision's shifted_window_attention between its two Linears - pad to multiples of 8, roll by -shift (0 on an
    axis of one window), 8 x 8 windows, softmax(normalize(q) normalize(k)^T scale + bias - 100 [regions differ]) v, windows
    reversed, rolled back, cropped - in one kernel that writes real tokens only.  shift: 0 or 4.
    Non-finite inputs: a score row that holds a NaN or +inf is all NaN; a NaN in V reaches every query of its (window, head);
    the other images keep their bits."""
    if qkv.ndim != 4 or qkv.shape[3] % (3 * HEAD_DIM) or qkv.dtype != torch.float32 or not qkv.is_contiguous() or not qkv.is_cuda or not qkv.numel():
        raise ValueError(f"swin.window_attention: needs a non-empty contiguous fp32 [N, H, W, 3 C] device tensor with C a multiple of "
                         f"{HEAD_DIM}, got {qkv.dtype} {tuple(qkv.shape)} on {qkv.device}")
    n, h, w, c3 = qkv.shape
    c = c3 // 3
    heads = c // HEAD_DIM
    for name, t, shape in (("qkv_bias", qkv_bias, (c3,)), ("scale", scale, (heads,)), ("bias", bias, (heads, WINDOW ** 2, WINDOW ** 2))):
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != qkv.device:
            raise ValueError(f"swin.window_attention: {name} must be a contiguous fp32 {shape} tensor on {qkv.device}, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    y = torch.empty(n, h, w, c, dtype=torch.float32, device=qkv.device)
    check(lib.ur_swin_attention_f32(qkv.data_ptr(), qkv_bias.data_ptr(), scale.data_ptr(), bias.data_ptr(), y.data_ptr(), n, h, w, heads,
                                    int(shift), stream()))
    return y


def layernorm_res(x: torch.Tensor, res: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = LN_EPS) -> torch.Tensor:
    """res + F.layer_norm(x) over the last axis of contiguous fp32 [..., D] tensors: f32net.layernorm_f32's fp64 moments and single
    rounding, then one fp32 addition - the post-norm residual of a V2 block.  A row of x that holds a NaN or an infinity is all NaN."""
    f32net._check_rows("swin.layernorm_res", x)
    d = x.shape[-1]
    if not torch.is_tensor(res) or res.shape != x.shape or res.dtype != torch.float32 or not res.is_contiguous() or res.device != x.device:
        raise ValueError(f"swin.layernorm_res: res must be a contiguous fp32 {tuple(x.shape)} tensor on {x.device}, got "
                         f"{getattr(res, 'dtype', type(res))} {tuple(getattr(res, 'shape', ()))}")
    for name, t in (("gamma", gamma), ("beta", beta)):
        if not torch.is_tensor(t) or tuple(t.shape) != (d,) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"swin.layernorm_res: {name} must be a contiguous fp32 ({d},) tensor on {x.device}, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    y = torch.empty_like(x)
    check(lib.ur_layernorm_res_f32(x.data_ptr(), res.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), x.numel() // d, d,
                                   float(eps), stream()))
    return y


def logits(x: torch.Tensor, wts: SwinWeights) -> torch.Tensor:
    """The network on an already-preprocessed NHWC fp32 input [N, image_size, image_size, 3] -> logits [N, classes]."""
    cfg = wts.config
    if x.ndim != 4 or x.shape[3] != 3 or x.shape[1] != cfg.image_size or x.shape[2] != cfg.image_size:
        raise ValueError(f"swin.logits: needs an NHWC [N, {cfg.image_size}, {cfg.image_size}, 3] input, got {tuple(x.shape)}: the "
                         "configuration's map sizes were checked for that image size")
    conv = lambda t, key, **kw: f32net.conv2d_f32(t, wts.linears[key], relu=False, **kw)      # noqa: E731
    norms = wts.norms
    t = f32net.layernorm_f32(conv(x, "features.0.0"), *norms["features.0.2"], LN_EPS)              # [N, H/4, W/4, E]
    stage = 0
    for pre, s, shift in wts.blocks:
        if s != stage:                                                        # PatchMergingV2: norm(reduction(cat of the 2 x 2 taps))
            stage = s
            t = f32net.layernorm_f32(conv(t, f"features.{2 * s}.reduction"), *norms[f"features.{2 * s}.norm"], LN_EPS)
        a = window_attention(conv(t, f"{pre}.attn.qkv"), *wts.attn[pre], shift)
        t = layernorm_res(conv(a, f"{pre}.attn.proj"), t, *norms[f"{pre}.norm1"])                 # x + norm1(attn(x)): post-norm
        h = f32net.gelu_f32(conv(t, f"{pre}.mlp.0"), inplace=True)
        t = layernorm_res(conv(h, f"{pre}.mlp.3"), t, *norms[f"{pre}.norm2"])                     # x + norm2(mlp(x))
    pooled = f32net.avgpool_f32(f32net.layernorm_f32(t, *norms["norm"], LN_EPS))                  # [N, C]
    return conv(pooled.view(x.shape[0], 1, 1, -1), "head").view(x.shape[0], wts.num_classes)


def forward(images: torch.Tensor, wts: SwinWeights) -> torch.Tensor:
    """ops.swin after its argument checks: the classifier's preprocess + network, logits [N, classes]."""
    if wts.config.image_size != classify.OUT_HW:
        raise ValueError(f"swin.forward: the evaluator's preprocess resizes to {classify.OUT_HW} x {classify.OUT_HW}, this network was "
                         f"configured for {wts.config.image_size} x {wts.config.image_size}; use swin.logits on an input of the "
                         "network's own size")
    return logits(classify.preprocess(images), wts)
