"""RVT scoring of the `cls` output on the GPU in exact fp32: the reference's own Robust Vision Transformers (`PoolingTransformer` of
src/modules/rvt/robust_models.py: rvt_tiny / rvt_small / rvt_base and their `_plus` variants) on the fp32 convolution of f32net.py -
the two stem convolutions, every Linear and every 1 x 1 convolution are that convolution on the NHWC token map [N,H,W,C], each
BatchNorm folded into the convolution before it - the LayerNorm, GELU, padded max-pool and mean of the existing scorers, and the
two kernels of csrc/rvt.hip: attention with head dimension 32 or 64 and the `_plus` models' position-aware attention scaling (the
scaled scores times sigmoid(att_mask) before the softmax), and the depthwise 3 x 3 convolution of the convolutional MLP and of the
head pooling between the two stages of rvt_tiny.  What the reference's `ClassificationMetric` builds for its `rvt` entry
(eval_classification.py): quantised image -> Resize((224, 224)) -> ImageNet Normalize -> RVT -> MulticlassAccuracy(top_k=1); the
preprocess and the accuracy are classify.py's.

The project ships NO weights.  `load_weights` reads the published RVT checkpoint ({"model": state dict}) a user of the metric
already has; `random_weights` makes seeded stand-ins for tests and timing, which say nothing about published accuracies.  Unlike the
ViT and Swin scorers, the key layout and the forward ARE checked against the reference's own module: tools/gen_golden_rvt.py loads
`random_state_dict` into `PoolingTransformer` with strict=True and stores its fp64 logits in tests/golden/rvt_0.npz.  Inputs other
than 224 x 224 for the `_plus` models (att_mask is 196 x 196 by construction) and head dimensions other than 32 / 64 are not
supported.
"""
import collections
import math

import torch

from . import classify, f32net
from .capi import check, lib
from .f32net import PackedConvF32, stream, take

RVTConfig = collections.namedtuple("RVTConfig", "image_size base_dims depth heads mlp_ratio use_mask masked_block")

ARCHS = {"rvt_tiny": RVTConfig(224, (32, 32), (10, 2), (6, 12), 4, False, None),
         "rvt_tiny_plus": RVTConfig(224, (32, 32), (10, 2), (6, 12), 4, True, 10),
         "rvt_small": RVTConfig(224, (64,), (12,), (6,), 4, False, None), "rvt_small_plus": RVTConfig(224, (64,), (12,), (6,), 4, True, 5),
         "rvt_base": RVTConfig(224, (64,), (12,), (12,), 4, False, None), "rvt_base_plus": RVTConfig(224, (64,), (12,), (12,), 4, True, 5)}
HEAD_DIMS = (32, 64)                                     # ur_rvt_attention_f32's head dimensions
LN_EPS = 1e-6                                            # partial(nn.LayerNorm, eps=1e-6), and the final norm
BN_EPS = 1e-5                                            # nn.BatchNorm2d's default
S_MAX = lib.ur_vit_attention_s_max()                     # tokens per image the attention kernel holds in LDS
STEM_CH = 32                                             # patch_embed.proj.0's output channels
MASK_SIDE = 14                                           # att_mask is [heads, 196, 196]
LINEAR_MLP_DIM = 768                                     # Mlp: `if in_features == 768` - Linears, else the convolutional branch


def stem_side(image_size: int) -> int:
    """The side of stage 0's token map: conv 7 / stride 2 / pad 2 -> max-pool 3 / stride 2 / pad 1 -> conv 4 / stride 4."""
    side = (image_size + 4 - 7) // 2 + 1
    side = (side - 1) // 2 + 1
    return (side - 4) // 4 + 1


def maps(cfg: RVTConfig):
    """The side of every stage's (square) token map; the head pooling between two stages is 3 x 3 / stride 2 / pad 1."""
    sides = [stem_side(cfg.image_size)]
    for _ in cfg.depth[1:]:
        sides.append((sides[-1] - 1) // 2 + 1)
    return tuple(sides)


def dims(cfg: RVTConfig):
    """The width of every stage: base_dims[s] * heads[s]."""
    return tuple(b * h for b, h in zip(cfg.base_dims, cfg.heads))


def config(arch_or_config) -> RVTConfig:
    """The checked RVTConfig of an ARCHS name or of an RVTConfig: ValueError for an unknown name, sizes below 1, base_dims, depth and
    heads that do not name the same one or two stages, a head dimension other than 32 / 64, an image too small for the stem, more
    tokens than the attention kernel takes, a second stage whose width is no multiple of the first's (the head pooling is a grouped
    convolution), an mlp_ratio other than an integer >= 1, or use_mask with a stage-0 map other than 14 x 14 or a masked_block
    outside [0, depth[0]].  The token maps are square by construction: the image is."""
    if isinstance(arch_or_config, str):
        if arch_or_config not in ARCHS:
            raise ValueError(f"unknown RVT arch {arch_or_config!r}: choose from {sorted(ARCHS)}")
        return ARCHS[arch_or_config]
    if not isinstance(arch_or_config, RVTConfig):
        raise ValueError(f"an RVT is named by one of {sorted(ARCHS)} or an rvt.RVTConfig, got {type(arch_or_config).__name__}")
    c = arch_or_config
    cfg = RVTConfig(c.image_size, *(tuple(v) if isinstance(v, (tuple, list)) else v for v in c[1:4]), c.mlp_ratio, c.use_mask, c.masked_block)
    ints = lambda vs: all(isinstance(v, int) and not isinstance(v, bool) and v >= 1 for v in vs)      # noqa: E731
    if not ints((cfg.image_size, cfg.mlp_ratio)) or not all(isinstance(v, tuple) and v and ints(v) for v in cfg[1:4]):
        raise ValueError(f"{cfg}: image_size, mlp_ratio and every base dimension, depth and head count must be an integer >= 1")
    if not len(cfg.base_dims) == len(cfg.depth) == len(cfg.heads) or len(cfg.depth) > 2:
        raise ValueError(f"{cfg}: base_dims, depth and heads must name the same one or two stages")
    if not isinstance(cfg.use_mask, bool):
        raise ValueError(f"{cfg}: use_mask must be True or False")
    for s, b in enumerate(cfg.base_dims):
        if b not in HEAD_DIMS:
            raise ValueError(f"{cfg}: stage {s} has head dimension {b}; the attention kernel takes {HEAD_DIMS[0]} or {HEAD_DIMS[1]}")
    if cfg.image_size < 15:
        raise ValueError(f"{cfg}: the stem needs an image of at least 15 x 15 for one token")
    sides, widths = maps(cfg), dims(cfg)
    if sides[0] ** 2 > S_MAX:
        raise ValueError(f"{cfg}: {sides[0] ** 2} tokens per image, the attention kernel takes at most {S_MAX}")
    if len(widths) == 2 and widths[1] % widths[0]:
        raise ValueError(f"{cfg}: the head pooling is a convolution with groups = {widths[0]}; stage 1's width {widths[1]} is no multiple")
    if cfg.use_mask:
        if sides[0] != MASK_SIDE:
            raise ValueError(f"{cfg}: use_mask needs a {MASK_SIDE} x {MASK_SIDE} stage-0 map (att_mask is [heads, 196, 196] by "
                             f"construction), this image gives {sides[0]} x {sides[0]}")
        if not (isinstance(cfg.masked_block, int) and not isinstance(cfg.masked_block, bool) and 0 <= cfg.masked_block <= cfg.depth[0]):
            raise ValueError(f"{cfg}: masked_block must be an integer in [0, {cfg.depth[0]}] with use_mask")
    return cfg


def block_keys(cfg: RVTConfig):
    """[(key prefix, stage, gated)] of every block in forward order: transformers.{s}.blocks.{i}; the first masked_block blocks of
    stage 0 carry an att_mask when use_mask."""
    return [(f"transformers.{s}.blocks.{i}", s, bool(cfg.use_mask and s == 0 and i < cfg.masked_block))
            for s, depth in enumerate(cfg.depth) for i in range(depth)]


def fold_bn_bias(w, b, gamma, beta, mean, var, eps: float = BN_EPS):
    """conv WITH a bias followed by eval-mode BatchNorm as one convolution, folded in fp64: (weight fp64, bias fp64) =
    (w * s, (b - mean) * s + beta), s = gamma / sqrt(var + eps).  (f32net.fold_bn is the fold of a convolution without a bias.)"""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * scale.view(-1, *([1] * (w.ndim - 1))), (b.double() - mean.double()) * scale + beta.double()


def pack_dw_weight(w: torch.Tensor) -> torch.Tensor:
    """A depthwise OIHW filter [Cout, 1, 3, 3] -> ur_dwconv3x3_f32's tap-major [9][Cout] (fp32, contiguous)."""
    return w.float().reshape(w.shape[0], 9).t().contiguous()


class RVTWeights:
    """One PoolingTransformer ready for the fp32 kernels: the stem, every Linear and every 1 x 1 convolution as a repacked
    convolution on the device with its BatchNorm folded in (in fp64, the convolution's own bias included), the depthwise filters
    repacked [9][C mult] with theirs, the LayerNorm vectors, and per gated block sigmoid(att_mask), computed once in fp64 and
    rounded to fp32.  `cpu` keeps the state dict (fp32 tensors under the reference's keys, as given): what a host restatement of
    the network needs."""

    def __init__(self, arch_or_config, sd: dict, dev=None, source: str = "state dict"):
        cfg = config(arch_or_config)                                         # every check first: nothing is uploaded for a bad file
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        self.arch = arch_or_config if isinstance(arch_or_config, str) else None
        self.config, self.device = cfg, dev
        widths, sides = dims(cfg), maps(cfg)
        cpu = {}
        get = lambda key, shape: take(sd, source, key, shape, keep=cpu)      # noqa: E731

        def folded(ckey, bkey, wshape):
            """(weight fp32, bias fp32) of conv `ckey` (with bias) + BatchNorm `bkey`."""
            cout = wshape[0]
            w, b = get(f"{ckey}.weight", wshape), get(f"{ckey}.bias", (cout,))
            bn = [get(f"{bkey}.{n}", (cout,)) for n in ("weight", "bias", "running_mean", "running_var")]
            if not bool((bn[3].double() + BN_EPS > 0).all()):
                raise ValueError(f"{source}: {bkey + '.running_var'!r} + eps is not positive: not a trained BatchNorm")
            fw, fb = fold_bn_bias(w, b, *bn)
            if not (bool(torch.isfinite(fw).all()) and bool(torch.isfinite(fb).all())):
                raise ValueError(f"{source}: folding {bkey!r} into {ckey!r} gives a non-finite value")
            return fw.float(), fb.float()

        pe = "patch_embed.proj"
        host = {f"{pe}.0": (*folded(f"{pe}.0", f"{pe}.1", (STEM_CH, 3, 7, 7)), 2, 2),           # key -> (OIHW weight, bias, stride, pad)
                f"{pe}.3": (get(f"{pe}.3.weight", (widths[0], STEM_CH, 4, 4)), get(f"{pe}.3.bias", (widths[0],)), 4, 0)}
        norms, dws, gates = {}, {}, {}
        for pre, s, gated in block_keys(cfg):
            d, heads = widths[s], cfg.heads[s]
            hid = d * cfg.mlp_ratio
            for ln in ("norm1", "norm2"):
                norms[f"{pre}.{ln}"] = [get(f"{pre}.{ln}.{n}", (d,)) for n in ("weight", "bias")]
            host[f"{pre}.attn.qkv"] = (get(f"{pre}.attn.qkv.weight", (3 * d, d)), get(f"{pre}.attn.qkv.bias", (3 * d,)), 1, 0)
            host[f"{pre}.attn.proj"] = (get(f"{pre}.attn.proj.weight", (d, d)), get(f"{pre}.attn.proj.bias", (d,)), 1, 0)
            if gated:
                mask = get(f"{pre}.attn.att_mask", (heads, MASK_SIDE ** 2, MASK_SIDE ** 2))
                gates[pre] = torch.sigmoid(mask.double()).float()
            if d == LINEAR_MLP_DIM:
                host[f"{pre}.mlp.fc1"] = (get(f"{pre}.mlp.fc1.weight", (hid, d)), get(f"{pre}.mlp.fc1.bias", (hid,)), 1, 0)
                host[f"{pre}.mlp.fc2"] = (get(f"{pre}.mlp.fc2.weight", (d, hid)), get(f"{pre}.mlp.fc2.bias", (d,)), 1, 0)
            else:
                host[f"{pre}.mlp.fc1"] = (*folded(f"{pre}.mlp.fc1", f"{pre}.mlp.bn1", (hid, d, 1, 1)), 1, 0)
                dw, db = folded(f"{pre}.mlp.dwconv", f"{pre}.mlp.bn2", (hid, 1, 3, 3))
                dws[f"{pre}.mlp.dwconv"] = (pack_dw_weight(dw), db, 1, 1)                     # (w [9][Cout], bias, mult, stride)
                host[f"{pre}.mlp.fc2"] = (*folded(f"{pre}.mlp.fc2", f"{pre}.mlp.bn3", (d, hid, 1, 1)), 1, 0)
        if len(widths) == 2:
            dws["pools.0.conv"] = (pack_dw_weight(get("pools.0.conv.weight", (widths[1], 1, 3, 3))), get("pools.0.conv.bias", (widths[1],)),
                                   widths[1] // widths[0], 2)
        norms["norm"] = [get(f"norm.{n}", (widths[-1],)) for n in ("weight", "bias")]
        hw = sd.get("head.weight")
        if not torch.is_tensor(hw) or hw.ndim != 2:
            raise ValueError(f"{source}: key 'head.weight' is missing or is no [classes, features] matrix")
        self.num_classes = int(hw.shape[0])
        host["head"] = (get("head.weight", (self.num_classes, widths[-1])), get("head.bias", (self.num_classes,)), 1, 0)
        self.cpu = cpu
        self.linears = {k: PackedConvF32(w if w.ndim == 4 else w.view(*w.shape, 1, 1), b, s, p, dev) for k, (w, b, s, p) in host.items()}
        self.norms = {k: tuple(t.contiguous().to(dev) for t in v) for k, v in norms.items()}
        self.dwconvs = {k: (w.to(dev), b.float().contiguous().to(dev), mult, stride) for k, (w, b, mult, stride) in dws.items()}
        self.gates = {k: g.contiguous().to(dev) for k, g in gates.items()}
        self.blocks = block_keys(cfg)
        self.maps, self.dims = sides, widths


def read_state_dict(path) -> dict:
    """The three wrappings of an RVT checkpoint: {"model": state dict} (the published files: `torch.load(path)["model"]` in the
    reference), a Lightning checkpoint (f32net.read_state_dict: its "state_dict" with a leading `model.` stripped), or a bare state
    dict."""
    sd = f32net.read_state_dict(path)
    if "model" in sd and isinstance(sd["model"], dict) and not torch.is_tensor(sd["model"]):
        sd = sd["model"]
    return sd


def load_weights(arch, path, dev=None) -> RVTWeights:
    """arch: one of ARCHS (or an RVTConfig); path: the user's RVT checkpoint - {"model": state dict} as published, a Lightning
    checkpoint of one, or the bare state dict: `patch_embed.proj.{0,1,3}.*`, per block `transformers.{s}.blocks.{i}.{norm1,norm2}.*`,
    `.attn.{qkv,proj}.*`, `.attn.att_mask` (the gated blocks), `.mlp.{fc1,fc2}.*` and, where the width is not 768,
    `.mlp.{bn1,dwconv,bn2,bn3}.*` with fc1.weight [4D, D, 1, 1]; `pools.0.conv.*` (two stages), `norm.*`, `head.*`.  The number of
    classes is head.weight's.  ValueError (file and key named) for a missing key, a wrong shape or a non-finite value."""
    config(arch)                                                     # an unknown arch, before the file is read
    return RVTWeights(arch, read_state_dict(path), dev, source=str(path))


def random_state_dict(arch_or_config, seed: int, num_classes: int = 1000) -> dict:
    """A seeded stand-in in the reference module's key layout (every parameter and buffer: strict=True loads it), for tests and
    timing ONLY: Linears and convolutions with std 1 / sqrt(fan_in) (proj and fc2 at half gain, so the residual stream does not grow
    with depth; the depthwise filters at std 1/3), small biases, LayerNorm and BatchNorm gamma in [0.5, 1.5] with a small beta,
    BatchNorm running_mean ~ 0.1 N(0, 1) and running_var in [0.5, 1.5], att_mask ~ N(0, 1) (the reference leaves it
    uninitialised), a uniform(+-1/sqrt(fan_in)) head: fp32 logits stay finite and O(1).  NOT trained weights - its predictions say
    nothing about any published accuracy."""
    cfg = config(arch_or_config)
    g = torch.Generator().manual_seed(seed)
    widths = dims(cfg)
    sd = {}

    def conv(prefix, cout, cin, k, gain=1.0, linear=False):
        shape = (cout, cin) if linear else (cout, cin, k, k)
        sd[f"{prefix}.weight"] = torch.randn(*shape, generator=g) * (gain / math.sqrt(cin * k * k))
        sd[f"{prefix}.bias"] = 0.05 * torch.randn(cout, generator=g)

    def norm(prefix, d, bn=False):
        sd[f"{prefix}.weight"] = 0.5 + torch.rand(d, generator=g)
        sd[f"{prefix}.bias"] = 0.1 * torch.randn(d, generator=g)
        if bn:
            sd[f"{prefix}.running_mean"] = 0.1 * torch.randn(d, generator=g)
            sd[f"{prefix}.running_var"] = 0.5 + torch.rand(d, generator=g)
            sd[f"{prefix}.num_batches_tracked"] = torch.tensor(0)
    conv("patch_embed.proj.0", STEM_CH, 3, 7)
    norm("patch_embed.proj.1", STEM_CH, bn=True)
    conv("patch_embed.proj.3", widths[0], STEM_CH, 4)
    for pre, s, gated in block_keys(cfg):
        d, heads = widths[s], cfg.heads[s]
        hid = d * cfg.mlp_ratio
        norm(f"{pre}.norm1", d)
        conv(f"{pre}.attn.qkv", 3 * d, d, 1, linear=True)
        conv(f"{pre}.attn.proj", d, d, 1, 0.5, linear=True)
        if gated:
            sd[f"{pre}.attn.att_mask"] = torch.randn(heads, MASK_SIDE ** 2, MASK_SIDE ** 2, generator=g)
        norm(f"{pre}.norm2", d)
        if d == LINEAR_MLP_DIM:
            conv(f"{pre}.mlp.fc1", hid, d, 1, linear=True)
            conv(f"{pre}.mlp.fc2", d, hid, 1, 0.5, linear=True)
        else:
            conv(f"{pre}.mlp.fc1", hid, d, 1)
            norm(f"{pre}.mlp.bn1", hid, bn=True)
            conv(f"{pre}.mlp.dwconv", hid, 1, 3)
            norm(f"{pre}.mlp.bn2", hid, bn=True)
            conv(f"{pre}.mlp.fc2", d, hid, 1, 0.5)
            norm(f"{pre}.mlp.bn3", d, bn=True)
    if len(widths) == 2:
        conv("pools.0.conv", widths[1], 1, 3)
    norm("norm", widths[-1])
    sd["head.weight"] = (2 * torch.rand(num_classes, widths[-1], generator=g) - 1) / math.sqrt(widths[-1])
    sd["head.bias"] = (2 * torch.rand(num_classes, generator=g) - 1) / math.sqrt(widths[-1])
    return sd


def random_weights(arch_or_config, seed: int = 0, num_classes: int = 1000, dev=None) -> RVTWeights:
    """The structure `load_weights` returns, with `random_state_dict`'s values.  For tests and timing ONLY: no trained weights
    exist where this project is developed, so no parity with any published accuracy is claimed."""
    return RVTWeights(arch_or_config, random_state_dict(arch_or_config, seed, num_classes), dev,
                      source=f"random_state_dict({arch_or_config!r}, {seed})")


# ---- launch wrappers of csrc/rvt.hip (fp32 device tensors) ----------------------------------------------------------------------

def attention(qkv: torch.Tensor, num_heads: int, gate: torch.Tensor = None) -> torch.Tensor:
    """qkv [N,S,3D] as the block's qkv Linear writes it (q | k | v, head h in columns d h .. d h + d - 1 of each, d = D / num_heads
    = 32 or 64), gate [num_heads,S,S] or None -> softmax((q k^T d^-0.5) * gate) v per (image, head), heads concatenated: [N,S,D].
    S <= S_MAX.  Without a gate and with d = 64 this is vit.attention, bit for bit.
    Non-finite inputs: a score row that holds a NaN or +inf is all NaN, a -inf score has weight 0, a gate of 0 against an infinite
    score is NaN, a NaN in V reaches every query of its (image, head); the other images keep their bits."""
    if (not torch.is_tensor(qkv) or qkv.ndim != 3 or qkv.dtype != torch.float32 or not qkv.is_contiguous() or not qkv.is_cuda or not qkv.numel()
            or not isinstance(num_heads, int) or num_heads < 1 or qkv.shape[2] % (3 * num_heads)):
        raise ValueError(f"rvt.attention: needs a non-empty contiguous fp32 [N, S, 3 D] device tensor with D a multiple of num_heads="
                         f"{num_heads}, got {getattr(qkv, 'dtype', type(qkv))} {tuple(getattr(qkv, 'shape', ()))} on {getattr(qkv, 'device', 'the host')}")
    n, s, d3 = qkv.shape
    d = d3 // 3
    if gate is not None and (not torch.is_tensor(gate) or tuple(gate.shape) != (num_heads, s, s) or gate.dtype != torch.float32
                             or gate.device != qkv.device or not gate.is_contiguous()):
        raise ValueError(f"rvt.attention: gate must be a contiguous fp32 ({num_heads}, {s}, {s}) tensor on {qkv.device}, got "
                         f"{getattr(gate, 'dtype', type(gate))} {tuple(getattr(gate, 'shape', ()))}")
    y = torch.empty(n, s, d, dtype=torch.float32, device=qkv.device)
    check(lib.ur_rvt_attention_f32(qkv.data_ptr(), None if gate is None else gate.data_ptr(), y.data_ptr(), n, s, num_heads, d // num_heads,
                                   stream()))
    return y


def dwconv3x3(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, mult: int = 1, stride: int = 1, gelu: bool = False) -> torch.Tensor:
    """x NHWC [N,H,W,C], w [9, C mult] (pack_dw_weight of the OIHW filter), bias [C mult] -> act(depthwise 3 x 3 convolution, pad 1,
    `stride` 1 or 2) [N,OH,OW,C mult]; output channel o reads input channel o // mult (F.conv2d with groups = C).  The taps are
    accumulated in row-major order with fmaf from 0, then the bias; gelu: f32net.gelu_f32's function on top, the same bits as
    applying it afterwards.  A tap in the padding is skipped: a non-finite input reaches only the outputs whose window holds it.
    A tensor that is not 16-byte aligned (a view into a larger buffer) takes the scalar path: the same bits."""
    def dense(t, nd):
        return torch.is_tensor(t) and t.ndim == nd and t.dtype == torch.float32 and t.is_cuda and t.numel() > 0 and t.is_contiguous()
    if not dense(x, 4):
        raise ValueError(f"rvt.dwconv3x3: needs a non-empty contiguous fp32 NHWC device tensor, got {getattr(x, 'dtype', type(x))} "
                         f"{tuple(getattr(x, 'shape', ()))} on {getattr(x, 'device', 'the host')}")
    n, h, wd, c = x.shape
    if not isinstance(mult, int) or mult < 1 or stride not in (1, 2):
        raise ValueError(f"rvt.dwconv3x3: mult must be an integer >= 1 and stride 1 or 2, got mult={mult!r}, stride={stride!r}")
    co = c * mult
    if not dense(w, 2) or tuple(w.shape) != (9, co) or not dense(bias, 1) or tuple(bias.shape) != (co,) or w.device != x.device or bias.device != x.device:
        raise ValueError(f"rvt.dwconv3x3: x {tuple(x.shape)} with mult={mult} needs dense fp32 w (9, {co}) and bias ({co},) on {x.device}, "
                         f"got {tuple(getattr(w, 'shape', ()))} and {tuple(getattr(bias, 'shape', ()))}")
    y = torch.empty(n, (h - 1) // stride + 1, (wd - 1) // stride + 1, co, dtype=torch.float32, device=x.device)
    check(lib.ur_dwconv3x3_f32(x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), n, h, wd, c, mult, stride, int(bool(gelu)), stream()))
    return y


def logits(x: torch.Tensor, wts: RVTWeights) -> torch.Tensor:
    """The network on an already-preprocessed NHWC fp32 input [N, image_size, image_size, 3] -> logits [N, classes] - always two
    axes.  (The reference's forward_features ends in `self.gap(x).squeeze()`, which drops the batch axis too at N = 1 and returns
    [classes]; that is not copied.)"""
    cfg = wts.config
    if x.ndim != 4 or x.shape[3] != 3 or x.shape[1] != cfg.image_size or x.shape[2] != cfg.image_size:
        raise ValueError(f"rvt.logits: needs an NHWC [N, {cfg.image_size}, {cfg.image_size}, 3] input, got {tuple(x.shape)}: the "
                         "configuration's token maps were checked for that image size")
    conv = lambda t, key, **kw: f32net.conv2d_f32(t, wts.linears[key], relu=False, **kw)      # noqa: E731
    norms = wts.norms
    n = x.shape[0]
    t = conv(f32net.maxpool2d_pad_f32(conv(x, "patch_embed.proj.0")), "patch_embed.proj.3")   # [N, 14, 14, D]: conv + BN, pool, conv
    stage = 0
    for pre, s, _gated in wts.blocks:
        if s != stage:                                                        # conv_head_pooling: groups = Cin, stride 2
            stage = s
            t = dwconv3x3(t, *wts.dwconvs["pools.0.conv"])
        _n, side, _w, d = t.shape
        qkv = conv(f32net.layernorm_f32(t, *norms[f"{pre}.norm1"], LN_EPS), f"{pre}.attn.qkv")
        a = attention(qkv.view(n, side * side, 3 * d), cfg.heads[s], wts.gates.get(pre))
        t = conv(a.view(n, side, side, d), f"{pre}.attn.proj", res=t)                         # x + attn
        h = f32net.gelu_f32(conv(f32net.layernorm_f32(t, *norms[f"{pre}.norm2"], LN_EPS), f"{pre}.mlp.fc1"), inplace=True)
        if f"{pre}.mlp.dwconv" in wts.dwconvs:                                                # gelu(bn2(dwconv(.))), BatchNorm folded in
            w, b, mult, stride = wts.dwconvs[f"{pre}.mlp.dwconv"]
            h = dwconv3x3(h, w, b, mult, stride, gelu=True)
        t = conv(h, f"{pre}.mlp.fc2", res=t)                                                  # x + mlp
    pooled = f32net.layernorm_f32(f32net.avgpool_f32(t), *norms["norm"], LN_EPS)              # norm(gap(x)): the mean first
    return conv(pooled.view(n, 1, 1, -1), "head").view(n, wts.num_classes)


def forward(images: torch.Tensor, wts: RVTWeights) -> torch.Tensor:
    """ops.rvt after its argument checks: the classifier's preprocess + network, logits [N, classes]."""
    if wts.config.image_size != classify.OUT_HW:
        raise ValueError(f"rvt.forward: the evaluator's preprocess resizes to {classify.OUT_HW} x {classify.OUT_HW}, this network was "
                         f"configured for {wts.config.image_size} x {wts.config.image_size}; use rvt.logits on an input of the "
                         "network's own size")
    return logits(classify.preprocess(images), wts)
