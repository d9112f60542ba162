"""ViT scoring of the `cls` output on the GPU in exact fp32: torchvision-layout VisionTransformers (vit_b_16 / vit_b_32 / vit_l_16 /
vit_l_32) on the fp32 convolution of f32net.py - every Linear, the patch embedding included, is that convolution on tokens
[N,1,S,D] - and the transformer kernels of csrc/vit.hip: LayerNorm, the exact-erf GELU, the class-token / positional-embedding
assembly and multi-head attention on the fp32 MFMA.  What the reference's `ClassificationMetric` builds for its `vit` entry
(eval_classification.py): quantised image -> Resize((224, 224)) -> ImageNet Normalize -> ViT -> MulticlassAccuracy(top_k=1); the
preprocess and the accuracy are classify.py's.

The project ships NO weights.  `load_weights` reads the torchvision state dict (or Lightning checkpoint) a user of the metric
already has; `random_weights` makes seeded stand-ins for tests and timing, which say nothing about published accuracies.
torchvision is not installed where this project is developed: the key layout is taken from its source (models/vision_transformer.py)
and has NOT been checked against the package.  timm-layout checkpoints, inputs of another size than the network's (positional-
embedding interpolation) and head dimensions other than 64 (vit_h_14) are not supported.
"""
import collections
import math

import torch

from . import classify, f32net
from .capi import check, lib
from .f32net import PackedConvF32, stream, take

ViTConfig = collections.namedtuple("ViTConfig", "image_size patch_size num_layers num_heads hidden_dim mlp_dim")

ARCHS = {"vit_b_16": ViTConfig(224, 16, 12, 12, 768, 3072), "vit_b_32": ViTConfig(224, 32, 12, 12, 768, 3072),
         "vit_l_16": ViTConfig(224, 16, 24, 16, 1024, 4096), "vit_l_32": ViTConfig(224, 32, 24, 16, 1024, 4096)}
HEAD_DIM = 64                                            # ur_vit_attention_f32's only head dimension
LN_EPS = 1e-6                                            # torchvision's VisionTransformer: partial(nn.LayerNorm, eps=1e-6)
S_MAX = lib.ur_vit_attention_s_max()                     # tokens per image the attention kernel holds in LDS
MLP_KEYS = (("mlp.0", "mlp.3"), ("mlp.linear_1", "mlp.linear_2"))      # today's spelling, and the one before torchvision 0.12


def config(arch_or_config) -> ViTConfig:
    """The checked ViTConfig of an ARCHS name or of a ViTConfig: ValueError for an unknown name, sizes below 1, an image that is no
    whole number of patches, hidden_dim / num_heads != 64, or more tokens than the attention kernel takes."""
    if isinstance(arch_or_config, str):
        if arch_or_config not in ARCHS:
            raise ValueError(f"unknown ViT arch {arch_or_config!r}: choose from {sorted(ARCHS)}")
        return ARCHS[arch_or_config]
    if not isinstance(arch_or_config, ViTConfig):
        raise ValueError(f"a ViT is named by one of {sorted(ARCHS)} or a vit.ViTConfig, got {type(arch_or_config).__name__}")
    cfg = arch_or_config
    if not all(isinstance(v, int) and v >= 1 for v in cfg):
        raise ValueError(f"{cfg}: every field must be an integer >= 1")
    if cfg.image_size % cfg.patch_size:
        raise ValueError(f"{cfg}: image_size must be a multiple of patch_size")
    if cfg.hidden_dim != cfg.num_heads * HEAD_DIM:
        raise ValueError(f"{cfg}: hidden_dim / num_heads must be {HEAD_DIM}, the attention kernel's head dimension")
    if seq_len(cfg) > S_MAX:
        raise ValueError(f"{cfg}: {seq_len(cfg)} tokens per image, the attention kernel takes at most {S_MAX}")
    return cfg


def seq_len(cfg: ViTConfig) -> int:
    """Tokens per image: the patches and the class token."""
    return (cfg.image_size // cfg.patch_size) ** 2 + 1


class ViTWeights:
    """One VisionTransformer ready for the fp32 kernels: every Linear and the patch embedding as a repacked convolution on the
    device, the LayerNorm vectors, the class token and the positional embedding.  `cpu` keeps the state dict (fp32 tensors under
    torchvision's keys, the MLP under `mlp.0` / `mlp.3`): what a host restatement of the network needs."""

    def __init__(self, arch_or_config, sd: dict, dev=None, source: str = "state dict"):
        cfg = config(arch_or_config)                                         # every check first: nothing is uploaded for a bad file
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        self.arch = arch_or_config if isinstance(arch_or_config, str) else None
        self.config, self.device, self.seq_len = cfg, dev, seq_len(cfg)
        d, p, s = cfg.hidden_dim, cfg.patch_size, self.seq_len
        cpu = {}
        host = {"conv_proj": (take(sd, source, "conv_proj.weight", (d, 3, p, p), keep=cpu), take(sd, source, "conv_proj.bias", (d,), keep=cpu))}
        cls = take(sd, source, "class_token", (1, 1, d), keep=cpu)
        pos = take(sd, source, "encoder.pos_embedding", (1, s, d), keep=cpu)
        norms = {}
        for i in range(cfg.num_layers):
            pre = f"encoder.layers.encoder_layer_{i}"
            spelling = next((k for k in MLP_KEYS if f"{pre}.{k[0]}.weight" in sd), MLP_KEYS[0])
            for ln in ("ln_1", "ln_2"):
                norms[f"{pre}.{ln}"] = [take(sd, source, f"{pre}.{ln}.{n}", (d,), keep=cpu) for n in ("weight", "bias")]
            host[f"{pre}.in_proj"] = (take(sd, source, f"{pre}.self_attention.in_proj_weight", (3 * d, d), keep=cpu),
                                      take(sd, source, f"{pre}.self_attention.in_proj_bias", (3 * d,), keep=cpu))
            host[f"{pre}.out_proj"] = (take(sd, source, f"{pre}.self_attention.out_proj.weight", (d, d), keep=cpu),
                                       take(sd, source, f"{pre}.self_attention.out_proj.bias", (d,), keep=cpu))
            for name, key, canon, shape in (("fc1", spelling[0], MLP_KEYS[0][0], (cfg.mlp_dim, d)), ("fc2", spelling[1], MLP_KEYS[0][1], (d, cfg.mlp_dim))):
                w, b = take(sd, source, f"{pre}.{key}.weight", shape), take(sd, source, f"{pre}.{key}.bias", shape[:1])
                cpu[f"{pre}.{canon}.weight"], cpu[f"{pre}.{canon}.bias"] = w, b           # `cpu` has one spelling, today's
                host[f"{pre}.{name}"] = (w, b)
        norms["encoder.ln"] = [take(sd, source, f"encoder.ln.{n}", (d,), keep=cpu) for n in ("weight", "bias")]
        hw = sd.get("heads.head.weight")
        if not torch.is_tensor(hw) or hw.ndim != 2:
            raise ValueError(f"{source}: key 'heads.head.weight' is missing or is no [classes, features] matrix")
        self.num_classes = int(hw.shape[0])
        host["head"] = (take(sd, source, "heads.head.weight", (self.num_classes, d), keep=cpu),
                        take(sd, source, "heads.head.bias", (self.num_classes,), keep=cpu))
        self.cpu = cpu
        self.linears = {k: PackedConvF32(w if w.ndim == 4 else w.view(*w.shape, 1, 1), b, p if k == "conv_proj" else 1, 0, dev)
                        for k, (w, b) in host.items()}
        self.norms = {k: tuple(t.contiguous().to(dev) for t in v) for k, v in norms.items()}
        self.class_token = cls.reshape(d).contiguous().to(dev)
        self.pos = pos.reshape(s, d).contiguous().to(dev)
        self.layers = [f"encoder.layers.encoder_layer_{i}" for i in range(cfg.num_layers)]


def load_weights(arch, path, dev=None) -> ViTWeights:
    """arch: one of ARCHS (or a ViTConfig); path: the user's torchvision state dict (`conv_proj.*`, `class_token`,
    `encoder.pos_embedding`, `encoder.layers.encoder_layer_{i}.{ln_1,ln_2}.*`, `.self_attention.in_proj_{weight,bias}`,
    `.self_attention.out_proj.*`, `.mlp.{0,3}.*` or the older `.mlp.linear_{1,2}.*`, `encoder.ln.*`, `heads.head.*`) or a Lightning
    checkpoint of one.  The number of classes is heads.head.weight's.  ValueError (file and key named) for a missing key, a wrong
    shape or a non-finite value."""
    config(arch)                                                     # an unknown arch, before the file is read
    return ViTWeights(arch, f32net.read_state_dict(path), dev, source=str(path))


def random_state_dict(arch_or_config, seed: int, num_classes: int = 1000) -> dict:
    """A seeded stand-in in torchvision's key layout, for tests and timing ONLY: Linears with std 1 / sqrt(fan_in) (out_proj and
    fc2 at half gain, so the residual stream does not grow with depth), small biases, LayerNorm gamma in [0.5, 1.5] with a small
    beta, a class token and a positional embedding of std 0.5 and 0.2, a uniform(+-1/sqrt(fan_in)) head: fp32 logits stay finite
    and O(1).  NOT trained weights - its predictions say nothing about any published accuracy."""
    cfg = config(arch_or_config)
    g = torch.Generator().manual_seed(seed)
    d, p = cfg.hidden_dim, cfg.patch_size

    def linear(prefix, cout, cin, gain=1.0, sep="."):
        sd[f"{prefix}{sep}weight"] = torch.randn(cout, cin, generator=g) * (gain / math.sqrt(cin))
        sd[f"{prefix}{sep}bias"] = 0.05 * torch.randn(cout, generator=g)

    def norm(prefix):
        sd[f"{prefix}.weight"] = 0.5 + torch.rand(d, generator=g)
        sd[f"{prefix}.bias"] = 0.1 * torch.randn(d, generator=g)
    sd = {"conv_proj.weight": torch.randn(d, 3, p, p, generator=g) / math.sqrt(3 * p * p), "conv_proj.bias": 0.05 * torch.randn(d, generator=g),
          "class_token": 0.5 * torch.randn(1, 1, d, generator=g), "encoder.pos_embedding": 0.2 * torch.randn(1, seq_len(cfg), d, generator=g)}
    for i in range(cfg.num_layers):
        pre = f"encoder.layers.encoder_layer_{i}"
        norm(f"{pre}.ln_1")
        linear(f"{pre}.self_attention.in_proj", 3 * d, d, sep="_")
        linear(f"{pre}.self_attention.out_proj", d, d, 0.5)
        norm(f"{pre}.ln_2")
        linear(f"{pre}.mlp.0", cfg.mlp_dim, d)
        linear(f"{pre}.mlp.3", d, cfg.mlp_dim, 0.5)
    norm("encoder.ln")
    sd["heads.head.weight"] = (2 * torch.rand(num_classes, d, generator=g) - 1) / math.sqrt(d)
    sd["heads.head.bias"] = (2 * torch.rand(num_classes, generator=g) - 1) / math.sqrt(d)
    return sd


def random_weights(arch_or_config, seed: int = 0, num_classes: int = 1000, dev=None) -> ViTWeights:
    """The structure `load_weights` returns, with `random_state_dict`'s values.  For tests and timing ONLY: no trained weights
    exist where this project is developed, so no parity with any published accuracy is claimed."""
    return ViTWeights(arch_or_config, random_state_dict(arch_or_config, seed, num_classes), dev,
                      source=f"random_state_dict({arch_or_config!r}, {seed})")


# ---- launch wrappers of csrc/vit.hip (fp32 device tensors, token-major) ---------------------------------------------------------

def embed(patches: torch.Tensor, class_token: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """patches [N,P,D], class_token [D], pos [P+1,D] -> tokens [N,P+1,D]: token 0 = class_token + pos[0], token 1 + p = patch p +
    pos[1 + p]."""
    n, p, d = patches.shape
    if tuple(class_token.shape) != (d,) or tuple(pos.shape) != (p + 1, d):
        raise ValueError(f"vit.embed: patches {tuple(patches.shape)} need a class token ({d},) and a positional embedding ({p + 1}, {d}), "
                         f"got {tuple(class_token.shape)} and {tuple(pos.shape)}")
    y = torch.empty(n, p + 1, d, dtype=torch.float32, device=patches.device)
    check(lib.ur_vit_embed_f32(patches.data_ptr(), class_token.data_ptr(), pos.data_ptr(), y.data_ptr(), n, p, d, stream()))
    return y


def attention(qkv: torch.Tensor, num_heads: int) -> torch.Tensor:
    """qkv [N,S,3D] as nn.MultiheadAttention's in_proj writes it (q | k | v, head h in columns 64 h .. 64 h + 63 of each) ->
    softmax(q k^T / 8) v per (image, head), heads concatenated: [N,S,D].  D = 64 num_heads, S <= S_MAX.
    Non-finite inputs: a score row that holds a NaN or +inf is all NaN, a -inf score has weight 0, a NaN in V reaches every query
    of its (image, head); the other images keep their bits."""
    if qkv.ndim != 3 or qkv.shape[2] % 3 or qkv.dtype != torch.float32 or not qkv.is_contiguous() or not qkv.is_cuda:
        raise ValueError(f"vit.attention: needs a contiguous fp32 [N, S, 3 D] device tensor, got {qkv.dtype} {tuple(qkv.shape)} on {qkv.device}")
    n, s, d3 = qkv.shape
    y = torch.empty(n, s, d3 // 3, dtype=torch.float32, device=qkv.device)
    check(lib.ur_vit_attention_f32(qkv.data_ptr(), y.data_ptr(), n, s, num_heads, HEAD_DIM, d3 // 3, stream()))
    return y


def _linear(x: torch.Tensor, pc: PackedConvF32, res: torch.Tensor = None) -> torch.Tensor:
    """A Linear on tokens [N,S,Cin] -> [N,S,Cout] (+ res): the 1x1 convolution on [N,1,S,Cin]."""
    n, s, _c = x.shape
    return f32net.conv2d_f32(x.view(n, 1, s, -1), pc, res=None if res is None else res.view(n, 1, s, -1), relu=False).view(n, s, pc.cout)


def logits(x: torch.Tensor, wts: ViTWeights) -> torch.Tensor:
    """The network on an already-preprocessed NHWC fp32 input [N, image_size, image_size, 3] -> logits [N, classes].  Another size
    would need the positional embedding interpolated, which is not supported."""
    cfg = wts.config
    if x.ndim != 4 or x.shape[3] != 3 or x.shape[1] != cfg.image_size or x.shape[2] != cfg.image_size:
        raise ValueError(f"vit.logits: needs an NHWC [N, {cfg.image_size}, {cfg.image_size}, 3] input, got {tuple(x.shape)}: the positional "
                         f"embedding covers {cfg.image_size // cfg.patch_size} x {cfg.image_size // cfg.patch_size} patches and is not interpolated")
    n, d = x.shape[0], cfg.hidden_dim
    lin, norms = wts.linears, wts.norms
    patches = f32net.conv2d_f32(x, lin["conv_proj"], relu=False)                          # [N, g, g, D]: row-major patches
    t = embed(patches.view(n, -1, d), wts.class_token, wts.pos)
    for pre in wts.layers:
        qkv = _linear(f32net.layernorm_f32(t, *norms[f"{pre}.ln_1"], LN_EPS), lin[f"{pre}.in_proj"])
        t = _linear(attention(qkv, cfg.num_heads), lin[f"{pre}.out_proj"], res=t)         # x + attn
        h = f32net.gelu_f32(_linear(f32net.layernorm_f32(t, *norms[f"{pre}.ln_2"], LN_EPS), lin[f"{pre}.fc1"]), inplace=True)
        t = _linear(h, lin[f"{pre}.fc2"], res=t)                                          # x + mlp
    cls = f32net.layernorm_f32(t, *norms["encoder.ln"], LN_EPS, first_row_of=wts.seq_len)  # the class-token rows only
    return _linear(cls.view(n, 1, d), lin["head"]).view(n, wts.num_classes)


def forward(images: torch.Tensor, wts: ViTWeights) -> torch.Tensor:
    """ops.vit after its argument checks: the classifier's preprocess + network, logits [N, classes]."""
    if wts.config.image_size != classify.OUT_HW:
        raise ValueError(f"vit.forward: the evaluator's preprocess resizes to {classify.OUT_HW} x {classify.OUT_HW}, this network takes "
                         f"{wts.config.image_size} x {wts.config.image_size} (positional-embedding interpolation is not supported); "
                         "use vit.logits on an input of the network's own size")
    return logits(classify.preprocess(images), wts)
