"""VGG scoring of the `cls` output on the GPU in exact fp32: torchvision's VGG configurations A, B, D and E (vgg11 / vgg13 / vgg16 /
vgg19 and their `_bn` variants) on the fp32 convolution of f32net.py - every 3 x 3 convolution with its ReLU in the epilogue and, in
the `_bn` variants, its BatchNorm folded in - and the three kernels of csrc/vgg.hip: the 2 x 2 max-pool, AdaptiveAvgPool2d((7, 7))
and the split-K Linear that streams the classifier's 494 MB of weights.  What the reference's `ClassificationMetric` builds for its
`vgg` entry (eval_classification.py): quantised image -> Resize((224, 224)) -> ImageNet Normalize -> VGG16 ->
MulticlassAccuracy(top_k=1); the preprocess and the accuracy are classify.py's.

The project ships NO weights.  `load_weights` reads a torchvision VGG state dict (or the reference's Lightning checkpoint of one) a
user of the metric already has; `random_weights` makes seeded stand-ins for tests and timing, which say nothing about published
accuracies.  torchvision is not installed where this is developed: the key layout (`features.{i}`, `classifier.{0,3,6}`) and the
NCHW flatten in front of classifier.0 are taken from torchvision's source as recalled, and are unchecked against the package and
against published accuracies.
"""
import ctypes as C
import math

import torch

from . import classify, f32net
from .capi import check, lib
from .f32net import BN_EPS, PackedConvF32, stream, take

# torchvision.models.vgg.cfgs: output channels of each 3 x 3 convolution, "M" a 2 x 2 max-pool
CFGS = {"A": (64, "M", 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"),
        "B": (64, 64, "M", 128, 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"),
        "D": (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"),
        "E": (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M")}
ARCHS = {"vgg11": ("A", False), "vgg13": ("B", False), "vgg16": ("D", False), "vgg19": ("E", False),
         "vgg11_bn": ("A", True), "vgg13_bn": ("B", True), "vgg16_bn": ("D", True), "vgg19_bn": ("E", True)}
POOL_OUT = 7                                             # AdaptiveAvgPool2d((7, 7))
FEATURES = 512 * POOL_OUT * POOL_OUT                     # classifier.0's inputs
MIN_HW = 32                                              # five 2 x 2 pools
LINEAR_KEYS = ("classifier.0", "classifier.3", "classifier.6")


def _arch(arch):
    if not isinstance(arch, str) or arch not in ARCHS:
        raise ValueError(f"unknown VGG arch {arch!r}: choose from {sorted(ARCHS)}")
    return ARCHS[arch]


def plan(arch):
    """The `features` Sequential of `arch` in order: ("conv", conv index, BatchNorm index or None, Cout, Cin) and ("pool", index)."""
    cfg, bn = _arch(arch)
    out, i, cin = [], 0, 3
    for v in CFGS[cfg]:
        if v == "M":
            out.append(("pool", i))
            i += 1
        else:
            out.append(("conv", i, i + 1 if bn else None, v, cin))
            i += 3 if bn else 2                          # conv, (BatchNorm,) ReLU
            cin = v
    return out


def conv_indices(arch):
    """The `features` indices of the convolutions of `arch`."""
    return [step[1] for step in plan(arch) if step[0] == "conv"]


def fold_bn_bias(w, b, gamma, beta, mean, var, eps: float = BN_EPS):
    """conv WITH a bias followed by eval-mode BatchNorm as one convolution, folded in fp64: (weight fp64, bias fp64) =
    (w * s, (b - mean) * s + beta), s = gamma / sqrt(var + eps)."""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * scale.view(-1, 1, 1, 1), (b.double() - mean.double()) * scale + beta.double()


# ---- the packed Linear ------------------------------------------------------------------------------------------------------------

def linear_wpack_dims(k: int, n: int):
    """(Kpad, Npad, S) of ur_vgg_linear_f32's weight layout and its split count for a [N, K] matrix."""
    kpad, npad, splits = C.c_int(), C.c_int(), C.c_int()
    check(lib.ur_vgg_linear_wpack_dims(k, n, kpad, npad, splits))
    return kpad.value, npad.value, splits.value


def pack_linear_weight(w: torch.Tensor) -> torch.Tensor:
    """A Linear's [N, K] fp32 matrix -> the kernel's layout (CPU tensor [Npad / 32, Kpad / 8, 64, 4]): element j of lane l in (column
    tile c, k block b) is W[32 c + (l & 31)][8 b + 4 (l >> 5) + j], zero for a column >= N or k >= K."""
    n, k = w.shape
    kpad, npad, _s = linear_wpack_dims(k, n)
    out = torch.zeros(npad // 32, kpad // 8, 2, 32, 4, dtype=torch.float32)
    for c in range(npad // 32):                          # by column tile: no second full-size copy of a 411 MB matrix
        rows = w[32 * c:32 * c + 32].float()
        tile = torch.zeros(32, kpad, dtype=torch.float32)
        tile[:rows.shape[0], :k] = rows
        out[c] = tile.view(32, kpad // 8, 2, 4).permute(1, 2, 0, 3)
    return out.view(npad // 32, kpad // 8, 64, 4)


def unpack_linear_weight(wp: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """pack_linear_weight's inverse: the [N, K] matrix a packed tensor holds (a host check of the layout)."""
    nct, nkb = wp.shape[:2]
    return wp.view(nct, nkb, 2, 32, 4).permute(0, 3, 1, 2, 4).reshape(nct * 32, nkb * 8)[:n, :k]


class PackedLinearF32:
    """One fp32 Linear ready for ur_vgg_linear_f32: the repacked matrix and the bias on the device, and its sizes."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, dev):
        self.n, self.k = weight.shape
        self.splits = linear_wpack_dims(self.k, self.n)[2]
        self.w = pack_linear_weight(weight).to(dev)
        self.bias = bias.float().contiguous().to(dev)


def nhwc_columns(w: torch.Tensor, channels: int = 512) -> torch.Tensor:
    """classifier.0's [N, C * 49] matrix with its columns moved from torchvision's NCHW flatten (c * 49 + h * 7 + w) to the NHWC
    flatten of the activations here ((h * 7 + w) * C + c)."""
    n = w.shape[0]
    return w.view(n, channels, POOL_OUT * POOL_OUT).permute(0, 2, 1).reshape(n, POOL_OUT * POOL_OUT * channels)


class VGGWeights:
    """One VGG ready for the fp32 kernels: every convolution repacked on the device (3 x 3, pad 1; in the `_bn` variants with its
    BatchNorm folded in in fp64, the convolution's own bias included), the three Linears packed for ur_vgg_linear_f32 -
    classifier.0 with its columns permuted to the NHWC flatten - and the class count and hidden width read from the file's shapes.
    `cpu` keeps the unfused fp32 state dict under torchvision's keys: what a host restatement of the network needs."""

    def __init__(self, arch: str, sd: dict, dev=None, source: str = "state dict"):
        _cfg, bn = _arch(arch)                                               # every check first: nothing is uploaded for a bad file
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        self.arch, self.device = arch, dev
        cpu = {}
        get = lambda key, shape: take(sd, source, key, shape, keep=cpu)      # noqa: E731
        host = {}
        for step in plan(arch):
            if step[0] != "conv":
                continue
            _kind, ci, bi, cout, cin = step
            w, b = get(f"features.{ci}.weight", (cout, cin, 3, 3)), get(f"features.{ci}.bias", (cout,))
            if bi is not None:
                bkey = f"features.{bi}"
                stats = [get(f"{bkey}.{n}", (cout,)) for n in ("weight", "bias", "running_mean", "running_var")]
                if not bool((stats[3].double() + BN_EPS > 0).all()):
                    raise ValueError(f"{source}: {bkey + '.running_var'!r} + eps is not positive: not a trained BatchNorm")
                fw, fb = fold_bn_bias(w, b, *stats)
                if not (bool(torch.isfinite(fw).all()) and bool(torch.isfinite(fb).all())):
                    raise ValueError(f"{source}: folding {bkey!r} into {'features.' + str(ci)!r} gives a non-finite value")
                w, b = fw.float(), fb.float()
            host[f"features.{ci}"] = (w, b)
        shapes = []
        for key in ("classifier.0.weight", "classifier.6.weight"):
            t = sd.get(key)
            if not torch.is_tensor(t) or t.ndim != 2:
                raise ValueError(f"{source}: key {key!r} is missing or is no [outputs, inputs] matrix")
            shapes.append(tuple(t.shape))
        self.hidden, self.num_classes = int(shapes[0][0]), int(shapes[1][0])
        linears = {}
        for key, n, k in (("classifier.0", self.hidden, FEATURES), ("classifier.3", self.hidden, self.hidden),
                          ("classifier.6", self.num_classes, self.hidden)):
            linears[key] = (get(f"{key}.weight", (n, k)), get(f"{key}.bias", (n,)))
        self.cpu = cpu
        self.plan = plan(arch)
        self.convs = {k: PackedConvF32(w, b, 1, 1, dev) for k, (w, b) in host.items()}
        self.linears = {k: PackedLinearF32(nhwc_columns(w) if k == "classifier.0" else w, b, dev) for k, (w, b) in linears.items()}


def load_weights(arch, path, dev=None) -> VGGWeights:
    """arch: one of ARCHS; path: the user's torchvision VGG state dict - `features.{i}.weight/bias` (and, in the `_bn` variants, the
    BatchNorm after each convolution) and `classifier.{0,3,6}.weight/bias` - or the reference's Lightning checkpoint of one
    (`state_dict` with a `model.` prefix).  The class count and the hidden width are classifier.6's and classifier.0's first axes.
    ValueError (file and key named) for a missing key, a wrong shape or a non-finite value, before anything is uploaded."""
    _arch(arch)                                                      # an unknown arch, before the file is read
    return VGGWeights(arch, f32net.read_state_dict(path), dev, source=str(path))


def random_state_dict(arch, seed: int, num_classes: int = 1000, hidden: int = 4096) -> dict:
    """A seeded stand-in in torchvision's key layout, for tests and timing ONLY: Kaiming-scaled convolutions (std sqrt(2 / fan_in))
    with small biases, BatchNorm as f32net.random_backbone draws it (gamma in [0.5, 1.5], running_var in [0.5, 1.5], small beta and
    running_mean), Linears uniform in +-1/sqrt(fan_in): fp32 logits stay finite.  NOT trained weights - its predictions say nothing
    about any published accuracy."""
    _arch(arch)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for step in plan(arch):
        if step[0] != "conv":
            continue
        _kind, ci, bi, cout, cin = step
        sd[f"features.{ci}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (cin * 9))
        sd[f"features.{ci}.bias"] = 0.05 * torch.randn(cout, generator=g)
        if bi is not None:
            sd[f"features.{bi}.weight"] = 0.5 + torch.rand(cout, generator=g)
            sd[f"features.{bi}.bias"] = 0.1 * torch.randn(cout, generator=g)
            sd[f"features.{bi}.running_mean"] = 0.1 * torch.randn(cout, generator=g)
            sd[f"features.{bi}.running_var"] = 0.5 + torch.rand(cout, generator=g)
            sd[f"features.{bi}.num_batches_tracked"] = torch.tensor(0)
    for key, n, k in (("classifier.0", hidden, FEATURES), ("classifier.3", hidden, hidden), ("classifier.6", num_classes, hidden)):
        sd[f"{key}.weight"] = (2 * torch.rand(n, k, generator=g) - 1) / math.sqrt(k)
        sd[f"{key}.bias"] = (2 * torch.rand(n, generator=g) - 1) / math.sqrt(k)
    return sd


def random_weights(arch, seed: int = 0, num_classes: int = 1000, dev=None, hidden: int = 4096) -> VGGWeights:
    """The structure `load_weights` returns, with `random_state_dict`'s values.  For tests and timing ONLY: no trained weights
    exist where this project is developed, so no parity with any published accuracy is claimed."""
    return VGGWeights(arch, random_state_dict(arch, seed, num_classes, hidden), dev, source=f"random_state_dict({arch!r}, {seed})")


# ---- launch wrappers of csrc/vgg.hip (fp32 device tensors) ------------------------------------------------------------------------

def _dense(t, nd):
    return torch.is_tensor(t) and t.ndim == nd and t.dtype == torch.float32 and t.is_cuda and t.numel() > 0 and t.is_contiguous()


def _describe(t):
    return f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', 'the host')}"


def linear(x: torch.Tensor, pl: PackedLinearF32, relu: bool = False) -> torch.Tensor:
    """act(x . W^T + bias) for x fp32 [M, K] -> [M, N] on ur_vgg_linear_f32: K split over the grid in S = ceil(K / 512) parts, the
    parts summed in a fixed order by a second launch.  Row i depends on row i of x alone: the same bits alone, in any batch, at any
    position; a NaN or an infinity in a row reaches that row only; relu keeps NaN and +inf and turns -inf into 0."""
    if not _dense(x, 2) or x.shape[1] != pl.k or x.device != pl.w.device:
        raise ValueError(f"vgg.linear: needs a non-empty contiguous fp32 [M, {pl.k}] tensor on {pl.w.device}, got {_describe(x)}")
    m = x.shape[0]
    ws_bytes = lib.ur_vgg_linear_ws_bytes(m, pl.k, pl.n)
    y = torch.empty(m, pl.n, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=x.device)
    check(lib.ur_vgg_linear_f32(x.data_ptr(), pl.w.data_ptr(), pl.bias.data_ptr(), y.data_ptr(), ws.data_ptr(), ws_bytes, m, pl.k, pl.n,
                                int(bool(relu)), stream()))
    return y


def maxpool2(x: torch.Tensor) -> torch.Tensor:
    """2 x 2 / stride 2 / no padding, floor mode, on NHWC fp32: an odd last row or column is not read.  NaN and -inf as
    f32net.maxpool2d_f32: a NaN tap is the window's maximum."""
    if not _dense(x, 4) or x.shape[1] < 2 or x.shape[2] < 2:
        raise ValueError(f"vgg.maxpool2: needs a contiguous fp32 NHWC device tensor with H, W >= 2, got {_describe(x)}")
    n, h, w, c = x.shape
    y = torch.empty(n, h // 2, w // 2, c, dtype=torch.float32, device=x.device)
    check(lib.ur_vgg_maxpool2_f32(x.data_ptr(), y.data_ptr(), n, h, w, c, stream()))
    return y


def avgpool7(x: torch.Tensor) -> torch.Tensor:
    """F.adaptive_avg_pool2d(x, (7, 7)) on NHWC fp32 [N,H,W,C] -> [N,7,7,C].  A 7 x 7 map is returned as it is, without a launch."""
    if not _dense(x, 4):
        raise ValueError(f"vgg.avgpool7: needs a non-empty contiguous fp32 NHWC device tensor, got {_describe(x)}")
    n, h, w, c = x.shape
    if h == POOL_OUT and w == POOL_OUT:
        return x
    y = torch.empty(n, POOL_OUT, POOL_OUT, c, dtype=torch.float32, device=x.device)
    check(lib.ur_vgg_avgpool7_f32(x.data_ptr(), y.data_ptr(), n, h, w, c, stream()))
    return y


def logits(x: torch.Tensor, wts: VGGWeights) -> torch.Tensor:
    """The network on an already-preprocessed NHWC fp32 input [N, H >= 32, W >= 32, 3] -> logits [N, classes].  Dropout is the
    identity in eval."""
    if not _dense(x, 4) or x.shape[3] != 3 or x.shape[1] < MIN_HW or x.shape[2] < MIN_HW:
        raise ValueError(f"vgg.logits: needs a contiguous fp32 NHWC [N, H >= {MIN_HW}, W >= {MIN_HW}, 3] device tensor (five 2 x 2 "
                         f"pools), got {_describe(x)}")
    for step in wts.plan:
        x = maxpool2(x) if step[0] == "pool" else f32net.conv2d_f32(x, wts.convs[f"features.{step[1]}"])
    f = avgpool7(x).view(x.shape[0], FEATURES)                      # the NHWC flatten: classifier.0's columns were permuted to it
    f = linear(f, wts.linears["classifier.0"], relu=True)
    f = linear(f, wts.linears["classifier.3"], relu=True)
    return linear(f, wts.linears["classifier.6"])


def forward(images: torch.Tensor, wts: VGGWeights) -> torch.Tensor:
    """ops.vgg after its argument checks: the classifier's preprocess + network, logits [N, classes]."""
    return logits(classify.preprocess(images), wts)
