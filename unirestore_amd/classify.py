"""Classifier scoring of the `cls` output on the GPU in exact fp32: torchvision-layout ResNets (18 / 50 / 101) on the fp32 layers
and the ResNet backbone of f32net.py and the kernels of csrc/classify.hip - weight loading, the evaluator's preprocess, the
launch wrappers, and the accuracy formulas.  What the reference's `ClassificationMetric` builds
(eval_classification.py:193-309): quantised image -> Resize((224, 224)) -> ImageNet Normalize -> ResNet -> MulticlassAccuracy(top_k=1).

The project ships NO weights.  `load_weights` reads the torchvision state dict (or Lightning checkpoint) a user of the metric
already has; `random_weights` makes seeded stand-ins for tests and timing, which say nothing about published accuracies.
"""
import functools
import math

import torch

from . import f32net
from .capi import check, lib
from .f32net import EXPANSION, PLANES, PackedConvF32, stream, take

# arch -> (block kind, blocks per stage); torchvision's layout, the stride on the 3x3 convolution (ResNet v1.5)
ARCHS = {"resnet18": ("basic", (2, 2, 2, 2)), "resnet50": ("bottleneck", (3, 4, 6, 3)), "resnet101": ("bottleneck", (3, 4, 23, 3))}
OUT_HW = 224                                             # T.Resize((224, 224))
MIN_HW = 32                                              # the smallest network input whose last stage still has one pixel
MAX_TAPS = 64                                            # ur_classify_preprocess's limit per output index


def conv_plan(arch: str):
    """[(conv key, bn key, Cout, Cin, kernel, stride, pad)] of every convolution of `arch`, in state-dict order."""
    if arch not in ARCHS:
        raise ValueError(f"unknown classifier arch {arch!r}: choose from {sorted(ARCHS)}")
    return f32net.resnet_plan(*ARCHS[arch])


class ClassifierWeights:
    """One ResNet ready for the fp32 kernels: every convolution with its BatchNorm folded in (fp64 fold, rounded to fp32, repacked,
    on the device) and the FC layer as a 1x1 convolution.  `cpu` keeps the UNFUSED state dict (fp32 tensors under torchvision's
    keys): what a host restatement of the network needs."""

    def __init__(self, arch: str, sd: dict, dev=None, source: str = "state dict"):
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        plan = conv_plan(arch)
        self.arch, self.device, self.kind = arch, dev, ARCHS[arch][0]
        self.cpu, self.convs = {}, {}
        folded = f32net.fold_convs(plan, sd, source, self.cpu)                # every check first: nothing is uploaded for a bad file
        if "fc.weight" not in sd or not torch.is_tensor(sd["fc.weight"]) or sd["fc.weight"].ndim != 2:
            raise ValueError(f"{source}: key 'fc.weight' is missing or is no [classes, features] matrix")
        feat = PLANES[-1] * EXPANSION[self.kind]
        self.num_classes = int(sd["fc.weight"].shape[0])
        fcw = take(sd, source, "fc.weight", (self.num_classes, feat), keep=self.cpu)
        fcb = take(sd, source, "fc.bias", (self.num_classes,), keep=self.cpu)
        for ckey, fw, fb, stride, pad in folded:
            self.convs[ckey] = PackedConvF32(fw, fb, stride, pad, dev)
        self.fc = PackedConvF32(fcw.view(self.num_classes, feat, 1, 1), fcb, 1, 0, dev)
        # the blocks in execution order: (conv keys of the main path, downsample key or None), by stage and flat
        self.stages = f32net.resnet_stages(self.kind, ARCHS[arch][1], self.convs)
        self.blocks = [b for blocks in self.stages for b in blocks]


def load_weights(arch: str, path, dev=None) -> ClassifierWeights:
    """arch: one of ARCHS; path: the user's torchvision state dict (`conv1.weight`, `bn1.*`, `layer{1..4}.{i}.conv{j}.weight`,
    `.bn{j}.*`, `.downsample.{0,1}.*`, `fc.*`; `num_batches_tracked` is ignored) or a Lightning checkpoint of one.  The number of
    classes is fc.weight's.  ValueError (file and key named) for a missing key, a wrong shape, a non-finite value or a
    non-positive running_var + eps."""
    conv_plan(arch)                                                  # an unknown arch, before the file is read
    return ClassifierWeights(arch, f32net.read_state_dict(path), dev, source=str(path))


def random_state_dict(arch: str, seed: int, num_classes: int = 1000) -> dict:
    """A seeded stand-in in torchvision's key layout, for tests and timing ONLY: Kaiming-scaled convolutions (std
    sqrt(2 / fan_in)), BatchNorm gamma in [0.5, 1.5] (halved on the last BatchNorm of every block, so the residual sums do not
    grow), running_var in [0.5, 1.5], small beta and running_mean, a uniform(+-1/sqrt(fan_in)) FC layer: fp32 logits stay
    finite.  NOT trained weights - its predictions say nothing about any published accuracy."""
    g = torch.Generator().manual_seed(seed)
    sd = f32net.random_backbone(conv_plan(arch), ARCHS[arch][0], g)
    feat = PLANES[-1] * EXPANSION[ARCHS[arch][0]]
    sd["fc.weight"] = (2 * torch.rand(num_classes, feat, generator=g) - 1) / math.sqrt(feat)
    sd["fc.bias"] = (2 * torch.rand(num_classes, generator=g) - 1) / math.sqrt(feat)
    return sd


def random_weights(arch: str, seed: int = 0, num_classes: int = 1000, dev=None) -> ClassifierWeights:
    """The structure `load_weights` returns, with `random_state_dict`'s values.  For tests and timing ONLY: no trained weights
    exist where this project is developed, so no parity with any published accuracy is claimed."""
    return ClassifierWeights(arch, random_state_dict(arch, seed, num_classes), dev, source=f"random_state_dict({arch!r}, {seed})")


# ---- the evaluator's preprocess: tap tables on the host ------------------------------------------------------------------------

def resize_table(n_in: int, n_out: int = OUT_HW):
    """One axis of torch's `interpolate(mode="bilinear", antialias=True, align_corners=False)`: (first [n_out] int32, count [n_out]
    int32, weights [n_out, taps] fp64, zero beyond an output's count), computed in fp64.  The triangle filter is widened by the
    scale when the axis shrinks (support = max(scale, 1)), which equals plain bilinear when it grows."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_table: sizes must be >= 1, got {n_in} -> {n_out}")
    scale = n_in / n_out
    support = max(scale, 1.0)
    first, rows = [], []
    for i in range(n_out):
        center = scale * (i + 0.5)
        lo, hi = max(0, int(center - support + 0.5)), min(n_in, int(center + support + 0.5))
        w = [max(0.0, 1.0 - abs((j - center + 0.5) / support)) for j in range(lo, hi)]
        total = math.fsum(w)
        first.append(lo)
        rows.append([v / total for v in w])
    taps = max(len(r) for r in rows)
    if taps > MAX_TAPS:
        raise ValueError(f"resize_table: {n_in} -> {n_out} needs {taps} taps per output, more than the kernel's {MAX_TAPS}")
    wt = torch.zeros(n_out, taps, dtype=torch.float64)
    for i, r in enumerate(rows):
        wt[i, :len(r)] = torch.tensor(r, dtype=torch.float64)
    return torch.tensor(first, dtype=torch.int32), torch.tensor([len(r) for r in rows], dtype=torch.int32), wt


@functools.lru_cache(maxsize=64)
def _device_table(n_in: int, dev_index: int):
    first, count, wt = resize_table(n_in)
    dev = torch.device("cuda", dev_index)
    return first.to(dev), count.to(dev), wt.float().contiguous().to(dev), int(wt.shape[1])


# ---- launch wrappers of csrc/classify.hip (fp32 device tensors, NHWC behind the preprocess) -------------------------------------

def preprocess(x: torch.Tensor) -> torch.Tensor:
    """fp32 NCHW [N,3,H,W] in [0,1] -> NHWC [N,224,224,3]: antialiased bilinear resize, then (v - mean_c) / std_c.  The first call
    for a new H or W uploads that axis's table: run a shape once eagerly before capturing it in a graph."""
    n, c, h, w = x.shape
    fw, cw, ww, tw = _device_table(w, x.device.index)
    fh, ch, wh, th = _device_table(h, x.device.index)
    tmp = torch.empty(n, 3, h, OUT_HW, dtype=torch.float32, device=x.device)
    y = torch.empty(n, OUT_HW, OUT_HW, 3, dtype=torch.float32, device=x.device)
    check(lib.ur_classify_preprocess(x.data_ptr(), tmp.data_ptr(), y.data_ptr(), n, c, h, w, fw.data_ptr(), cw.data_ptr(), ww.data_ptr(), tw,
                                     fh.data_ptr(), ch.data_ptr(), wh.data_ptr(), th, stream()))
    return y


def top1_counts(logits: torch.Tensor, labels: torch.Tensor):
    """logits fp32 [N,C], labels int64 [N] on the device, already checked to lie in [0, C) -> (pred int64 [N], counts int64 [3,C])."""
    n, c = logits.shape
    pred = torch.empty(n, dtype=torch.int64, device=logits.device)
    counts = torch.empty(3, c, dtype=torch.int64, device=logits.device)
    check(lib.ur_top1_counts(logits.data_ptr(), labels.data_ptr(), n, c, pred.data_ptr(), counts.data_ptr(), stream()))
    return pred, counts


def logits(x: torch.Tensor, wts: ClassifierWeights) -> torch.Tensor:
    """The network on an already-preprocessed NHWC fp32 input [N,H,W,3] of any H, W >= 32 -> logits [N, classes]."""
    n, h, w, c = x.shape
    if c != 3 or h < MIN_HW or w < MIN_HW:
        raise ValueError(f"classify.logits: needs an NHWC [N, H>={MIN_HW}, W>={MIN_HW}, 3] input, got {tuple(x.shape)}")
    pooled = f32net.avgpool_f32(f32net.resnet_trunk(x, wts.convs, wts.stages)[-1])
    return f32net.conv2d_f32(pooled.view(n, 1, 1, -1), wts.fc, relu=False).view(n, wts.num_classes)


def forward(images: torch.Tensor, wts: ClassifierWeights) -> torch.Tensor:
    """ops.classify after its argument checks: preprocess + network, logits [N, classes]."""
    return logits(preprocess(images), wts)


def accuracy(tp, targets, predicted):
    """(macro, micro) of the per-class counts, in host fp64.  micro = sum tp / sum targets.  macro is what the reference's
    torchmetrics `MulticlassAccuracy(top_k=1)` reports by default (average="macro"): the mean of tp_c / targets_c (0 where
    targets_c = 0) over the classes with targets_c + predicted_c > 0 - a class that is predicted but never a target counts as 0,
    a class seen on neither side is left out.  torchmetrics is not installed where this project is developed: the formula is taken
    from its documented behaviour and has NOT been checked against it.  No images: (0.0, 0.0)."""
    tp, targets, predicted = (torch.as_tensor(t).detach().cpu().double().reshape(-1) for t in (tp, targets, predicted))
    seen = (targets + predicted) > 0
    total = float(targets.sum())
    if total == 0 or not bool(seen.any()):
        return 0.0, 0.0
    per_class = torch.where(targets > 0, tp / targets.clamp(min=1), torch.zeros_like(tp))
    return float(per_class[seen].sum() / seen.sum()), float(tp.sum()) / total
