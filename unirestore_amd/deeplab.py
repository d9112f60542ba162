"""DeepLabV3+ scoring of the `seg` output on the GPU in exact fp32: the reference's second segmenter, `dlv3pr50` =
`deeplabv3plus_resnet50(num_classes=19, output_stride=16)` behind an ImageNet Normalize, on the fp32 layers and the ResNet
backbone of f32net.py and the kernels of csrc/segment.hip - what is this network's alone: its plans, its weight loading, the
network and the wrapper of its two-stage argmax.  The three-scale test-time augmentation, the checks and the preprocess launch
are segment.py's, shared with RefineNet-LW; the half-pixel resize and the broadcast are f32net.py's.  What the reference's
`SemanticSegmentationMetric` builds for this network: quantised image -> scales
(1, 0.8, 0.6), bilinear align_corners=True -> Normalize -> ResNet (layer4 dilated by 2, stride 16) -> ASPP (dilations 6, 12, 18
and a pooled branch) -> decoder on layer1's features -> the model's own align_corners=False resize to its input -> the
evaluator's align_corners=True resize to the label map -> mean -> argmax.  The confusion matrix and the mIoU are segment.py's
(`segment.confusion`, `segment.miou`).  No depthwise convolution is involved: the reference never calls
`convert_to_separable_conv` for this model.

The project ships NO weights.  `load_weights` reads the checkpoint a user of the metric already has; `random_weights` makes
seeded stand-ins for tests and timing, which say nothing about any published mIoU.
"""
import math

import torch

from . import f32net
from . import segment as _segment
from .capi import check, lib
from .f32net import PackedConvF32, broadcast_f32, stream, take, upsample_bilinear_hp_f32
from .segment import SCALES, scaled_size, segment        # `segment`: the one test-time augmentation, under this module's name too

# arch -> bottleneck blocks per stage (the torchvision layout, replace_stride_with_dilation = [False, False, True])
ARCHS = {"dlv3pr50": (3, 4, 6, 3), "dlv3pr101": (3, 4, 23, 3)}
# The smallest network input: one whole cell of the stride-16 map.  (The layers themselves run on anything - ASPP's padding equals
# its dilation - but below 16 px the 1/16 map is a single pixel that is mostly padding, which no use of the metric means.)
MIN_HW = 16
ASPP_DILATIONS = (6, 12, 18)
LOW_CH, ASPP_CH = 48, 256                                # the decoder's input: low-level channels 0..47, then ASPP's 48..303


def depths_of(arch):
    """segment.depths_of with this network's ARCHS."""
    return _segment.depths_of(arch, ARCHS, "DeepLabV3+")


def conv_plan(arch):
    """[(conv key, bn key, Cout, Cin, kernel, stride, pad, dilation)] of every backbone convolution, in state-dict order, keys under
    `backbone.`.  layer4 trades its stride for dilation: block 0's conv2 and downsample have stride 1 (conv2 still dilation 1, pad
    1), the later blocks' conv2 dilation 2 and pad 2."""
    plan = []
    for ckey, bkey, cout, cin, k, stride, pad in f32net.resnet_plan("bottleneck", depths_of(arch)):
        dil = 1
        if ckey.startswith("layer4."):
            stride = 1
            if k == 3 and not ckey.startswith("layer4.0."):
                dil = pad = 2
        plan.append((f"backbone.{ckey}", f"backbone.{bkey}", cout, cin, k, stride, pad, dil))
    return plan


def head_plan(num_classes: int = 19):
    """[(conv key, bn key or None, Cout, Cin, kernel, stride, pad, dilation)] of `DeepLabHeadV3Plus(2048, 256, classes, [6, 12,
    18])`, in state-dict order under `classifier.`; the last convolution has a bias and no BatchNorm."""
    c = "classifier"
    plan = [(f"{c}.project.0", f"{c}.project.1", LOW_CH, 256, 1, 1, 0, 1),
            (f"{c}.aspp.convs.0.0", f"{c}.aspp.convs.0.1", ASPP_CH, 2048, 1, 1, 0, 1)]
    plan += [(f"{c}.aspp.convs.{i}.0", f"{c}.aspp.convs.{i}.1", ASPP_CH, 2048, 3, 1, d, d) for i, d in enumerate(ASPP_DILATIONS, 1)]
    plan += [(f"{c}.aspp.convs.4.1", f"{c}.aspp.convs.4.2", ASPP_CH, 2048, 1, 1, 0, 1),
             (f"{c}.aspp.project.0", f"{c}.aspp.project.1", ASPP_CH, 5 * ASPP_CH, 1, 1, 0, 1),
             (f"{c}.classifier.0", f"{c}.classifier.1", 256, LOW_CH + ASPP_CH, 3, 1, 1, 1),
             (f"{c}.classifier.3", None, num_classes, 256, 1, 1, 0, 1)]
    return plan


CLF_KEY = "classifier.classifier.3"


class DeepLabWeights:
    """One DeepLabV3+ ready for the fp32 kernels: every convolution with its BatchNorm folded in (fp64 fold, rounded to fp32,
    repacked, on the device), the last one with its own bias.  `cpu` keeps the UNFUSED state dict (fp32 tensors under the reference
    module's keys): what a host restatement of the network needs.  `name`, `min_hw`, `prep`, `logits` and `tta_argmax` are what the
    test-time augmentation (segment.segment) reads."""
    name, min_hw = "deeplab", MIN_HW

    def __init__(self, arch, sd: dict, dev=None, source: str = "state dict"):
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        self.arch, self.device, self.depths = arch, dev, depths_of(arch)
        self.cpu, self.convs = {}, {}
        self.num_classes = _segment.class_count(sd, source, CLF_KEY, "256, 1, 1")
        plan = conv_plan(arch) + head_plan(self.num_classes)
        geometry = {e[0]: e[5:] for e in plan}
        ready = f32net.fold_convs([e[:7] for e in plan if e[1] is not None], sd, source, self.cpu)      # every check first
        ready.append((CLF_KEY, take(sd, source, f"{CLF_KEY}.weight", (self.num_classes, 256, 1, 1), keep=self.cpu),
                      take(sd, source, f"{CLF_KEY}.bias", (self.num_classes,), keep=self.cpu), 1, 0))
        for ckey, w, b, _stride, _pad in ready:
            stride, pad, dil = geometry[ckey]
            self.convs[ckey] = PackedConvF32(w, b, stride, pad, dev, dilation=dil)
        # the backbone under f32net's own keys, and its blocks in execution order
        self.backbone = {k[len("backbone."):]: v for k, v in self.convs.items() if k.startswith("backbone.")}
        self.stages = f32net.resnet_stages("bottleneck", self.depths, self.backbone)

    def prep(self, images, size):
        return prep(images, size)

    def logits(self, x):
        return logits(x, self)

    def tta_argmax(self, maps, in_sizes, size, want_avg=False):
        return tta_argmax(maps, in_sizes, size, want_avg)


def read_state_dict(path) -> dict:
    """What the reference's loader reads: a dict with `model_state` (the published checkpoints), a Lightning checkpoint whose
    `state_dict` keeps the keys under `model.1.` (the network behind the Normalize) with that prefix stripped, or a bare state
    dict."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(ckpt, dict) and isinstance(ckpt.get("model_state"), dict):
        return ckpt["model_state"]
    if isinstance(ckpt, dict) and isinstance(ckpt.get("state_dict"), dict):
        return {k[len("model.1."):]: v for k, v in ckpt["state_dict"].items() if k.startswith("model.1.")}
    if not isinstance(ckpt, dict):
        raise ValueError(f"{path}: not a state dict")
    return ckpt


def load_weights(arch, path, dev=None) -> DeepLabWeights:
    """arch: one of ARCHS; path: the user's checkpoint of the reference's DeepLabV3+ (`backbone.*`, `classifier.project.*`,
    `classifier.aspp.*`, `classifier.classifier.*`; `num_batches_tracked` is ignored) in one of `read_state_dict`'s three forms.
    The number of classes is classifier.classifier.3.weight's.  ValueError (file and key named) for a missing key, a wrong shape, a
    non-finite value or a non-positive running_var + eps - before anything is uploaded."""
    depths_of(arch)                                                  # an unknown arch, before the file is read
    return DeepLabWeights(arch, read_state_dict(path), dev, source=str(path))


def random_state_dict(arch, seed: int, num_classes: int = 19) -> dict:
    """A seeded stand-in in the reference module's key layout, for tests and timing ONLY: segment.random_state_dict's recipe (Kaiming
    convolutions, BatchNorm gamma in [0.5, 1.5], halved on the last BatchNorm of every block, running_var in [0.5, 1.5], small beta
    and running_mean) for the backbone - whose input here is the normalised image, so conv1 is not scaled - and for the head's
    conv + BatchNorm pairs.  The convolutions that take a backbone stage's features are scaled down by 1.2 per block in front of
    them beyond one per stage, the rate at which the stand-in residual sums grow, and the last convolution is zero-mean with std
    4 sqrt(1 / 256): fp32 logits stay O(10) at every depth.  NOT trained weights."""
    g = torch.Generator().manual_seed(seed)
    depths = depths_of(arch)
    sd = f32net.random_backbone([e[:7] for e in conv_plan(arch)], "bottleneck", g)
    head = head_plan(num_classes)
    sd.update(f32net.random_backbone([e[:7] for e in head[:-1]], "bottleneck", g))
    for key, blocks in [("classifier.project.0", depths[0] - 1)] + [(f"classifier.aspp.convs.{i}.{1 if i == 4 else 0}", sum(depths) - 4)
                                                                    for i in range(5)]:
        sd[f"{key}.weight"] = sd[f"{key}.weight"] * 1.2 ** -blocks
    sd[f"{CLF_KEY}.weight"] = torch.randn(num_classes, 256, 1, 1, generator=g) * (4.0 * math.sqrt(1.0 / 256))
    sd[f"{CLF_KEY}.bias"] = 0.1 * torch.randn(num_classes, generator=g)
    return sd


def random_weights(arch, seed: int = 0, num_classes: int = 19, dev=None) -> DeepLabWeights:
    """The structure `load_weights` returns, with `random_state_dict`'s values.  For tests and timing ONLY: no trained weights
    exist where this project is developed, so no parity with any published mIoU is claimed."""
    return DeepLabWeights(arch, random_state_dict(arch, seed, num_classes), dev, source=f"random_state_dict({arch!r}, {seed})")


# ---- launch wrappers of csrc/segment.hip (fp32 device tensors, NHWC behind the preprocess) --------------------------------------

def prep(x: torch.Tensor, size=None) -> torch.Tensor:
    """segment.prep with this network's arithmetic: fp32 NCHW [N,3,H,W] in [0,1] -> NHWC [N,h,w,3], bilinear align_corners=True
    resize, then (v - mean_c) / std_c with the ImageNet constants, channels in R, G, B order."""
    return _segment.prep(x, size, lib.ur_dlv3_prep)


def tta_argmax(maps, in_sizes, size, want_avg: bool = False):
    """One to three NHWC fp32 classifier maps q_i [N,hq_i,wq_i,C] with the network input sizes in_sizes[i] = (hs_i, ws_i) they came
    from -> pred uint8 [N,H,W] at size = (H, W).  Per pixel and class, map i is resized to (hs_i, ws_i) with half-pixel centres
    (the model's own resize) and from there to (H, W) with align_corners=True (the evaluator's), in one kernel that stores neither;
    the maps are averaged as ((a + b) + c) / len(maps); ties go to the lowest class and a NaN is the maximum, as torch.argmax has
    it.  want_avg: also return the averaged logits fp32 [N,H,W,C] - for tests."""
    in_sizes = [tuple(s) for s in in_sizes]
    maps, pred, avg, ptr = _segment.tta_setup(maps, size, want_avg, in_sizes)
    (n, oh, ow), c, dev = pred.shape, maps[0].shape[3], pred.device
    aiy, awy = f32net._device_tables(tuple(s[0] for s in in_sizes), oh, dev.index)
    aix, awx = f32net._device_tables(tuple(s[1] for s in in_sizes), ow, dev.index)
    hiy, hwy = f32net._device_tables_hp(tuple((m.shape[1], s[0]) for m, s in zip(maps, in_sizes)), dev.index)
    hix, hwx = f32net._device_tables_hp(tuple((m.shape[2], s[1]) for m, s in zip(maps, in_sizes)), dev.index)
    dims = [v for m, s in zip(maps, in_sizes) for v in (m.shape[1], m.shape[2], s[0], s[1])] + [0] * (4 * (3 - len(maps)))
    check(lib.ur_dlv3_tta_argmax(*ptr, len(maps), n, c, *dims, oh, ow, aiy.data_ptr(), awy.data_ptr(), aix.data_ptr(), awx.data_ptr(),
                                 hiy.data_ptr(), hwy.data_ptr(), hix.data_ptr(), hwx.data_ptr(), pred.data_ptr(),
                                 None if avg is None else avg.data_ptr(), stream()))
    return (pred, avg) if want_avg else pred


# ---- the network ---------------------------------------------------------------------------------------------------------------

def logits(x: torch.Tensor, wts: DeepLabWeights) -> torch.Tensor:
    """The network on an already-normalised NHWC fp32 input [N,H,W,3], H, W >= 16 -> the classifier's map NHWC [N, H/4, W/4,
    classes] (layer1's resolution; the model's final resize to the input size is folded into `tta_argmax`), in the op order of the
    reference's `DeepLabHeadV3Plus.forward`; dropout is the identity in eval.  ASPP's five branches write their channel slices of
    one 1280-channel tensor, the low-level projection and the resized ASPP output theirs of the decoder's 304-channel input: no
    concat copy."""
    n, h, w, c = x.shape
    if c != 3 or h < MIN_HW or w < MIN_HW:
        raise ValueError(f"deeplab.logits: needs an NHWC [N, H>={MIN_HW}, W>={MIN_HW}, 3] input, got {tuple(x.shape)}")
    cv = wts.convs
    low, _l2, _l3, out = f32net.resnet_trunk(x, wts.backbone, wts.stages)
    cat = torch.empty(n, low.shape[1], low.shape[2], LOW_CH + ASPP_CH, dtype=torch.float32, device=x.device)
    f32net.conv2d_f32(low, cv["classifier.project.0"], out=(cat, 0))
    branches = torch.empty(n, out.shape[1], out.shape[2], 5 * ASPP_CH, dtype=torch.float32, device=x.device)
    for i in range(4):
        f32net.conv2d_f32(out, cv[f"classifier.aspp.convs.{i}.0"], out=(branches, i * ASPP_CH))
    pooled = f32net.conv2d_f32(f32net.avgpool_f32(out).view(n, 1, 1, -1), cv["classifier.aspp.convs.4.1"])      # per image
    broadcast_f32(pooled.view(n, ASPP_CH), branches, 4 * ASPP_CH)
    aspp = f32net.conv2d_f32(branches, cv["classifier.aspp.project.0"])
    upsample_bilinear_hp_f32(aspp, cat.shape[1:3], out=(cat, LOW_CH))
    return f32net.conv2d_f32(f32net.conv2d_f32(cat, cv["classifier.classifier.0"]), cv[CLF_KEY], relu=False)
