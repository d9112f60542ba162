"""Segmenter scoring of the `seg` output on the GPU in exact fp32: the module of the segmenter family.  It holds once what the
two networks share - the evaluator's three-scale test-time augmentation (`segment`, written against the small surface both
weights classes expose: `name`, `min_hw`, `prep`, `logits`, `tta_argmax`), the arch and class-count checks, the launch wrappers
of csrc/segment.hip, the confusion matrix and the mIoU formula - and RefineNet-LightWeight (ResNet-50 / 101 / 152 backbone) on
the fp32 layers and the ResNet backbone of f32net.py; DeepLabV3+ is deeplab.py.  What the reference's
`SemanticSegmentationMetric` builds (eval_semantic_segmentation.py:170-251): quantised image -> scales (1, 0.8, 0.6), bilinear
align_corners=True -> the segmenter (x * 255 - mean, BGR, ResNetLW) -> every scale's logits resized to the label map -> mean ->
argmax -> MulticlassJaccardIndex(19, ignore_index=255).

The project ships NO weights.  `load_weights` reads the state dict (or Lightning checkpoint) a user of the metric already has;
`random_weights` makes seeded stand-ins for tests and timing, which say nothing about any published mIoU.
"""
import math

import torch

from . import f32net
from .capi import check, lib
from .f32net import PackedConvF32, stream, take

# arch -> bottleneck blocks per stage (the torchvision layout, the stride on the 3x3 convolution)
ARCHS = {"rflw50": (3, 4, 6, 3), "rflw101": (3, 4, 23, 3), "rflw152": (3, 8, 36, 3)}
MIN_HW = 32                                              # the smallest network input whose last stage still has one pixel
SCALES = (1, 0.8, 0.6)                                   # the reference's test-time augmentation
CRP_STAGES = 4


def depths_of(arch, archs=ARCHS, noun="segmenter"):
    """archs[arch], or `arch` itself when it is a tuple of four block counts (tests build a (1, 1, 1, 1) network).  archs, noun:
    the network's arch table and what the error calls it."""
    if isinstance(arch, (tuple, list)) and len(arch) == 4 and all(isinstance(d, int) and d >= 1 for d in arch):
        return tuple(arch)
    if not isinstance(arch, str) or arch not in archs:
        raise ValueError(f"unknown {noun} arch {arch!r}: choose from {sorted(archs)}")
    return archs[arch]


def class_count(sd, source, key, filter_shape):
    """The number of classes: the output channels of the last convolution `key`, a [classes, *filter_shape] filter.  ValueError
    (`source` named) when it is missing, is no 4-D tensor or has more classes than the one-byte prediction holds."""
    clf = sd.get(f"{key}.weight") if isinstance(sd, dict) else None
    if not torch.is_tensor(clf) or clf.ndim != 4:
        raise ValueError(f"{source}: key '{key}.weight' is missing or is no [classes, {filter_shape}] filter")
    if not 1 <= clf.shape[0] <= 255:
        raise ValueError(f"{source}: '{key}.weight' has {clf.shape[0]} classes, the one-byte prediction holds 1..255")
    return int(clf.shape[0])


def conv_plan(arch):
    """[(conv key, bn key, Cout, Cin, kernel, stride, pad)] of every backbone convolution, in state-dict order."""
    return f32net.resnet_plan("bottleneck", depths_of(arch))


def head_plan(num_classes: int = 19):
    """[(conv key, Cout, Cin, kernel)] of the light-weight RefineNet head (bias-free but for clf_conv), in execution order."""
    plan = []
    for g, (cin_l, mid) in enumerate(((2048, 512), (1024, 256), (512, 256), (256, 256)), 1):
        plan.append((f"p_ims1d2_outl{g}_dimred", mid, cin_l, 1))
        if g > 1:
            plan.append((f"adapt_stage{g}_b2_joint_varout_dimred", mid, mid, 1))
        plan += [(f"mflow_conv_g{g}_pool.0.{i}_outvar_dimred", mid, mid, 1) for i in range(1, CRP_STAGES + 1)]
        if g < 4:
            plan.append((f"mflow_conv_g{g}_b3_joint_varout_dimred", 256, mid, 1))
    plan.append(("clf_conv", num_classes, 256, 3))
    return plan


class SegmenterWeights:
    """One RefineNet-LW ready for the fp32 kernels: every backbone convolution with its BatchNorm folded in (fp64 fold, rounded to
    fp32, repacked, on the device), the head's bias-free convolutions with a zero bias, clf_conv with its own.  `cpu` keeps the
    UNFUSED state dict (fp32 tensors under the reference module's keys): what a host restatement of the network needs.  `name`,
    `min_hw`, `prep`, `logits` and `tta_argmax` are what the test-time augmentation (`segment`) reads; deeplab.DeepLabWeights has
    the same five."""
    name, min_hw = "segment", MIN_HW

    def __init__(self, arch, sd: dict, dev=None, source: str = "state dict"):
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        self.arch, self.device, self.depths = arch, dev, depths_of(arch)
        self.cpu, self.convs = {}, {}
        ready = f32net.fold_convs(conv_plan(arch), sd, source, self.cpu)      # every check first: nothing is uploaded for a bad file
        self.num_classes = class_count(sd, source, "clf_conv", "256, 3, 3")
        for ckey, cout, cin, k in head_plan(self.num_classes):
            w = take(sd, source, f"{ckey}.weight", (cout, cin, k, k), keep=self.cpu)
            b = take(sd, source, "clf_conv.bias", (cout,), keep=self.cpu) if ckey == "clf_conv" else torch.zeros(cout)
            ready.append((ckey, w, b, 1, k // 2))
        for ckey, w, b, stride, pad in ready:
            self.convs[ckey] = PackedConvF32(w, b, stride, pad, dev)
        # the backbone's blocks in execution order, by stage: (conv keys of the main path, downsample key or None)
        self.stages = f32net.resnet_stages("bottleneck", self.depths, self.convs)

    def prep(self, images, size):
        return prep(images, size)

    def logits(self, x):
        return logits(x, self)

    def tta_argmax(self, maps, in_sizes, size, want_avg=False):
        return tta_argmax(maps, size, want_avg)                      # the evaluator resizes this network's logits once: no in_sizes


def load_weights(arch, path, dev=None) -> SegmenterWeights:
    """arch: one of ARCHS; path: the user's state dict of the reference's `ResNetLW` (`conv1`, `bn1`, `layer{1..4}.*`,
    `p_ims1d2_outl{1..4}_dimred`, `adapt_stage{2..4}_b2_joint_varout_dimred`, `mflow_conv_g{1..4}_pool.0.{1..4}_outvar_dimred`,
    `mflow_conv_g{1..3}_b3_joint_varout_dimred`, `clf_conv.{weight,bias}`; `num_batches_tracked` is ignored) or a Lightning
    checkpoint of one.  The number of classes is clf_conv.weight's.  ValueError (file and key named) for a missing key, a wrong
    shape, a non-finite value or a non-positive running_var + eps."""
    depths_of(arch)                                                  # an unknown arch, before the file is read
    return SegmenterWeights(arch, f32net.read_state_dict(path), dev, source=str(path))


def random_state_dict(arch, seed: int, num_classes: int = 19) -> dict:
    """A seeded stand-in in the reference module's key layout, for tests and timing ONLY.  The backbone follows
    classify.random_state_dict (Kaiming-scaled convolutions, BatchNorm gamma in [0.5, 1.5], halved on the last BatchNorm of every
    block, running_var in [0.5, 1.5], small beta and running_mean) except that conv1 is 255 times smaller: this network's input is
    the 0..255 image minus its mean, not a unit-variance one.  The head's convolutions are zero-mean with std sqrt(1 / fan_in)
    (half that inside the chained residual pooling, whose four stages add up; four times that in clf_conv), and the convolution
    that takes a backbone stage's features is scaled down by 1.2 per block in front of it beyond one per stage, the rate at which
    the stand-in residual sums grow: fp32 logits stay O(10) at every depth.  NOT trained weights -
    its predictions say nothing about any published mIoU."""
    g = torch.Generator().manual_seed(seed)
    sd = f32net.random_backbone(conv_plan(arch), "bottleneck", g, conv1_gain=1.0 / 255.0)
    depths = depths_of(arch)
    for ckey, cout, cin, k in head_plan(num_classes):
        gain = 0.5 if "_pool." in ckey else 4.0 if ckey == "clf_conv" else 1.0
        if ckey.startswith("p_ims1d2_outl"):                         # stage 5 - g's features: about 1.2 x per block beyond the first
            li = 5 - int(ckey[len("p_ims1d2_outl")])
            gain = 1.2 ** -(sum(depths[:li]) - li)
        sd[f"{ckey}.weight"] = torch.randn(cout, cin, k, k, generator=g) * (gain * math.sqrt(1.0 / (cin * k * k)))
    sd["clf_conv.bias"] = 0.1 * torch.randn(num_classes, generator=g)
    return sd


def random_weights(arch, seed: int = 0, num_classes: int = 19, dev=None) -> SegmenterWeights:
    """The structure `load_weights` returns, with `random_state_dict`'s values.  For tests and timing ONLY: no trained weights
    exist where this project is developed, so no parity with any published mIoU is claimed."""
    return SegmenterWeights(arch, random_state_dict(arch, seed, num_classes), dev, source=f"random_state_dict({arch!r}, {seed})")


# ---- sizes on the host ---------------------------------------------------------------------------------------------------------

def scaled_size(n: int, s) -> int:
    """The output size of `F.interpolate(scale_factor=s)` for an axis of n: floor(n * s) in host double."""
    return math.floor(n * s)


# ---- launch wrappers of csrc/segment.hip (fp32 device tensors, NHWC behind the preprocess) --------------------------------------

def prep(x: torch.Tensor, size=None, entry=lib.ur_seg_prep) -> torch.Tensor:
    """fp32 NCHW [N,3,H,W] in [0,1] -> NHWC [N,h,w,3] (size = (h, w), default the input's): bilinear align_corners=True resize, then
    the network's own arithmetic - with `entry` ur_seg_prep, RefineNet-LW's v * 255 - mean_c, channels in B, G, R order; with
    ur_dlv3_prep, DeepLabV3+'s (deeplab.prep).  At the input's own size the resize is the identity, bit for bit (finite images).
    The first call for a new pair of sizes uploads its tables: run a shape once eagerly before capturing it in a graph."""
    n, c, h, w = x.shape
    oh, ow = (h, w) if size is None else size
    iy, wy = f32net._device_tables((h,), oh, x.device.index)
    ix, wx = f32net._device_tables((w,), ow, x.device.index)
    y = torch.empty(n, oh, ow, 3, dtype=torch.float32, device=x.device)
    check(entry(x.data_ptr(), y.data_ptr(), n, c, h, w, oh, ow, iy.data_ptr(), wy.data_ptr(), ix.data_ptr(), wx.data_ptr(), stream()))
    return y


def tta_setup(maps, size, want_avg, in_sizes=None):
    """What both `tta_argmax`s start with: the checks on one to three NHWC fp32 maps [N,h_i,w_i,C] (and, when given, on as many
    input sizes) -> (maps as a list, pred uint8 [N,H,W], avg fp32 [N,H,W,C] or None, the map pointers padded to three)."""
    maps = list(maps)
    if not 1 <= len(maps) <= 3 or (in_sizes is not None and len(in_sizes) != len(maps)):
        raise ValueError(f"tta_argmax: needs 1 to 3 logit maps, got {len(maps)}" if in_sizes is None else
                         f"tta_argmax: needs 1 to 3 maps and as many input sizes, got {len(maps)} and {len(in_sizes)}")
    n, _h, _w, c = maps[0].shape
    dev = maps[0].device
    for m in maps:
        if m.ndim != 4 or m.dtype != torch.float32 or not m.is_contiguous() or m.shape[0] != n or m.shape[3] != c or m.device != dev:
            raise ValueError(f"tta_argmax: every map must be a contiguous fp32 [{n}, h, w, {c}] tensor on {dev}, got "
                             f"{m.dtype} {tuple(m.shape)} on {m.device}")
    pred = torch.empty(n, *size, dtype=torch.uint8, device=dev)
    avg = torch.empty(n, *size, c, dtype=torch.float32, device=dev) if want_avg else None
    return maps, pred, avg, [m.data_ptr() for m in maps] + [None] * (3 - len(maps))


def tta_argmax(maps, size, want_avg: bool = False):
    """One to three NHWC fp32 logit maps [N,h_i,w_i,C] -> pred uint8 [N,H,W] at size = (H, W): per pixel and class the maps are
    sampled bilinearly (align_corners=True) and averaged as ((a + b) + c) / len(maps); ties go to the lowest class and a NaN is the
    maximum, as torch.argmax has it.  want_avg: also return the averaged logits fp32 [N,H,W,C] - for tests; without it no
    full-resolution logit tensor is ever written."""
    maps, pred, avg, ptr = tta_setup(maps, size, want_avg)
    (n, oh, ow), c, dev = pred.shape, maps[0].shape[3], pred.device
    iy, wy = f32net._device_tables(tuple(m.shape[1] for m in maps), oh, dev.index)
    ix, wx = f32net._device_tables(tuple(m.shape[2] for m in maps), ow, dev.index)
    hw = [v for m in maps for v in m.shape[1:3]] + [0] * (2 * (3 - len(maps)))
    check(lib.ur_seg_tta_argmax(*ptr, len(maps), n, c, *hw, oh, ow, iy.data_ptr(), wy.data_ptr(), ix.data_ptr(), wx.data_ptr(), pred.data_ptr(),
                                None if avg is None else avg.data_ptr(), stream()))
    return (pred, avg) if want_avg else pred


def confusion(pred: torch.Tensor, target: torch.Tensor, classes: int = 19, ignore_index: int = 255) -> torch.Tensor:
    """pred uint8, target uint8 or int64, of one shape, contiguous on one device -> int64 [classes, classes] with conf[target][pred],
    over the pixels whose target lies in [0, classes) and is not ignore_index.  The arguments are NOT checked (ops.confusion does)."""
    p = pred.numel()
    ws = torch.empty(int(lib.ur_seg_confusion_ws_bytes(p, classes)) // 4, dtype=torch.int32, device=pred.device)
    conf = torch.empty(classes, classes, dtype=torch.int64, device=pred.device)
    check(lib.ur_seg_confusion(pred.data_ptr(), target.data_ptr(), int(target.dtype == torch.int64), p, classes, ignore_index, ws.data_ptr(),
                               ws.numel() * 4, conf.data_ptr(), stream()))
    return conf


# ---- the network ---------------------------------------------------------------------------------------------------------------

def _crp(x, wts, g):
    """Chained residual pooling: four times top = conv(maxpool5(top)), x = top + x.  `top` feeds the next pool, so the sum is a
    kernel of its own - except in the last stage, where it is the convolution's residual input (the same single rounding)."""
    top = x
    for i in range(1, CRP_STAGES + 1):
        pc = wts.convs[f"mflow_conv_g{g}_pool.0.{i}_outvar_dimred"]
        if i == CRP_STAGES:
            return f32net.conv2d_f32(f32net.maxpool5_f32(top), pc, res=x, relu=False)
        top = f32net.conv2d_f32(f32net.maxpool5_f32(top), pc, relu=False)
        x = f32net.add_f32(top, x)


def logits(x: torch.Tensor, wts: SegmenterWeights) -> torch.Tensor:
    """The network on an already-preprocessed NHWC fp32 input [N,H,W,3], H, W >= 32 -> logits NHWC [N, H/4, W/4, classes] (the
    quarter-resolution map of layer1), in the op order of the reference's `ResNetLW.forward`; dropout is the identity in eval."""
    n, h, w, c = x.shape
    if c != 3 or h < MIN_HW or w < MIN_HW:
        raise ValueError(f"segment.logits: needs an NHWC [N, H>={MIN_HW}, W>={MIN_HW}, 3] input, got {tuple(x.shape)}")
    cv = wts.convs
    l1, l2, l3, l4 = f32net.resnet_trunk(x, cv, wts.stages)
    x = _crp(f32net.conv2d_f32(l4, cv["p_ims1d2_outl1_dimred"]), wts, 1)
    for g, skip in ((2, l3), (3, l2), (4, l1)):
        x = f32net.conv2d_f32(x, cv[f"mflow_conv_g{g - 1}_b3_joint_varout_dimred"], relu=False)
        x = f32net.upsample_bilinear_ac_f32(x, skip.shape[1:3])
        s = f32net.conv2d_f32(skip, cv[f"p_ims1d2_outl{g}_dimred"], relu=False)
        x = _crp(f32net.conv2d_f32(s, cv[f"adapt_stage{g}_b2_joint_varout_dimred"], res=x), wts, g)
    return f32net.conv2d_f32(x, cv["clf_conv"], relu=False)


def segment(images: torch.Tensor, wts, size=None, scales=SCALES) -> torch.Tensor:
    """ops.segment and ops.deeplab after their argument checks, for either network's weights: pred uint8 [N,H,W] at `size`
    (default: the images' own).  For each scale s the image is resized to (floor(H s), floor(W s)), preprocessed and run through
    the network; one kernel resizes the scales' maps to `size` (DeepLabV3+'s through its own half-pixel resize to the scale's
    input first), averages them and takes the argmax.  ValueError when the smallest scale's input falls below the network's
    `min_hw` (32 px for RefineNet-LW, 16 for DeepLabV3+) on a side."""
    n, _c, h, w = images.shape
    scales = tuple(scales)
    if not 1 <= len(scales) <= 3:
        raise ValueError(f"{wts.name}: needs 1 to 3 scales, got {scales}")
    sizes = [(scaled_size(h, s), scaled_size(w, s)) for s in scales]
    small = min(sizes)
    if min(min(sz) for sz in sizes) < wts.min_hw:
        raise ValueError(f"{wts.name}: {h} x {w} images at scales {scales} give a {small[0]} x {small[1]} input, below the network's "
                         f"{wts.min_hw} px")
    maps = [wts.logits(wts.prep(images, sz)) for sz in sizes]
    return wts.tta_argmax(maps, sizes, (h, w) if size is None else tuple(size))


def miou(conf):
    """(mIoU, pixel accuracy, per-class IoU list) of a confusion matrix conf[target][pred], in host fp64.  iou_c = diag_c /
    (row_c + col_c - diag_c); the mean runs over the classes with a non-zero denominator - a class that is neither a target nor a
    prediction is left out (per-class IoU NaN), one that is predicted but never a target counts 0.  That is the reference's own
    `mIoU.compute` (nanmean over diag / (rows + cols - diag)) and the documented macro behaviour of current torchmetrics'
    MulticlassJaccardIndex.  torchmetrics is not installed where this project is developed: the formula is taken from its
    documentation and has NOT been checked against it.  Pixel accuracy = sum diag / sum conf.  No pixels: (0.0, 0.0, [])."""
    conf = torch.as_tensor(conf).detach().cpu().double()
    total = float(conf.sum())
    if total == 0:
        return 0.0, 0.0, []
    diag = torch.diag(conf)
    den = conf.sum(dim=1) + conf.sum(dim=0) - diag
    seen = den > 0
    iou = torch.where(seen, diag / den.clamp(min=1), torch.full_like(diag, float("nan")))
    return float(iou[seen].sum() / seen.sum()), float(diag.sum()) / total, iou.tolist()
