"""Host restatement of the segmenter scoring (three-scale test-time augmentation, RefineNet-LW preprocess and network, multi-scale
average + argmax, confusion matrix, mIoU) and of each of its stages, in plain torch on the CPU, written from the architecture:
BatchNorm stays UNFUSED (conv2d, then batch_norm), every resize is torch's own `interpolate(align_corners=True)`.
dtype=torch.float64 is the yardstick; torch.float32 is what an fp32 host evaluation of the same restatement computes - its
distance from fp64 is the source of every GPU tolerance (GPU_FACTOR x, the rule of classify_reference.py).  Tensors are NCHW
here; the HIP kernels keep NHWC - `nhwc` / `nchw` convert.  The weights are seeded stand-ins: nothing here says anything about
any published mIoU."""
import functools

import torch
import torch.nn.functional as F

from classify_reference import GPU_FACTOR, _conv_bn, images, nchw, nhwc, varied_images  # noqa: F401  (shared helpers, re-exported)

MEAN = (123.68, 116.779, 103.939)            # R, G, B of the 0..255 image
SCALES = (1, 0.8, 0.6)
TINY = (1, 1, 1, 1)                          # the smallest bottleneck backbone: one block per stage

# ---- the cases ----------------------------------------------------------------------------------------------------------------
# (image shape, scale): the smallest legal input, an even batch, odd sizes
PREP_CASES = (((1, 3, 54, 54), 0.6), ((2, 3, 64, 96), 0.8), ((1, 3, 97, 131), 0.6))
# (N, C, h, w, H, W)
UPSAMPLE_CASES = ((2, 19, 1, 1, 3, 5), (1, 256, 2, 2, 4, 6), (2, 19, 3, 4, 5, 7), (1, 256, 3, 4, 5, 7), (1, 20, 5, 6, 9, 16))
# name -> (N, C, map sizes, (H, W))
TTA_CASES = {
    "three_19": (2, 19, ((16, 24), (12, 19), (9, 14)), (64, 96)),
    "two_19": (1, 19, ((16, 24), (9, 14)), (64, 96)),
    "one_19": (1, 19, ((16, 24),), (33, 47)),
    "three_5": (2, 5, ((7, 9), (5, 8), (4, 5)), (21, 30)),
    "to_1x1": (2, 19, ((4, 6), (3, 5), (2, 3)), (1, 1)),
}
# name -> (arch, weight seed, image seed, N, H, W): scale-1 logits, and the three-scale prediction
NET_CASES = {
    "tiny_2x64x96": (TINY, 3, 11, 2, 64, 96),
    "rflw101_1x64x96": ("rflw101", 5, 12, 1, 64, 96),
}
MAX_LEFT_OUT = 0.005                         # of the pixels may be undecidable (fp64 top-2 gap <= 2 x bound x max |logit|)
MIN_CLASSES = 5

# ---- the tolerances: fp32's OWN error against fp64 on these cases, measured with the restatement below on the CPU (measure_*;
# torch 2.x CPU kernels), and GPU_FACTOR x that for the GPU.
# prep / upsample / tta: fp32 arithmetic on the fp32-rounded fp64 interpolation matrices (what a table-driven fp32 kernel computes,
# up to its summation order) - NOT torch's own fp32 interpolate, which builds its weights in fp32.
E32_PREP = 3.54e-05                          # max |prep32 - prep64| over the cases, absolute, on values up to 151
E32_UPSAMPLE = 5.23e-08                      # max |up32 - up64| / max |x| over the cases
E32_TTA = 5.86e-08                           # max |avg32 - avg64| / max |logit| over the cases
# per NET_CASES entry, max |logits32 - logits64| / max |logits64| at scale 1
E32_LOGITS = {"tiny_2x64x96": 9.88e-07, "rflw101_1x64x96": 9.55e-07}
# the same for the three-scale averaged logits at the image's size (what the argmax sees)
E32_TTA_LOGITS = {"tiny_2x64x96": 6.14e-07, "rflw101_1x64x96": 6.73e-07}
# Measured on an MI355X against fp64 (test_segment_gpu.py and test_f32net_gpu.py print each figure): prep 3.45e-05 .. 3.53e-05; up-sample 0 (1 x 1 source)
# .. 5.23e-08; averaged logits 3.08e-08 .. 5.86e-08 of max |logit|; scale-1 logits 1.42e-06 (depth (1, 1, 1, 1)) and 1.09e-06
# (rflw101) of max |logit|; no pixel left out and no argmax flip on either network.
PREP_TOL = GPU_FACTOR * E32_PREP
UPSAMPLE_TOL = GPU_FACTOR * E32_UPSAMPLE
TTA_TOL = GPU_FACTOR * E32_TTA
LOGITS_TOL = {k: GPU_FACTOR * v for k, v in E32_LOGITS.items()}      # also absorbs the fp32 rounding of the folded weights
TTA_LOGITS_TOL = {k: GPU_FACTOR * v for k, v in E32_TTA_LOGITS.items()}


# ---- resizes ------------------------------------------------------------------------------------------------------------------

def resize_ac(x, size, dtype=torch.float64):
    return F.interpolate(x.to(dtype), size=tuple(size), mode="bilinear", align_corners=True)


@functools.lru_cache(maxsize=None)
def ac_matrix(n_in, n_out):
    """[n_out, n_in] fp64: torch's align_corners=True bilinear resize of one axis as a matrix, read off torch itself by resizing
    the identity (the other axis has size 1 and stays)."""
    eye = torch.eye(n_in, dtype=torch.float64).view(1, n_in, 1, n_in)
    return resize_ac(eye, (1, n_out))[0, :, 0, :].t().contiguous()


def resize_ac_einsum32(x, size):
    """The resize as fp32 arithmetic on the fp32-rounded fp64 matrices."""
    ah, aw = ac_matrix(x.shape[2], size[0]).float(), ac_matrix(x.shape[3], size[1]).float()
    return torch.einsum("nchx,yh->ncyx", torch.einsum("nchw,xw->nchx", x.float(), aw), ah)


def scaled_hw(h, w, s):
    """The size `F.interpolate(scale_factor=s)` gives, asked of torch itself."""
    return tuple(F.interpolate(torch.zeros(1, 1, h, w), scale_factor=s, mode="bilinear", align_corners=True).shape[2:])


def preprocess(x, dtype=torch.float64):
    """The segmenter's own preprocess on a [0,1] NCHW image: x * 255 - mean, then RGB -> BGR."""
    mean = torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)
    return (x.to(dtype) * 255.0 - mean)[:, [2, 1, 0]]


def prep(x, size, dtype=torch.float64):
    """One scale: resize the [0,1] image, then preprocess."""
    return preprocess(resize_ac(x, size, dtype), dtype)


def prep_einsum32(x, size):
    return preprocess(resize_ac_einsum32(x, size), torch.float32)


def measure_prep(case):
    shape, s = case
    x = images(shape, sum(shape))
    size = scaled_hw(shape[2], shape[3], s)
    return float((prep_einsum32(x, size).double() - prep(x, size)).abs().max())


def upsample_case(case):
    n, c, h, w, _H, _W = case
    return torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(sum(case)))


def measure_upsample(case):
    x = upsample_case(case)
    return float((resize_ac_einsum32(x, case[4:]).double() - resize_ac(x, case[4:])).abs().max() / x.abs().max())


def maxpool5(x):
    return F.max_pool2d(x, kernel_size=5, stride=1, padding=2)


# ---- multi-scale average + argmax ---------------------------------------------------------------------------------------------

def tta_average(maps, size, dtype=torch.float64):
    """NCHW logit maps -> their mean at `size`, ((a + b) + c) / n."""
    total = None
    for m in maps:
        up = resize_ac(m, size, dtype)
        total = up if total is None else total + up
    return total / len(maps)


def tta_average_einsum32(maps, size):
    total = None
    for m in maps:
        up = resize_ac_einsum32(m, size)
        total = up if total is None else total + up
    return total / torch.tensor(float(len(maps)), dtype=torch.float32)


def tta_case(name):
    n, c, sizes, _size = TTA_CASES[name]
    g = torch.Generator().manual_seed(sorted(TTA_CASES).index(name) + 50)
    return [3.0 * torch.randn(n, c, h, w, generator=g) for h, w in sizes]


def measure_tta(name):
    maps, size = tta_case(name), TTA_CASES[name][3]
    want = tta_average(maps, size)
    return float((tta_average_einsum32(maps, size).double() - want).abs().max() / max(float(m.abs().max()) for m in maps))


def top2_gap(logits):
    """Per pixel of NCHW logits: the best class's logit minus the second best."""
    top = logits.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def decidable(avg64, bound):
    """The pixels whose fp64 argmax an implementation within `bound` (absolute) of avg64 must reproduce."""
    return top2_gap(avg64) > 2 * bound


# ---- the network (ResNetLW: the torchvision-layout bottleneck ResNet + the light-weight RefineNet head) ------------------------

def _conv(x, sd, key, pad=0):
    b = sd.get(f"{key}.bias")
    return F.conv2d(x, sd[f"{key}.weight"].to(x.dtype), None if b is None else b.to(x.dtype), padding=pad)


def _crp(x, sd, g):
    top = x
    for i in range(1, 5):
        top = _conv(maxpool5(top), sd, f"mflow_conv_g{g}_pool.0.{i}_outvar_dimred")
        x = top + x
    return x


def refinenet(x, sd, depths, dtype=torch.float64):
    """x: the network's NCHW input (already preprocessed), sd: a ResNetLW state dict -> logits [N, classes, H/4, W/4] of dtype."""
    x = x.to(dtype)
    x = F.max_pool2d(F.relu(_conv_bn(x, sd, "conv1", "bn1", 2, 3)), kernel_size=3, stride=2, padding=1)
    feats = []
    for li, depth in enumerate(depths, 1):
        for bi in range(depth):
            p = f"layer{li}.{bi}"
            stride = 2 if (li > 1 and bi == 0) else 1
            identity = x
            out = F.relu(_conv_bn(x, sd, f"{p}.conv1", f"{p}.bn1"))
            out = F.relu(_conv_bn(out, sd, f"{p}.conv2", f"{p}.bn2", stride, 1))
            out = _conv_bn(out, sd, f"{p}.conv3", f"{p}.bn3")
            if f"{p}.downsample.0.weight" in sd:
                identity = _conv_bn(x, sd, f"{p}.downsample.0", f"{p}.downsample.1", stride, 0)
            x = F.relu(out + identity)
        feats.append(x)
    l1, l2, l3, l4 = feats
    y = _crp(F.relu(_conv(l4, sd, "p_ims1d2_outl1_dimred")), sd, 1)
    for g, skip in ((2, l3), (3, l2), (4, l1)):
        y = resize_ac(_conv(y, sd, f"mflow_conv_g{g - 1}_b3_joint_varout_dimred"), skip.shape[2:], dtype)
        s = _conv(_conv(skip, sd, f"p_ims1d2_outl{g}_dimred"), sd, f"adapt_stage{g}_b2_joint_varout_dimred")
        y = _crp(F.relu(s + y), sd, g)
    return _conv(y, sd, "clf_conv", pad=1)


def depths(arch):
    from unirestore_amd import segment
    return segment.depths_of(arch)


@functools.lru_cache(maxsize=None)
def state_dict(arch, seed, classes=19):
    """The seeded stand-in weights of a case (host only; callers must not modify them)."""
    from unirestore_amd import segment
    return segment.random_state_dict(arch, seed, classes)


def net_images(name):
    _arch, _wseed, iseed, n, h, w = NET_CASES[name]
    return varied_images(n, h, w, iseed)


def tta_logits(x, sd, depths_, size=None, scales=SCALES, dtype=torch.float64):
    """The metric's logits: for every scale resize, run the network, resize the logits to `size`; then the mean."""
    h, w = x.shape[2:]
    maps = [refinenet(prep(x, scaled_hw(h, w, s), dtype), sd, depths_, dtype) for s in scales]
    return tta_average(maps, (h, w) if size is None else size, dtype)


@functools.lru_cache(maxsize=None)
def net_reference(name):
    """(fp64 scale-1 logits, fp64 three-scale averaged logits) of a NET_CASES entry (once per process; do not modify)."""
    arch, wseed = NET_CASES[name][:2]
    x, sd = net_images(name), state_dict(arch, wseed)
    return refinenet(preprocess(x), sd, depths(arch)), tta_logits(x, sd, depths(arch))


def measure_logits(name):
    """(scale-1, three-scale) max |fp32 - fp64| / max |fp64|, the fp32 run resizing with the fp32-rounded fp64 matrices."""
    arch, wseed = NET_CASES[name][:2]
    x, sd, d = net_images(name), state_dict(arch, wseed), depths(arch)
    want1, want3 = net_reference(name)
    got1 = refinenet(preprocess(x, torch.float32), sd, d, torch.float32).double()
    h, w = x.shape[2:]
    maps = [refinenet(prep_einsum32(x, scaled_hw(h, w, s)), sd, d, torch.float32) for s in SCALES]
    got3 = tta_average_einsum32(maps, (h, w)).double()
    return float((got1 - want1).abs().max() / want1.abs().max()), float((got3 - want3).abs().max() / want3.abs().max())


# ---- confusion matrix and mIoU ------------------------------------------------------------------------------------------------

CITYSCAPES_TRAIN_ID = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13, 27: 14, 28: 15,
                       31: 16, 32: 17, 33: 18}      # the public labelId -> trainId table (cityscapesScripts labels.py); the rest is 255


def confusion(pred, target, classes=19, ignore_index=255):
    """int64 [classes, classes], conf[target][pred], by numpy bincount over the pixels with a target in [0, classes)."""
    import numpy as np
    pred, target = np.asarray(pred, dtype=np.int64).reshape(-1), np.asarray(target, dtype=np.int64).reshape(-1)
    keep = (target >= 0) & (target < classes) & (target != ignore_index)
    return np.bincount(classes * target[keep] + pred[keep], minlength=classes * classes).reshape(classes, classes)


def miou(conf):
    """(mIoU, pixel accuracy) written out class by class in Python numbers."""
    conf = [[int(v) for v in row] for row in conf]
    c = len(conf)
    ious = []
    for k in range(c):
        den = sum(conf[k]) + sum(conf[j][k] for j in range(c)) - conf[k][k]
        if den > 0:
            ious.append(conf[k][k] / den)
    total = sum(sum(row) for row in conf)
    return (sum(ious) / len(ious) if ious else 0.0), (sum(conf[k][k] for k in range(c)) / total if total else 0.0)


def miou_hist(conf):
    """The reference's own `mIoU.compute`: nanmean of diag / (rows + cols - diag) on a float histogram."""
    hist = torch.as_tensor(conf).float()
    diag = torch.diag(hist)
    return float(torch.nanmean(diag / (hist.sum(dim=1) + hist.sum(dim=0) - diag)))
