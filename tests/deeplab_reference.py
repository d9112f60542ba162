"""Host restatement of the DeepLabV3+ scoring (three-scale test-time augmentation, ImageNet Normalize, dilated ResNet, ASPP,
decoder, the model's half-pixel resize, the evaluator's align_corners=True resize, average + argmax) and of each of its stages,
in plain torch on the CPU, written from the architecture: BatchNorm stays UNFUSED (conv2d, then batch_norm), the concats are
torch.cat, every resize is torch's own `interpolate`.  dtype=torch.float64 is the yardstick; torch.float32 is what an fp32 host
evaluation of the same restatement computes - its distance from fp64 is the source of every GPU tolerance (GPU_FACTOR x, the rule
of segment_reference.py).  Tensors are NCHW here; the HIP kernels keep NHWC.  The weights are seeded stand-ins: nothing here says
anything about any published mIoU."""
import functools
import math

import torch
import torch.nn.functional as F

from classify_reference import GPU_FACTOR, _conv_bn, images, nchw, nhwc, varied_images  # noqa: F401  (shared helpers, re-exported)
from segment_reference import (MAX_LEFT_OUT, MIN_CLASSES, ac_matrix, decidable, resize_ac, resize_ac_einsum32, scaled_hw,  # noqa: F401
                               top2_gap)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # R, G, B of the [0,1] image
SCALES = (1, 0.8, 0.6)
TINY = (1, 1, 1, 1)                          # the smallest bottleneck backbone: one block per stage
ASPP_DILATIONS = (6, 12, 18)

# ---- the cases ----------------------------------------------------------------------------------------------------------------
# name -> (N, H, W, Cin, Cout, k, stride, pad, dil, residual, relu)
CONV_CASES = {
    "d6_all_side_taps_outside": (2, 4, 6, 64, 256, 3, 1, 6, 6, False, True),      # every off-centre tap is padding
    "d18_horizontal_taps_only": (1, 5, 20, 64, 256, 3, 1, 18, 18, False, True),   # W = 20 > 18: live taps left and right only
    "d2_cout_tail": (1, 7, 7, 32, 48, 3, 1, 2, 2, False, True),
    "d2_scalar_k_tail": (2, 9, 11, 3, 19, 3, 1, 2, 2, False, False),              # Cin = 3: the scalar gather, K = 27
    "d3_stride2": (1, 13, 13, 20, 64, 3, 2, 3, 3, False, True),
    "1x1_m_tail_one_row": (1, 3, 43, 8, 64, 1, 1, 0, 1, False, False),            # M = 129: one row in the second block
    "d2_res_relu": (2, 6, 5, 64, 64, 3, 1, 2, 2, True, True),                     # layer4's conv2 shape with a residual
}
SLICE_CASE = (1, 6, 9, 256, 256, 3, 1, 2, 2)                                      # into channels 48..303 of a 304-channel buffer
# (image shape, scale)
PREP_CASES = (((1, 3, 27, 27), 0.6), ((2, 3, 64, 96), 0.8), ((1, 3, 97, 131), 0.6))
# (N, C, h, w, H, W): the half-pixel resize
UPSAMPLE_CASES = ((2, 48, 1, 1, 5, 5), (2, 19, 1, 1, 5, 5), (1, 48, 3, 4, 12, 16), (1, 19, 3, 4, 12, 16), (2, 48, 4, 5, 16, 20),
                  (2, 19, 4, 5, 16, 20), (1, 48, 5, 6, 9, 16), (1, 19, 5, 6, 9, 16))
# name -> (N, C, ((hq, wq), (hs, ws)) per map, (H, W))
TTA_CASES = {
    "three_19": (2, 19, (((16, 24), (64, 96)), ((13, 19), (51, 76)), ((10, 15), (38, 57))), (64, 96)),
    "two_19": (1, 19, (((16, 24), (64, 96)), ((10, 15), (38, 57))), (64, 96)),
    "one_19": (1, 19, (((16, 24), (64, 96)),), (33, 47)),
    "three_19_odd": (1, 19, (((25, 33), (97, 131)), ((20, 26), (77, 104)), ((15, 20), (58, 78))), (97, 131)),
    "three_5_to_1x1": (2, 5, (((4, 6), (16, 24)), ((3, 5), (12, 19)), ((3, 4), (9, 14))), (1, 1)),
}
# name -> (arch, weight seed, image seed, N, H, W): scale-1 classifier map, and the three-scale prediction
NET_CASES = {
    "tiny_2x64x96": (TINY, 3, 11, 2, 64, 96),
    "tiny_1x64x320": (TINY, 4, 13, 1, 64, 320),
    "dlv3pr50_1x64x96": ("dlv3pr50", 5, 12, 1, 64, 96),
}

# ---- the tolerances: fp32's OWN error against fp64 on these cases, measured with the restatement below on the CPU (measure_*;
# torch 2.x CPU kernels), and GPU_FACTOR x that for the GPU.  The resizes of the fp32 runs are fp32 arithmetic on the fp32-rounded
# fp64 interpolation matrices (what a table-driven fp32 kernel computes, up to its summation order) - NOT torch's own fp32
# interpolate, which builds its weights in fp32.
# max |y32 - y64| / (sum|a b| + |bias| + |res|) per CONV_CASES entry
E32_CONV = {"d6_all_side_taps_outside": 1.04e-07, "d18_horizontal_taps_only": 1.56e-07, "d2_cout_tail": 1.62e-07,
            "d2_scalar_k_tail": 1.74e-07, "d3_stride2": 1.19e-07, "1x1_m_tail_one_row": 1.55e-07, "d2_res_relu": 6.95e-08}
E32_SLICE = 6.11e-08                         # the same for SLICE_CASE
E32_PREP = 7.03e-07                          # max |prep32 - prep64| over the cases, absolute, on values up to 2.64
E32_UPSAMPLE = 7.74e-08                      # max |up32 - up64| / max |x| over the cases
E32_TTA = 8.70e-08                           # max |avg32 - avg64| / max |logit| over the cases
# per NET_CASES entry, max |q32 - q64| / max |q64| of the classifier's quarter-resolution map at scale 1 (|max| 25 .. 47)
E32_LOGITS = {"tiny_2x64x96": 7.01e-07, "tiny_1x64x320": 8.28e-07, "dlv3pr50_1x64x96": 1.33e-06}
# the same for the three-scale averaged logits at the image's size (what the argmax sees)
E32_TTA_LOGITS = {"tiny_2x64x96": 3.60e-07, "tiny_1x64x320": 5.45e-07, "dlv3pr50_1x64x96": 7.26e-07}
# Measured on an MI355X against fp64 (test_deeplab_gpu.py prints each figure): dilated convolutions 9.8e-08 .. 2.7e-07, the slice
# 6.4e-08; prep 4.9e-07 .. 7.0e-07; half-pixel up-sample 6.2e-08 .. 8.2e-08; two-stage averaged logits 8.3e-09 .. 8.7e-08 of max
# |logit|; scale-1 maps 8.3e-07, 9.1e-07 (depth (1, 1, 1, 1)) and 1.4e-06 (dlv3pr50) of max |logit|, three-scale logits 4.1e-07 ..
# 6.2e-07; at most 0.016 % of the pixels left out and no argmax flip on the others.
CONV_TOL = {k: GPU_FACTOR * v for k, v in E32_CONV.items()}
SLICE_TOL = GPU_FACTOR * E32_SLICE
PREP_TOL = GPU_FACTOR * E32_PREP
UPSAMPLE_TOL = GPU_FACTOR * E32_UPSAMPLE
TTA_TOL = GPU_FACTOR * E32_TTA
LOGITS_TOL = {k: GPU_FACTOR * v for k, v in E32_LOGITS.items()}      # also absorbs the fp32 rounding of the folded weights
TTA_LOGITS_TOL = {k: GPU_FACTOR * v for k, v in E32_TTA_LOGITS.items()}


# ---- the dilated convolution --------------------------------------------------------------------------------------------------

def conv(x, w, b, stride, pad, dil, res=None, relu=True, dtype=torch.float64):
    """act(conv(x) + bias + res)."""
    y = F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), stride=stride, padding=pad, dilation=dil)
    if res is not None:
        y = y + res.to(dtype)
    return F.relu(y) if relu else y


def conv_abs(x, w, b, stride, pad, dil, res=None):
    """sum |a b| + |bias| + |res| of every output element, fp64: the scale its rounding errors are proportional to."""
    y = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=stride, padding=pad, dilation=dil)
    return y if res is None else y + res.double().abs()


def _conv_tensors(geometry, has_res, seed):
    n, h, w_, cin, cout, k, stride, pad, dil = geometry
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w_, generator=g)
    if cin != 3:
        x = F.relu(x)
    wt = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
    b = 0.1 * torch.randn(cout, generator=g)
    oh, ow = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w_ + 2 * pad - dil * (k - 1) - 1) // stride + 1
    res = torch.randn(n, cout, oh, ow, generator=g) if has_res else None
    return x, wt, b, res


def conv_case(name):
    """(x [N,Cin,H,W], w, bias, res or None) of a CONV_CASES entry: post-ReLU activations (raw for Cin = 3), Kaiming filter."""
    return _conv_tensors(CONV_CASES[name][:9], CONV_CASES[name][9], 2000 + sorted(CONV_CASES).index(name))


def slice_case():
    return _conv_tensors(SLICE_CASE, False, 2100)[:3]


def measure_conv(name):
    stride, pad, dil, _has_res, relu = CONV_CASES[name][6:]
    x, wt, b, res = conv_case(name)
    y32 = conv(x, wt, b, stride, pad, dil, res, relu, torch.float32).double()
    return float(((y32 - conv(x, wt, b, stride, pad, dil, res, relu)).abs() / conv_abs(x, wt, b, stride, pad, dil, res)).max())


def measure_slice():
    stride, pad, dil = SLICE_CASE[6:]
    x, wt, b = slice_case()
    y32 = conv(x, wt, b, stride, pad, dil, None, True, torch.float32).double()
    return float(((y32 - conv(x, wt, b, stride, pad, dil)).abs() / conv_abs(x, wt, b, stride, pad, dil)).max())


# ---- resizes ------------------------------------------------------------------------------------------------------------------

def resize_hp(x, size, dtype=torch.float64):
    return F.interpolate(x.to(dtype), size=tuple(size), mode="bilinear", align_corners=False)


@functools.lru_cache(maxsize=None)
def hp_matrix(n_in, n_out):
    """[n_out, n_in] fp64: torch's align_corners=False bilinear resize of one axis as a matrix, read off torch itself by resizing
    the identity (the other axis has size 1 and stays)."""
    eye = torch.eye(n_in, dtype=torch.float64).view(1, n_in, 1, n_in)
    return resize_hp(eye, (1, n_out))[0, :, 0, :].t().contiguous()


def table_matrix(idx, wt, n_in):
    """An (idx, wt) axis table as the [n_out, n_in] fp64 matrix the kernels apply: idx + 1 clamped to the axis."""
    m = torch.zeros(len(idx), n_in, dtype=torch.float64)
    for o, (i, (a, b)) in enumerate(zip(idx.tolist(), wt.tolist())):
        m[o, i] += a
        m[o, min(i + 1, n_in - 1)] += b
    return m


def resize_hp_einsum32(x, size):
    """The resize as fp32 arithmetic on the fp32-rounded fp64 matrices."""
    ah, aw = hp_matrix(x.shape[2], size[0]).float(), hp_matrix(x.shape[3], size[1]).float()
    return torch.einsum("nchx,yh->ncyx", torch.einsum("nchw,xw->nchx", x.float(), aw), ah)


def preprocess(x, dtype=torch.float64):
    """torchvision's Normalize on a [0,1] NCHW image: (x - mean) / std, channels stay R, G, B."""
    mean, std = (torch.tensor(v, dtype=dtype).view(1, 3, 1, 1) for v in (MEAN, STD))
    return (x.to(dtype) - mean) / std


def prep(x, size, dtype=torch.float64):
    """One scale: resize the [0,1] image (align_corners=True), then normalise."""
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
    return float((resize_hp_einsum32(x, case[4:]).double() - resize_hp(x, case[4:])).abs().max() / x.abs().max())


# ---- two-stage multi-scale average + argmax -----------------------------------------------------------------------------------

def tta_average(maps, in_sizes, size, dtype=torch.float64):
    """NCHW classifier maps -> each to its network input size (half-pixel, the model's resize), on to `size` (align_corners=True,
    the evaluator's), then the mean ((a + b) + c) / n."""
    total = None
    for m, s in zip(maps, in_sizes):
        up = resize_ac(resize_hp(m, s, dtype), size, dtype)
        total = up if total is None else total + up
    return total / len(maps)


def tta_average_einsum32(maps, in_sizes, size):
    total = None
    for m, s in zip(maps, in_sizes):
        up = resize_ac_einsum32(resize_hp_einsum32(m, s), size)
        total = up if total is None else total + up
    return total / torch.tensor(float(len(maps)), dtype=torch.float32)


def tta_case(name):
    n, c, sizes, _size = TTA_CASES[name]
    g = torch.Generator().manual_seed(sorted(TTA_CASES).index(name) + 70)
    return [3.0 * torch.randn(n, c, hq, wq, generator=g) for (hq, wq), _s in sizes]


def measure_tta(name):
    maps, in_sizes, size = tta_case(name), [s for _q, s in TTA_CASES[name][2]], TTA_CASES[name][3]
    want = tta_average(maps, in_sizes, size)
    return float((tta_average_einsum32(maps, in_sizes, size).double() - want).abs().max() / max(float(m.abs().max()) for m in maps))


# ---- the network (the torchvision-layout bottleneck ResNet, layer4 dilated, + DeepLabHeadV3Plus) --------------------------------

def _cbr(x, sd, ckey, bkey, pad=0, dil=1):
    w = sd[f"{ckey}.weight"].to(x.dtype)
    y = F.conv2d(x, w, None, padding=pad, dilation=dil)
    bn = [sd[f"{bkey}.{n}"].to(x.dtype) for n in ("running_mean", "running_var", "weight", "bias")]
    return F.relu(F.batch_norm(y, *bn, training=False, eps=1e-5))


def deeplab(x, sd, depths, dtype=torch.float64, resize=resize_hp):
    """x: the network's NCHW input (already normalised), sd: a DeepLabV3+ state dict -> the classifier's map [N, classes, H/4, W/4]
    of dtype (the model's output is `resize_hp` of it to x's size).  `resize`: the half-pixel resize to use."""
    x = x.to(dtype)
    b = "backbone"
    x = F.max_pool2d(F.relu(_conv_bn(x, sd, f"{b}.conv1", f"{b}.bn1", 2, 3)), kernel_size=3, stride=2, padding=1)
    feats = []
    for li, depth in enumerate(depths, 1):
        for bi in range(depth):
            p = f"{b}.layer{li}.{bi}"
            stride = 2 if (li in (2, 3) and bi == 0) else 1          # layer4: replace_stride_with_dilation
            dil = 2 if (li == 4 and bi > 0) else 1
            identity = x
            out = F.relu(_conv_bn(x, sd, f"{p}.conv1", f"{p}.bn1"))
            w2 = sd[f"{p}.conv2.weight"].to(dtype)
            out = F.conv2d(out, w2, None, stride=stride, padding=dil, dilation=dil)
            bn = [sd[f"{p}.bn2.{n}"].to(dtype) for n in ("running_mean", "running_var", "weight", "bias")]
            out = F.relu(F.batch_norm(out, *bn, training=False, eps=1e-5))
            out = _conv_bn(out, sd, f"{p}.conv3", f"{p}.bn3")
            if f"{p}.downsample.0.weight" in sd:
                identity = _conv_bn(x, sd, f"{p}.downsample.0", f"{p}.downsample.1", stride, 0)
            x = F.relu(out + identity)
        feats.append(x)
    low, out = feats[0], feats[3]
    c = "classifier"
    low = _cbr(low, sd, f"{c}.project.0", f"{c}.project.1")
    branches = [_cbr(out, sd, f"{c}.aspp.convs.0.0", f"{c}.aspp.convs.0.1")]
    branches += [_cbr(out, sd, f"{c}.aspp.convs.{i}.0", f"{c}.aspp.convs.{i}.1", d, d) for i, d in enumerate(ASPP_DILATIONS, 1)]
    pooled = _cbr(out.mean(dim=(2, 3), keepdim=True), sd, f"{c}.aspp.convs.4.1", f"{c}.aspp.convs.4.2")
    branches.append(pooled.expand(-1, -1, out.shape[2], out.shape[3]))      # the bilinear resize of a 1 x 1 map
    aspp = _cbr(torch.cat(branches, dim=1), sd, f"{c}.aspp.project.0", f"{c}.aspp.project.1")
    y = torch.cat([low, resize(aspp, low.shape[2:]).to(dtype)], dim=1)
    y = _cbr(y, sd, f"{c}.classifier.0", f"{c}.classifier.1", 1)
    return F.conv2d(y, sd[f"{c}.classifier.3.weight"].to(dtype), sd[f"{c}.classifier.3.bias"].to(dtype))


def depths(arch):
    from unirestore_amd import deeplab as dl
    return dl.depths_of(arch)


@functools.lru_cache(maxsize=None)
def state_dict(arch, seed, classes=19):
    """The seeded stand-in weights of a case (host only; callers must not modify them)."""
    from unirestore_amd import deeplab as dl
    return dl.random_state_dict(arch, seed, classes)


def net_images(name):
    _arch, _wseed, iseed, n, h, w = NET_CASES[name]
    return varied_images(n, h, w, iseed)


def tta_logits(x, sd, depths_, size=None, scales=SCALES, dtype=torch.float64):
    """The metric's logits: for every scale resize, run the network, its own resize to that input, the evaluator's to `size`; then
    the mean."""
    h, w = x.shape[2:]
    sizes = [scaled_hw(h, w, s) for s in scales]
    maps = [deeplab(prep(x, sz, dtype), sd, depths_, dtype) for sz in sizes]
    return tta_average(maps, sizes, (h, w) if size is None else size, dtype)


@functools.lru_cache(maxsize=None)
def net_reference(name):
    """(fp64 scale-1 classifier map, fp64 three-scale averaged logits) of a NET_CASES entry (once per process; do not modify)."""
    arch, wseed = NET_CASES[name][:2]
    x, sd = net_images(name), state_dict(arch, wseed)
    return deeplab(preprocess(x), sd, depths(arch)), tta_logits(x, sd, depths(arch))


def measure_logits(name):
    """(scale-1, three-scale) max |fp32 - fp64| / max |fp64|, the fp32 run resizing with the fp32-rounded fp64 matrices."""
    arch, wseed = NET_CASES[name][:2]
    x, sd, d = net_images(name), state_dict(arch, wseed), depths(arch)
    want1, want3 = net_reference(name)
    got1 = deeplab(preprocess(x, torch.float32), sd, d, torch.float32, resize_hp_einsum32).double()
    h, w = x.shape[2:]
    sizes = [scaled_hw(h, w, s) for s in SCALES]
    maps = [deeplab(prep_einsum32(x, sz), sd, d, torch.float32, resize_hp_einsum32) for sz in sizes]
    got3 = tta_average_einsum32(maps, sizes, (h, w)).double()
    return float((got1 - want1).abs().max() / want1.abs().max()), float((got3 - want3).abs().max() / want3.abs().max())
