"""Host restatement of the classifier scoring (evaluator preprocess, torchvision-layout ResNet-18 / 50 / 101, top-1, accuracy) and
of each of its stages, in plain torch on the CPU, written from the torchvision architecture: BatchNorm stays UNFUSED (conv2d, then
batch_norm), the preprocess is torch's own `interpolate(antialias=True)`.  dtype=torch.float64 is the yardstick; torch.float32 is
what an fp32 host evaluation of the same restatement computes - its distance from fp64 is the source of every GPU tolerance.
Tensors are NCHW here; the HIP kernels keep NHWC - `nhwc` / `nchw` convert.  The weights are seeded stand-ins: nothing here says
anything about published accuracies."""
import functools
import math

import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)                 # IMAGENET_DEFAULT_MEAN / STD
STD = (0.229, 0.224, 0.225)
BLOCKS = {"resnet18": ("basic", (2, 2, 2, 2)), "resnet50": ("bottleneck", (3, 4, 6, 3)), "resnet101": ("bottleneck", (3, 4, 23, 3))}
GPU_FACTOR = 8                               # the rule of lpips_reference.py: a GPU bound is 8 x fp32's own measured error

# ---- the cases ----------------------------------------------------------------------------------------------------------------
PREP_CASES = ((2, 3, 300, 517), (1, 3, 96, 80), (2, 3, 160, 512), (1, 3, 224, 224), (1, 3, 7, 1000), (1, 3, 960, 1664), (1, 3, 1, 1))
# name -> (N, H, W, Cin, Cout, k, stride, pad, residual, relu)
CONV_CASES = {
    "1x1_64_256_res_relu": (2, 9, 7, 64, 256, 1, 1, 0, True, True),            # M = 126: one partial block
    "1x1_64_256_res_no_relu": (2, 9, 7, 64, 256, 1, 1, 0, True, False),
    "1x1_s2_256_512": (2, 9, 7, 256, 512, 1, 2, 0, False, False),               # the downsample path: 9x7 -> 5x4
    "3x3_s2_128_128": (2, 9, 7, 128, 128, 3, 2, 1, False, True),
    "3x3_64_64_res": (2, 9, 7, 64, 64, 3, 1, 1, True, True),                    # BasicBlock's second convolution
    "7x7_s2_3_64": (1, 33, 47, 3, 64, 7, 2, 3, False, True),                    # the stem: Cin = 3, the scalar gather
    "fc_2048_1000": (3, 1, 1, 2048, 1000, 1, 1, 0, False, False),               # Cout tail, M = 3 < 32
}
AVGPOOL_CASES = ((2, 512, 1, 1), (2, 512, 2, 2), (2, 512, 7, 7), (1, 2048, 1, 1), (3, 2048, 2, 2), (2, 2048, 7, 7))
# name -> (arch, classes, weight seed, image seed, N, H, W): `logits` on an already-preprocessed input
NET_CASES = {
    "resnet50_4x64x64": ("resnet50", 1000, 1, 1, 4, 64, 64),
    "resnet50_3x33x47": ("resnet50", 1000, 1, 2, 3, 33, 47),                    # odd maps, the final map is 2 x 2
    "resnet18_200_2x64x64": ("resnet18", 200, 7, 3, 2, 64, 64),
    "resnet101_2x32x32": ("resnet101", 1000, 9, 4, 2, 32, 32),                  # the final map is 1 x 1
}
FORWARD_CASE = ("resnet50", 1000, 1, 6, (3, 3, 75, 101))                       # arch, classes, weight seed, image seed, image shape

# ---- the tolerances: fp32's OWN error against fp64 on these cases, measured with the restatement below on the CPU (measure_*;
# torch 2.x CPU kernels), and GPU_FACTOR x that for the GPU - the factor allows for the different summation order of an MFMA K loop
# against a blocked CPU convolution, both being single-rounding fp32 sums.
# preprocess: max |einsum32 - fp64| over the cases, absolute; einsum32 = the resize as two fp32 matrix products with the fp32-
# rounded fp64 resize matrices, then the fp32 normalisation - NOT torch's own fp32 interpolate, which builds its weights in fp32 and
# is further from fp64 (TORCH32_PREP, per case); the kernel must be no further from fp64 than that either.
E32_PREP = 7.75e-07
TORCH32_PREP = {(2, 3, 300, 517): 4.80e-05, (1, 3, 96, 80): 3.11e-05, (2, 3, 160, 512): 5.24e-05, (1, 3, 224, 224): 3.44e-07,
                (1, 3, 7, 1000): 2.94e-05, (1, 3, 960, 1664): 1.50e-05, (1, 3, 1, 1): 3.44e-07}      # (rounded up)
# convolutions: per case, max over outputs of |conv32 - conv64| / (sum |a b| + |bias| + |res|)
E32_CONV = {"1x1_64_256_res_relu": 1.76e-07, "1x1_64_256_res_no_relu": 2.26e-07, "1x1_s2_256_512": 1.07e-07, "3x3_s2_128_128": 4.56e-08,
            "3x3_64_64_res": 7.18e-08, "7x7_s2_3_64": 1.97e-07, "fc_2048_1000": 4.36e-08}
E32_AVGPOOL = 2.03e-07                       # max over the cases of |mean32 - mean64| / mean |x|
# per NET_CASES entry, max |logits32 - logits64| / max |logits64| (the stand-in logits reach |max| 14 .. 540)
E32_LOGITS = {"resnet50_4x64x64": 4.06e-07, "resnet50_3x33x47": 3.82e-07, "resnet18_200_2x64x64": 3.10e-07, "resnet101_2x32x32": 8.28e-07}
E32_FORWARD = 2.71e-07                       # the same for FORWARD_CASE (preprocess + network; |max| 196)
# Measured on an MI355X against fp64 (test_classify_gpu.py and test_f32net_gpu.py print each figure): preprocess 6.5e-07 .. 7.2e-07 on the resizing cases,
# 3.43e-07 on the identity resize (torch's own figure), 1.2e-07 at 1 x 1; convolutions 4.2e-08 (FC) .. 2.3e-07; average pool up to
# 5.9e-08; logits 3.9e-07, 5.1e-07, 4.0e-07, 7.0e-07 of max |logit| on the four NET_CASES; forward 2.8e-07.
PREP_TOL = GPU_FACTOR * E32_PREP
CONV_TOL = {k: GPU_FACTOR * v for k, v in E32_CONV.items()}
AVGPOOL_TOL = GPU_FACTOR * E32_AVGPOOL
LOGITS_TOL = {k: GPU_FACTOR * v for k, v in E32_LOGITS.items()}      # also absorbs the fp32 rounding of the folded weights
FORWARD_TOL = GPU_FACTOR * E32_FORWARD


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def quantise(x):
    return torch.round(x.clamp(0, 1) * 255) / 255


def images(shape, seed):
    """fp32 images on the 8-bit grid."""
    return quantise(torch.rand(shape, generator=torch.Generator().manual_seed(seed)))


def varied_images(n, h, w, seed):
    """[n,3,h,w] fp32 on the 8-bit grid, varied strongly from image to image: every channel of every image sits near 0 or near
    0.85 (a colour cast), with noise of a random amplitude on top.  Networks with random weights are nearly blind to fine detail,
    so the images must differ in the large to be told apart."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        base = torch.rand(3, h, w, generator=g)
        level = (torch.rand(3, 1, 1, generator=g) > 0.5).float() * 0.8 + 0.1 * torch.rand(3, 1, 1, generator=g)
        amp = 0.05 + 0.25 * torch.rand(1, generator=g)
        out.append(level + amp * (base - 0.5))
    return quantise(torch.stack(out))


# ---- preprocess ---------------------------------------------------------------------------------------------------------------

def normalise(x, dtype=torch.float64):
    mean = torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    return (x.to(dtype) - mean) / std


def preprocess(x, dtype=torch.float64, size=224):
    """[N,3,H,W] in [0,1] -> [N,3,224,224]: T.Resize((224, 224)) on a tensor (bilinear, antialias) and the ImageNet Normalize."""
    y = F.interpolate(x.to(dtype), size=(size, size), mode="bilinear", antialias=True, align_corners=False)
    return normalise(y, dtype)


@functools.lru_cache(maxsize=None)
def resize_matrix(n_in, n_out=224):
    """[n_out, n_in] fp64: torch's antialiased bilinear resize of one axis as a matrix, read off torch itself by resizing the
    identity (the other axis has size 1 and stays)."""
    eye = torch.eye(n_in, dtype=torch.float64).view(1, n_in, 1, n_in)
    return F.interpolate(eye, size=(1, n_out), mode="bilinear", antialias=True, align_corners=False)[0, :, 0, :].t().contiguous()


def preprocess_einsum32(x, size=224):
    """The preprocess as fp32 arithmetic on the fp32-rounded resize matrices, the W axis first: what a table-driven fp32
    implementation computes, up to its summation order."""
    ah, aw = resize_matrix(x.shape[2], size).float(), resize_matrix(x.shape[3], size).float()
    t = torch.einsum("nchw,xw->nchx", x.float(), aw)
    return normalise(torch.einsum("nchx,yh->ncyx", t, ah), torch.float32)


def measure_prep(shape, seed=0):
    """(einsum32's, torch fp32 interpolate's) max |error| against fp64 on one case."""
    x = images(shape, seed + sum(shape))
    want = preprocess(x)
    return float((preprocess_einsum32(x).double() - want).abs().max()), float((preprocess(x, torch.float32).double() - want).abs().max())


# ---- the layers ---------------------------------------------------------------------------------------------------------------

def conv(x, w, b, stride, pad, res=None, relu=True, dtype=torch.float64):
    """act(conv(x) + bias + res)."""
    y = F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), stride=stride, padding=pad)
    if res is not None:
        y = y + res.to(dtype)
    return F.relu(y) if relu else y


def conv_abs(x, w, b, stride, pad, res=None):
    """sum |a b| + |bias| + |res| of every output element, fp64: the scale its rounding errors are proportional to."""
    y = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=stride, padding=pad)
    return y if res is None else y + res.double().abs()


def conv_case(name):
    """(x [N,Cin,H,W], w, bias, res or None) of a CONV_CASES entry: post-ReLU activations (raw for the stem), Kaiming filter."""
    n, h, w_, cin, cout, k, stride, pad, has_res, _relu = CONV_CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CONV_CASES).index(name))
    x = torch.randn(n, cin, h, w_, generator=g)
    if cin != 3:
        x = F.relu(x)
    wt = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
    b = 0.1 * torch.randn(cout, generator=g)
    oh, ow = (h + 2 * pad - k) // stride + 1, (w_ + 2 * pad - k) // stride + 1
    res = torch.randn(n, cout, oh, ow, generator=g) if has_res else None
    return x, wt, b, res


def measure_conv(name):
    n, h, w_, cin, cout, k, stride, pad, _has_res, relu = CONV_CASES[name]
    x, wt, b, res = conv_case(name)
    y32 = conv(x, wt, b, stride, pad, res, relu, torch.float32).double()
    return float(((y32 - conv(x, wt, b, stride, pad, res, relu)).abs() / conv_abs(x, wt, b, stride, pad, res)).max())


def maxpool(x):
    return F.max_pool2d(x, kernel_size=3, stride=2, padding=1)


def avgpool(x, dtype=torch.float64):
    """[N,C,H,W] -> [N,C]."""
    return x.to(dtype).mean(dim=(2, 3))


def avgpool_case(shape):
    return F.relu(torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))) + 0.01


def measure_avgpool(shape):
    x = avgpool_case(shape)
    return float(((avgpool(x, torch.float32).double() - avgpool(x)).abs() / x.double().abs().mean(dim=(2, 3))).max())


# ---- the network (torchvision.models.resnet: BasicBlock / Bottleneck, the stride on the 3x3, v1.5) ----------------------------

def _bn(x, sd, key):
    return F.batch_norm(x, sd[f"{key}.running_mean"].to(x.dtype), sd[f"{key}.running_var"].to(x.dtype), sd[f"{key}.weight"].to(x.dtype),
                        sd[f"{key}.bias"].to(x.dtype), training=False, eps=1e-5)


def _conv_bn(x, sd, ckey, bkey, stride=1, pad=0):
    return _bn(F.conv2d(x, sd[f"{ckey}.weight"].to(x.dtype), None, stride=stride, padding=pad), sd, bkey)


def resnet(x, sd, arch, dtype=torch.float64):
    """x: the network's NCHW input (already preprocessed), sd: a torchvision state dict -> logits [N, classes] of dtype."""
    kind, depths = BLOCKS[arch]
    x = x.to(dtype)
    x = F.max_pool2d(F.relu(_conv_bn(x, sd, "conv1", "bn1", 2, 3)), kernel_size=3, stride=2, padding=1)
    for li, depth in enumerate(depths, 1):
        for bi in range(depth):
            p = f"layer{li}.{bi}"
            stride = 2 if (li > 1 and bi == 0) else 1
            identity = x
            if kind == "basic":
                out = F.relu(_conv_bn(x, sd, f"{p}.conv1", f"{p}.bn1", stride, 1))
                out = _conv_bn(out, sd, f"{p}.conv2", f"{p}.bn2", 1, 1)
            else:
                out = F.relu(_conv_bn(x, sd, f"{p}.conv1", f"{p}.bn1"))
                out = F.relu(_conv_bn(out, sd, f"{p}.conv2", f"{p}.bn2", stride, 1))
                out = _conv_bn(out, sd, f"{p}.conv3", f"{p}.bn3")
            if f"{p}.downsample.0.weight" in sd:
                identity = _conv_bn(x, sd, f"{p}.downsample.0", f"{p}.downsample.1", stride, 0)
            x = F.relu(out + identity)
    x = x.mean(dim=(2, 3))
    return F.linear(x, sd["fc.weight"].to(dtype), sd["fc.bias"].to(dtype))


@functools.lru_cache(maxsize=None)
def state_dict(arch, seed, classes):
    """The seeded stand-in weights of a case (host only; callers must not modify them)."""
    from unirestore_amd import classify
    return classify.random_state_dict(arch, seed, classes)


def net_input(name):
    """The already-preprocessed NCHW fp32 input of a NET_CASES entry: varied images, normalised (no resize)."""
    _arch, _classes, _wseed, iseed, n, h, w = NET_CASES[name]
    return normalise(varied_images(n, h, w, iseed), torch.float32)


@functools.lru_cache(maxsize=None)
def net_reference(name):
    """fp64 logits of a NET_CASES entry (computed once per process; callers must not modify them)."""
    arch, classes, wseed = NET_CASES[name][:3]
    return resnet(net_input(name), state_dict(arch, wseed, classes), arch)


def measure_logits(name):
    arch, classes, wseed = NET_CASES[name][:3]
    want = net_reference(name)
    got = resnet(net_input(name), state_dict(arch, wseed, classes), arch, torch.float32).double()
    return float((got - want).abs().max() / want.abs().max())


def forward_images():
    return varied_images(FORWARD_CASE[4][0], FORWARD_CASE[4][2], FORWARD_CASE[4][3], FORWARD_CASE[3])


@functools.lru_cache(maxsize=None)
def forward_reference():
    arch, classes, wseed = FORWARD_CASE[:3]
    return resnet(preprocess(forward_images()), state_dict(arch, wseed, classes), arch)


def measure_forward():
    arch, classes, wseed = FORWARD_CASE[:3]
    want = forward_reference()
    got = resnet(preprocess_einsum32(forward_images()), state_dict(arch, wseed, classes), arch, torch.float32).double()
    return float((got - want).abs().max() / want.abs().max())


def top2_gap(logits):
    """Per image: the best logit minus the second best."""
    top = logits.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


# ---- accuracy -----------------------------------------------------------------------------------------------------------------

def counts(pred, labels, classes):
    """(tp, targets, predicted) int64 [classes] by numpy bincount."""
    import numpy as np
    pred, labels = np.asarray(pred, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    return (np.bincount(labels[pred == labels], minlength=classes), np.bincount(labels, minlength=classes),
            np.bincount(pred, minlength=classes))


def accuracy(tp, targets, predicted):
    """(macro, micro) written out class by class in Python floats: macro = the mean of tp_c / targets_c (0 without targets) over
    the classes that appear as a target or a prediction; micro = sum tp / sum targets."""
    per_class = []
    for t, g, p in zip((int(v) for v in tp), (int(v) for v in targets), (int(v) for v in predicted)):
        if g + p > 0:
            per_class.append(t / g if g > 0 else 0.0)
    total = sum(int(v) for v in targets)
    return (sum(per_class) / len(per_class) if per_class else 0.0), (sum(int(v) for v in tp) / total if total else 0.0)
