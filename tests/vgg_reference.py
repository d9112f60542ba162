"""Host restatement of the VGG scoring (torchvision.models.vgg: `features` of 3 x 3 convolutions, optional BatchNorm, ReLU and
2 x 2 max-pools, AdaptiveAvgPool2d((7, 7)), flatten, three Linears with ReLU between them; Dropout is the identity in eval) and of
the three kernels of csrc/vgg.hip, built from torch's own operators on the CPU and nothing of the project's: F.conv2d, F.batch_norm,
F.relu, F.max_pool2d(2, 2), F.adaptive_avg_pool2d, torch.flatten, F.linear.  It is written NCHW as torchvision writes it, with an
explicit BatchNorm after each convolution and the NCHW flatten, and it reads the SAME state dict the GPU weights are built from - so
it shares nothing with the loader's fold, its column permutation of classifier.0 or the kernels' index arithmetic.
dtype=torch.float64 is the yardstick.  The source of every GPU tolerance is the distance from fp64 of an fp32 evaluation that IEEE
arithmetic alone defines (the `*32` functions below: separately rounded fp32 multiplications and additions in a stated order; in
the convolutions exact blocks of 72 products added to an fp32 accumulator) - NOT of torch's own fp32 operators, whose summation order is the BLAS / oneDNN
kernel's that the CPU at hand selects: between two x86 machines with different vector extensions F.linear's error on these very cases
differed by up to 2.1 x, more than the 4 .. 16 window test_vgg_cpu.py holds the constants to can take.
The weights are seeded stand-ins (vgg.random_state_dict): nothing here says anything about published accuracies.  torchvision is not installed where this was written: the layer order is its source's as
recalled."""
import functools

import torch
import torch.nn.functional as F

import classify_reference as CR

GPU_FACTOR = 8                               # the rule of classify_reference.py: a GPU bound is 8 x fp32's own measured error
BN_EPS = 1e-5

# ---- the cases ----------------------------------------------------------------------------------------------------------------
# The Linear: (K, N) - shorter than one split of 512 (7, 392), no multiple of the 64-k step, the 32-column wave tile or the
# 128-column workgroup tile (7, 1000 / 5, 10, 200, 1000), two to eight splits (1000, 4096), and classifier.0's own 49 splits on a
# 6.4 MB matrix (25088 x 64).  Every case has LIN_ROWS rows; a test with M rows takes the first M (a row's result depends on that
# row alone, in the restatement as in the kernel), M over one row, one row short of a tile, a tile, one row more, and three tiles.
LIN_SHAPES = ((7, 5), (392, 10), (1000, 200), (4096, 1000), (25088, 64))
LIN_MS = (1, 31, 32, 33, 65)
LIN_ROWS = 65
LIN_CASES = {f"K{k}_N{n}{'_relu' if relu else ''}": (k, n, relu) for k, n in LIN_SHAPES for relu in (False, True)}
LIN_REAL = (3, 25088, 4096)                  # (M, K, N): classifier.0 at its real size, once
# The max-pool: (N, H, W, C) - float4 path, odd edges dropped, the scalar path (C = 5), an odd map on the float4 path
POOL_CASES = ((2, 6, 6, 64), (1, 7, 5, 8), (1, 2, 2, 5), (1, 3, 3, 4))
# The adaptive average pool: (N, H, W, C) - maps smaller than the output (1 x 1, 2 x 2), the identity (7 x 7), overlapping windows of
# unequal sizes (10 x 13, 15 x 8); C = 64 and C = 5
AVG_CASES = tuple((2, h, w, c) for h, w in ((1, 1), (2, 2), (7, 7), (10, 13), (15, 8)) for c in (64, 5))
# name -> (arch, hidden, classes, weight seed, image seed, (N, H, W))
NET_CASES = {"vgg11_32": ("vgg11", 64, 10, 71, 72, (3, 32, 32)),                  # the final map is 1 x 1, replicated to 7 x 7
             "vgg16_bn_75x101": ("vgg16_bn", 96, 200, 73, 74, (2, 75, 101)),      # odd maps at every pool; the BatchNorm fold
             "vgg19_64": ("vgg19", 64, 10, 75, 76, (2, 64, 64))}
SMALL = "vgg11_32"                           # the network of the tests that need no particular one
FULL = ("vgg16", 4096, 1000, 77)             # arch, hidden, classes, weight seed: torchvision's own sizes, 138 M parameters
FORWARD_SHAPE = (2, 3, 75, 101)              # ops.vgg end to end with FULL: 8-bit images, resized to 224 x 224
PROPERTY_SHAPE = (4, 3, 40, 52)              # the images of the batch-place, determinism and NaN tests (SMALL behind the preprocess)
CALLER_ARCH = "vgg11"

# ---- the tolerances: fp32's OWN error against fp64 on these cases, measured on the CPU with the IEEE-defined fp32 evaluations
# below (measure_*: the same figures on every machine), and GPU_FACTOR x that for the GPU.
# the Linear: per case, max over the 65 x N outputs of |linear32 - linear64| / (sum |a b| + |bias|)
E32_LIN = {"K7_N5": 9.12e-08, "K7_N5_relu": 9.12e-08, "K392_N10": 1.17e-07, "K392_N10_relu": 1.17e-07, "K1000_N200": 1.99e-07,
           "K1000_N200_relu": 1.99e-07, "K4096_N1000": 2.32e-07, "K4096_N1000_relu": 2.32e-07, "K25088_N64": 1.69e-07,
           "K25088_N64_relu": 1.69e-07}
E32_LIN_REAL = 1.58e-07
# the average pool: per case, max |avgpool7_32 - pool64| / max |pool64| (0: a window of one value is exact)
E32_AVG = {"2x1x1x64": 0.0, "2x1x1x5": 0.0, "2x2x2x64": 3.94e-08, "2x2x2x5": 2.42e-08, "2x7x7x64": 0.0, "2x7x7x5": 0.0,
           "2x10x13x64": 9.34e-08, "2x10x13x5": 9.90e-08, "2x15x8x64": 1.02e-07, "2x15x8x5": 9.50e-08}
# per NET_CASES entry, max |vgg32 - logits64| / max |logits64| (the stand-in logits reach |max| 0.24 .. 3.7)
E32_LOGITS = {"vgg11_32": 4.14e-06, "vgg16_bn_75x101": 1.78e-06, "vgg19_64": 1.60e-06}
# the same for FULL behind preprocess32 on FORWARD_SHAPE (|max| 0.74)
E32_FORWARD = 2.26e-06
# Measured on an MI355X against fp64 (test_vgg_gpu.py prints each figure): the Linear 7.7e-09 .. 1.05e-07 over the cases and row
# counts, 1.1e-08 at the real size; the average pool 0 on the exact cases, 2.0e-08 .. 4.2e-08 on the others; logits 1.35e-06,
# 6.8e-07 and 5.4e-07 of max |logit| on the three NET_CASES; forward 7.0e-07.
LIN_TOL = {k: GPU_FACTOR * v for k, v in E32_LIN.items()}
LIN_REAL_TOL = GPU_FACTOR * E32_LIN_REAL
AVG_TOL = {k: GPU_FACTOR * v for k, v in E32_AVG.items()}
LOGITS_TOL = {k: GPU_FACTOR * v for k, v in E32_LOGITS.items()}
FORWARD_TOL = GPU_FACTOR * E32_FORWARD


def _gen(*key):
    """A generator seeded by a tuple of integers."""
    seed = 0
    for k in key:
        seed = (seed * 1000003 + k + 1) % ((1 << 31) - 1)
    return torch.Generator().manual_seed(seed)


def rel_err(got, want):
    """max |got - want| / max |want| in fp64 (0 / 0 = 0: a case whose result is all zeros)."""
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    return err / scale if scale > 0 else err


top2_gap = CR.top2_gap


# ---- the Linear -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lin_case(k, n):
    """(x [65, K], w [N, K], bias [N]) fp32 of a LIN_SHAPES entry (callers must not modify them): post-ReLU activations, every row at a scale of
    its own, a uniform +-1/sqrt(K) matrix, a bias of the outputs' size."""
    g = _gen(81, k, n)
    x = F.relu(torch.randn(LIN_ROWS, k, generator=g)) * (0.5 + torch.rand(LIN_ROWS, 1, generator=g))
    w = (2 * torch.rand(n, k, generator=g) - 1) / k ** 0.5
    return x, w, 0.3 * torch.randn(n, generator=g)


def linear(x, w, b, relu, dtype=torch.float64):
    y = F.linear(x.to(dtype), w.to(dtype), b.to(dtype))
    return F.relu(y) if relu else y


def linear_abs(x, w, b):
    """sum |a b| + |bias| of every output element, fp64: the scale its rounding errors are proportional to."""
    return F.linear(x.double().abs(), w.double().abs(), b.double().abs())


@functools.lru_cache(maxsize=None)
def lin_reference(name):
    """(fp64 result [65, N], fp64 scale [65, N]) of a LIN_CASES entry."""
    k, n, relu = LIN_CASES[name]
    x, w, b = lin_case(k, n)
    return linear(x, w, b, relu), linear_abs(x, w, b)


def linear32(x, w, b, relu):
    """The Linear in fp32 as IEEE arithmetic alone defines it: acc = 0, then for k ascending acc = fl(acc + fl(x_k w_k)) - two
    separately rounded elementwise operations, no fused multiply-add, no blocking - then fl(acc + bias).  The same bits on every
    machine, whatever its BLAS does."""
    x, wt = x.float(), w.float().t().contiguous()                 # [M, K], [K, N]
    acc = torch.zeros(x.shape[0], wt.shape[1], dtype=torch.float32)
    prod = torch.empty_like(acc)
    for k in range(x.shape[1]):
        torch.mul(x[:, k:k + 1], wt[k:k + 1], out=prod)
        acc.add_(prod)
    y = acc + b.float()
    return F.relu(y) if relu else y


def measure_lin(name):
    k, n, relu = LIN_CASES[name]
    want, scale = lin_reference(name)
    return float(((linear32(*lin_case(k, n), relu).double() - want).abs() / scale).max())


@functools.lru_cache(maxsize=None)
def lin_real_case():
    """(x [3, 25088], w [4096, 25088], bias) fp32 at classifier.0's real size."""
    m, k, n = LIN_REAL
    g = _gen(82)
    return F.relu(torch.randn(m, k, generator=g)), (2 * torch.rand(n, k, generator=g) - 1) / k ** 0.5, 0.3 * torch.randn(n, generator=g)


@functools.lru_cache(maxsize=None)
def lin_real_reference():
    """(fp64 result, fp64 scale) of the real-size case, by 512 output columns at a time (no fp64 copy of the 411 MB matrix)."""
    x, w, b = lin_real_case()
    outs, scales = [], []
    for n0 in range(0, w.shape[0], 512):
        outs.append(linear(x, w[n0:n0 + 512], b[n0:n0 + 512], True))
        scales.append(linear_abs(x, w[n0:n0 + 512], b[n0:n0 + 512]))
    return torch.cat(outs, dim=1), torch.cat(scales, dim=1)


def measure_lin_real():
    want, scale = lin_real_reference()
    return float(((linear32(*lin_real_case(), True).double() - want).abs() / scale).max())


# ---- the pools ----------------------------------------------------------------------------------------------------------------------

def pool_case(shape):
    """NCHW fp32 of a POOL_CASES entry (N, H, W, C)."""
    n, h, w, c = shape
    return torch.randn(n, c, h, w, generator=_gen(83, *shape))


def maxpool2(x):
    return F.max_pool2d(x, kernel_size=2, stride=2)


def avg_name(shape):
    return "x".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def avg_case(shape):
    """NCHW fp32 of an AVG_CASES entry (N, H, W, C): post-ReLU values."""
    n, h, w, c = shape
    return F.relu(torch.randn(n, c, h, w, generator=_gen(84, *shape))) + 0.01


def avgpool7(x, dtype=torch.float64):
    return F.adaptive_avg_pool2d(x.to(dtype), (7, 7))


def avgpool7_32(x):
    """The adaptive average pool in fp32 as IEEE arithmetic alone defines it: per output the window's values added one by one in
    row-major order from 0, then one division by the count."""
    x = x.float()
    n, c, h, w = x.shape
    out = torch.empty(n, c, 7, 7, dtype=torch.float32)
    for i in range(7):
        h0, h1 = i * h // 7, -(-(i + 1) * h // 7)
        for j in range(7):
            w0, w1 = j * w // 7, -(-(j + 1) * w // 7)
            acc = torch.zeros(n, c, dtype=torch.float32)
            for ih in range(h0, h1):
                for iw in range(w0, w1):
                    acc = acc + x[:, :, ih, iw]
            out[:, :, i, j] = acc / float((h1 - h0) * (w1 - w0))
    return out


def measure_avg(shape):
    x = avg_case(shape)
    return rel_err(avgpool7_32(x), avgpool7(x))


# ---- the network (torchvision.models.vgg.VGG.forward) -----------------------------------------------------------------------------

def vgg(x, sd, dtype=torch.float64):
    """x: the network's NCHW input (already preprocessed), sd: a state dict in torchvision's layout -> logits [N, classes].  The
    `features` Sequential is walked by index: a 4-d weight is a convolution (followed by a BatchNorm when the next index has
    running statistics, then a ReLU), an index without parameters after a ReLU is the max-pool."""
    x = x.to(dtype)
    p = lambda key: sd[key].to(dtype)                             # noqa: E731
    last = max(int(k.split(".")[1]) for k in sd if k.startswith("features."))
    i = 0
    while i <= last + 2:                                          # (+2: the ReLU and the max-pool after the last parameters)
        if f"features.{i}.weight" in sd and sd[f"features.{i}.weight"].ndim == 4:
            x = F.conv2d(x, p(f"features.{i}.weight"), p(f"features.{i}.bias"), padding=1)
            i += 1
            if f"features.{i}.running_mean" in sd:
                x = F.batch_norm(x, p(f"features.{i}.running_mean"), p(f"features.{i}.running_var"), p(f"features.{i}.weight"),
                                 p(f"features.{i}.bias"), False, 0.1, BN_EPS)
                i += 1
            x = F.relu(x)
            i += 1
        else:
            x = F.max_pool2d(x, kernel_size=2, stride=2)
            i += 1
    x = torch.flatten(F.adaptive_avg_pool2d(x, (7, 7)), 1)
    x = F.relu(F.linear(x, p("classifier.0.weight"), p("classifier.0.bias")))
    x = F.relu(F.linear(x, p("classifier.3.weight"), p("classifier.3.bias")))
    return F.linear(x, p("classifier.6.weight"), p("classifier.6.bias"))


CONV32_BLOCK = 8                             # input channels per exactly summed block of conv32


def conv32(x, w, b):
    """A 3 x 3 / pad 1 convolution with an fp32 accumulator, defined by IEEE rounding alone: the 72 products of CONV32_BLOCK input
    channels x 9 taps are summed exactly (an fp64 F.conv2d of fp32 operands: 53 bits hold them; the order of that sum moves the
    result by 1e-16, far below an fp32 rounding), and the blocks are added to the accumulator in ascending channel order, one fp32
    rounding each, from 0; then the bias, one more.  Exact blocks make its error a LOWER estimate of what an fp32 convolution with
    product-by-product sums has (K / 72 roundings per output, not K): bounds taken from it are the tighter ones."""
    acc = torch.zeros(x.shape[0], w.shape[0], x.shape[2], x.shape[3], dtype=torch.float32)
    for c in range(0, x.shape[1], CONV32_BLOCK):
        acc = (acc.double() + F.conv2d(x[:, c:c + CONV32_BLOCK].double(), w[:, c:c + CONV32_BLOCK].double(), padding=1)).float()
    return acc + b.float().view(1, -1, 1, 1)


def preprocess32(x, size=224):
    """The preprocess in fp32 as IEEE arithmetic alone defines it: the resize as two products with the fp32-rounded fp64 resize
    matrices, the W axis first, each a k-ordered sum of separately rounded products (CR.preprocess_einsum32 is the same products
    in the order the CPU's BLAS picks), then the fp32 normalisation."""
    ah, aw = CR.resize_matrix(x.shape[2], size).float(), CR.resize_matrix(x.shape[3], size).float()      # [size, n_in]
    x = x.float()
    t = torch.zeros(*x.shape[:3], size, dtype=torch.float32)
    for k in range(x.shape[3]):
        t = t + x[:, :, :, k:k + 1] * aw[:, k]
    y = torch.zeros(*x.shape[:2], size, size, dtype=torch.float32)
    for k in range(x.shape[2]):
        y = y + t[:, :, k:k + 1, :] * ah[:, k].view(size, 1)
    return CR.normalise(y, torch.float32)


def vgg32(x, sd):
    """`vgg` as an fp32 implementation computes it, every operator defined by IEEE rounding alone, so that the measured distance
    from fp64 is the same on every machine: conv32, the BatchNorm as separately rounded elementwise fp32 operations in
    F.batch_norm's order ((x - mean) / sqrt(var + eps) * gamma + beta), ReLU and max-pool (exact), avgpool7_32, linear32."""
    x = x.float()
    p = lambda key: sd[key].float()                               # noqa: E731
    v = lambda key: sd[key].float().view(1, -1, 1, 1)             # noqa: E731
    last = max(int(k.split(".")[1]) for k in sd if k.startswith("features."))
    i = 0
    while i <= last + 2:
        if f"features.{i}.weight" in sd and sd[f"features.{i}.weight"].ndim == 4:
            x = conv32(x, p(f"features.{i}.weight"), p(f"features.{i}.bias"))
            i += 1
            if f"features.{i}.running_mean" in sd:
                x = (x - v(f"features.{i}.running_mean")) / torch.sqrt(v(f"features.{i}.running_var") + BN_EPS) * v(f"features.{i}.weight") \
                    + v(f"features.{i}.bias")
                i += 1
            x = F.relu(x)
            i += 1
        else:
            x = F.max_pool2d(x, kernel_size=2, stride=2)
            i += 1
    x = torch.flatten(avgpool7_32(x), 1)
    x = linear32(x, p("classifier.0.weight"), p("classifier.0.bias"), True)
    x = linear32(x, p("classifier.3.weight"), p("classifier.3.bias"), True)
    return linear32(x, p("classifier.6.weight"), p("classifier.6.bias"), False)


@functools.lru_cache(maxsize=None)
def state_dict(arch, seed, classes, hidden):
    """The seeded stand-in weights of a case (host only, built once per process; callers must not modify them)."""
    from unirestore_amd import vgg as M
    return M.random_state_dict(arch, seed, classes, hidden)


def net_state_dict(name):
    arch, hidden, classes, wseed = NET_CASES[name][:4]
    return state_dict(arch, wseed, classes, hidden)


def net_input(name):
    """The already-preprocessed NCHW fp32 input of a NET_CASES entry: 8-bit images of the case's size, normalised."""
    n, h, w = NET_CASES[name][5]
    return CR.normalise(CR.varied_images(n, h, w, NET_CASES[name][4]), torch.float32)


@functools.lru_cache(maxsize=None)
def net_reference(name):
    """fp64 logits of a NET_CASES entry (computed once per process; callers must not modify them)."""
    return vgg(net_input(name), net_state_dict(name))


def measure_logits(name):
    return rel_err(vgg32(net_input(name), net_state_dict(name)), net_reference(name))


def full_state_dict():
    arch, hidden, classes, wseed = FULL
    return state_dict(arch, wseed, classes, hidden)


def forward_images():
    return CR.varied_images(FORWARD_SHAPE[0], FORWARD_SHAPE[2], FORWARD_SHAPE[3], 78)


@functools.lru_cache(maxsize=None)
def forward_reference():
    """fp64 logits of FULL on FORWARD_SHAPE's images: preprocess + network."""
    return vgg(CR.preprocess(forward_images()), full_state_dict())


def measure_forward():
    return rel_err(vgg32(preprocess32(forward_images()), full_state_dict()), forward_reference())


def property_images(seed=12):
    n, _c, h, w = PROPERTY_SHAPE
    return CR.varied_images(n, h, w, seed)
