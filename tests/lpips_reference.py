"""Host restatement of LPIPS (AlexNet, v0.1 linear layers, normalize=True) and of each of its stages, in torch on the CPU.
dtype=torch.float64 is the yardstick; dtype=torch.float32 is what the reference's own fp32 path computes (autocast off).
Tensors are NCHW here; the HIP kernels keep NHWC - `nhwc` / `nchw` convert.  Also the end-to-end cases and the functions that
measure fp32's own error against fp64 (the source of every GPU tolerance)."""
import functools

import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CONVS = ((64, 3, 11, 4, 2), (192, 64, 5, 1, 2), (384, 192, 3, 1, 1), (256, 384, 3, 1, 1), (256, 256, 3, 1, 1))   # Cout, Cin, k, stride, pad
POOL_BEFORE = (False, True, True, False, False)
WEIGHT_SEED = 11

# the end-to-end cases: shape -> seed
E2E_CASES = {(2, 3, 31, 31): 1, (3, 3, 33, 47): 2, (1, 3, 96, 80): 3, (2, 3, 64, 64): 4, (1, 3, 512, 512): 5}

# ---- the tolerances: fp32's OWN error against fp64, measured on the end-to-end cases with the host restatement below
# (measure_e32; torch 2.x CPU convolutions, WEIGHT_SEED 11), and 8 x that for the GPU - the factor allows for the different
# summation order of an MFMA K loop against a blocked CPU convolution, both being single-rounding fp32 sums.
#   case            metric e32   conv1..conv5 e32 / sum|a b|                              layer e32 / layer_abs
#   [2,3,31,31]     1.82e-10     2.20e-07 6.81e-08 5.42e-08 5.25e-08 6.78e-08             1.38e-08
#   [3,3,33,47]     4.81e-11     2.10e-07 7.02e-08 3.80e-08 4.19e-08 4.63e-08             1.59e-08
#   [1,3,96,80]     6.78e-12     2.39e-07 8.34e-08 4.24e-08 5.13e-08 4.45e-08             1.17e-08
#   [2,3,64,64]     2.20e-10     2.00e-07 7.93e-08 4.65e-08 3.82e-08 4.19e-08             1.19e-08
#   [1,3,512,512]   6.69e-11     3.46e-07 8.46e-08 5.46e-08 4.99e-08 4.51e-08             7.03e-09
# (the metric itself is about 6e-4 with these random weights; the input scaling is off by 3.09e-07, one ulp at 2.6)
# Measured on an MI355X against fp64 (test_lpips_gpu.py and test_f32net_gpu.py print each figure): metric 4.4e-11 1.6e-10 3.8e-12 5.5e-11 1.2e-11;
# convolutions 4.9e-08 .. 1.4e-07 of sum|a b|; tap distance 2.7e-09 .. 5.1e-08 of layer_abs; input scaling 3.09e-07.
E32_METRIC = 2.20e-10                                            # max |ref_fp32 - ref_fp64|, absolute
E32_CONV = (3.47e-7, 8.47e-8, 5.47e-8, 5.25e-8, 6.79e-8)         # per conv, relative to sum |a b| + |bias|
E32_LAYER = 1.59e-8                                              # relative to layer_abs
E32_PREP = 3.09e-7                                               # absolute
GPU_FACTOR = 8
METRIC_TOL = GPU_FACTOR * E32_METRIC                             # 1.76e-09
CONV_TOL = tuple(GPU_FACTOR * e for e in E32_CONV)               # 2.78e-06 6.78e-07 4.38e-07 4.20e-07 5.43e-07
LAYER_TOL = GPU_FACTOR * E32_LAYER                               # 1.27e-07
PREP_TOL = GPU_FACTOR * E32_PREP                                 # 2.47e-06


def images(shape, seed):
    """(pred, target) on the 8-bit grid, fp32: a random target and a noisy copy - what the evaluator passes."""
    g = torch.Generator().manual_seed(seed)
    tgt = torch.rand(shape, generator=g)
    pred = (tgt + 0.08 * torch.randn(shape, generator=g)).clamp(0, 1)
    q = lambda x: torch.round(x * 255) / 255
    return q(pred), q(tgt)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def scale_input(x, dtype=torch.float64):
    """[N,3,H,W] in [0,1] -> ((2x - 1) - shift) / scale."""
    x = x.to(dtype)
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    return ((2 * x - 1) - shift) / scale


def conv(x, w, b, stride, pad, relu=True, dtype=torch.float64):
    y = F.conv2d(x.to(dtype), w.to(dtype), None if b is None else b.to(dtype), stride=stride, padding=pad)
    return F.relu(y) if relu else y


def conv_abs(x, w, b, stride, pad):
    """sum |a b| (+ |bias|) of every output element, fp64: the scale rounding errors of a dot product are proportional to."""
    return F.conv2d(x.double().abs(), w.double().abs(), None if b is None else b.double().abs(), stride=stride, padding=pad)


def pool(x):
    return F.max_pool2d(x, kernel_size=3, stride=2)


def unit(f):
    return f / (torch.sqrt((f * f).sum(dim=1, keepdim=True)) + 1e-10)       # eps added to the norm, not under the root


def layer(f_pred, f_tgt, lin, dtype=torch.float64):
    """One tap: [N,C,H,W] features of both images, lin [C] -> [N] mean over pixels of sum_c lin_c (u_pred - u_tgt)^2."""
    d = (unit(f_pred.to(dtype)) - unit(f_tgt.to(dtype))) ** 2
    return (d * lin.to(dtype).view(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def layer_abs(f_pred, f_tgt, lin):
    """The scale a tap's rounding error is proportional to, fp64: an error eps |u| in each normalised feature moves
    (u_pred - u_tgt)^2 by 2 |u_pred - u_tgt| eps (|u_pred| + |u_tgt|), so: mean over pixels of
    sum_c lin_c |u_pred - u_tgt| (|u_pred| + |u_tgt|).  (Scaling by the value itself would not do: for near-identical images the
    value is far smaller than its error scale, for unrelated ones it is not.)"""
    up, ut = unit(f_pred.double()), unit(f_tgt.double())
    d = (up - ut).abs() * (up.abs() + ut.abs())
    return (d * lin.double().view(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def features(x, cpu_weights, dtype=torch.float64):
    """The five taps of [N,3,H,W] images in [0,1]; cpu_weights: LpipsWeights.cpu (conv{i}.weight, conv{i}.bias)."""
    taps, f = [], scale_input(x, dtype)
    for i, ((_co, _ci, _k, stride, pad), p) in enumerate(zip(CONVS, POOL_BEFORE)):
        if p:
            f = pool(f)
        f = conv(f, cpu_weights[f"conv{i}.weight"], cpu_weights[f"conv{i}.bias"], stride, pad, True, dtype)
        taps.append(f)
    return taps


def lpips(pred, target, cpu_weights, dtype=torch.float64):
    """[N] of dtype: the whole metric."""
    n = pred.shape[0]
    taps = features(torch.cat([pred, target]), cpu_weights, dtype)
    total = torch.zeros(n, dtype=dtype)
    for i, f in enumerate(taps):
        total = total + layer(f[:n], f[n:], cpu_weights[f"lin{i}"], dtype)
    return total


@functools.lru_cache(maxsize=None)
def weights_cpu():
    """The random stand-in weights of the tests, as LpipsWeights.cpu holds them (host only: no GPU needed)."""
    from unirestore_amd import lpips as L
    asd, lsd = L.random_state_dicts(WEIGHT_SEED)
    out = {}
    for i, c in enumerate(L.CONVS):
        out[f"conv{i}.weight"], out[f"conv{i}.bias"] = asd[f"features.{c[0]}.weight"], asd[f"features.{c[0]}.bias"]
        out[f"lin{i}"] = lsd[f"lin{i}.model.1.weight"].reshape(-1)
    return out


@functools.lru_cache(maxsize=None)
def e2e_reference(shape):
    """fp64 LPIPS of the case (computed once per process; callers must not modify it)."""
    pred, tgt = images(shape, E2E_CASES[shape])
    return lpips(pred, tgt, weights_cpu(), torch.float64)


def measure_e32(shape):
    """fp32's own error against fp64 on one end-to-end case -> dict: 'metric' = max |ref32 - ref64|; 'conv' = per conv, max over
    outputs of |conv32 - conv64| / sum|a b| on the SAME fp32 input (the fp32 chain's); 'layer' = max over taps and images of
    |layer32 - layer64| / layer_abs on the same fp32 features; 'prep' = max |scale32 - scale64|."""
    w = weights_cpu()
    pred, tgt = images(shape, E2E_CASES[shape])
    n = pred.shape[0]
    out = {"metric": float((lpips(pred, tgt, w, torch.float32).double() - e2e_reference(shape)).abs().max())}
    x = torch.cat([pred, tgt])
    f = scale_input(x, torch.float32)
    out["prep"] = float((f.double() - scale_input(x, torch.float64)).abs().max())
    out["conv"], out["layer"] = [], 0.0
    for i, ((_co, _ci, _k, stride, pad), p) in enumerate(zip(CONVS, POOL_BEFORE)):
        if p:
            f = pool(f)
        cw, cb = w[f"conv{i}.weight"], w[f"conv{i}.bias"]
        y32 = conv(f, cw, cb, stride, pad, False, torch.float32)
        y64 = conv(f, cw, cb, stride, pad, False, torch.float64)
        out["conv"].append(float(((y32.double() - y64).abs() / conv_abs(f, cw, cb, stride, pad)).max()))
        f = F.relu(y32)
        l32 = layer(f[:n], f[n:], w[f"lin{i}"], torch.float32).double()
        l64 = layer(f[:n], f[n:], w[f"lin{i}"], torch.float64)
        out["layer"] = max(out["layer"], float(((l32 - l64).abs() / layer_abs(f[:n], f[n:], w[f"lin{i}"])).max()))
    return out
