"""The antialiased 8-bit resize of ur_resize_u8 (the specification is the comment above its declaration in include/unirestore_hip.h)
restated in numpy: per axis the fp64 filter weights, their common fixed-point precision, the integer weights, and the two int32
passes, width first.  test_resize_cpu.py holds it against torch's CPU `interpolate(uint8, antialias=True)` byte for byte;
test_resize_gpu.py holds the kernels against it.  Nothing here is imported from the package under test."""
import math

import numpy as np

INTERP_SIZE = {"bilinear": 2, "bicubic": 4}


def triangle(t: float) -> float:
    t = abs(t)
    return 1.0 - t if t < 1.0 else 0.0


def keys_cubic(t: float, a: float = -0.5) -> float:
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


FILTER = {"bilinear": triangle, "bicubic": keys_cubic}


def axis_weights(n_in: int, n_out: int, mode: str):
    """-> (bounds int64 [n_out, 2] = (xmin, xsize), weights fp64 [n_out, K] normalised per row, zero beyond xsize, K)."""
    f, isz = FILTER[mode], INTERP_SIZE[mode]
    scale = n_in / n_out
    support = isz / 2 * scale if scale >= 1.0 else isz / 2
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    k = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int64)
    weights = np.zeros((n_out, k), dtype=np.float64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        xmin = max(int(c - support + 0.5), 0)
        xsize = min(int(c + support + 0.5), n_in) - xmin
        w = [f((j + xmin - c + 0.5) * inv) for j in range(xsize)]
        total = 0.0
        for v in w:
            total += v
        bounds[i] = (xmin, xsize)
        weights[i, :xsize] = [v / total for v in w] if total != 0.0 else w
    return bounds, weights, k


def axis_tables(n_in: int, n_out: int, mode: str):
    """-> (bounds int32 [n_out, 2], integer weights int32 [n_out, K], K, p)."""
    bounds, weights, k = axis_weights(n_in, n_out, mode)
    wmax = float(weights.max())
    p = 22
    for cand in range(22):
        if int(0.5 + wmax * (1 << (cand + 1))) >= (1 << 15):
            p = cand
            break
    scaled = weights * float(1 << p)
    ints = np.where(weights < 0, np.trunc(scaled - 0.5), np.trunc(scaled + 0.5)).astype(np.int64)
    return bounds.astype(np.int32), ints.astype(np.int32), k, p


def _wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def resize_axis(x: np.ndarray, axis: int, n_out: int, mode: str) -> np.ndarray:
    """One pass along `axis` of a uint8 array; a pass between equal lengths returns x itself."""
    n_in = x.shape[axis]
    if n_in == n_out:
        return x
    bounds, ints, _, p = axis_tables(n_in, n_out, mode)
    src = np.moveaxis(x, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
    for i in range(n_out):
        xmin, xsize = int(bounds[i, 0]), int(bounds[i, 1])
        w = ints[i, :xsize].astype(np.int64).reshape((xsize,) + (1,) * (src.ndim - 1))
        acc = _wrap32((1 << (p - 1)) + (w * src[xmin:xmin + xsize]).sum(0))           # int32 accumulation
        out[i] = np.clip(acc >> p, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(x: np.ndarray, size, mode: str = "bilinear") -> np.ndarray:
    """x uint8 [N, H, W, 3] -> uint8 [N, oh, ow, 3]: along the width into a uint8 intermediate, then along the height."""
    oh, ow = size
    assert x.dtype == np.uint8 and x.ndim == 4 and min(oh, ow) >= 2 and min(x.shape[1:3]) >= 2
    y = resize_axis(resize_axis(x, 2, ow, mode), 1, oh, mode)
    return np.ascontiguousarray(y) if y is not x else x.copy()


def torch_cpu_exact() -> bool:
    """Whether torch's CPU interpolate takes its integer uint8 path here (AVX2 or AVX512 builds)."""
    import torch
    return any(t in torch.backends.cpu.get_cpu_capability().upper() for t in ("AVX2", "AVX512"))


def torch_resize(x: np.ndarray, size, mode: str = "bilinear") -> np.ndarray:
    """torch's CPU result for the same call, what torchvision v2's resize of a uint8 tensor runs."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous()
    y = F.interpolate(t, size=tuple(size), mode=mode, antialias=True, align_corners=False)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def short_edge_size(h: int, w: int, s: int):
    """torchvision's output size for resize(img, (s,))."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(s * long / short)
    return (new_long, s) if w <= h else (s, new_long)
