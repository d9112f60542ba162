"""Antialiased resize of 8-bit images on the GPU (csrc/resize.hip; the kernels' specification is the ur_resize_u8 comment of
include/unirestore_hip.h, the notes are DESIGN.md 6s), and the reference's resize-down / corrupt / resize-back wrapper built on it.

`resize_u8` returns the bytes torch's CPU `interpolate(uint8, mode, antialias=True)` gives, which is what torchvision v2's
`TF.resize` runs on the uint8 tensor `read_image` returns and so what the reference's IRCorruptDataset._degrade_image calls twice
per image (src/data/dataset_ir.py).  This module is the planner: per axis it builds the (xmin, xsize) table and the fixed-point
weights on the host in fp64 (`axis_tables`); the two kernels only apply tables, so bilinear and bicubic are the same kernels.
`around` is the wrapper itself; `inside` is the one body of `corrupt.degrade`, `distort.degrade` and `jpeg.degrade`, which put a
degradation inside it.  An image's short edge is a pure function of (seed, stem): `draw_short_edge`.
"""
import hashlib
from functools import lru_cache

import numpy as np

MODES = {"bilinear": 2, "bicubic": 4}               # -> the filter's interpolation size
MIN_SIDE = 2                                        # torch's CPU code paths disagree with each other at an output side of 1


def check_mode(mode) -> str:
    if mode not in MODES:
        raise ValueError(f"resize mode {mode!r}: choose from {', '.join(MODES)}")
    return mode


def _filter(t: np.ndarray, mode: str) -> np.ndarray:
    t = np.abs(t)
    if mode == "bilinear":
        return np.where(t < 1.0, 1.0 - t, 0.0)
    a = -0.5                                        # the Keys cubic, in the reference's order of operations
    return np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0, np.where(t < 2.0, (((t - 5.0) * t + 8.0) * t - 4.0) * a, 0.0))


@lru_cache(maxsize=256)
def axis_tables(n_in: int, n_out: int, mode: str = "bilinear"):
    """One axis n_in -> n_out: (bounds int32 [n_out, 2] = (xmin, xsize), integer weights int32 [n_out, K], K, p), everything in fp64
    as the ur_resize_u8 comment states it.  The arrays are shared by every caller: they are read-only."""
    check_mode(mode)
    if min(n_in, n_out) < 1:
        raise ValueError(f"axis_tables: lengths must be positive, got {n_in} -> {n_out}")
    scale = n_in / n_out
    half = MODES[mode] / 2
    support = half * scale if scale >= 1.0 else half
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    k = int(np.ceil(support)) * 2 + 1
    c = scale * (np.arange(n_out, dtype=np.float64) + 0.5)
    xmin = np.maximum((c - support + 0.5).astype(np.int64), 0)                      # (the cast truncates towards zero)
    xsize = np.minimum((c + support + 0.5).astype(np.int64), n_in) - xmin
    j = np.arange(k, dtype=np.int64)[None, :]
    w = np.where(j < xsize[:, None], _filter((j + xmin[:, None] - c[:, None] + 0.5) * inv, mode), 0.0)
    total = np.cumsum(w, axis=1)[:, -1:]                                            # added in ascending j; the empty slots add 0
    w = np.where(total != 0.0, w / np.where(total != 0.0, total, 1.0), w)
    wmax = float(w.max())
    p = next((q for q in range(22) if int(0.5 + wmax * (1 << (q + 1))) >= (1 << 15)), 22)
    ints = np.trunc(w * float(1 << p) + np.where(w < 0, -0.5, 0.5)).astype(np.int32)
    bounds = np.stack([xmin, xsize], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    ints.setflags(write=False)
    return bounds, ints, k, p


def check_size(size):
    if not isinstance(size, (tuple, list)) or len(size) != 2 or any(isinstance(s, bool) or not hasattr(s, "__index__") for s in size) or \
            min(int(s) for s in size) < MIN_SIDE:
        raise ValueError(f"resize: size must be two integers (oh, ow), both >= {MIN_SIDE}, got {size!r}")
    return int(size[0]), int(size[1])


def resize_u8(images_u8, size, mode: str = "bilinear"):
    """images_u8: device uint8 [N, H, W, 3] -> uint8 [N, oh, ow, 3], size = (oh, ow); all four sides >= 2.  Byte for byte what torch's
    CPU interpolate(uint8 NCHW, size, mode, antialias=True) returns: along the width first, into a uint8 intermediate."""
    import torch

    from . import ops
    oh, ow = check_size(size)
    check_mode(mode)
    ops.check_u8_images("resize_u8", images_u8, min_side=MIN_SIDE)
    _, h, w, _ = images_u8.shape

    def upload(n_in, n_out):
        bounds, ints, k, p = axis_tables(n_in, n_out, mode)
        # (copies: the cached arrays are read-only, which torch.from_numpy warns about)
        return torch.from_numpy(bounds.copy()).to(images_u8.device), torch.from_numpy(ints.copy()).to(images_u8.device), k, p
    return ops.resize_u8(images_u8, (oh, ow), upload(w, ow), upload(h, oh))


def short_edge_size(h: int, w: int, s: int):
    """torchvision's output (oh, ow) of resize(img, (s,)): the short side becomes s, the long side int(s * long / short) (a float
    division, truncated); with w <= h the width is the short side."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(s * long / short)
    return (new_long, s) if w <= h else (s, new_long)


def check_range(resize, minimum: int = MIN_SIDE):
    """(lo, hi) or "LO,HI" -> (lo, hi): two integers with minimum <= lo < hi, the half-open range a short edge is drawn from."""
    if isinstance(resize, str):
        parts = [s.strip() for s in resize.split(",")]
        if len(parts) != 2 or not all(s.isdigit() for s in parts):
            raise ValueError(f"resize {resize!r}: give two integers LO,HI")
        resize = [int(s) for s in parts]
    if not isinstance(resize, (tuple, list)) or len(resize) != 2 or any(isinstance(s, bool) or not hasattr(s, "__index__") for s in resize):
        raise ValueError(f"resize {resize!r}: give two integers (lo, hi)")
    lo, hi = int(resize[0]), int(resize[1])
    if lo >= hi:
        raise ValueError(f"resize ({lo}, {hi}): lo must be below hi (the short edge is drawn from [lo, hi))")
    if lo < minimum:
        raise ValueError(f"resize ({lo}, {hi}): lo must be >= {minimum}, the smallest side the degradation inside takes")
    return lo, hi


def draw_short_edge(seed: int, stem: str, lo: int, hi: int) -> int:
    """The short edge of the image named `stem`, uniform over the integers of [lo, hi), from sha256 of (seed, stem)."""
    if lo >= hi:
        raise ValueError(f"draw_short_edge: empty range [{lo}, {hi})")
    h = int.from_bytes(hashlib.sha256(f"{seed}\0corrupt\0{stem}\0resize".encode()).digest()[:8], "little")
    return lo + min(int((h >> 11) * 2.0 ** -53 * (hi - lo)), hi - lo - 1)


def per_image(who: str, n: int, seeds, stems):
    """One integer seed -> n of it, stems None -> n empty names; lists pass through.  -> (seeds, stems), both of length n."""
    seeds = [seeds] * n if hasattr(seeds, "__index__") else list(seeds)
    stems = [""] * n if stems is None else list(stems)
    if len(seeds) != n or len(stems) != n:
        raise ValueError(f"{who}: {n} images but {len(seeds)} seeds and {len(stems)} stems")
    return seeds, stems


def drawn_sizes(h: int, w: int, seeds, stems, lo: int, hi: int) -> list:
    """The resized (oh, ow) of every H x W image of a batch: its short edge drawn from [lo, hi) by its own (seed, stem)."""
    return [short_edge_size(h, w, draw_short_edge(s, t, lo, hi)) for s, t in zip(seeds, stems)]


def inside(images_u8, seeds, stems, resize, fn, minimum: int, who: str, min_side: int = 32):
    """A degradation inside the wrapper: resize = (lo, hi) with lo >= minimum, images of H, W >= min_side; image n is resized to
    its drawn size (`drawn_sizes`), fn(batch, seeds, stems) -> uint8 of batch's shape degrades every group of equal resized shape
    under its members' own seeds and stems, and `around` resizes the results back.  -> uint8 of the input's shape."""
    from . import ops
    lo, hi = check_range(resize, minimum)
    ops.check_u8_images(who, images_u8, min_side=min_side)
    n, h, w, _ = images_u8.shape
    seeds, stems = per_image(who, n, seeds, stems)
    return around(images_u8, drawn_sizes(h, w, seeds, stems, lo, hi),
                  lambda batch, idx: fn(batch, [seeds[i] for i in idx], [stems[i] for i in idx]))


def around(images_u8, sizes, fn, mode: str = "bilinear"):
    """The reference's wrapper: image n is resized to sizes[n] = (h, w), fn(batch, indices) -> uint8 of batch's shape is called once
    per group of images with equal resized shape (groups and their members in input order; indices = the members' places in
    images_u8), and every result is resized back to (H, W).  -> uint8 [N, H, W, 3].  An image's result depends on its own bytes,
    its own size and what fn does with it - not on the batch around it."""
    import torch

    from . import ops
    ops.check_u8_images("resize.around", images_u8, min_side=MIN_SIDE)
    n, h, w, _ = images_u8.shape
    sizes = [check_size(tuple(s)) for s in sizes]
    if len(sizes) != n:
        raise ValueError(f"resize.around: {n} images but {len(sizes)} sizes")
    groups = {}
    for i, s in enumerate(sizes):
        groups.setdefault(s, []).append(i)
    out = torch.empty_like(images_u8)
    for s, idx in groups.items():
        where = torch.tensor(idx, device=images_u8.device)
        small = resize_u8(images_u8.index_select(0, where) if len(idx) < n else images_u8, s, mode)
        done = fn(small, list(idx))
        if not isinstance(done, torch.Tensor) or done.dtype != torch.uint8 or done.shape != small.shape:
            raise ValueError(f"resize.around: fn must return uint8 {tuple(small.shape)}, got {getattr(done, 'dtype', type(done))} "
                             f"{tuple(getattr(done, 'shape', ()))}")
        out.index_copy_(0, where, resize_u8(done.contiguous(), (h, w), mode))
    return out
