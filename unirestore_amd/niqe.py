"""NIQE, the closed-form no-reference quality score (Mittal et al., "Making a completely blind image quality analyzer"), on the
GPU in fp64: the kernels of csrc/niqe.hip chained into the 36 natural-scene-statistics features of every 96 x 96 block, and the
score of an image against a user's pristine model on the host.  What the reference's evaluator reports in `eval_mode: NR`
(eval_image_restoration.py:106-108,189-203) through pyiqa's `niqe`.

The steps, as this project defines them (a restatement of pyiqa's port of the MATLAB code; pyiqa is not installed where this
project is developed, so AGREEMENT WITH ITS PUBLISHED NUMBERS HAS NOT BEEN CHECKED):
  1. luma of the [0,1] image on the 0..255 scale ("yiq": BT.601 weights; "ycbcr": the 16..235 studio range), rounded half to
     even, cropped to the top-left multiple of 96 per side;
  2. the MSCN field (y - mu) / (sigma + 1) under a 7 x 7 Gaussian of sigma 7/6, replicate border at the crop's edge;
  3. per block the six moments of the field and of its products with four circularly rolled copies of the block;
  4. an asymmetric-generalised-Gaussian fit of each of the five fields by a search over alpha = 0.2, 0.201, .., 10 -> 18 features;
  5. the same on the antialiased bicubic halving of the luma with 48 x 48 blocks -> 36 features per block;
  6. score = sqrt(d^T pinv((cov_p + cov) / 2) d), d = mu_p - nanmean of the block rows, cov = the sample covariance of the rows
     without a NaN; NaN when fewer than two rows are NaN-free.
Inside a perfectly flat region y - mu is rounding noise whose signs decide that block's features: two correct implementations
disagree there.  That is a property of NIQE.

The project ships NO pristine model.  `load_params` reads the file a user of the metric already has (pyiqa's
niqe_modelparameters.mat or a .pt / .npz with the same two keys); `random_params` makes a seeded stand-in for tests and timing.
"""
import functools
import math
import os

import torch

from .capi import check, lib
from .f32net import stream

BLOCK = 96                                               # block edge at the first scale; BLOCK // 2 at the second
MIN_BLOCKS = 2                                           # a covariance needs two rows
COLOR_SPACES = ("yiq", "ycbcr")
FEATURES = 36
GRID = 9801                                              # alpha = 0.2 + 0.001 i
KEYS = ("mu_prisparam", "cov_prisparam")
EXTENSIONS = (".pt", ".pth", ".npz", ".mat")


class NiqeParams:
    """The pristine model of a NIQE score: mu fp64 [36] and cov fp64 [36, 36] (kept on the host, where the score's algebra runs)
    and the device the features are computed on.  ValueError (source and key named) for a wrong shape or a non-finite value."""

    def __init__(self, mu, cov, dev=None, source: str = "NiqeParams"):
        vals = {}
        for key, v, shapes in ((KEYS[0], mu, ((FEATURES,), (1, FEATURES))), (KEYS[1], cov, ((FEATURES, FEATURES),))):
            try:
                t = torch.as_tensor(v).detach().to(device="cpu", dtype=torch.float64)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError(f"{source}: {key!r} is no numeric array") from None
            if tuple(t.shape) not in shapes:
                raise ValueError(f"{source}: {key!r} has shape {tuple(t.shape)}, expected {' or '.join(str(list(s)) for s in shapes)}")
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"{source}: {key!r} holds a non-finite value")
            vals[key] = t
        self.mu = vals[KEYS[0]].reshape(FEATURES).clone()
        self.cov = vals[KEYS[1]].clone()
        self.source = source
        self.device = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)


def load_params(path, dev=None) -> NiqeParams:
    """The pristine model of a file with the keys `mu_prisparam` ([36] or [1, 36]) and `cov_prisparam` ([36, 36]): a .pt / .pth
    dict, an .npz, or the original niqe_modelparameters.mat (read with scipy.io.loadmat, imported only then).  ValueError (file
    and key named) for an unknown extension, a missing key, a wrong shape or a non-finite value."""
    path = str(path)
    ext = os.path.splitext(path)[1].lower()
    if ext not in EXTENSIONS:
        raise ValueError(f"{path}: unknown extension {ext!r} for NIQE parameters, expected one of {list(EXTENSIONS)}")
    if ext == ".mat":
        try:
            from scipy.io import loadmat
        except ImportError:
            raise ImportError(f"{path}: reading a .mat file needs scipy (scipy.io.loadmat), which is not installed; convert the file "
                              f"to an .npz or .pt with the keys {list(KEYS)}") from None
        d = loadmat(path)
    elif ext == ".npz":
        import numpy as np
        with np.load(path) as z:
            d = {k: z[k] for k in z.files}
    else:
        d = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(d, dict):
            raise ValueError(f"{path}: holds a {type(d).__name__}, expected a dict with the keys {list(KEYS)}")
    for key in KEYS:
        if key not in d:
            raise ValueError(f"{path}: key {key!r} is missing")
    return NiqeParams(d[KEYS[0]], d[KEYS[1]], dev, source=path)


def random_params(seed: int = 0, dev=None) -> NiqeParams:
    """A seeded symmetric positive definite stand-in for a pristine model, for tests and timing ONLY: mu standard normal,
    cov = A A^T / 36 + 0.1 I.  NOT fitted to any image - its scores say nothing about quality."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(FEATURES, generator=g, dtype=torch.float64)
    a = torch.randn(FEATURES, FEATURES, generator=g, dtype=torch.float64)
    return NiqeParams(mu, a @ a.T / FEATURES + 0.1 * torch.eye(FEATURES, dtype=torch.float64), dev, source=f"random_params({seed})")


# ---- tables on the host ------------------------------------------------------------------------------------------------------------

HALVE_TAPS = tuple(v / 2 for v in (-0.0234375, -0.0703125, 0.2265625, 0.8671875, 0.8671875, 0.2265625, -0.0703125, -0.0234375))


def gaussian7():
    """The seven weights of one axis of the MSCN window: exp(-(k - 3)^2 / (2 sigma^2)), sigma = 7/6, normalised to sum 1."""
    sigma = 7.0 / 6.0
    w = [math.exp(-((k - 3) ** 2) / (2.0 * sigma * sigma)) for k in range(7)]
    s = 0.0
    for v in w:
        s += v
    return [v / s for v in w]


@functools.lru_cache(maxsize=None)
def alpha_tables():
    """(alpha, rho, scale, mean_ratio), fp64 [9801] on the host: alpha = 0.2 + 0.001 i, rho = Gamma(2/a)^2 / (Gamma(1/a) Gamma(3/a))
    (strictly increasing), scale = sqrt(Gamma(1/a) / Gamma(3/a)), mean_ratio = Gamma(2/a) / Gamma(1/a)."""
    alpha = [0.2 + 0.001 * i for i in range(GRID)]
    g1, g2, g3 = ([math.gamma(k / a) for a in alpha] for k in (1.0, 2.0, 3.0))
    rho = [b * b / (a * c) for a, b, c in zip(g1, g2, g3)]
    scale = [math.sqrt(a / c) for a, c in zip(g1, g3)]
    ratio = [b / a for a, b in zip(g1, g2)]
    return tuple(torch.tensor(v, dtype=torch.float64) for v in (alpha, rho, scale, ratio))


@functools.lru_cache(maxsize=None)                       # never evicted: a captured graph keeps reading the tables it was captured with
def _device_tables(dev_index: int):
    dev = torch.device("cuda", dev_index)
    return tuple(t.to(dev) for t in alpha_tables()[1:])


# ---- launch wrappers (fp64 device tensors in and out: contiguous, checked here; the shapes are checked by the library) -------------

def _f64(t: torch.Tensor, name: str, ndim: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.ndim != ndim or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"niqe.{name}: needs a contiguous {ndim}-d fp64 device tensor, got {getattr(t, 'dtype', type(t))} "
                         f"{tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
    return t


def crop_hw(h: int, w: int):
    """The top-left crop NIQE works on: the largest multiples of BLOCK."""
    return h // BLOCK * BLOCK, w // BLOCK * BLOCK


def luma(x: torch.Tensor, color_space: str = "yiq") -> torch.Tensor:
    """fp32 NCHW [N,3,H,W] in [0,1] -> the rounded 0..255 luma of the top-left (H // 96 * 96, W // 96 * 96) crop, fp64 [N,h,w]."""
    if color_space not in COLOR_SPACES:
        raise ValueError(f"niqe: unknown color_space {color_space!r}, choose from {COLOR_SPACES}")
    n, _c, h, w = x.shape
    ch, cw = crop_hw(h, w)
    y = torch.empty(n, ch, cw, dtype=torch.float64, device=x.device)
    check(lib.ur_niqe_luma(x.data_ptr(), y.data_ptr(), n, h, w, ch, cw, COLOR_SPACES.index(color_space), stream()))
    return y


def mscn(y: torch.Tensor) -> torch.Tensor:
    """fp64 [N,h,w] -> its MSCN field (y - mu) / (sigma + 1), replicate border at the field's edge."""
    n, h, w = _f64(y, "mscn", 3).shape
    m = torch.empty_like(y)
    check(lib.ur_niqe_mscn(y.data_ptr(), m.data_ptr(), n, h, w, stream()))
    return m


def block_moments(field: torch.Tensor, bs: int = BLOCK) -> torch.Tensor:
    """fp64 [N,h,w] (h, w multiples of bs, bs 96 or 48) -> fp64 [N, blocks, 5, 6]: per block (row-major) and field (M, then its
    products with the block rolled by (0,1), (1,0), (1,1), (1,-1)) the count and sum of squares of the negative entries, the same
    of the positive ones, sum |v| and sum v^2."""
    n, h, w = _f64(field, "block_moments", 3).shape
    out = torch.empty(n, max(h // bs, 0) * max(w // bs, 0) if bs in (96, 48) else 0, 5, 6, dtype=torch.float64, device=field.device)
    check(lib.ur_niqe_block_moments(field.data_ptr(), out.data_ptr(), n, h, w, bs, stream()))
    return out


def halve(y: torch.Tensor) -> torch.Tensor:
    """fp64 [N,h,w] (h, w even, >= 4) -> halve(y / 255) * 255, fp64 [N,h/2,w/2]: MATLAB's antialiased bicubic imresize(., 0.5)."""
    n, h, w = _f64(y, "halve", 3).shape
    out = torch.empty(n, h // 2, w // 2, dtype=torch.float64, device=y.device)
    check(lib.ur_niqe_halve(y.data_ptr(), out.data_ptr(), n, h, w, stream()))
    return out


def fit(moments: torch.Tensor, block_pixels: int = None, out=None, col_off: int = 0, want_index: bool = False):
    """fp64 moments [N, blocks, 5, 6] -> the 18 features of every block, fp64 [N, blocks, 18] - or written into columns
    col_off .. col_off + 17 of `out` [N, blocks, ld].  block_pixels: the pixel count P of the moments' blocks, 96 * 96 unless given
    (the moments do not hold it: the two counts leave the zeros out).  want_index: also return the alpha grid indices int32
    [N, blocks, 5] (-1 where the features are NaN).  The first call on a device uploads the three alpha tables: run once eagerly
    before capturing."""
    n, b = _f64(moments, "fit", 4).shape[:2]
    if tuple(moments.shape[2:]) != (5, 6):
        raise ValueError(f"niqe.fit: moments must be [N, blocks, 5, 6], got {tuple(moments.shape)}")
    rho, scale, ratio = _device_tables(moments.device.index)
    feat = torch.empty(n, b, 18, dtype=torch.float64, device=moments.device) if out is None else out
    idx = torch.empty(n, b, 5, dtype=torch.int32, device=moments.device) if want_index else None
    check(lib.ur_niqe_fit(moments.data_ptr(), rho.data_ptr(), scale.data_ptr(), ratio.data_ptr(), feat.data_ptr(),
                          None if idx is None else idx.data_ptr(), n * b, BLOCK * BLOCK if block_pixels is None else int(block_pixels),
                          feat.shape[2], col_off, stream()))
    return (feat, idx) if want_index else feat


def block_features(images: torch.Tensor, color_space: str = "yiq") -> torch.Tensor:
    """fp32 NCHW [N,3,H,W] in [0,1] (H, W >= 96) -> fp64 [N, blocks, 36] on the device: the 18 features of every 96 x 96 block of
    the cropped luma, then the 18 of the matching 48 x 48 block of its halving.  Eight launches, no host sync; two calls give the
    same bits, eagerly or replayed from a captured graph (run a device's first call eagerly: it uploads the alpha tables)."""
    y = luma(images, color_space)
    n, h, w = y.shape
    feats = torch.empty(n, (h // BLOCK) * (w // BLOCK), FEATURES, dtype=torch.float64, device=y.device)
    fit(block_moments(mscn(y), BLOCK), BLOCK * BLOCK, out=feats, col_off=0)
    half = BLOCK // 2
    fit(block_moments(mscn(halve(y)), half), half * half, out=feats, col_off=18)
    return feats


def score(features: torch.Tensor, params: NiqeParams) -> torch.Tensor:
    """Block features [N, blocks, 36] (or one image's [blocks, 36]) -> the NIQE score of every image, fp64 [N] on the features'
    device.  The features are copied to the host (a sync) and the 36-dimensional algebra runs there in fp64: mu = nanmean of the
    rows, cov = the sample covariance (ddof = 1) of the rows without a NaN, sqrt(d^T pinv((cov_p + cov) / 2) d).  NaN for an
    image with fewer than two NaN-free rows."""
    f = features.detach().to(device="cpu", dtype=torch.float64)
    if f.ndim == 2:
        f = f[None]
    out = torch.full((f.shape[0],), float("nan"), dtype=torch.float64)
    for i, rows in enumerate(f):
        good = rows[~torch.isnan(rows).any(dim=1)]
        if good.shape[0] < MIN_BLOCKS:
            continue
        mu = torch.nanmean(rows, dim=0)
        c = good - good.mean(dim=0)
        cov = c.T @ c / (good.shape[0] - 1)
        d = params.mu - mu
        out[i] = torch.sqrt(d @ torch.linalg.pinv((params.cov + cov) / 2) @ d)
    return out.to(features.device)


def fit_params(images: torch.Tensor, color_space: str = "yiq", dev=None) -> NiqeParams:
    """The pristine model of a batch of clean images (fp32 NCHW on the device): the mean and the sample covariance of the block
    features of all their blocks, rows with a NaN left out.  The original's selection of the sharpest blocks (by their mean local
    deviation) is NOT applied: every block counts."""
    rows = block_features(images, color_space).reshape(-1, FEATURES).cpu()
    rows = rows[~torch.isnan(rows).any(dim=1)]
    if rows.shape[0] < MIN_BLOCKS:
        raise ValueError(f"fit_params: {rows.shape[0]} NaN-free block(s), a covariance needs {MIN_BLOCKS}")
    c = rows - rows.mean(dim=0)
    return NiqeParams(rows.mean(dim=0), c.T @ c / (rows.shape[0] - 1), images.device if dev is None else dev, source="fit_params")


def forward(images: torch.Tensor, params: NiqeParams, color_space: str = "yiq") -> torch.Tensor:
    """ops.niqe after its argument checks."""
    return score(block_features(images, color_space), params)
