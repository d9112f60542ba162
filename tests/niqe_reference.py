"""An fp64 host restatement of the NIQE block features and score, written from the definition (luma, MSCN field, block moments
of the five fields, AGGD fit over the alpha grid, the bicubic halving, the Mahalanobis-like score) and independent of
unirestore_amd: the yardstick of tests/test_niqe_gpu.py.  It filters with the 49-tap 2-D Gaussian, rolls every block with
torch.roll and picks alpha with an argmin over the whole grid.

Every sum is written as a chain of elementwise additions in a stated order, so a run gives the same bits on every host.
order=0 is the yardstick.  order=1 is the same mathematics with a second summation order - a separable Gaussian, block sums and
halving taps added from the far end - whose distance from order 0 measures how far two correct fp64 implementations lie apart
(tests/test_niqe_cpu.py turns that into the GPU tolerances).
"""
import math

import torch

BLOCK = 96
GRID = 9801
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
HALVE_TAPS = tuple(v / 2 for v in (-0.0234375, -0.0703125, 0.2265625, 0.8671875, 0.8671875, 0.2265625, -0.0703125, -0.0234375))
_F64 = torch.float64


def cubic(x: float, a: float = -0.5) -> float:
    """The cubic convolution kernel."""
    x = abs(x)
    if x <= 1:
        return (a + 2) * x ** 3 - (a + 3) * x ** 2 + 1
    if x < 2:
        return a * x ** 3 - 5 * a * x ** 2 + 8 * a * x - 4 * a
    return 0.0


def halve_taps_from_kernel():
    """The eight taps of an output of imresize(., 0.5) with antialiasing: the cubic kernel stretched by 2, sampled at the input
    centres around the output centre (input index 2 o + 0.5), scaled by 1/2 and normalised."""
    w = [0.5 * cubic(0.5 * (k - 3 - 0.5)) for k in range(8)]
    s = sum(w)
    return [v / s for v in w]


def gaussian1d():
    sigma = 7.0 / 6.0
    w = [math.exp(-((k - 3) ** 2) / (2 * sigma * sigma)) for k in range(7)]
    s = sum(w)
    return [v / s for v in w]


def gaussian2d():
    sigma = 7.0 / 6.0
    w = [[math.exp(-((i - 3) ** 2 + (j - 3) ** 2) / (2 * sigma * sigma)) for j in range(7)] for i in range(7)]
    s = sum(sum(r) for r in w)
    return [[v / s for v in r] for r in w]


_TABLES = None


def tables():
    """(alpha, rho, sqrt(Gamma(1/a) / Gamma(3/a)), Gamma(2/a) / Gamma(1/a)) over alpha = 0.2 + 0.001 i, i < 9801."""
    global _TABLES
    if _TABLES is None:
        alpha = [0.2 + 0.001 * i for i in range(GRID)]
        rho, scale, ratio = [], [], []
        for a in alpha:
            g1, g2, g3 = math.gamma(1 / a), math.gamma(2 / a), math.gamma(3 / a)
            rho.append(g2 * g2 / (g1 * g3))
            scale.append(math.sqrt(g1 / g3))
            ratio.append(g2 / g1)
        _TABLES = tuple(torch.tensor(v, dtype=_F64) for v in (alpha, rho, scale, ratio))
    return _TABLES


def luma(x: torch.Tensor, color_space: str = "yiq") -> torch.Tensor:
    """fp32 [N,3,H,W] in [0,1] -> rounded luma fp64 [N,h,w] of the top-left crop to multiples of 96."""
    n, _c, h, w = x.shape
    x = x.detach().cpu().to(_F64)[:, :, :h // BLOCK * BLOCK, :w // BLOCK * BLOCK]
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    if color_space == "yiq":
        y = ((0.299 * r + 0.587 * g) + 0.114 * b) * 255.0
    elif color_space == "ycbcr":
        y = ((16.0 + 65.481 * r) + 128.553 * g) + 24.966 * b
    else:
        raise ValueError(color_space)
    return torch.round(y)


def _pad3(y):
    return torch.nn.functional.pad(y[:, None], (3, 3, 3, 3), mode="replicate")[:, 0]


def _filter(y: torch.Tensor, order: int) -> torch.Tensor:
    n, h, w = y.shape
    p = _pad3(y)
    if order == 0:                                             # 49 taps, row-major
        k = gaussian2d()
        out = torch.zeros_like(y)
        for i in range(7):
            for j in range(7):
                out = out + k[i][j] * p[:, i:i + h, j:j + w]
        return out
    g = gaussian1d()                                           # separable: along the rows of the image first, then down the columns
    t = torch.zeros(n, h + 6, w, dtype=_F64)
    for j in range(7):
        t = t + g[j] * p[:, :, j:j + w]
    out = torch.zeros_like(y)
    for i in range(7):
        out = out + g[i] * t[:, i:i + h]
    return out


def mscn(y: torch.Tensor, order: int = 0) -> torch.Tensor:
    mu = _filter(y, order)
    sigma = torch.sqrt(torch.abs(_filter(y * y, order) - mu * mu))
    return (y - mu) / (sigma + 1.0)


def _blocks(f: torch.Tensor, bs: int) -> torch.Tensor:
    """[N,h,w] -> [N, blocks, bs, bs], blocks row-major."""
    n, h, w = f.shape
    return f.reshape(n, h // bs, bs, w // bs, bs).permute(0, 1, 3, 2, 4).reshape(n, (h // bs) * (w // bs), bs, bs)


def _sum2(v: torch.Tensor, order: int) -> torch.Tensor:
    """The sum over the last two axes as a chain: down the rows, then along the columns (from the far end for order 1)."""
    rows = range(v.shape[-2]) if order == 0 else range(v.shape[-2] - 1, -1, -1)
    acc = torch.zeros(v.shape[:-2] + v.shape[-1:], dtype=_F64)
    for r in rows:
        acc = acc + v[..., r, :]
    cols = range(acc.shape[-1]) if order == 0 else range(acc.shape[-1] - 1, -1, -1)
    tot = torch.zeros(acc.shape[:-1], dtype=_F64)
    for c in cols:
        tot = tot + acc[..., c]
    return tot


def block_moments(field: torch.Tensor, bs: int, order: int = 0) -> torch.Tensor:
    """[N,h,w] -> [N, blocks, 5, 6]."""
    b = _blocks(field, bs)
    fields = torch.stack([b] + [b * torch.roll(b, s, dims=(-2, -1)) for s in SHIFTS], dim=2)        # [N, B, 5, bs, bs]
    sq = fields * fields
    neg, pos = (fields < 0).to(_F64), (fields > 0).to(_F64)
    zero = torch.zeros_like(sq)
    parts = [neg, torch.where(fields < 0, sq, zero), pos, torch.where(fields > 0, sq, zero), torch.abs(fields), sq]
    return torch.stack([_sum2(p, order) for p in parts], dim=-1)


def fit_ratio(moments: torch.Tensor, pixels: int):
    """(l, r, R) of moments [..., 6]."""
    nn_, sn, npos, sp, sa, ss = moments.unbind(-1)
    l, r = torch.sqrt(sn / nn_), torch.sqrt(sp / npos)
    gam = l / r
    g2 = gam * gam
    ma = sa / pixels
    rhat = (ma * ma) / (ss / pixels)
    return l, r, ((rhat * (g2 * gam + 1.0)) * (gam + 1.0)) / ((g2 + 1.0) * (g2 + 1.0))


def fit(moments: torch.Tensor, pixels: int):
    """moments [N, B, 5, 6] -> (features [N, B, 18], alpha index int64 [N, B, 5] with -1 where R is NaN)."""
    alpha, rho, scale, ratio = tables()
    l, r, R = fit_ratio(moments, pixels)
    bad = torch.isnan(R)
    idx = torch.argmin((rho - torch.where(bad, torch.zeros_like(R), R)[..., None]) ** 2, dim=-1)      # the first minimum
    nan = torch.full_like(R, float("nan"))
    a = torch.where(bad, nan, alpha[idx])
    bl, br = torch.where(bad, nan, l * scale[idx]), torch.where(bad, nan, r * scale[idx])
    mean = torch.where(bad, nan, (br - bl) * ratio[idx])
    cols = [a[..., 0], (bl[..., 0] + br[..., 0]) / 2.0]
    for k in range(1, 5):
        cols += [a[..., k], mean[..., k], bl[..., k], br[..., k]]
    return torch.stack(cols, dim=-1), torch.where(bad, torch.full_like(idx, -1), idx)


def _mirror(i: int, n: int) -> int:
    return -i - 1 if i < 0 else (2 * n - 1 - i if i >= n else i)


def _halve_axis(x: torch.Tensor, axis: int, order: int) -> torch.Tensor:
    n = x.shape[axis]
    ks = range(8) if order == 0 else range(7, -1, -1)
    out = None
    for k in ks:
        idx = torch.tensor([_mirror(2 * o - 3 + k, n) for o in range(n // 2)])
        term = HALVE_TAPS[k] * x.index_select(axis, idx)
        out = term if out is None else out + term
    return out


def halve(y: torch.Tensor, order: int = 0) -> torch.Tensor:
    """[N,h,w] -> halve(y / 255) * 255: down the rows first, then along the columns."""
    return _halve_axis(_halve_axis(y / 255.0, 1, order), 2, order) * 255.0


def pipeline(x: torch.Tensor, color_space: str = "yiq", order: int = 0) -> dict:
    """Every intermediate of the block features of fp32 images x, by name."""
    y = luma(x, color_space)
    m1 = mscn(y, order)
    mom1 = block_moments(m1, BLOCK, order)
    f1, i1 = fit(mom1, BLOCK * BLOCK)
    y2 = halve(y, order)
    m2 = mscn(y2, order)
    half = BLOCK // 2
    mom2 = block_moments(m2, half, order)
    f2, i2 = fit(mom2, half * half)
    return dict(luma=y, mscn1=m1, moments1=mom1, features1=f1, index1=i1, halve=y2, mscn2=m2, moments2=mom2, features2=f2, index2=i2,
                features=torch.cat([f1, f2], dim=-1), R1=fit_ratio(mom1, BLOCK * BLOCK)[2], R2=fit_ratio(mom2, half * half)[2])


def score(features: torch.Tensor, mu_p: torch.Tensor, cov_p: torch.Tensor) -> torch.Tensor:
    """[N, B, 36] -> fp64 [N]."""
    out = []
    for rows in features.to(_F64):
        good = rows[~torch.isnan(rows).any(dim=1)]
        if good.shape[0] < 2:
            out.append(float("nan"))
            continue
        mu = torch.stack([c[~torch.isnan(c)].mean() for c in rows.T])
        cov = torch.cov(good.T, correction=1)
        d = mu_p.to(_F64).reshape(-1) - mu
        out.append(float(torch.sqrt(d @ torch.linalg.pinv((cov_p.to(_F64) + cov) / 2) @ d)))
    return torch.tensor(out, dtype=_F64)


def midpoint_margin(R: torch.Tensor) -> float:
    """The smallest relative distance of a finite R from the nearest midpoint between two neighbouring rho grid values: an
    implementation whose R lies closer than this to the yardstick's picks the same alpha."""
    rho = tables()[1]
    mids = (rho[:-1] + rho[1:]) / 2
    r = R[~torch.isnan(R)].reshape(-1)
    if r.numel() == 0:
        return float("inf")
    j = torch.searchsorted(mids, r).clamp(1, mids.numel() - 1)
    d = torch.minimum((mids[j] - r).abs(), (mids[j - 1] - r).abs())
    return float((d / r.abs()).min())
