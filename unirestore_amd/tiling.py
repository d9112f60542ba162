"""Tile plan of tiled latent sampling (aggregation sampling, as in StableSR): overlapping fixed-size latent tiles run through
the UNet / Controller as one batch; their noise predictions are blended back with Gaussian weights before every DDIM step
(csrc/elementwise.hip ur_latent_tiles_blend_ddim).

Host arithmetic only: origins, tile size and the per-tile normalised blend weights, computed once per latent shape.
"""
import numpy as np


def axis_origins(length: int, tile: int, stride: int):
    """Tile origins along one axis: 0, s, 2s, ... while pos + n < L, then one tile flush with the edge at L - n (duplicates
    removed).  L <= n: a single tile of length L.  Returns (origins, tile length)."""
    if length <= tile:
        return [0], length
    out, pos = [], 0
    while pos + tile < length:
        out.append(pos)
        pos += stride
    if length - tile not in out:
        out.append(length - tile)
    return out, tile


def default_tile_stride(tile: int) -> int:
    """3/4 of the tile, rounded down to a multiple of 8 (64 -> 48)."""
    return max(8, tile * 3 // 4 // 8 * 8)


def check_tile_stride(tile: int, stride: int):
    """ValueError unless tile, stride are multiples of 8 with 32 <= tile and 8 <= stride <= tile."""
    if not (isinstance(tile, (int, np.integer)) and isinstance(stride, (int, np.integer)) and
            not isinstance(tile, bool) and not isinstance(stride, bool)):
        raise ValueError(f"tile / stride must be integers, got {tile!r} / {stride!r}")
    if tile % 8 or stride % 8 or tile < 32 or stride < 8 or stride > tile:
        raise ValueError(f"latent tiling needs tile, stride multiples of 8 with 32 <= tile and 8 <= stride <= tile "
                         f"(got tile={tile}, stride={stride})")


def _gauss(n: int) -> np.ndarray:
    """g(i) = exp(-(i - (n-1)/2)^2 / (2 (0.1 n)^2)): variance 0.01 in tile-normalised coordinates (fp64)."""
    i = np.arange(n, dtype=np.float64)
    return np.exp(-((i - (n - 1) / 2) ** 2) / (2 * (0.1 * n) ** 2))


def latent_tile_plan(lh: int, lw: int, tile: int, stride: int):
    """-> (origins [(y0, x0)] row-major (y then x), (th, tw), wn fp32 [T, th, tw]).

    wn[k] = w_k / sum_j w_j per latent pixel, normalised in fp64 and rounded to fp32; w_k(i, j) = g(i) g(j).  A pixel covered
    by one tile only gets exactly 1.0.  In the tile batch, image b's tile k sits at index b*T + k."""
    check_tile_stride(tile, stride)
    if lh < 1 or lw < 1:
        raise ValueError(f"empty latent {lh}x{lw}")
    ys, th = axis_origins(lh, tile, stride)
    xs, tw = axis_origins(lw, tile, stride)
    origins = [(y, x) for y in ys for x in xs]
    w = np.outer(_gauss(th), _gauss(tw))
    acc = np.zeros((lh, lw), dtype=np.float64)
    for y, x in origins:
        acc[y:y + th, x:x + tw] += w
    wn = np.stack([w / acc[y:y + th, x:x + tw] for y, x in origins])    # singly covered: w / w, exactly 1 (w >= e^-12.5 > 0)
    return origins, (th, tw), wn.astype(np.float32)
