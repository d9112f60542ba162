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


# ---- multi-task decode (DiffUIE.forward_tasks): how many tasks one fanned-out decoder batch may hold ---------------------------
# ur_conv2d_nhwc addresses its inputs with 32-bit element offsets and refuses N*H*W*ld >= 2^31 (csrc/igemm.hip)
TASK_CHUNK_MAX_ELEMS = 1 << 31


def task_chunks(n_images: int, n_tasks: int, out_h: int, out_w: int, widest_channels: int):
    """Split `n_tasks` into the fewest, near-equal runs of consecutive tasks [(first_task, n), ...] whose fanned-out batch of
    n * n_images images keeps the decoder's largest conv input below the launcher's limit:
    n * n_images * out_h * out_w * widest_channels < TASK_CHUNK_MAX_ELEMS.  out_h * out_w * widest_channels stands for the largest
    H*W*ld of one image over the convs that run fanned out.  Chunk sizes differ by at most one task.  A single task that does not
    fit is returned as chunks of one (the launcher's own error then surfaces, as in a single-task forward)."""
    if n_images < 1 or n_tasks < 1 or out_h < 1 or out_w < 1 or widest_channels < 1:
        raise ValueError(f"task_chunks: positive sizes needed, got {(n_images, n_tasks, out_h, out_w, widest_channels)}")
    per_task = n_images * out_h * out_w * widest_channels
    most = max((TASK_CHUNK_MAX_ELEMS - 1) // per_task, 1)
    n_chunks = -(-n_tasks // most)
    base, rem = divmod(n_tasks, n_chunks)
    out, first = [], 0
    for i in range(n_chunks):
        n = base + (1 if i < rem else 0)
        out.append((first, n))
        first += n
    return out
