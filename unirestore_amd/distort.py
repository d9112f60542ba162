"""Glass blur, snow and elastic transform of clean 8-bit images on the GPU (csrc/distort.hip; the kernels' specification is the
ur_distort_* comment of include/unirestore_hip.h, the derivations are DESIGN.md 6t).

The three ImageNet-C corruptions of the reference (src/data/corruption) that work on float fields between their u8 ends.  They are
siblings of `unirestore_amd.corrupt`, not members of corrupt.NAMES (corrupt still lists them as unbuilt), and follow its rules: this
module is the planner - it builds the small tables on the host in fp64 and launches the primitives of `ops` - and an image's
randomness is a pure function of (seed, stem): corrupt.corruption_seed keys the device draws, `snow_angle` is the one host scalar.
  glass_blur         gaussian (u8) -> `iterations` local shuffles (ur_distort_shuffle) -> gaussian
  snow               the keyed normal layer, zoomed and thresholded (ur_distort_snow_layer) -> motion blur, rounding, the blend with
                     the whitened image and the layer's own rotation (ur_distort_snow)
  elastic_transform  two smoothed keyed uniform fields (ur_distort_field) -> bilinear warp (ur_distort_warp)
`distort` works at the size it is given; `degrade` is `distort` inside the reference's resize-down / resize-back wrapper
(unirestore_amd.resize.inside).  Of the reference's names only frost and spatter stay unbuilt (DESIGN.md 6t says why).
"""
import numpy as np

from . import corrupt as _cr
from .corrupt import check_severity, corruption_seed, draw_severity, gaussian_taps, motion_taps, pack_taps  # noqa: F401 (the planner's parts)

NAMES = ("glass_blur", "snow", "elastic_transform")
UNBUILT = ("frost", "spatter")
SUBSETS = {"all": NAMES}
SEVERITY = {
    "glass_blur": ((0.7, 1, 2), (0.9, 2, 1), (1, 2, 3), (1.1, 3, 2), (1.5, 4, 2)),                  # sigma, delta, iterations
    # loc, scale, zoom, threshold, blur radius, blur sigma, keep
    "snow": ((0.1, 0.3, 3, 0.5, 10, 4, 0.8), (0.2, 0.3, 2, 0.5, 12, 4, 0.7), (0.55, 0.3, 4, 0.9, 12, 8, 0.7),
             (0.55, 0.3, 4.5, 0.85, 12, 8, 0.65), (0.55, 0.3, 2.5, 0.85, 12, 12, 0.55)),
    "elastic_transform": (250 * 0.05, 250 * 0.065, 250 * 0.085, 250 * 0.1, 250 * 0.12),             # alpha
}
DRAW_GLASS, DRAW_SNOW, DRAW_ELASTIC = 32, 40, 48   # csrc/distort.hip: glass iteration i takes 32 + 2 i (dy) and 33 + 2 i (dx)


def check_name(name: str) -> str:
    if name in UNBUILT:
        raise NotImplementedError(f"corruption {name!r} is not built (frost needs the reference's photographs, spatter its Canny / "
                                  f"distance-transform path; built here: {', '.join(NAMES)})")
    if name not in NAMES:
        hint = f"; {name!r} is unirestore_amd.corrupt's" if name in _cr.NAMES else \
            "; JPEG compression is unirestore_amd.jpeg's" if name == "jpeg_compression" else ""
        raise ValueError(f"unknown corruption {name!r}: choose from {', '.join(NAMES)}{hint}")
    return name


def expand(corruptions) -> list:
    """One name, "all", a comma-separated string or a list of names -> the corruptions it names, in order, each once."""
    if isinstance(corruptions, str):
        corruptions = [c for c in corruptions.split(",") if c]
    out = []
    for c in corruptions:
        members = list(SUBSETS[c]) if c in SUBSETS else [check_name(c)]
        out += [m for m in members if m not in out]
    if not out:
        raise ValueError("no corruption named")
    return out


def snow_angle(seed: int, stem: str) -> float:
    """The angle of an image's snow streaks in degrees, uniform in [-135, -45)."""
    return -135.0 + 90.0 * (_cr._hash64(f"{seed}\0corrupt\0{stem}\0snow_angle") >> 11) * 2.0 ** -53


def snow_geometry(h: int, w: int, zoom: float):
    """(top, left, ch, cw, oh, ow) of the reference's clipped_zoom: the centre crop ceil(H / zoom) x ceil(W / zoom) and the size
    round(ch zoom) x round(cw zoom) (round half to even) scipy.ndimage.zoom resamples it to; oh >= H and ow >= W."""
    return tuple(int(v) for v in _cr.zoom_layers(h, w, [zoom])[0])


def elastic_taps(h: int, w: int):
    """(taps along the height, taps along the width) of scipy.ndimage.gaussian_filter(sigma=(0.01 H, 0.01 W), truncate=3):
    normalised exp(-k^2 / 2 sigma^2), k = -r..r, r = int(3 sigma + 0.5), per axis."""
    out = []
    for n in (h, w):
        sigma = 0.01 * n
        r = int(3.0 * sigma + 0.5)
        t = np.exp(-0.5 / (sigma * sigma) * np.arange(-r, r + 1, dtype=np.float64) ** 2)
        out.append(t / t.sum())
    return tuple(out)


choose = _cr.choose                                # the (corruption, severity) of one image, as corrupt draws it


def distort(images_u8, name: str, severity: int, seeds, stems=None, out_kind: int = 0):
    """images_u8: device uint8 [N, H, W, 3] (H, W >= 32) -> the corrupted batch, uint8 (out_kind 1: the fp32 values before the
    floor).  seeds: one integer for the whole batch or one per image; stems: one name per image (default: empty names).  Image
    n's draws are keyed by corruption_seed(seeds[n], stems[n]) and its snow streaks lie along snow_angle(seeds[n], stems[n]): the
    result of an image does not depend on the batch around it."""
    import torch

    from . import ops
    from .resize import per_image
    check_name(name)
    sev = check_severity(severity)
    ops.check_u8_images("distort", images_u8)
    n, h, w, _ = images_u8.shape
    seeds, stems = per_image("distort", n, seeds, stems)
    dev = images_u8.device
    c = SEVERITY[name][sev - 1]

    def table(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keys = ops.noise_keys([corruption_seed(s, t) for s, t in zip(seeds, stems)]).to(dev)
    if name == "glass_blur":
        sigma, delta, iterations = c
        taps = table(gaussian_taps(sigma).astype(np.float32))
        a = ops.corrupt_filter_sep(images_u8, taps, 0)
        for i in range(iterations):
            a = ops.distort_shuffle(a, keys, delta, DRAW_GLASS + 2 * i)
        return ops.corrupt_filter_sep(a, taps, out_kind)
    if name == "snow":
        loc, scale, zoom, thr, radius, sigma, keep = c
        geometry = snow_geometry(h, w, zoom)
        field = ops.distort_snow_layer(keys, n, h, w, geometry, loc, scale, thr)
        lists = [motion_taps(geometry[4], geometry[5], radius, sigma, snow_angle(s, t)) for s, t in zip(seeds, stems)]
        taps = np.zeros((n, max(len(t) for t in lists), 3))                    # shorter lists end in weight-0 taps
        for i, t in enumerate(lists):
            taps[i, :len(t)] = t
        return ops.distort_snow(images_u8, field, table(pack_taps(taps)), keep, out_kind)
    ty, tx = elastic_taps(h, w)                                                 # elastic_transform
    field = ops.distort_field(keys, n, h, w, table(ty.astype(np.float32)), table(tx.astype(np.float32)), 0.005 * h, c)
    return ops.distort_warp(images_u8, field, out_kind)


def degrade(images_u8, name: str, severity: int, seeds, stems=None, resize=None):
    """`distort` as the reference degrades an image, exactly as corrupt.degrade: resize None is `distort` itself; resize = (lo, hi),
    lo >= 32, resizes image n so that its short edge is resize.draw_short_edge(seeds[n], stems[n], lo, hi), corrupts it at that
    size under its own seed and stem, and resizes it back: uint8 of the input's shape."""
    if resize is None:
        return distort(images_u8, name, severity, seeds, stems)
    from . import resize as rz
    check_name(name)
    check_severity(severity)
    return rz.inside(images_u8, seeds, stems, resize, lambda batch, s, t: distort(batch, name, severity, s, t), 32, "degrade")
