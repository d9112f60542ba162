"""ImageNet-C style corruptions of clean 8-bit images on the GPU (csrc/corrupt.hip; the kernels' specification is the ur_corrupt_*
comment of include/unirestore_hip.h, the derivations are DESIGN.md 6q).

The names, severity constants and subsets are the reference's (src/data/corruption).  Thirteen corruptions are built; the other six
names raise NotImplementedError.  This module is the planner: it builds the small tables a corruption needs on the host in fp64
(Gaussian taps, the defocus disk, motion taps, zoom layers, the Poisson table, the pixelate tables) and launches the primitives of
`ops`.  An image's randomness is a pure function of (seed, stem): `corruption_seed` keys the device draws, `motion_angle` is the one
host scalar.  `corrupt` works at the size it is given; `degrade` is `corrupt` inside the reference's resize-down / resize-back
wrapper (unirestore_amd.resize.inside) when a short-edge range is given, and `corrupt` itself when none is.
"""
import hashlib
import math
import os
from functools import lru_cache

import numpy as np

# the reference's order (corruption_tuple): subsets are slices of it
ALL = ("gaussian_noise", "shot_noise", "impulse_noise", "defocus_blur", "glass_blur", "motion_blur", "zoom_blur", "snow", "frost",
       "fog", "brightness", "contrast", "elastic_transform", "pixelate", "jpeg_compression", "speckle_noise", "gaussian_blur",
       "spatter", "saturate")
UNBUILT = ("glass_blur", "snow", "frost", "spatter", "elastic_transform", "jpeg_compression")
NAMES = tuple(n for n in ALL if n not in UNBUILT)
SUBSETS = {"common": ALL[:15], "validation": ALL[15:], "all": ALL, "noise": ALL[0:3], "blur": ALL[3:7], "weather": ALL[7:11],
           "digital": ALL[11:15]}
SEVERITY = {
    "gaussian_noise": (0.08, 0.12, 0.18, 0.26, 0.38),
    "speckle_noise": (0.15, 0.2, 0.35, 0.45, 0.6),
    "impulse_noise": (0.03, 0.06, 0.09, 0.17, 0.27),
    "shot_noise": (60, 25, 12, 5, 3),
    "gaussian_blur": (1, 2, 3, 4, 6),
    "defocus_blur": ((3, 0.1), (4, 0.5), (6, 0.5), (8, 0.5), (10, 0.5)),
    "motion_blur": ((10, 3), (15, 5), (15, 8), (15, 12), (20, 15)),
    "zoom_blur": ((1.11, 0.01), (1.16, 0.01), (1.21, 0.02), (1.26, 0.02), (1.31, 0.03)),      # np.arange(1, end, step)
    "fog": ((1.5, 2), (2.0, 2), (2.5, 1.7), (2.5, 1.5), (3.0, 1.4)),
    "contrast": (0.4, 0.3, 0.2, 0.1, 0.05),
    "brightness": (0.1, 0.2, 0.3, 0.4, 0.5),
    "saturate": ((0.3, 0), (0.1, 0), (2, 0), (5, 0.1), (20, 0.2)),
    "pixelate": (0.6, 0.5, 0.4, 0.3, 0.25),
}
MIXED_P = (0.05, 0.25, 0.4, 0.25, 0.05)           # the reference's per-image severity draw
NOISE_MODES = {"gaussian_noise": 0, "speckle_noise": 1, "impulse_noise": 2, "shot_noise": 3}
COLOR_MODES = {"contrast": 0, "brightness": 1, "saturate": 2}


def _hash64(text: str) -> int:
    return int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "little")


def corruption_seed(seed: int, stem: str) -> int:
    """The 64-bit seed of every device draw of the image named `stem` (distinct from cli.image_seed: the corruption and the model
    noise of one file are unrelated)."""
    return _hash64(f"{seed}\0corrupt\0{stem}")


def motion_angle(seed: int, stem: str) -> float:
    """The motion-blur angle of an image in degrees, uniform in [-45, 45)."""
    return -45.0 + 90.0 * (_hash64(f"{seed}\0corrupt\0{stem}\0angle") >> 11) * 2.0 ** -53


def check_name(name: str) -> str:
    if name in UNBUILT:
        hint = "; JPEG compression is a module of its own: unirestore_amd.jpeg.roundtrip, `cli jpeg`" if name == "jpeg_compression" else \
            "; it is built in a module of its own: unirestore_amd.distort.distort, `cli distort`" if name in ("glass_blur", "snow", "elastic_transform") else ""
        raise NotImplementedError(f"corruption {name!r} is not built (built: {', '.join(NAMES)}){hint}")
    if name not in NAMES:
        raise ValueError(f"unknown corruption {name!r}: choose from {', '.join(NAMES)}")
    return name


def check_severity(severity) -> int:
    if isinstance(severity, bool) or not isinstance(severity, int) or not 1 <= severity <= 5:
        raise ValueError(f"severity must be an integer in [1, 5], got {severity!r}")
    return severity


def expand(corruptions) -> list:
    """A subset name, one corruption name, a comma-separated string or a list of names -> the built corruptions it names, in order,
    each once ("clean" only when it is named).  A subset drops its unbuilt members (`skipped` lists them); an unbuilt corruption
    named directly raises NotImplementedError."""
    if isinstance(corruptions, str):
        corruptions = [c for c in corruptions.split(",") if c]
    out = []
    for c in corruptions:
        members = [m for m in SUBSETS[c] if m not in UNBUILT] if c in SUBSETS else [c if c == "clean" else check_name(c)]
        out += [m for m in members if m not in out]
    if not out:
        raise ValueError("no corruption named")
    return out


def skipped(corruptions) -> list:
    """The unbuilt members of the subsets in `corruptions` (see `expand`)."""
    if isinstance(corruptions, str):
        corruptions = [c for c in corruptions.split(",") if c]
    out = []
    for c in corruptions:
        out += [m for m in SUBSETS.get(c, ()) if m in UNBUILT and m not in out]
    return out


def draw_severity(seed: int, stem: str) -> int:
    """The reference's per-image severity draw (p = MIXED_P over 1..5) from sha256 of (seed, stem)."""
    u = (_hash64(f"{seed}\0corrupt\0{stem}\0severity") >> 11) * 2.0 ** -53
    return 1 + min(int(np.searchsorted(np.cumsum(MIXED_P), u, side="right")), 4)


def choose(seed: int, stem: str, names, severity):
    """The (corruption, severity) of one image from sha256 of (seed, stem) alone: a uniform pick from `names`, and for severity
    "mixed" `draw_severity`."""
    name = names[_hash64(f"{seed}\0corrupt\0{stem}\0choice") % len(names)]
    return name, draw_severity(seed, stem) if severity == "mixed" else check_severity(severity)


# ------------------------------------------------------------------------------------------ host-side builders (fp64)
def gaussian_taps(sigma: float) -> np.ndarray:
    """Normalised taps exp(-k^2 / 2 sigma^2), k = -r..r, r = int(4 sigma + 0.5) (scipy.ndimage.gaussian_filter, truncate = 4)."""
    r = int(4.0 * sigma + 0.5)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return w / w.sum()


def reflect101(i: np.ndarray, n: int) -> np.ndarray:
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def disk_kernel(radius: int, alias: float) -> np.ndarray:
    """The defocus kernel: the 0 / 1 disk of `radius` on a 17 x 17 grid (radius <= 8) or (2 radius + 1)^2, normalised, smoothed by a
    separable 3-tap (5-tap for radius > 8) Gaussian of sigma `alias` with a reflect-101 border."""
    half, ks = (8, 3) if radius <= 8 else (radius, 5)
    g = np.arange(-half, half + 1)
    xx, yy = np.meshgrid(g, g)
    k = (xx ** 2 + yy ** 2 <= radius ** 2).astype(np.float64)
    k /= k.sum()
    d = np.arange(ks) - (ks - 1) / 2.0
    t = np.exp(-d ** 2 / (2.0 * alias * alias))
    t /= t.sum()
    n = k.shape[0]
    idx = reflect101(np.arange(n)[:, None] + (np.arange(ks) - ks // 2)[None, :], n)          # [n, ks]
    k = (k[:, idx] * t).sum(-1)                    # along x
    return (k[idx, :] * t[None, :, None]).sum(1)   # along y


def kernel_taps(k: np.ndarray) -> np.ndarray:
    """A correlation kernel [n, n] (anchor at its centre) -> the tap list [(tx, ty, w)] in row-major order."""
    n = k.shape[0]
    r = n // 2
    return np.array([(j - r, i - r, k[i, j]) for i in range(n) for j in range(n)], dtype=np.float64)


def motion_taps(h: int, w: int, radius: int, sigma: float, angle: float) -> np.ndarray:
    """The reference's _motion_blur as a tap list [(tx, ty, weight)]: 2 radius + 1 Gaussian weights along the direction `angle`
    (degrees), normalised over ALL of them; the list ends before the first tap whose shift reaches the image's height or width,
    and what is dropped is not made up for.  (tx, ty) = (-dx, -dy): shifting the image by dx reads the pixel at x - dx."""
    width = 2 * radius + 1
    i = np.arange(width, dtype=np.float64)
    k = np.exp(-(i ** 2) / (2.0 * sigma ** 2)) / (math.sqrt(2.0 * math.pi) * sigma)
    k = k / k.sum()
    p0, p1 = width * math.sin(math.radians(angle)), width * math.cos(math.radians(angle))
    hyp = math.hypot(p0, p1)
    taps = []
    for t in range(width):
        dy, dx = -math.ceil(t * p0 / hyp - 0.5), -math.ceil(t * p1 / hyp - 0.5)
        if abs(dy) >= h or abs(dx) >= w:
            break
        taps.append((-dx, -dy, k[t]))
    return np.array(taps, dtype=np.float64).reshape(-1, 3)


def zoom_factors(severity: int) -> np.ndarray:
    end, step = SEVERITY["zoom_blur"][check_severity(severity) - 1]
    return np.arange(1, end, step)


def zoom_layers(h: int, w: int, factors) -> np.ndarray:
    """int32 [K, 6] = (top, left, ch, cw, oh, ow) per factor z: the centre crop ceil(H/z) x ceil(W/z) and the size round(ch z) x
    round(cw z) scipy.ndimage.zoom resamples it to."""
    rows = []
    for z in factors:
        ch, cw = int(np.ceil(h / float(z))), int(np.ceil(w / float(z)))
        rows.append(((h - ch) // 2, (w - cw) // 2, ch, cw, int(round(ch * z)), int(round(cw * z))))
    return np.array(rows, dtype=np.int32)


@lru_cache(maxsize=8)
def poisson_table(c: int) -> np.ndarray:
    """uint32 [256, 128]: T[x][k] = floor(2^24 CDF(k)) of Poisson(x c / 255).  A 24-bit uniform integer v maps to the number of k
    with T[x][k] <= v (at most 127): integer compares only.  The mass beyond k = 127 is 3.2e-14 at the largest mean, 60."""
    lam = np.arange(256, dtype=np.float64)[:, None] * c / 255.0
    k = np.arange(128, dtype=np.float64)[None, :]
    lgam = np.cumsum(np.log(np.maximum(k, 1.0)), axis=1)                       # ln k!
    with np.errstate(divide="ignore", invalid="ignore"):
        pmf = np.exp(-lam + k * np.log(lam) - lgam)
    pmf[0] = 0.0
    pmf[0, 0] = 1.0                                 # mean 0: all the mass at k = 0
    fwd = np.cumsum(pmf, axis=1)
    tail = np.cumsum(pmf[:, ::-1], axis=1)[:, ::-1] - pmf                       # the mass above k: accurate where the CDF is near 1
    cdf = np.where(fwd <= 0.5, fwd, 1.0 - tail)
    return np.floor(cdf * 2.0 ** 24).astype(np.uint32)


def box_table(n_in: int, n_out: int) -> np.ndarray:
    """int32 [n_out, 2] = (first, count) of the source indices Pillow's BOX filter gives weight 1 when it reduces n_in to n_out."""
    scale = n_in / n_out
    rows = []
    for xx in range(n_out):
        centre = (xx + 0.5) * scale
        lo, hi = max(int(centre - scale / 2 + 0.5), 0), min(int(centre + scale / 2 + 0.5), n_in)
        on = [x for x in range(lo, hi) if -0.5 < (x + 0.5 - centre) / scale <= 0.5]
        rows.append((on[0], len(on)))
    return np.array(rows, dtype=np.int32)


def nearest_table(n_small: int, n_large: int) -> np.ndarray:
    """int32 [n_large]: the source index of Pillow's NEAREST enlargement, with the position accumulated step by step as Pillow
    does (the closed form (x + 0.5) s differs in a few columns at odd sizes)."""
    s = n_small / n_large
    pos, out = 0.5 * s, []
    for _ in range(n_large):
        out.append(min(int(pos), n_small - 1))
        pos += s
    return np.array(out, dtype=np.int32)


def pixelate_tables(h: int, w: int, c: float):
    """(small_h, small_w, hbox, vbox, ymap, xmap) of PIL's resize((int(W c), int(H c)), BOX) then resize((W, H), NEAREST)."""
    sh, sw = int(h * c), int(w * c)
    return sh, sw, box_table(w, sw), box_table(h, sh), nearest_table(sh, h), nearest_table(sw, w)


def pack_taps(taps: np.ndarray) -> np.ndarray:
    """[..., T, 3] (tx, ty, w) in fp64 -> int32 [..., T, 3] with the fp32 bits of w in the third column (ur_corrupt_taps)."""
    out = np.empty(taps.shape, dtype=np.int32)
    out[..., :2] = taps[..., :2].astype(np.int32)
    out[..., 2] = taps[..., 2].astype(np.float32).view(np.int32)
    return out


# ------------------------------------------------------------------------------------------ plan and launch
def corrupt(images_u8, name: str, severity: int, seeds, stems=None, out_kind: int = 0):
    """images_u8: device uint8 [N, H, W, 3] (H, W >= 32) -> the corrupted batch, uint8 (out_kind 1: the fp32 values before the
    floor).  seeds: one integer for the whole batch or one per image; stems: one name per image (default: empty names).  Image
    n's draws are keyed by corruption_seed(seeds[n], stems[n]) and its motion-blur angle is motion_angle(seeds[n], stems[n]):
    the result of an image does not depend on the batch around it.  "clean" returns the input."""
    import torch

    from . import ops
    from .resize import per_image
    if name == "clean":
        return images_u8.float() if out_kind else images_u8.clone()
    check_name(name)
    sev = check_severity(severity)
    ops.check_u8_images("corrupt", images_u8)
    n, h, w, _ = images_u8.shape
    seeds, stems = per_image("corrupt", n, seeds, stems)
    dev = images_u8.device
    c = SEVERITY[name][sev - 1]

    def table(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def keys():
        return ops.noise_keys([corruption_seed(s, t) for s, t in zip(seeds, stems)]).to(dev)

    if name in NOISE_MODES:
        mode = NOISE_MODES[name]
        scale = 255.0 * c if mode == 0 else float(c)
        return ops.corrupt_noise(images_u8, keys(), mode, scale, table(poisson_table(c).view(np.int32)) if mode == 3 else None, out_kind)
    if name == "gaussian_blur":
        return ops.corrupt_filter_sep(images_u8, table(gaussian_taps(c).astype(np.float32)), out_kind)
    if name == "defocus_blur":
        return ops.corrupt_taps(images_u8, table(pack_taps(kernel_taps(disk_kernel(*c)))), border=1, out_kind=out_kind)
    if name == "motion_blur":
        lists = [motion_taps(h, w, c[0], c[1], motion_angle(s, t)) for s, t in zip(seeds, stems)]
        taps = np.zeros((n, max(len(t) for t in lists), 3))                    # shorter lists end in weight-0 taps
        for i, t in enumerate(lists):
            taps[i, :len(t)] = t
        return ops.corrupt_taps(images_u8, table(pack_taps(taps)), border=0, out_kind=out_kind)
    if name == "zoom_blur":
        return ops.corrupt_zoom(images_u8, table(zoom_layers(h, w, zoom_factors(sev))), out_kind)
    if name in COLOR_MODES:
        a, b = (c, 0.0) if name == "contrast" else (255.0 * c, 0.0) if name == "brightness" else c
        return ops.corrupt_color(images_u8, COLOR_MODES[name], a, b, out_kind)
    if name == "pixelate":
        sh, sw, hbox, vbox, ymap, xmap = pixelate_tables(h, w, c)
        return ops.corrupt_pixelate(images_u8, sh, sw, table(hbox), table(vbox), table(ymap), table(xmap), out_kind)
    return ops.corrupt_fog(images_u8, keys(), 255.0 * c[0], c[1], out_kind)      # fog


def degrade(images_u8, name: str, severity: int, seeds, stems=None, resize=None):
    """`corrupt` as the reference degrades an image (IRCorruptDataset._degrade_image).  resize None: `corrupt` itself.  resize =
    (lo, hi), lo >= 32: image n is resized so that its short edge is resize.draw_short_edge(seeds[n], stems[n], lo, hi)
    (torchvision's rule for a one-element size, antialiased bilinear on the bytes), corrupted at that size under its own seed and
    stem, and resized back: uint8 of the input's shape.  "clean" returns the input unresized, as the reference does."""
    if resize is None or name == "clean":
        return corrupt(images_u8, name, severity, seeds, stems)
    from . import resize as rz
    check_name(name)
    check_severity(severity)
    return rz.inside(images_u8, seeds, stems, resize, lambda batch, s, t: corrupt(batch, name, severity, s, t), 32, "degrade")


# ------------------------------------------------------------------------------------------ files
def clean_inputs(source: str) -> list:
    """A folder -> its image files sorted by name; a list file -> the clean image of every line: the `hq` column of an `lq hq
    [label]` line, the only column otherwise (paths relative to the list file's folder)."""
    from . import imageio
    if os.path.isdir(source):
        return imageio.list_inputs(source)
    if not os.path.isfile(source):
        raise FileNotFoundError(f"{source!r}: no such folder or list file")
    base = os.path.dirname(os.path.abspath(source))
    out = []
    with open(source) as f:
        for line in f:
            cols = line.split()
            if cols and not cols[0].startswith("#"):
                p = cols[1] if len(cols) >= 2 else cols[0]
                out.append(p if os.path.isabs(p) else os.path.join(base, p))
    return out


def stem_of(path: str) -> str:
    return os.path.splitext(os.path.basename(path))[0]


def check_inputs(source: str) -> list:
    """The clean image paths of `source`, checked: at least one, all present, no two with the same stem."""
    paths = clean_inputs(source)
    if not paths:
        raise ValueError(f"{source!r}: no image file found")
    missing = [p for p in paths if not os.path.isfile(p)]
    if missing:
        raise FileNotFoundError(f"{source!r}: {len(missing)} listed file(s) do not exist, first {missing[0]!r}")
    stems = {}
    for p in paths:
        if stem_of(p) in stems:
            raise ValueError(f"{source!r}: {stems[stem_of(p)]!r} and {p!r} share the stem {stem_of(p)!r} (it names the output and seeds the draws)")
        stems[stem_of(p)] = p
    return paths


def plan_files(paths, sizes, names, severity, seed: int, batch_size: int):
    """[(corruption, severity, [indices])]: every file's (corruption, severity) from `choose`, files grouped by (shape, corruption,
    severity) in input order, groups cut into batches, batches ordered by their first member."""
    groups = {}
    for i, (p, hw) in enumerate(zip(paths, sizes)):
        name, sev = choose(seed, stem_of(p), names, severity)
        groups.setdefault((tuple(hw), name, sev), []).append(i)
    cuts = [(k[1], k[2], idx[s:s + batch_size]) for k, idx in groups.items() for s in range(0, len(idx), batch_size)]
    cuts.sort(key=lambda c: c[2][0])
    return cuts
