"""fp64 references and per-element bounds of the corruption kernels (csrc/corrupt.hip): the one statement of both; the tests
(test_corrupt_cpu.py, test_corrupt_gpu.py) only apply them.  numpy only; the keyed draws come from keyed_noise_reference.

Every function takes ONE image x uint8 [H, W, 3] and returns the fp64 value v on the 0-255 scale, clamped to [0, 255]; the 8-bit
result is floor(v).  The semantics are the reference project's ImageNet-C functions (skimage / scipy / OpenCV / Pillow calls restated
from their documentation), written here from the specification in include/unirestore_hip.h - nothing is shared with
unirestore_amd/corrupt.py except the Poisson table, which is an input (test_corrupt_cpu.py checks it against scipy).

Bounds on |fp32 value - fp64 value|, 0-255 scale (u = 2^-24, the unit roundoff of fp32; X = 255; nothing below is fitted to a kernel's
output; clamping is 1-Lipschitz, so a bound on v holds for clamp(v))

gaussian_noise   v = x + s n, s = fl(255 sigma).  The kernel's normal is within 1e-5 of the fp64 one (the keyed noise's own bound) and
                 |n| <= 5.77: s 1e-5 from the normal, u |s n| each for the rounding of s and of the product, u |v| for the sum:
                                  |err| <= 1e-5 s + 4 u (x + s |n|)
speckle_noise    v = x + x (c n): the same with s = c x:     |err| <= 1e-5 c x + 4 u (x + c x |n|)
impulse_noise    an integer decision on exact uniforms (the amount is compared as the fp32 number the kernel receives): 0.
shot_noise       k is an integer count of integer compares; v = fl(255 k / c) is one correctly rounded division: |err| <= u v, and
                 the floor is exact because 255 k / c is an integer or at least 1/60 away from one.
pixelate         integers throughout: 0.
gaussian_blur    two passes of n = 2 r + 1 taps.  A pass computes fl(sum_k fl(w_k) t_k) by sequential (fused or not) accumulation:
                 with non-negative weights that sum to 1 and |t| <= X the standard bound is (n + 1) u X (n - 1 additions, the
                 products, the rounding of the taps); the second pass passes the first's error on with gain 1 and adds its own:
                                  |err| <= 2 (n + 2) u X
defocus_blur     one sum of T = 289 or 441 non-negative taps of total weight S (S <= 1.02: the reflected smoothing of a disk that
motion_blur      touches its grid's edge gains a little), motion: T <= 41, S <= 1:      |err| <= (T + 2) u S X
zoom_blur        per layer: the cell is exact (integer division); fx, fy are one rounding each; a = p0 + fx (p1 - p0) makes three
                 roundings of values <= X (3 u X), b likewise, b - a inherits 6 u X and rounds once, fy (b - a) and the sum round
                 once each: <= 12 u X per layer.  K layers are added to x one by one, partial sums <= (K + 1) X: K (K + 1) u X.
                 After the division by K + 1 (one more rounding, u X):  (12 K + K (K + 1)) u X / (K + 1) + u X <=
                                  |err| <= (K + 14) u X
contrast         v = (x - m) a + m with m = fl(exact mean): u X for m (entering twice with opposite signs, net factor 1 - a), and
                 one rounding each for the difference, the product and the sum:       |err| <= 5 u X
brightness       S = delta / V: one rounding (<= u).  h6 = base + q, |q| <= 1: u for the quotient, 4 u for the sum (half an ulp
saturate         below 8); the + 6 of a negative hue is the only sum in that case: |h6 err| <= 5 u, and f = h6 - floor(h6) is exact.
                 The output is continuous and piecewise linear in h6 with slope <= V S <= X, so a floor that falls on the other
                 side of an integer changes nothing beyond that slope.  saturate: S' = clamp(S a + b), 3 u (the unclamped value is
                 <= 1 where it matters); brightness: V' = clamp(V + fl(255 c)): 2 u X.  p = V (1 - S): 5 u X; q = V (1 - f S): f S
                 carries 5 u + 3 u + u, the difference and the product one rounding each: 11 u X; t = V (1 - (1 - f) S): 12 u X;
                 plus V's own 2 u X:                                               |err| <= 16 u X
fog              map: a new cell is fl(fl(sum of 4) / 4 + r).  With A = max |map| the three additions err <= 3 u A after the
                 division, r = fl(w fl(w t)) with w = fl(wibble), t exact: 4 u w^2, the last sum u (A + w^2); the average passes
                 older errors on with gain 1.  Two dependent steps per level (squares, then diamonds), L = log2 M levels,
                 sum_l w_l^2 <= 1e4 / (1 - decay^-2) =: Q:           E = 8 L u A + 10 u Q   on every cell.
                 f = (map - lo) / (hi - lo) with R = hi - lo: numerator and denominator err <= 2 E + u R each, one division:
                 |f err| <= 4 E / R + 3 u.  v = (x + c f) g, g = m / (m + c) <= 1 (3 u from c, the sum and the division):
                                  |err| <= c (4 E / R + 3 u) + 9 u (X + c)
                 A and R are the fp64 map's own maximum magnitude and range.
"""
import math

import numpy as np

import keyed_noise_reference as kn

U = 2.0 ** -24
X = 255.0
DRAW = {"gaussian_noise": 16, "speckle_noise": 17, "impulse_flip": 18, "impulse_salt": 19, "shot_noise": 20, "fog": 21}
EXACT = ("impulse_noise", "shot_noise", "pixelate")        # the 8-bit result must equal the reference's everywhere

# severity constants (index severity - 1), restated from the reference's corruptions.py
C = {
    "gaussian_noise": (0.08, 0.12, 0.18, 0.26, 0.38), "speckle_noise": (0.15, 0.2, 0.35, 0.45, 0.6),
    "impulse_noise": (0.03, 0.06, 0.09, 0.17, 0.27), "shot_noise": (60, 25, 12, 5, 3), "gaussian_blur": (1, 2, 3, 4, 6),
    "defocus_blur": ((3, 0.1), (4, 0.5), (6, 0.5), (8, 0.5), (10, 0.5)), "motion_blur": ((10, 3), (15, 5), (15, 8), (15, 12), (20, 15)),
    "zoom_blur": (np.arange(1, 1.11, 0.01), np.arange(1, 1.16, 0.01), np.arange(1, 1.21, 0.02), np.arange(1, 1.26, 0.02),
                  np.arange(1, 1.31, 0.03)),
    "fog": ((1.5, 2), (2.0, 2), (2.5, 1.7), (2.5, 1.5), (3.0, 1.4)), "contrast": (0.4, 0.3, 0.2, 0.1, 0.05),
    "brightness": (0.1, 0.2, 0.3, 0.4, 0.5), "saturate": ((0.3, 0), (0.1, 0), (2, 0), (5, 0.1), (20, 0.2)),
    "pixelate": (0.6, 0.5, 0.4, 0.3, 0.25),
}
NAMES = tuple(C)


def _f32(v):
    return float(np.float32(v))


def _clip(v):
    return np.clip(v, 0.0, X)


# ------------------------------------------------------------------------------------------ noise
def gaussian_noise(x, sev, key):
    x = x.astype(np.float64)
    s = _f32(X * C["gaussian_noise"][sev - 1])
    n = kn.normals(key, DRAW["gaussian_noise"], x.size).reshape(x.shape)
    return _clip(x + s * n), 1e-5 * s + 4 * U * (x + s * np.abs(n))


def speckle_noise(x, sev, key):
    x = x.astype(np.float64)
    c = _f32(C["speckle_noise"][sev - 1])
    n = kn.normals(key, DRAW["speckle_noise"], x.size).reshape(x.shape)
    return _clip(x + x * (c * n)), 1e-5 * c * x + 4 * U * (x + c * x * np.abs(n))


def impulse_noise(x, sev, key):
    amount = _f32(C["impulse_noise"][sev - 1])
    u1 = kn.uniforms(kn.words(key, DRAW["impulse_flip"], x.size)).reshape(x.shape)
    u2 = kn.uniforms(kn.words(key, DRAW["impulse_salt"], x.size)).reshape(x.shape)
    return np.where(u1 < amount, np.where(u2 < 0.5, X, 0.0), x.astype(np.float64)), np.zeros(x.shape)


def shot_noise(x, sev, key, table):
    """table: uint32 [256, 128], T[x][k] = floor(2^24 CDF(k)) of Poisson(x c / 255)."""
    c = C["shot_noise"][sev - 1]
    v24 = (kn.words(key, DRAW["shot_noise"], x.size) >> np.uint32(8)).reshape(x.shape)
    k = np.zeros(x.shape, dtype=np.int64)
    for value in np.unique(x):                      # the number of entries <= v in a non-decreasing row
        at = x == value
        k[at] = np.searchsorted(table[value], v24[at], side="right")
    k = np.minimum(k, 127)
    v = _clip(k * X / c)
    return v, U * v


# ------------------------------------------------------------------------------------------ blur
def gaussian_taps(sigma):
    r = int(4 * sigma + 0.5)
    w = np.exp(-np.arange(-r, r + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return w / w.sum()


def _take(v, idx, axis):
    return np.take(v, idx, axis=axis)


def filter_axis(v, taps, axis):
    """sum_k taps[k + r] v[clamp(i + k)] along `axis` (replicate border)."""
    r, n = len(taps) // 2, v.shape[axis]
    return sum(taps[k + r] * _take(v, np.clip(np.arange(n) + k, 0, n - 1), axis) for k in range(-r, r + 1))


def gaussian_blur(x, sev):
    taps = gaussian_taps(C["gaussian_blur"][sev - 1])
    v = filter_axis(filter_axis(x.astype(np.float64), taps, 0), taps, 1)
    return _clip(v), np.full(x.shape, 2 * (len(taps) + 2) * U * X)


def reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def disk_kernel(radius, alias):
    half, ks = (8, 3) if radius <= 8 else (radius, 5)
    g = np.arange(-half, half + 1)
    k = ((g[None, :] ** 2 + g[:, None] ** 2) <= radius ** 2).astype(np.float64)
    k /= k.sum()
    t = np.exp(-(np.arange(ks) - (ks - 1) / 2.0) ** 2 / (2.0 * alias ** 2))
    t /= t.sum()
    n = len(g)
    for axis in (1, 0):                             # a separable Gaussian, reflect-101 border
        k = sum(t[d + ks // 2] * _take(k, reflect101(np.arange(n) + d, n), axis) for d in range(-(ks // 2), ks // 2 + 1))
    return k


def correlate_reflect101(v, k):
    """sum_{i,j} k[i][j] v[reflect(y + i - r)][reflect(x + j - r)] per channel (cv2.filter2D's default border)."""
    r, (h, w) = k.shape[0] // 2, v.shape[:2]
    out = np.zeros(v.shape)
    for i in range(k.shape[0]):
        rows = _take(v, reflect101(np.arange(h) + i - r, h), 0)
        for j in range(k.shape[1]):
            if k[i, j] != 0.0:
                out += k[i, j] * _take(rows, reflect101(np.arange(w) + j - r, w), 1)
    return out


def defocus_blur(x, sev):
    k = disk_kernel(*C["defocus_blur"][sev - 1])
    return _clip(correlate_reflect101(x.astype(np.float64), k)), np.full(x.shape, (k.size + 2) * U * k.sum() * X)


def motion_angle(seed, stem):
    import hashlib
    word = int.from_bytes(hashlib.sha256(f"{seed}\0corrupt\0{stem}\0angle".encode()).digest()[:8], "little")
    return -45.0 + 90.0 * (word >> 11) * 2.0 ** -53


def motion_shifts(h, w, radius, sigma, angle):
    """[(dx, dy, weight)] of the reference's _motion_blur: the image shifted by (dx, dy) with its edge repeated, weights normalised
    over all 2 radius + 1 taps, the loop left at the first shift that reaches the image's size."""
    width = 2 * radius + 1
    k = np.array([math.exp(-(i * i) / (2.0 * sigma * sigma)) / (math.sqrt(2 * math.pi) * sigma) for i in range(width)])
    k /= k.sum()
    py, px = width * math.sin(math.radians(angle)), width * math.cos(math.radians(angle))
    hyp = math.hypot(py, px)
    out = []
    for i in range(width):
        dy, dx = -math.ceil(i * py / hyp - 0.5), -math.ceil(i * px / hyp - 0.5)
        if abs(dy) >= h or abs(dx) >= w:
            break
        out.append((dx, dy, k[i]))
    return out


def motion_blur(x, sev, angle):
    h, w = x.shape[:2]
    v, out, total = x.astype(np.float64), np.zeros(x.shape), 0.0
    shifts = motion_shifts(h, w, *C["motion_blur"][sev - 1], angle)
    for dx, dy, wt in shifts:                       # shifted[y][x] = image[clamp(y - dy)][clamp(x - dx)]
        rows = _take(v, np.clip(np.arange(h) - dy, 0, h - 1), 0)
        out += wt * _take(rows, np.clip(np.arange(w) - dx, 0, w - 1), 1)
        total += wt
    return _clip(out), np.full(x.shape, (len(shifts) + 2) * U * total * X)


def zoom_layer(v, z):
    """The reference's clipped_zoom followed by its [:H, :W] crop: the centre crop ceil(H/z) x ceil(W/z) resampled bilinearly to
    round(ch z) x round(cw z) (scipy.ndimage.zoom, order 1: output index o reads input position o (in - 1) / (out - 1)).  Pixels
    the resampled crop does not reach stay 0."""
    h, w = v.shape[:2]
    ch, cw = int(np.ceil(h / float(z))), int(np.ceil(w / float(z)))
    top, left = (h - ch) // 2, (w - cw) // 2
    crop = v[top:top + ch, left:left + cw]
    oh, ow = int(round(ch * z)), int(round(cw * z))

    def axis_weights(n_in, n_out, n_used):
        pos = np.arange(min(n_out, n_used)) * (n_in - 1) / (n_out - 1)
        i0 = np.minimum(np.floor(pos).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), pos - i0

    y0, y1, fy = axis_weights(ch, oh, h)
    x0, x1, fx = axis_weights(cw, ow, w)
    rows = crop[y0] * (1 - fy)[:, None, None] + crop[y1] * fy[:, None, None]
    lay = rows[:, x0] * (1 - fx)[None, :, None] + rows[:, x1] * fx[None, :, None]
    out = np.zeros(v.shape)
    out[:lay.shape[0], :lay.shape[1]] = lay
    return out


def zoom_blur(x, sev):
    v, factors = x.astype(np.float64), C["zoom_blur"][sev - 1]
    out = (v + sum(zoom_layer(v, z) for z in factors)) / (len(factors) + 1)
    return _clip(out), np.full(x.shape, (len(factors) + 14) * U * X)


# ------------------------------------------------------------------------------------------ weather
def plasma_map(m, decay, key):
    """The reference's plasma_fractal on an m x m map before its normalisation, every cell's uniform keyed by the cell's index."""
    u = kn.uniforms(kn.words(key, DRAW["fog"], m * m)).reshape(m, m)
    a = np.zeros((m, m))
    step, wib = m, 100.0
    while step >= 2:
        wf, half = _f32(wib), step // 2

        def term(rows, cols):
            return wf * (wf * (2.0 * u[rows][:, cols] - 1.0))
        corner = a[0:m:step, 0:m:step]
        sq = corner + np.roll(corner, -1, 0)
        sq = sq + np.roll(sq, -1, 1)
        c_idx, h_idx = np.arange(0, m, step), np.arange(half, m, step)
        a[half:m:step, half:m:step] = sq / 4 + term(h_idx, h_idx)
        dr, ul = a[half:m:step, half:m:step], a[0:m:step, 0:m:step]
        a[0:m:step, half:m:step] = ((dr + np.roll(dr, 1, 0)) + (ul + np.roll(ul, -1, 1))) / 4 + term(c_idx, h_idx)
        a[half:m:step, 0:m:step] = ((dr + np.roll(dr, 1, 1)) + (ul + np.roll(ul, -1, 0))) / 4 + term(h_idx, c_idx)
        step //= 2
        wib /= decay
    return a


def fog(x, sev, key):
    c, decay = C["fog"][sev - 1]
    h, w = x.shape[:2]
    m = 1 << (max(h, w, 32) - 1).bit_length()
    raw = plasma_map(m, decay, key)
    lo, hi = raw.min(), raw.max()
    f = ((raw - lo) / (hi - lo))[:h, :w, None]
    c255, mx = _f32(X * c), float(x.max())
    v = (x.astype(np.float64) + c255 * f) * (mx / (mx + c255))
    levels = m.bit_length() - 1
    e_map = 8 * levels * U * np.abs(raw).max() + 10 * U * 1e4 / (1 - decay ** -2.0)
    return _clip(v), np.full(x.shape, c255 * (4 * e_map / (hi - lo) + 3 * U) + 9 * U * (X + c255))


# ------------------------------------------------------------------------------------------ digital
def contrast(x, sev):
    a = _f32(C["contrast"][sev - 1])
    v = x.astype(np.float64)
    mean = v.reshape(-1, 3).sum(0) / (x.shape[0] * x.shape[1])                  # integers below 2^53: exact
    return _clip((v - mean) * a + mean), np.full(x.shape, 5 * U * X)


def rgb2hsv(rgb):
    """skimage.color.rgb2hsv on [..., 3] (any scale: H and S are ratios, V keeps the scale)."""
    rgb = np.asarray(rgb, dtype=np.float64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    v = rgb.max(-1)
    delta = v - rgb.min(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(delta == 0, 0.0, delta / v)
        hue = np.where(r == v, (g - b) / delta, 0.0)
        hue = np.where(g == v, 2.0 + (b - r) / delta, hue)           # later assignments win, as in skimage
        hue = np.where(b == v, 4.0 + (r - g) / delta, hue)
    hue = np.where(delta == 0, 0.0, (hue / 6.0) % 1.0)
    return np.stack([hue, s, v], -1)


def hsv2rgb(hsv):
    """skimage.color.hsv2rgb."""
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    hi = np.floor(h * 6.0)
    f = h * 6.0 - hi
    p, q, t = v * (1 - s), v * (1 - f * s), v * (1 - (1 - f) * s)
    hi = hi.astype(np.int64) % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    return np.stack([np.choose(hi, [row[k] for row in table]) for k in range(3)], -1)


def brightness(x, sev):
    hsv = rgb2hsv(x)
    hsv[..., 2] = np.clip(hsv[..., 2] + _f32(X * C["brightness"][sev - 1]), 0, X)
    return _clip(hsv2rgb(hsv)), np.full(x.shape, 16 * U * X)


def saturate(x, sev):
    a, b = C["saturate"][sev - 1]
    hsv = rgb2hsv(x)
    hsv[..., 1] = np.clip(hsv[..., 1] * _f32(a) + _f32(b), 0, 1)
    return _clip(hsv2rgb(hsv)), np.full(x.shape, 16 * U * X)


def box_reduce(v, n_out, axis):
    """Pillow's BOX reduction of an integer array along `axis`, rounded half up to integers."""
    n_in = v.shape[axis]
    scale = n_in / n_out
    cols = []
    for xx in range(n_out):
        centre = (xx + 0.5) * scale
        lo, hi = max(int(centre - scale / 2 + 0.5), 0), min(int(centre + scale / 2 + 0.5), n_in)
        on = [i for i in range(lo, hi) if -0.5 < (i + 0.5 - centre) / scale <= 0.5]
        s = _take(v, on, axis).sum(axis)
        cols.append((2 * s + len(on)) // (2 * len(on)))              # floor(mean + 0.5) in integers
    return np.stack(cols, axis)


def nearest_index(n_small, n_large):
    s = n_small / n_large
    pos, out = 0.5 * s, []
    for _ in range(n_large):
        out.append(min(int(pos), n_small - 1))
        pos += s
    return np.array(out)


def pixelate(x, sev):
    c = C["pixelate"][sev - 1]
    h, w = x.shape[:2]
    sh, sw = int(h * c), int(w * c)
    small = box_reduce(box_reduce(x.astype(np.int64), sw, 1), sh, 0)
    return small[nearest_index(sh, h)][:, nearest_index(sw, w)].astype(np.float64), np.zeros(x.shape)


def run(name, x, sev, key=None, angle=None, table=None):
    """(value fp64 [H, W, 3], bound [H, W, 3]) of corruption `name` at severity `sev`; key = the image's 64-bit corruption seed,
    angle = its motion-blur angle in degrees, table = the Poisson table of the severity's constant (shot_noise)."""
    if name == "shot_noise":
        return shot_noise(x, sev, key, table)
    if name in ("gaussian_noise", "speckle_noise", "impulse_noise", "fog"):
        return globals()[name](x, sev, key)
    if name == "motion_blur":
        return motion_blur(x, sev, angle)
    return globals()[name](x, sev)
