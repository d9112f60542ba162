"""fp64 references and per-element bounds of the colour fix kernels (csrc/colorfix.hip): the one statement of both; the tests
(test_colorfix_cpu.py, test_colorfix_gpu.py) only apply them.  numpy only.

Arrays are [..., H, W, 3]: `c` the decoder's conv_out output (fp32 values), `s` the encoder's input x0 (16-bit values), both widened
to fp64 here.  Every function works per image and channel over the whole H x W canvas.

wavelet    out = c + L(s - c),  L = B_16 B_8 B_4 B_2 B_1,  B_r(v)[y, x] = sum_{i,j in {-1,0,1}} k_i k_j v[clamp(y + i r), clamp(x + j r)],
           k = (1/4, 1/2, 1/4), clamp to the canvas at EVERY level.  B_r is linear (clamping is an index map), so this equals the usual
           a-trous statement `wavelet_atrous`: (c - L c) + L s, the restored image's high frequencies on the input's level-5 low band.
adain      out = (c - mu_c) (sigma_s / sigma_c) + mu_s,  sigma = sqrt(var + 1e-5), var unbiased (divided by P - 1), P = H W.

Bounds (u = 2^-24, the unit roundoff of fp32; nothing below is fitted to a kernel's output)

wavelet    The kernel forms d = fl(s - c) (s widens exactly): one rounding, |error| <= u M with M = max |s - c| over the image.  Each
           of the ten 1-D passes computes fl(fl(lo + hi) / 4 + mid / 2): the scalings by powers of two are exact, so a pass makes two
           rounded additions of values <= 2 M and <= M, each error <= u M after its scaling (u 2M / 4 and u M), and - a convex
           combination has gain <= 1 - passes the error it received on unchanged: <= 2 u M per pass, 20 u M over ten.  The last
           operation fl(c + L d) rounds a value <= max|c| + M once.  First order total: 21 u M + u (max|c| + M) = 22 u M + u max|c|;
           stated as            |out - ref| <= 24 u (M + max|c|)
           which leaves the second-order terms ((1 + u)^22 - 1 - 22 u < 3e-13) far inside the spare 2 u M.
adain      The statistics pass sums in fp64: per thread at most 64 pixels in sequence, then a 6-step butterfly, 3 additions across
           the waves and one sequential addition per 16384-pixel part in the finalize - a chain of D <= 80 + P / 16384 additions, so a
           relative error <= D 2^-53 on sum and sum of squares.  With |x| <= ~1 and sigma^2 >= 1e-5 that moves sigma by less than
           D 2^-53 (1 + mu^2 / sigma^2) / 2 <= 1e-14 1e5 = 1e-9 relative for any canvas below 2^24 pixels: 0.02 u.  What is left is fp32:
           a_f = fl(a) and b_f = fl(b) (a = sigma_s / sigma_c, b = mu_s - a mu_c): |a_f - a| <= u |a|, |b_f - b| <= u |b|;
           the product fl(a_f c): u |a c|; the sum: u (|a c| + |b|) (a fused multiply-add makes only this last rounding).
           First order total u (3 |a c| + 2 |b|); stated per element as
                                |out - ref| <= 4 u (|a c| + |b|)
           with the spare u (|a c| + 2 |b|) over the statistics term and the second-order terms.
"""
import numpy as np

U = 2.0 ** -24
LEVELS = (1, 2, 4, 8, 16)
HALO = sum(LEVELS)                         # 31
EPS = 1e-5


def _shift(v, off, axis):
    """v[clamp(i + off)] along `axis` (replicate border)."""
    n = v.shape[axis]
    return np.take(v, np.clip(np.arange(n) + off, 0, n - 1), axis=axis)


def blur_axis(v, r, axis):
    return 0.25 * (_shift(v, -r, axis) + _shift(v, r, axis)) + 0.5 * v          # a constant comes back exactly


def blur(v, r):
    """B_r on [..., H, W, C]."""
    return blur_axis(blur_axis(v, r, -3), r, -2)


def low(v):
    """L = B_16 ... B_1, clamped at every level."""
    v = np.asarray(v, dtype=np.float64)
    for r in LEVELS:
        v = blur(v, r)
    return v


def wavelet(c, s):
    c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
    return c + low(s - c)


def wavelet_atrous(c, s):
    """The usual statement: high frequencies of the restored image + level-5 low frequencies of the input."""
    c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
    return (c - low(c)) + low(s)


def composed_taps():
    """The 63 weights of the five dilated kernels convolved with each other (offsets -31 .. 31)."""
    w = np.ones(1)
    for r in LEVELS:
        k = np.zeros(2 * r + 1)
        k[0], k[r], k[2 * r] = 0.25, 0.5, 0.25
        w = np.convolve(w, k)
    return w


def low_single_clamp(v):
    """NOT the definition: one 63-tap filter per axis with ONE clamp.  Equal to `low` more than 31 pixels from every border, different
    near one (clamp(clamp(x + 2) - 1) != clamp(x + 1)): the cases must be able to tell the two apart."""
    v = np.asarray(v, dtype=np.float64)
    w = composed_taps()
    for axis in (-3, -2):
        v = sum(w[t + HALO] * _shift(v, t, axis) for t in range(-HALO, HALO + 1))
    return v


def wavelet_bound(c, s):
    """Per-element bound of `wavelet`, one value per image: [..., 1, 1, 1]."""
    c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
    m = np.abs(s - c).max(axis=(-3, -2, -1), keepdims=True)
    return 24 * U * (m + np.abs(c).max(axis=(-3, -2, -1), keepdims=True))


def emulate_wavelet_f32(c, s):
    """The kernel's arithmetic in its own order, in numpy fp32: d = s - c; the five vertical levels, then the five horizontal ones,
    each fl(fl(lo + hi) / 4 + mid / 2); out = fl(c + L d).  Strips and halos do not change a value, so the whole canvas at once."""
    c = np.asarray(c, dtype=np.float32)
    v = np.asarray(s, dtype=np.float32) - c
    q, h = np.float32(0.25), np.float32(0.5)
    for axis in (-3, -2):
        for r in LEVELS:
            t = _shift(v, -r, axis) + _shift(v, r, axis)
            v = q * t + h * v
            assert v.dtype == np.float32
    return c + v


def emulate_wavelet_strips_f32(c, s, vr=66, hr=4, hc=66, halo=HALO):
    """The kernel's strips, step by step, in numpy fp32 ([N,H,W,3]): pass 1 runs the vertical levels on windows of vr rows plus a halo
    that ends at the image edge, every tap clamped to the window, and keeps the vr owned rows; pass 2 walks each band of hr rows left
    to right in steps of hc columns, in place: the left halo comes from a carry of the previous step's pass-1 columns, the right halo
    from memory.  Must equal `emulate_wavelet_f32` bit for bit: strips, halos and the in-place walk change no value."""
    c = np.asarray(c, dtype=np.float32)
    d = np.asarray(s, dtype=np.float32) - c
    n, h, w, _ = c.shape
    q, half = np.float32(0.25), np.float32(0.5)

    def levels(win, axis):
        for r in LEVELS:
            win = q * (_shift(win, -r, axis) + _shift(win, r, axis)) + half * win
        return win
    out = np.full_like(c, np.nan)
    for y0 in range(0, h, vr):
        g0, g1 = max(0, y0 - halo), min(h, y0 + vr + halo)
        own = min(vr, h - y0)
        out[:, y0:y0 + own] = levels(d[:, g0:g1], 1)[:, y0 - g0:y0 - g0 + own]
    for y0 in range(0, h, hr):
        band = out[:, y0:y0 + hr]                                # a view: stores below land in `out`, as in the kernel
        carry = None
        for x0 in range(0, w, hc):
            g0, g1 = max(0, x0 - halo), min(w, x0 + hc + halo)
            lead = x0 - g0
            win = np.concatenate([carry[:, :, :lead], band[:, :, x0:g1]], axis=2) if lead else band[:, :, x0:g1].copy()
            if x0 + hc < w:
                carry = win[:, :, lead + hc - halo:lead + hc].copy()
            own = min(hc, w - x0)
            band[:, :, x0:x0 + own] = c[:, y0:y0 + hr, x0:x0 + own] + levels(win, 2)[:, :, lead:lead + own]
    return out


def adain_coefficients(c, s):
    """fp64 (a, b) per image and channel, [..., 1, 1, 3]: out = a c + b."""
    c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
    ax = (-3, -2)
    mu_c, mu_s = c.mean(axis=ax, keepdims=True), s.mean(axis=ax, keepdims=True)
    sd_c = np.sqrt(c.var(axis=ax, ddof=1, keepdims=True) + EPS)
    sd_s = np.sqrt(s.var(axis=ax, ddof=1, keepdims=True) + EPS)
    a = sd_s / sd_c
    return a, mu_s - a * mu_c


def adain(c, s):
    c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
    ax = (-3, -2)
    mu_c, mu_s = c.mean(axis=ax, keepdims=True), s.mean(axis=ax, keepdims=True)
    sd_c = np.sqrt(c.var(axis=ax, ddof=1, keepdims=True) + EPS)
    sd_s = np.sqrt(s.var(axis=ax, ddof=1, keepdims=True) + EPS)
    return (c - mu_c) * (sd_s / sd_c) + mu_s


def adain_bound(c, s):
    """Per-element bound of `adain`, the shape of c."""
    c = np.asarray(c, dtype=np.float64)
    a, b = adain_coefficients(c, s)
    return 4 * U * (np.abs(a * c) + np.abs(b))


def fix(mode, c, s):
    return {"wavelet": wavelet, "adain": adain}[mode](c, s)


def bound(mode, c, s):
    return {"wavelet": wavelet_bound, "adain": adain_bound}[mode](c, s)
