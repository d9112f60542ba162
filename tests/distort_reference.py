"""fp64 references, per-element bounds and ambiguity masks of glass blur, snow and elastic transform (csrc/distort.hip): the one
statement of all three; the tests (test_distort_cpu.py, test_distort_gpu.py) only apply them.  numpy only; the keyed draws come from
keyed_noise_reference, the Gaussian taps / replicate filter / motion shifts that the older corruptions already state from
corrupt_reference.  Nothing is shared with unirestore_amd/distort.py.

Every stage takes ONE image (x uint8 [H, W, 3]) or one image's field and returns fp64 values with a bound on |fp32 - fp64| per
element.  The semantics are the reference project's glass_blur / snow / elastic_transform (skimage / scipy calls restated from their
documentation; test_distort_cpu.py holds them against scipy itself), written from the specification in include/unirestore_hip.h.
u = 2^-24 is the unit roundoff of fp32, X = 255; nothing below is fitted to a kernel's output; clamping is 1-Lipschitz, so a bound on
v holds for clamp(v); a fused multiply-add only removes a rounding.

Quantisation steps are not covered by widening a tolerance but by an AMBIGUITY MASK: an element whose fp64 value +- its bound
straddles the decision is ambiguous, the mask holds the size of the jump the other decision would make, the mask is pushed through
the later linear stages (gather, non-negative taps, the mirror) in fp64 like a value, and what arrives is added to the bound.

gaussian (u8 in)  corrupt_reference's gaussian_blur: two passes of n = 2 r + 1 non-negative taps that sum to 1:  2 (n + 2) u X.
glass floor       a = floor(g): ambiguous where floor(g - b) != floor(g + b); jump 1.
shuffle           a gather of whole pixels by exact integers: 0.  It moves values and mask alike.
glass_blur        gaussian(shuffled a) carries its own 2 (n + 2) u X plus gaussian(shuffled mask).
snow layer        l = loc + s n with the kernel's normal within 1e-5 of the fp64 one and |l| <= A := loc + 5.77 s: the product and
                  the sum round once each, e0 = 1e-5 s + 2 u A.  The cell of the bilinear sample is exact (integers); fx, fy are one
                  rounding each (u, times a difference <= 2 A).  a = p0 + fx (p1 - p0): the difference, the product (2 u A each), the
                  sum (u A) and fx's own 2 u A: 7 u A, while the e0 of p0, p1 pass with weights (1 - fx) + fx = 1.  v = a + fy (b - a)
                  repeats that with a, b in the place of p0, p1:       |err| <= e0 + 14 u A = 1e-5 s + 16 u A =: e_l
snow threshold    v < thr (thr as the fp32 number the kernel receives): ambiguous where |v - thr| <= e_l; jump = clamp(v), on
                  the 0-255 scale 255 clamp(v).  Elsewhere the clamped value keeps e_l - except where v + e_l < thr (0 on both
                  sides) or v - e_l >= 1 (1 on both sides): those cells, most of a layer, are exact.
snow blur         s = sum of T <= 41 non-negative taps of total weight S <= 1 over field values in [0, 1]: (T + 2) u S, plus the
                  same taps applied to the cells' own errors e_in (S e_in when all cells carry the same); r = 255 s rounds once
                  more:                                          e_r = 255 ((T + 2) u S + taps(e_in)) + u X
                  plus 255 * (the taps applied to the threshold mask).
snow rint         L = rint(r), half to even: ambiguous where rint(r - e_r) != rint(r + e_r).  |rint(p) - rint(q)| <= |p - q| + 1,
                  so the jump is e_r + 1 (1 when the field is exact and e_r is a few 1e-4).
snow blend        g = c_R R + c_G G + c_B B (the three fp32 coefficients; products u X in total, two sums 2 u X): 3 u X.
                  t = 1.5 g + 127.5 <= 2 X: 1.5 * 3 u X carried, u 1.5 X and u 2 X for the product and the sum: 8 u X, and so has
                  max(x, t).  keep x: u X.  (1 - keep) max: u for the difference and u for the product, both times 2 X, plus the
                  8 u X carried: 12 u X.  Their sum <= 2 X: 2 u X.  L + L' is an exact integer <= 2 X, the last sum <= 4 X: 4 u X.
                                  |err| <= 19 u X (20 u X is used) + mask[y][x] + mask[H-1-y][W-1-x]
elastic field     f = m (2u - 1) with m the fp32 number the kernel receives: u m.  A pass of n taps: (n + 1) u m as for the
                  Gaussian above, the earlier error passing with gain 1; the product with alpha (fp32, as received) rounds once:
                                  |err| <= (n_y + n_x + 6) u m alpha
warp              the position p = fl(y + d) is off by u |p| plus the field's own error e_f.  The reflected bilinear surface is
                  continuous and piecewise linear with slope <= X along each axis, so a position error - also one that crosses into
                  the next cell - costs X times itself.  f = p - floor(p) is exact.  a = p0 + fx (p1 - p0) with an exact
                  difference: 2 u X; b - a: 4 u X carried + u X; fy (b - a): + u X; the last sum: 2 u X + 6 u X + u X = 9 u X:
                                  |err| <= X (u (|py| + |px|) + e_fy + e_fx) + 10 u X
"""
import hashlib
import math

import numpy as np

import corrupt_reference as cref
import keyed_noise_reference as kn

U = 2.0 ** -24
X = 255.0
DRAW = {"glass": 32, "snow": 40, "elastic_dy": 48, "elastic_dx": 49}       # glass: iteration i takes 32 + 2 i (dy) and 33 + 2 i (dx)

# severity constants (index severity - 1), restated from the reference's corruptions.py
C = {
    "glass_blur": ((0.7, 1, 2), (0.9, 2, 1), (1, 2, 3), (1.1, 3, 2), (1.5, 4, 2)),                  # sigma, delta, iterations
    "snow": ((0.1, 0.3, 3, 0.5, 10, 4, 0.8), (0.2, 0.3, 2, 0.5, 12, 4, 0.7), (0.55, 0.3, 4, 0.9, 12, 8, 0.7),
             (0.55, 0.3, 4.5, 0.85, 12, 8, 0.65), (0.55, 0.3, 2.5, 0.85, 12, 12, 0.55)),    # loc, scale, zoom, thr, radius, sigma, keep
    "elastic_transform": tuple(250 * a for a in (0.05, 0.065, 0.085, 0.1, 0.12)),
}
NAMES = tuple(C)
GREY = (0.299, 0.587, 0.114)


def _f32(v):
    return float(np.float32(v))


def _clip(v):
    return np.clip(v, 0.0, X)


# ------------------------------------------------------------------------------------------ glass blur
def gaussian_u8(a, sigma):
    """(clamped fp64 value, bound) of skimage's gaussian (truncate 4, `nearest` border) of an integer image on the 0-255 scale."""
    taps = cref.gaussian_taps(sigma)
    v = cref.filter_axis(cref.filter_axis(a.astype(np.float64), taps, 0), taps, 1)
    return _clip(v), 2 * (len(taps) + 2) * U * X


def floor_mask(v, bound):
    """1.0 where floor(v - bound) != floor(v + bound) inside [0, 255] (the two floors are then one apart), else 0.0."""
    return (np.floor(_clip(v - bound)) != np.floor(_clip(v + bound))).astype(np.float64)


def shuffle_offsets(h, w, key, delta, draw):
    """(dy, dx) int64 [H, W]: ((word * 2 delta) >> 32) - delta of element y W + x of draws `draw` / `draw + 1`; 0 outside the
    interior delta <= y < H - delta, delta <= x < W - delta."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    inside = (yy >= delta) & (yy < h - delta) & (xx >= delta) & (xx < w - delta)
    out = []
    for d in (draw, draw + 1):
        word = kn.words(key, d, h * w).astype(np.uint64).reshape(h, w)
        out.append(np.where(inside, ((word * np.uint64(2 * delta)) >> np.uint64(32)).astype(np.int64) - delta, 0))
    return out


def shuffle(a, key, delta, draw):
    """One iteration of the reference's vectorised glass shuffle on [H, W, ...]: every interior pixel takes the whole pixel at
    (y + dy, x + dx) of `a`; the border is copied."""
    h, w = a.shape[:2]
    dy, dx = shuffle_offsets(h, w, key, delta, draw)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return a[yy + dy, xx + dx]


def glass_blur(x, sev, key):
    """-> (value fp64 [H, W, 3], bound, info): info["share"] = the share of ambiguous elements of the intermediate floor,
    info["mask"] = the propagated mask (already inside the bound)."""
    sigma, delta, iterations = C["glass_blur"][sev - 1]
    g, b = gaussian_u8(x, sigma)
    a, mask = np.floor(g), floor_mask(g, b)
    share = float(mask.mean())
    for i in range(iterations):
        a, mask = shuffle(a, key, delta, DRAW["glass"] + 2 * i), shuffle(mask, key, delta, DRAW["glass"] + 2 * i)
    v, b2 = gaussian_u8(a, sigma)
    taps = cref.gaussian_taps(sigma)
    mask = cref.filter_axis(cref.filter_axis(mask, taps, 0), taps, 1)
    return v, b2 + mask, dict(share=share, mask=mask)


# ------------------------------------------------------------------------------------------ snow
def snow_angle(seed, stem):
    word = int.from_bytes(hashlib.sha256(f"{seed}\0corrupt\0{stem}\0snow_angle".encode()).digest()[:8], "little")
    return -135.0 + 90.0 * (word >> 11) * 2.0 ** -53


def snow_geometry(h, w, zoom):
    """(top, left, ch, cw, oh, ow) of clipped_zoom: the centre crop ceil(H / z) x ceil(W / z), resampled by scipy.ndimage.zoom to
    round(ch z) x round(cw z) (Python's round: half to even)."""
    ch, cw = int(math.ceil(h / float(zoom))), int(math.ceil(w / float(zoom)))
    return (h - ch) // 2, (w - cw) // 2, ch, cw, int(round(ch * float(zoom))), int(round(cw * float(zoom)))


def zoom_linear(crop, oh, ow):
    """scipy.ndimage.zoom(order=1) of [ch, cw] to [oh, ow]: output index o reads position o (in - 1) / (out - 1); the cell in
    integers, as the kernel takes it."""
    def axis(n_in, n_out):
        num = np.arange(n_out) * (n_in - 1)
        i0 = num // (n_out - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), (num - i0 * (n_out - 1)) / (n_out - 1)
    y0, y1, fy = axis(crop.shape[0], oh)
    x0, x1, fx = axis(crop.shape[1], ow)
    a = crop[y0][:, x0] + fx[None, :] * (crop[y0][:, x1] - crop[y0][:, x0])
    b = crop[y1][:, x0] + fx[None, :] * (crop[y1][:, x1] - crop[y1][:, x0])
    return a + fy[:, None] * (b - a)


def snow_layer(h, w, sev, key):
    """Steps 1-3 -> (field fp64 [oh, ow] in [0, 1], bound e_l, ambiguous bool [oh, ow], kept = the clamped value an ambiguous cell
    has on the branch that keeps it: the field itself holds the reference's own decision, exact bool [oh, ow] = the cells whose
    fp32 value IS the reference's: v + e_l < thr gives 0 and v - e_l >= 1 gives 1 in both)."""
    loc, scale, zoom, thr = C["snow"][sev - 1][:4]
    loc, scale, thr = _f32(loc), _f32(scale), _f32(thr)
    top, left, ch, cw, oh, ow = snow_geometry(h, w, zoom)
    layer = loc + scale * kn.normals(key, DRAW["snow"], h * w).reshape(h, w)
    v = zoom_linear(layer[top:top + ch, left:left + cw], oh, ow)
    e_l = 1e-5 * scale + 16 * U * (loc + kn.MAX_ABS * scale)
    kept = np.clip(v, 0.0, 1.0)
    return np.where(v < thr, 0.0, kept), e_l, np.abs(v - thr) <= e_l, kept, (v + e_l < thr) | (v - e_l >= 1.0)


def taps_clamped(field, shifts):
    """sum_t w_t field[clamp(y - dy_t)][clamp(x - dx_t)] over the whole field (the reference's _motion_blur: shifts with the edge
    repeated) and the total weight."""
    oh, ow = field.shape
    out, total = np.zeros(field.shape), 0.0
    for dx, dy, wt in shifts:
        rows = np.take(field, np.clip(np.arange(oh) - dy, 0, oh - 1), axis=0)
        out += wt * np.take(rows, np.clip(np.arange(ow) - dx, 0, ow - 1), axis=1)
        total += wt
    return out, total


def snow_blend(x, field, shifts, keep, field_err=0.0, field_mask=None):
    """Steps 4-6 from a given field [oh, ow] -> (value fp64 [H, W, 3], bound, info).  field_err: a bound on the error the field's
    cells carry, one number or one per cell (0 for a field handed to the kernel as it is); field_mask: the jump (0-1 scale) of its
    ambiguous cells.
    info: share = the share of ambiguous roundings among the H x W cells of L, mask = the propagated mask [H, W]."""
    h, w = x.shape[:2]
    keep = _f32(keep)
    s, total = taps_clamped(field, shifts)
    r = X * s
    e_in = taps_clamped(field_err, shifts)[0] if isinstance(field_err, np.ndarray) else total * field_err
    e_r = X * ((len(shifts) + 2) * U * total + e_in) + U * X
    if field_mask is not None:
        e_r = e_r + X * taps_clamped(field_mask, shifts)[0]
    r, e_r = r[:h, :w], np.broadcast_to(e_r, s.shape)[:h, :w]
    amb = np.rint(_clip(r - e_r)) != np.rint(_clip(r + e_r))
    lay = np.rint(_clip(r))                        # np.rint: half to even, as rintf
    mask = np.where(amb, e_r + 1.0, 0.0)
    xv = x.astype(np.float64)
    grey = sum(_f32(c) * xv[..., k] for k, c in enumerate(GREY))[..., None]
    v = keep * xv + (1.0 - keep) * np.maximum(xv, 1.5 * grey + 127.5) + (lay + lay[::-1, ::-1])[..., None]
    mask2 = (mask + mask[::-1, ::-1])[..., None]
    return _clip(v), 20 * U * X + np.broadcast_to(mask2, x.shape), dict(share=float(amb.mean()), mask=mask2[..., 0])


def snow(x, sev, key, angle):
    """-> (value, bound, info): info["share"] = the larger of the ambiguous shares of the threshold and of the rounding."""
    h, w = x.shape[:2]
    radius, sigma, keep = C["snow"][sev - 1][4:]
    field, e_l, amb, kept, exact = snow_layer(h, w, sev, key)
    shifts = cref.motion_shifts(field.shape[0], field.shape[1], radius, sigma, angle)
    v, bound, info = snow_blend(x, field, shifts, keep, np.where(exact, 0.0, e_l), np.where(amb, kept, 0.0))
    return v, bound, dict(share=max(info["share"], float(amb.mean())), mask=info["mask"])


# ------------------------------------------------------------------------------------------ elastic transform
def reflect_sym(i, n):
    """Half-sample-symmetric reflection (d c b a | a b c d | d c b a), periodic: scipy's `reflect`."""
    p = np.mod(i, 2 * n)
    return np.where(p < n, p, 2 * n - 1 - p)


def elastic_taps(n):
    """scipy.ndimage.gaussian_filter1d's kernel for sigma = 0.01 n, truncate = 3."""
    sigma = 0.01 * n
    r = int(3.0 * sigma + 0.5)
    t = np.exp(-np.arange(-r, r + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return t / t.sum()


def filter_reflect(v, taps, axis):
    r, n = len(taps) // 2, v.shape[axis]
    return sum(taps[k + r] * np.take(v, reflect_sym(np.arange(n) + k, n), axis=axis) for k in range(-r, r + 1))


def elastic_field(h, w, sev, key):
    """Steps 1-2 -> (field fp64 [2, H, W] = (dy, dx), bound)."""
    m, alpha = _f32(0.005 * h), _f32(C["elastic_transform"][sev - 1])
    ty, tx = elastic_taps(h), elastic_taps(w)
    planes = []
    for draw in (DRAW["elastic_dy"], DRAW["elastic_dx"]):
        f = m * (2.0 * kn.uniforms(kn.words(key, draw, h * w)).reshape(h, w) - 1.0)
        planes.append(alpha * filter_reflect(filter_reflect(f, ty, 0), tx, 1))
    return np.stack(planes), (len(ty) + len(tx) + 6) * U * m * alpha


def warp(x, field, field_err=0.0):
    """Step 3: map_coordinates(order=1, mode="reflect") of every channel at (y + dy, x + dx) -> (value fp64 [H, W, 3], bound)."""
    h, w = x.shape[:2]
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    py, px = yy + field[0], xx + field[1]
    iy, ix = np.floor(py), np.floor(px)
    fy, fx = (py - iy)[..., None], (px - ix)[..., None]
    y0, y1 = reflect_sym(iy.astype(np.int64), h), reflect_sym(iy.astype(np.int64) + 1, h)
    x0, x1 = reflect_sym(ix.astype(np.int64), w), reflect_sym(ix.astype(np.int64) + 1, w)
    v = x.astype(np.float64)
    a = v[y0, x0] + fx * (v[y0, x1] - v[y0, x0])
    b = v[y1, x0] + fx * (v[y1, x1] - v[y1, x0])
    bound = X * (U * (np.abs(py) + np.abs(px)) + 2 * field_err) + 10 * U * X
    return _clip(a + fy * (b - a)), np.broadcast_to(bound[..., None], x.shape)


def elastic_transform(x, sev, key):
    """-> (value, bound, info): the warp of the fp64 field, whose bound (it covers the fp32 store) enters as the warp's e_f."""
    field, e_f = elastic_field(x.shape[0], x.shape[1], sev, key)
    v, bound = warp(x, field, e_f)
    return v, bound, dict(share=0.0, mask=np.zeros(x.shape[:2]))


def run(name, x, sev, key, angle=None):
    """(value fp64 [H, W, 3], bound [H, W, 3], info) of `name` at severity `sev`; key = the image's 64-bit corruption seed, angle =
    its snow angle in degrees."""
    if name == "snow":
        return snow(x, sev, key, angle)
    return globals()[name](x, sev, key)
