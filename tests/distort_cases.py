"""Case tables of the glass blur / snow / elastic transform tests (test_distort_cpu.py, test_distort_gpu.py): shapes, inputs, seeds,
the host-made inputs of the single stages and the refusals of the C ABI.

Shapes (N, H, W): corrupt_cases.SHAPES.  (1, 32, 32): the smallest size that is not refused; delta = 4 leaves a 24 x 24 interior and
the elastic radii are 1 and 1.  (2, 33, 47): odd sizes whose H * W is no multiple of 4 (the last Philox counter is partial); zoom 4.5
gives a snow layer of 36 rows (> H), and the elastic radii differ (1 and 2 at 33 x 47, 2 and 3 at 64 x 96).  (3, 40, 32): three
images (alone == image 2 of 3), H > W.  (1, 64, 96): several workgroups per image.
"""
import numpy as np

from corrupt_cases import KINDS, SHAPES, images, stems  # noqa: F401 (the corruption tests' own images)

# "two seeds per image": every case runs under both.  Under these two the share of ambiguous intermediate elements of every `random`
# case stays below the 1 % cap (test_distort_cpu.py asserts it on the reference alone; the largest is 0.63 %).  Two kinds of image
# exceed it, and one of each is kept as UNCAPPED, a case that runs end to end without the cap, so that what the masks are for is
# compared too.  Seed 7 at (1, 32, 32), severity 3: at this image's angle one tap has 255 w = 4.4996, so every cell whose streak
# meets a single clamped flake through that tap rounds within 5e-4 of a half (1.9 % of L).  Seed 131, severity 1: a cell of the
# layer lies within its 5e-6 of the threshold (about one 32 x 32 image in a hundred has one); its jump of 0.5 spreads along a whole
# streak and its mirror image (1.2 % of L).
SEED_SETS = (42, 11)
UNCAPPED = (("snow", (1, 32, 32), 3, 7), ("snow", (1, 32, 32), 1, 131))
SEVS = (1, 2, 3, 4, 5)
DELTAS = (1, 2, 3, 4)
DRAW_PAIRS = (32, 34, 36)                          # every (dy, dx) draw pair glass blur takes: (32, 33), (34, 35), (36, 37)


def snow_field(n, oh, ow, seed=0):
    """A host-made snow layer fp32 [N, oh, ow] in [0, 1]: mostly 0 (below the threshold), the rest spread over (0.5, 1], some
    cells exactly 1 (clamped): what ur_distort_snow_layer hands on, with every value present."""
    rng = np.random.default_rng(7000 + 100 * oh + ow + seed)
    f = rng.random((n, oh, ow))
    f = np.where(f < 0.7, 0.0, np.where(f > 0.97, 1.0, 0.5 + 0.5 * rng.random((n, oh, ow))))
    return f.astype(np.float32)


def warp_field(n, h, w, kind):
    """Host-made displacement fields fp32 [N, 2, H, W].  "zero": all zeros (the warp returns x).  "smooth": within 0.15 H, like
    the elastic fields.  "outward": every pixel is pushed away from the centre by 2.5 times its distance from it plus a fraction,
    so the samples of the border rows and columns lie outside EVERY edge, by more than one image size at the corners (the periodic
    part of the reflection)."""
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    if kind == "zero":
        f = np.zeros((n, 2, h, w))
    elif kind == "smooth":
        f = np.stack([np.stack([0.15 * h * np.sin(0.11 * yy + 0.07 * xx + i), 0.15 * h * np.cos(0.05 * yy - 0.13 * xx + i)]) for i in range(n)])
    else:
        rng = np.random.default_rng(50 + h + w)
        f = np.stack([np.stack([2.5 * (yy - (h - 1) / 2), 2.5 * (xx - (w - 1) / 2)]) + rng.random((2, h, w)) for _ in range(n)])
    return f.astype(np.float32)


# ---- refusals: one wrong argument in an otherwise valid call (placeholder pointers: nothing is launched) ----------------------------
_X, _O, _K, _T, _WS, _F = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
_ORDER = {
    "ur_distort_shuffle": ("x", "keys", "out", "N", "H", "W", "delta", "draw", "stream"),
    "ur_distort_snow_layer": ("keys", "field", "N", "H", "W", "top", "left", "ch", "cw", "oh", "ow", "loc", "scale", "thr", "stream"),
    "ur_distort_snow": ("x", "field", "taps", "n_taps", "out", "N", "H", "W", "oh", "ow", "keep", "ws", "ws_bytes", "out_kind", "stream"),
    "ur_distort_field": ("keys", "taps", "ry", "taps_x", "rx", "field", "N", "H", "W", "m", "alpha", "ws", "ws_bytes", "stream"),
    "ur_distort_warp": ("x", "field", "out", "N", "H", "W", "out_kind", "stream"),
}
_VALID = dict(x=_X, keys=_K, out=_O, field=_F, N=2, H=32, W=40, delta=2, draw=32, stream=None, top=10, left=13, ch=11, cw=14, oh=33, ow=42,
              loc=0.55, scale=0.3, thr=0.9, taps=_T, taps_x=_T + 256, n_taps=25, keep=0.7, ws=_WS, ws_bytes=1 << 24, out_kind=0, ry=1, rx=2,
              m=0.16, alpha=21.25)
_SHAPE = [("N = 0", dict(N=0)), ("N < 0", dict(N=-2)), ("H = 31", dict(H=31)), ("W = 31", dict(W=31)), ("H < 0", dict(H=-32)),
          ("W = 0", dict(W=0)), ("2^31 elements", dict(N=4, H=16384, W=16384, oh=16384, ow=16384))]
_IMAGE = [("null x", dict(x=None)), ("null out", dict(out=None)), ("out == x", dict(out=_X))] + _SHAPE
_OUT_KIND = [("out_kind = 2", dict(out_kind=2)), ("out_kind = -1", dict(out_kind=-1)), ("fp32 out off 4 bytes", dict(out=_O + 2, out_kind=1))]
_WS_WRONG = [("null workspace", dict(ws=None)), ("workspace off 8 bytes", dict(ws=_WS + 4)), ("workspace too small", dict(ws_bytes=8))]
_ENLARGED = [("oh < H", dict(oh=31)), ("ow < W", dict(ow=39)), ("oh > 32768", dict(oh=32769)), ("2^31 field cells", dict(oh=32768, ow=32768))]
_FIELD = [("null field", dict(field=None)), ("field off 4 bytes", dict(field=_F + 2))]
_ROWS = {
    "ur_distort_shuffle": _IMAGE + [("null keys", dict(keys=None)), ("delta = 0", dict(delta=0)), ("delta = 5", dict(delta=5)),
                                    ("delta < 0", dict(delta=-1)), ("draw + 1 overflows", dict(draw=0xFFFFFFFF))],
    "ur_distort_snow_layer": _SHAPE + _FIELD + _ENLARGED + [
        ("null keys", dict(keys=None)), ("top < 0", dict(top=-1)), ("left < 0", dict(left=-1)), ("ch = 0", dict(ch=0)), ("cw = 0", dict(cw=0)),
        ("crop below the image", dict(top=22)), ("crop right of the image", dict(left=27)), ("scale = 0", dict(scale=0.0))],
    "ur_distort_snow": _IMAGE + _OUT_KIND + _FIELD + _ENLARGED + _WS_WRONG + [
        ("null taps", dict(taps=None)), ("taps off 4 bytes", dict(taps=_T + 2)), ("n_taps = 0", dict(n_taps=0)), ("n_taps = 65", dict(n_taps=65)),
        ("keep < 0", dict(keep=-0.1)), ("keep > 1", dict(keep=1.5)), ("N = 65536", dict(N=65536, ws_bytes=1 << 30))],
    "ur_distort_field": _SHAPE + _FIELD + _WS_WRONG + [
        ("null keys", dict(keys=None)), ("null taps_y", dict(taps=None)), ("null taps_x", dict(taps_x=None)), ("taps_y off 4 bytes", dict(taps=_T + 1)),
        ("taps_x off 4 bytes", dict(taps_x=_T + 258)), ("ry < 0", dict(ry=-1)), ("rx = 256", dict(rx=256)), ("m < 0", dict(m=-1.0)),
        ("field == ws", dict(field=_WS))],
    "ur_distort_warp": _IMAGE + _OUT_KIND + _FIELD,
}
WS_BYTES = ("ur_distort_snow_ws_bytes", "ur_distort_field_ws_bytes")


def refusals():
    """[(label, export, argument list)]."""
    rows = []
    for fn, order in _ORDER.items():
        for label, kw in _ROWS[fn]:
            a = dict(_VALID)
            a.update(kw)
            rows.append((f"{fn}: {label}", fn, [a[k] for k in order]))
    return rows


def valid_calls():
    """[(export, argument list)] of the valid call every refusal differs from by one argument (never launched by the CPU tests)."""
    return [(fn, [_VALID[k] for k in order]) for fn, order in _ORDER.items()]
