"""Case tables of the resize tests (test_resize_cpu.py, test_resize_gpu.py): (N, H, W) -> (oh, ow), image kinds, the refusals of the C
ABI.

Each case is the smallest at which a kernel of ur_resize_u8 can go wrong.  67 x 93 -> 23 x 32: a non-integer reduction, W * 3 = 279
no multiple of 4.  23 x 32 -> 67 x 93: an enlargement (support 1).  67 x 93 -> 66 x 94: one axis down, one up.  40 x 52 -> 40 x 31 and
-> 17 x 52: one pass skipped.  40 x 52 -> 40 x 52: a copy.  128 x 96 -> 8 x 6: 16 x, the largest K (33 bilinear, 65 bicubic).
32 x 32 -> 64 x 64.  N = 3 with three different images: the batch strides.
"""
import numpy as np

MODES = ("bilinear", "bicubic")
CASES = [((1, 67, 93), (23, 32)), ((1, 23, 32), (67, 93)), ((1, 67, 93), (66, 94)), ((1, 40, 52), (40, 31)), ((1, 40, 52), (17, 52)),
         ((1, 40, 52), (40, 52)), ((1, 128, 96), (8, 6)), ((1, 32, 32), (64, 64)), ((3, 45, 37), (29, 50))]
# the CPU cross-check of the restatement with torch runs these too: the issue's "four shapes x nine sizes" in small
CPU_SHAPES = [(1, 67, 93), (2, 40, 52), (1, 96, 128), (1, 33, 31)]
CPU_SIZES = [(23, 32), (134, 186), (66, 94), (40, 31), (17, 52), (24, 32), (192, 256), (2, 2), (50, 47)]
KINDS = ("random", "checker", "zeros", "white")


def images(shape, kind="random"):
    """uint8 [N, H, W, 3]: uniform random; a 1-pixel 0 / 255 checkerboard (G in opposite phase, every other image inverted);
    constant 0; constant 255 (the rounded weights do not always sum to 2^p: a constant need not come back constant)."""
    n, h, w = shape
    if kind == "zeros":
        return np.zeros((n, h, w, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((n, h, w, 3), 255, dtype=np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        c = (((yy + xx) & 1) * 255).astype(np.uint8)
        one = np.stack([c, 255 - c, c], -1)
        return np.ascontiguousarray(np.stack([one if i % 2 == 0 else 255 - one for i in range(n)]))
    return np.random.default_rng(9000 * h + 9 * w + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


# ---- refusals: one wrong argument in an otherwise valid call (placeholder pointers: nothing is launched) ----------------------------
_X, _O, _T, _WS = 0x10000, 0x20000, 0x30000, 0x50000
ORDER = ("x", "out", "N", "H", "W", "oh", "ow", "xb", "xw", "xK", "xp", "yb", "yw", "yK", "yp", "ws", "ws_bytes", "stream")
VALID = dict(x=_X, out=_O, N=2, H=67, W=93, oh=23, ow=32, xb=_T, xw=_T + 0x1000, xK=9, xp=16, yb=_T + 0x2000, yw=_T + 0x3000, yK=9, yp=16,
             ws=_WS, ws_bytes=None, stream=None)                     # None: the exact need
WRONG = [("null x", dict(x=None)), ("null out", dict(out=None)), ("null workspace", dict(ws=None)), ("null width bounds", dict(xb=None)),
         ("null width weights", dict(xw=None)), ("null height bounds", dict(yb=None)), ("null height weights", dict(yw=None)),
         ("N = 0", dict(N=0)), ("N < 0", dict(N=-1)), ("H = 1", dict(H=1)), ("W = 1", dict(W=1)), ("oh = 1", dict(oh=1)), ("ow = 1", dict(ow=1)),
         ("H < 0", dict(H=-67)), ("ow = 0", dict(ow=0)), ("width K = 0", dict(xK=0)), ("height K = 0", dict(yK=0)),
         ("width K too large", dict(xK=1 << 20)), ("width p = 0", dict(xp=0)), ("height p = 23", dict(yp=23)), ("width p < 0", dict(xp=-3)),
         ("workspace one byte short", dict(ws_bytes=-1)), ("workspace off 8 bytes", dict(ws=_WS + 4)), ("misaligned table", dict(xw=_T + 0x1002)),
         ("out == x", dict(out=_X)), ("2^31 elements", dict(N=4, H=16384, W=16384, ws_bytes=1 << 40)),
         ("2^31 output elements", dict(N=4, oh=16384, ow=16384, ws_bytes=1 << 40))]


def refusals(ws_bytes_of):
    """[(label, argument list)] of ur_resize_u8; ws_bytes_of(N, H, W, oh, ow) = ur_resize_u8_ws_bytes."""
    rows = []
    for label, kw in WRONG:
        a = dict(VALID)
        a.update({k: v for k, v in kw.items() if k != "ws_bytes"})
        need = ws_bytes_of(*(VALID[k] for k in ("N", "H", "W", "oh", "ow")))
        short = kw.get("ws_bytes")
        a["ws_bytes"] = need if short is None else need - 1 if short == -1 else short
        rows.append((label, [a[k] for k in ORDER]))
    return rows
