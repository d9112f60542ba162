"""Case tables of the JPEG tests (test_jpeg_cpu.py, test_jpeg_gpu.py): shapes, image kinds, qualities, the refusals of the C ABI.

Shapes (N, H, W).  (1, 16, 16): one MCU, the smallest size accepted.  (2, 33, 47): both sizes odd, chroma edge replication in both
directions.  (3, 40, 32): H even and ch = 20, no multiple of 8: the reduced chroma rows 20..23 must copy row 19 (the padding-order
trap); three images.  (1, 64, 96): several MCUs, no padding.  (1, 17, 31).  (1, 48, 49): cw = 25.
"""
import numpy as np

SHAPES = [(1, 16, 16), (2, 33, 47), (3, 40, 32), (1, 64, 96), (1, 17, 31), (1, 48, 49)]
KINDS = ("smooth", "random", "zeros", "white", "ramp", "checker", "binary")
QUALITIES = (1, 7, 10, 15, 18, 25, 49, 50, 51, 75, 95, 100)
SUBSAMPLINGS = (2, 0)                              # Pillow's codes: 4:2:0, 4:4:4


def images(shape, kind="smooth"):
    """uint8 [N, H, W, 3]: smooth plus mild noise; uniform random; constant 0; constant 255; a grey ramp; a 1-pixel 0 / 255
    checkerboard with G in opposite phase (the inverse DCT's clamp and the colour clamp); random 0 / 255."""
    n, h, w = shape
    rng = np.random.default_rng(7000 * h + 7 * w + KINDS.index(kind))
    if kind == "zeros":
        return np.zeros((n, h, w, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((n, h, w, 3), 255, dtype=np.uint8)
    if kind == "ramp":
        ramp = np.linspace(0, 255, h * w).astype(np.uint8).reshape(1, h, w, 1)
        return np.ascontiguousarray(np.broadcast_to(ramp, (n, h, w, 3)))
    if kind == "random":
        return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (n, h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "checker":
        c = (((yy + xx) & 1) * 255).astype(np.uint8)
        one = np.stack([c, 255 - c, c], -1)
        return np.ascontiguousarray(np.stack([one if i % 2 == 0 else 255 - one for i in range(n)]))
    phase = rng.uniform(0, 6.28, (n, 1, 1, 3))
    freq = rng.uniform(0.05, 0.25, (n, 1, 1, 3))
    base = 128 + 90 * np.sin(freq * xx[None, :, :, None] + phase) * np.cos(0.7 * freq * yy[None, :, :, None] - phase)
    return np.clip(base + rng.normal(0, 4, (n, h, w, 3)), 0, 255).astype(np.uint8)


# ---- refusals: one wrong argument in an otherwise valid call (placeholder pointers: nothing is launched) ----------------------------
_X, _O, _WS = 0x10000, 0x20000, 0x50000
ORDER = ("x", "out", "N", "H", "W", "quality", "subsampling", "ws", "ws_bytes", "stream")
VALID = dict(x=_X, out=_O, N=2, H=33, W=47, quality=25, subsampling=2, ws=_WS, ws_bytes=None, stream=None)      # None: the exact need
WRONG = [("null x", dict(x=None)), ("null out", dict(out=None)), ("null workspace", dict(ws=None)), ("N = 0", dict(N=0)),
         ("N < 0", dict(N=-2)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("H < 0", dict(H=-33)), ("W < 0", dict(W=-47)),
         ("H = 15", dict(H=15)), ("W = 15", dict(W=15)), ("quality = 0", dict(quality=0)), ("quality = 101", dict(quality=101)),
         ("quality < 0", dict(quality=-5)), ("subsampling = 1", dict(subsampling=1)), ("subsampling = 3", dict(subsampling=3)),
         ("subsampling = -1", dict(subsampling=-1)), ("workspace one byte short", dict(ws_bytes=-1)),
         ("workspace one byte short, 4:4:4", dict(ws_bytes=-1, subsampling=0)), ("workspace off 8 bytes", dict(ws=_WS + 4)),
         ("out == x", dict(out=_X)), ("2^31 elements", dict(N=4, H=16384, W=16384, ws_bytes=1 << 40))]


def refusals(ws_bytes_of):
    """[(label, argument list)] of ur_jpeg_roundtrip; ws_bytes_of(N, H, W, subsampling) = ur_jpeg_roundtrip_ws_bytes."""
    rows = []
    for label, kw in WRONG:
        a = dict(VALID)
        a.update({k: v for k, v in kw.items() if k != "ws_bytes"})
        need = ws_bytes_of(VALID["N"], VALID["H"], VALID["W"], a["subsampling"] if a["subsampling"] in (0, 2) else 2)
        short = kw.get("ws_bytes")
        a["ws_bytes"] = need if short is None else need - 1 if short == -1 else short
        rows.append((label, [a[k] for k in ORDER]))
    return rows
