"""Case tables of the corruption tests (test_corrupt_cpu.py, test_corrupt_gpu.py): shapes, inputs, seeds and the refusals of the C ABI.

Shapes (N, H, W).  (1, 32, 32): the smallest size that is not refused; motion blur's radius 20 breaks off, sigma 6's radius 24 almost
spans the side.  (2, 33, 47): odd sizes whose H * W * 3 is no multiple of 4 (the last Philox counter is partial), a fog map of 64
cropped on both sides, zoom outputs larger than the image.  (3, 40, 32): three images (alone == image 2 of 3), H != W the other
way round.  (1, 64, 96): several workgroups per image, a fog map of 128.
"""
import numpy as np

SHAPES = [(1, 32, 32), (2, 33, 47), (3, 40, 32), (1, 64, 96)]
SEED_SETS = (42, 7)                                # "two seeds per image": every case runs under both
KINDS = ("random", "zeros", "white", "ramp")


def stems(n):
    return [f"img{i}" for i in range(n)]


def images(shape, kind="random"):
    """uint8 [N, H, W, 3]: seeded random bytes; constant 0; constant 255; a grey ramp (delta = 0 in HSV, the extremes of m / (m + c))."""
    n, h, w = shape
    if kind == "zeros":
        return np.zeros((n, h, w, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((n, h, w, 3), 255, dtype=np.uint8)
    if kind == "ramp":
        ramp = np.linspace(0, 255, h * w).astype(np.uint8).reshape(1, h, w, 1)
        return np.ascontiguousarray(np.broadcast_to(ramp, (n, h, w, 3)))
    rng = np.random.default_rng(1000 * h + w)
    x = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    x[:, : h // 4, : w // 4] //= 8                   # a dark corner: small Poisson means, small V
    return x


def colour_grid():
    """uint8 [1, 36, 36, 3] for the HSV round trip: greys, the six hue-sector edges (two channels equal) and mixed colours."""
    levels = (0, 1, 64, 128, 254, 255)
    cols = [(a, b, c) for a in levels for b in levels for c in levels]            # 216 colours: every tie pattern among them
    rng = np.random.default_rng(5)
    cols += [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(36 * 36 - len(cols))]
    return np.array(cols, dtype=np.uint8).reshape(1, 36, 36, 3)


# ---- refusals: one wrong argument in an otherwise valid call (placeholder pointers: nothing is launched) ----------------------------
_X, _O, _K, _T, _WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
_ORDER = {
    "ur_corrupt_noise": ("x", "keys", "out", "N", "H", "W", "mode", "c", "table", "out_kind", "stream"),
    "ur_corrupt_filter_sep": ("x", "taps", "radius", "out", "N", "H", "W", "ws", "ws_bytes", "out_kind", "stream"),
    "ur_corrupt_taps": ("x", "taps", "n_taps", "per_image", "border", "out", "N", "H", "W", "out_kind", "stream"),
    "ur_corrupt_zoom": ("x", "taps", "n_layers", "out", "N", "H", "W", "out_kind", "stream"),
    "ur_corrupt_color": ("x", "out", "N", "H", "W", "mode", "a", "b", "ws", "ws_bytes", "out_kind", "stream"),
    "ur_corrupt_pixelate": ("x", "out", "N", "H", "W", "small_h", "small_w", "hbox", "vbox", "ymap", "xmap", "ws", "ws_bytes", "out_kind",
                            "stream"),
    "ur_corrupt_fog": ("x", "keys", "out", "N", "H", "W", "c", "decay", "ws", "ws_bytes", "out_kind", "stream"),
}
_VALID = dict(x=_X, keys=_K, out=_O, N=2, H=32, W=40, mode=0, c=20.0, table=_T, out_kind=0, stream=None, taps=_T, radius=4, ws=_WS,
              ws_bytes=1 << 24, n_taps=9, per_image=0, border=0, n_layers=11, a=0.4, b=0.0, small_h=16, small_w=20, hbox=_T, vbox=_T + 256,
              ymap=_T + 512, xmap=_T + 1024, decay=2.0)
# wrong in every export
_COMMON = [("null x", dict(x=None)), ("null out", dict(out=None)), ("N = 0", dict(N=0)), ("N < 0", dict(N=-2)), ("H = 31", dict(H=31)),
           ("W = 31", dict(W=31)), ("H < 0", dict(H=-32)), ("W = 0", dict(W=0)), ("out_kind = 2", dict(out_kind=2)),
           ("out_kind = -1", dict(out_kind=-1)), ("fp32 out off 4 bytes", dict(out=_O + 2, out_kind=1)), ("out == x", dict(out=_X)),
           ("2^31 elements", dict(N=4, H=16384, W=16384))]
_WS_WRONG = [("null workspace", dict(ws=None)), ("workspace off 8 bytes", dict(ws=_WS + 4)), ("workspace too small", dict(ws_bytes=8))]
_OWN = {
    "ur_corrupt_noise": [("null keys", dict(keys=None)), ("mode = 4", dict(mode=4)), ("mode = -1", dict(mode=-1)),
                         ("shot without a table", dict(mode=3, table=None)), ("table off 4 bytes", dict(mode=3, table=_T + 2)),
                         ("c = 0", dict(c=0.0))],
    "ur_corrupt_filter_sep": [("null taps", dict(taps=None)), ("taps off 4 bytes", dict(taps=_T + 1)), ("radius < 0", dict(radius=-1)),
                              ("radius = 256", dict(radius=256))] + _WS_WRONG,
    "ur_corrupt_taps": [("null taps", dict(taps=None)), ("taps off 4 bytes", dict(taps=_T + 2)), ("n_taps = 0", dict(n_taps=0)),
                        ("n_taps = 4097", dict(n_taps=4097)), ("per_image = 2", dict(per_image=2)), ("border = 2", dict(border=2)),
                        ("border = -1", dict(border=-1))],
    "ur_corrupt_zoom": [("null layers", dict(taps=None)), ("layers off 4 bytes", dict(taps=_T + 2)), ("n_layers = 0", dict(n_layers=0)),
                        ("n_layers = 65", dict(n_layers=65))],
    "ur_corrupt_color": [("mode = 3", dict(mode=3)), ("mode = -1", dict(mode=-1))] + _WS_WRONG,
    "ur_corrupt_pixelate": [("null hbox", dict(hbox=None)), ("null vbox", dict(vbox=None)), ("null ymap", dict(ymap=None)),
                            ("null xmap", dict(xmap=None)), ("xmap off 4 bytes", dict(xmap=_T + 1026)), ("small_h = 0", dict(small_h=0)),
                            ("small_w = 0", dict(small_w=0)), ("small_h > H", dict(small_h=33)), ("small_w > W", dict(small_w=41))] + _WS_WRONG,
    "ur_corrupt_fog": [("null keys", dict(keys=None)), ("c = 0", dict(c=0.0)), ("decay = 1", dict(decay=1.0)),
                       ("H > 16384", dict(H=16385, N=1))] + _WS_WRONG,
}


def refusals():
    """[(label, export, argument list)]."""
    rows = []
    for fn, order in _ORDER.items():
        for label, kw in _COMMON + _OWN[fn]:
            a = dict(_VALID)
            a.update(kw)
            rows.append((f"{fn}: {label}", fn, [a[k] for k in order]))
    return rows
