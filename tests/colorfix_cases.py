"""Cases of the colour fix tests: shapes, data, the plan-level view of csrc/colorfix.hip's strips, and the refusal table.

A shape is (N, src_n, H, W, ld_c, ld_s).  The strip constants mirror the kernel's (CF_VR, CF_VC, CF_HR, CF_HC, CF_HALO): the column
pass cuts H into strips of VR rows (and W into VC columns without a halo), the row pass cuts W into steps of HC columns (and H into
HR rows without a halo); a strip that touches no image edge has a 31-pixel halo on both sides.
"""
import numpy as np
import torch

VR, VC, HR, HC, HALO = 66, 16, 4, 66, 31
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MODES = ("wavelet", "adain")

# the smallest shapes that can still go wrong
SMALL = [
    (1, 1, 1, 1, 8, 8),            # wavelet only: adain must refuse a single pixel
    (1, 1, 1, 40, 8, 8),
    (2, 2, 3, 5, 8, 8),
    (2, 1, 17, 33, 4, 8),
    (3, 3, 31, 32, 8, 16),
    (1, 1, 63, 64, 3, 8),
]
# from the strip sizes: in each axis an interior strip (a halo on both sides) and an extent that is no multiple of the strip
STRIPS = [
    (1, 1, 170, 200, 8, 8),        # H = 2 * 66 + 38, W = 3 * 66 + 2   (an interior strip needs an extent >= 66 + 31 + 66 = 163)
    (2, 1, 199, 170, 4, 16),       # H = 3 * 66 + 1,  W = 2 * 66 + 38
]
FANOUT = (4, 2, 20, 24, 8, 8)      # distinct sources: image n must read source n % 2
SHAPES = SMALL + STRIPS + [FANOUT]


def shape_id(sh):
    return "n{}s{}_{}x{}_ld{}_{}".format(*sh)


def runs(mode, sh):
    """adain needs two pixels."""
    return mode == "wavelet" or sh[2] * sh[3] >= 2


def plan(sh):
    """What the kernel's strips look like on a shape."""
    n, src_n, h, w, ld_c, ld_s = sh

    def axis(extent, strip):
        starts = list(range(0, extent, strip))
        both = [a for a in starts if a - HALO >= 0 and a + strip + HALO <= extent]       # the window is clamped at neither end
        return dict(strips=len(starts), interior=len(both), ragged=extent % strip != 0)
    return dict(rows=axis(h, VR), cols=axis(w, HC), col_tiles=-(-w // VC), row_tiles=-(-h // HR), w_tail=w % VC, h_tail=h % HR,
                both_clamps_in_one_tap_set=min(h, w) < 16, fanout=n // src_n, scalar_c=ld_c % 4 != 0, scalar_s=ld_s % 4 != 0)


PROPERTIES = {
    "a single pixel": lambda sh: sh[2] * sh[3] == 1,
    "one row": lambda sh: sh[2] == 1 and sh[3] > 1,
    "an extent below 16 (both clamps act in one tap set)": lambda sh: plan(sh)["both_clamps_in_one_tap_set"],
    "an extent between 16 and 31 (the clamp acts at the last levels only)": lambda sh: 16 <= min(sh[2], sh[3]) <= 31,
    "an interior row strip": lambda sh: plan(sh)["rows"]["interior"] > 0,
    "an interior column step": lambda sh: plan(sh)["cols"]["interior"] > 0,
    "H no multiple of the row strip, more than one strip": lambda sh: plan(sh)["rows"]["ragged"] and plan(sh)["rows"]["strips"] > 1,
    "W no multiple of the column step, more than one step": lambda sh: plan(sh)["cols"]["ragged"] and plan(sh)["cols"]["strips"] > 1,
    "a last column step narrower than the halo (it still feeds on the carry)": lambda sh: plan(sh)["cols"]["strips"] > 1 and 0 < sh[3] % HC < HALO,
    "W no multiple of the column tile": lambda sh: plan(sh)["w_tail"] != 0 and sh[3] > VC,
    "H no multiple of the row tile": lambda sh: plan(sh)["h_tail"] != 0 and sh[2] > HR,
    "more images than sources": lambda sh: plan(sh)["fanout"] > 1 and sh[1] > 1,
    "one source for every image": lambda sh: sh[0] > 1 and sh[1] == 1,
    "ld_c = 3 (scalar accesses)": lambda sh: sh[4] == 3,
    "ld_c = 4": lambda sh: sh[4] == 4,
    "ld_s = 16": lambda sh: sh[5] == 16,
    "more than one image": lambda sh: sh[0] > 1,
}


def make(sh, dtype, seed=0):
    """(c fp32 [N,H,W,3], s `dtype` [src_n,H,W,3]) in about [-1, 1]: a textured source, and a restored image that differs from it by a
    smooth colour cast per image and channel, a gain and fine detail - what the fix is for."""
    n, src_n, h, w = sh[:4]
    g = torch.Generator().manual_seed(1000 + seed)
    s = (torch.rand(src_n, h, w, 3, generator=g) * 1.6 - 0.8).to(dtype)
    yy = torch.linspace(-1, 1, h).view(1, h, 1, 1)
    xx = torch.linspace(-1, 1, w).view(1, 1, w, 1)
    cast = 0.15 * torch.randn(n, 1, 1, 3, generator=g) + 0.08 * yy * torch.randn(n, 1, 1, 3, generator=g) + 0.08 * xx
    gain = 1.0 + 0.2 * torch.randn(n, 1, 1, 3, generator=g)
    c = s.float().repeat(n // src_n, 1, 1, 1) * gain + cast + 0.05 * torch.randn(n, h, w, 3, generator=g)
    return c.float().contiguous(), s.contiguous()


def padded(t, ld, fill=float("nan")):
    """[.., 3] -> [.., ld] with `fill` in the padding channels."""
    out = torch.full((*t.shape[:-1], ld), fill, dtype=t.dtype)
    out[..., :3] = t
    return out


def source_of(s, n):
    """fp64 [N,H,W,3]: row n is source n % src_n."""
    a = s.double().numpy()
    return a[np.arange(n) % a.shape[0]]


# ---- refusals: one wrong argument in an otherwise valid call (placeholder pointers: nothing is launched) ----------------------------
_C, _S, _O, _WS = 0x10000, 0x20000, 0x30000, 0x40000


def _wavelet(**kw):
    a = dict(c=_C, ld_c=8, s=_S, ld_s=8, out=_O, N=4, src_n=2, H=20, W=24, dtype=0, stream=None)
    a.update(kw)
    return [a[k] for k in ("c", "ld_c", "s", "ld_s", "out", "N", "src_n", "H", "W", "dtype", "stream")]


def _adain(**kw):
    a = dict(c=_C, ld_c=8, s=_S, ld_s=8, out=_O, N=4, src_n=2, H=20, W=24, dtype=0, ws=_WS, ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return [a[k] for k in ("c", "ld_c", "s", "ld_s", "out", "N", "src_n", "H", "W", "dtype", "ws", "ws_bytes", "stream")]


_WRONG = [("null c", dict(c=None)), ("null src", dict(s=None)), ("null out", dict(out=None)), ("N = 0", dict(N=0)), ("N < 0", dict(N=-4)),
          ("src_n = 0", dict(src_n=0)), ("src_n < 0", dict(src_n=-2)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("H < 0", dict(H=-20)),
          ("W < 0", dict(W=-24)), ("N % src_n != 0", dict(src_n=3)), ("src_n > N", dict(src_n=8)), ("ld_c = 2", dict(ld_c=2)),
          ("ld_s = 2", dict(ld_s=2)), ("ld_c = 0", dict(ld_c=0)), ("dtype = 2", dict(dtype=2)), ("dtype = -1", dict(dtype=-1)),
          ("out == c", dict(out=_C))]


def refusals():
    rows = [(f"wavelet: {name}", "ur_color_fix_wavelet", _wavelet(**kw)) for name, kw in _WRONG]
    rows += [(f"adain: {name}", "ur_color_fix_adain", _adain(**kw)) for name, kw in _WRONG]
    rows += [("adain: null workspace", "ur_color_fix_adain", _adain(ws=None)),
             ("adain: H * W = 1", "ur_color_fix_adain", _adain(H=1, W=1)),
             ("adain: workspace too small", "ur_color_fix_adain", _adain(ws_bytes=64)),
             ("adain: workspace not 8-byte aligned", "ur_color_fix_adain", _adain(ws=_WS + 4))]
    return rows
