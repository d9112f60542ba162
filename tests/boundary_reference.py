"""fp64 references, per-element bounds and CPU emulations of the image / latent boundary parity matrix
(tests/test_boundary_launchers_gpu.py, tests/test_boundary_reference_cpu.py; the cases are tests/boundary_cases.py).

Every reference is fp64 torch on the inputs as stored (16-bit or fp32 tensors, 8-bit code values, fp32 scalars as the C ABI receives
them: mul, add, scale, sa, sb, c_x, c_e are rounded to fp32 first).  The references run on whatever device their inputs are on.  NaN
never satisfies a bound.

Notation as in norm_reference: u = 2^-24 (fp32 unit roundoff), U_OUT = 2^-8 / 2^-11 (bf16 / fp16), ABS_OUT = 2^-24 for fp16 outputs.  A
kernel that computes an fp32 value v' with |v' - ref| <= E and then rounds it to 16 bits stores y with

    |y - ref| <= U_OUT |ref| + (1 + U_OUT) E + ABS_OUT                                                          (OUT)

An fp32 output is judged at E itself (its own rounding is part of E).  Every E below is a worst-case count of roundings, valid whether
or not the compiler fuses a product with the add that follows; no constant was fitted to a GPU result.  `compare` is conv_reference's.

Layout and scaled casts (nchw_to_nhwc_kernel, nhwc_to_nchw_kernel, f32_to_bf16_kernel): y = x mul + add, one product and one add:
               E = 2 u (|x mul| + |add|)        (ur_f32_to_bf16_scaled has no add: E = u |x mul|; mul = 1: E = 0, the store is the
                                                 rounding of x itself and must equal torch's x.to(dtype) bit for bit)
           Padding channels [C, Cpad) must be zero BITS; input columns [C, ld) are NaN and must never be read.
add_noise sa z0 + sb noise, ddim_step c_x zt + c_e eps (two products, one add, as axpy in norm_reference):
               E = 2 u (|sa z0| + |sb noise|)
           The fp32 state is judged at E, the 16-bit copy at (OUT), and the copy must be exactly the 16-bit rounding of the fp32 state
           the kernel stored.  Padding channels of the state leave as zero bits whatever came in.
vae_sample (mean + exp(0.5 clamp(logvar, -30, 20)) noise) scale.  The reference clamps in fp64.  a = 0.5 lv is exact; expf of a rounded
           argument is allowed e(a) = (|a| + 2) u relative, as tfa in norm_reference takes it.  T = exp(a) noise:
               E = |scale| ( |T| (e(a) + u) + u (|mean| + |T|) ) + u |ref|
Tiles      gather is exact: the 16-bit rounding of the window, zeros for a tile that does not lie inside the latent on all four sides.
           blend, at a pixel covered by K valid tiles: acc = sum_k w_k e_k is K products and K - 1 adds (the first add, to 0, is exact),
           each add bounded by u sum|w e|; then c_e acc, c_x z and their sum:
               E = 2 u |c_x z| + (K + 2) u |c_e| sum_k |w_k e_k|
           (tests/test_tiling_gpu.py takes 8 u of both terms: that is K <= 6.)  K = 0: the pixel gets c_x z, one rounding.  Every slot of a
           valid tile is the 16-bit rounding of the stored fp32 state, bit for bit; the slots of a skipped tile are not written and its
           eps is not read.  The ORDER of the sum (ascending k) is inside E for ordinary data; TILE_CASES carries a probe pixel with
           power-of-two weights (1/4, 1/4, 1/2), eps = (2^26, 4, -2^25) and z = 0: every product is exact, 2^24 + 1 rounds back to 2^24,
           and only ascending order stores exactly 0 (descending stores c_e).

Bicubic (image_resize_pad_kernel, image_unpad_resize_kernel and the two ragged 8-bit kernels).  The reference is PyTorch's
upsample_bicubic2d in fp64: A = -0.75, align_corners=False, source index real = scale (dst + 0.5) - 0.5 NOT clamped, the four tap
indices floor(real) - 1 .. + 2 clamped to the image.  scale is the fp32-ROUNDED (float)in / out, which is part of the definition
(PyTorch does the same); the rest is fp64.  Reflect padding and the crop are index maps and add nothing.  With s the samples (the
pixels for the inbound kernels; x mul + add, an fp32 value, for the outbound ones), w_y, w_x the weights and M >= |s| the magnitude
(|x mul| + |add| outbound), the fp32 value of sum_a w_y[a] sum_b w_x[b] s[a][b] differs from the reference by three terms:
  1. accumulation    every product w_x s is rounded, joins at most 3 adds of its row and, times w_y, at most 4 adds of the column,
                     each add bounded by u times the sum of magnitudes: 10 u S, S = sum |w_y||w_x| M.  Outbound the sample itself
                     carries 2 u M: 12 u S.  The 8-bit inbound sample code / 255 is correctly rounded: 11 u S.
  2. fractional position   real is fl(scale (dst + 0.5)) - 0.5 in fp32 (dst + 0.5 is exact).  The product p carries u |p| = u (|real| + 0.5);
                     p - 0.5 is exact for p >= 0.25 (Sterbenz below 1, a common exponent grid above) and carries at most u / 2
                     below; one fused multiply-add instead carries u |real|: |d real| <= u (|real| + 1) either way.  t = real - floor(real)
                     is exact for real >= 0 and carries at most u for real in (-0.5, 0): dt = u (|real| + 1) + u (the commonly quoted
                     2 u (|real| + 1) counts the exact subtraction as a rounding).  First order in dt, per axis:
                     dt_y sum_a |dw_y[a]/dt| sum_b |w_x[b]| M + the same with x and y exchanged.  The interpolant is C1 across integer
                     real (at t = 1 the weights are (0, 0, 1, 0) and dw/dt agrees with t = 0 of the next cell), so a floorf that falls on
                     the other side of an integer than the fp64 floor does stays inside this first-order term; RESIZE_IN 5 -> 13 has
                     such an output (real = 2 exactly in real arithmetic at dst = 6).
  3. cubic weights in fp32   an ABSOLUTE error per weight.  The outer taps are ((A y - 5A) y + 8A) y - 4A with y in [1, 2]: the partial
                     results are up to 1.5, 3, 4.5, 3.75, 3.75 in magnitude before the last add cancels them to at most 0.07; carrying
                     u times each magnitude through the remaining factors y <= 2 gives 1.5 -> 4.5 -> 13.6 -> 17.4 -> 38.2 u: dw = 40 u with
                     the rounding of y = t + 1 itself.  The inner taps ((A + 2) x - (A + 3)) x x + 1 stay below 2.25: 6.5 u, dw = 8 u.
                     The term is dw_y[a] sum_b |w_x[b]| M + |w_y[a]| dw_x[b] M summed over the taps.  It does not scale with |w|.
  An axis that is not resized while the other is (scale = 1) has real = dst, t = 0 and weights (0, 1, 0, 0) exactly in fp32: dt = dw = 0
  on that axis, the identity tap is exact.  No resize at all is one fused multiply-add: E = 2 u M (3 u M from 8-bit samples).
  Inbound, v mul + add follows the sum: E = |mul| E_v + 2 u (|v mul| + |add|), then (OUT).
  Non-finite samples (outbound, quantize = 1): any of the taps' samples non-finite AS AN fp32 VALUE (a finite 3e38 times mul = 2
  overflows) gives NaN, whatever its weight; nothing else may be NaN.  +-1e30 clamp to 1.0 / 0.0 through the ordinary rule below.
Quantised outputs (quantize = 1, 8-bit egress).  v = 255 ref, E_q = 255 E + u |v| (the product with 255).  The stored code must be
           clamp(round_half_even(v), 0, 255) wherever v is farther than E_q from every half-integer in [0.5, 254.5]; inside that tie
           zone it may differ by one.  The fp32 output is code / 255, a correctly rounded division: checked as bits.  CONDITION: the tie
           zone holds at most TIE_SHARE_MAX = 3 % of a case's elements, computed from the reference alone (CPU test).  Exact ties are
           planted where the path is exact (no resize, fp32 input, x = 2 s - 1 with fl(255 s) = k + 0.5): there the code must be the
           even neighbour, which is what tells round-half-even from round-half-up.
8-bit ingest: the reference divides the code value by 255 in fp64; the kernel's fp32 division is correctly rounded, u relative (above).
Ragged entry points: besides the bound they give the bits of ur_image_resize_pad_nhwc / ur_image_unpad_resize_nchw(quantize = 1).

Whole-tensor tolerances: REL_TOL of norm_reference for 16-bit outputs, 1e-6 for the fp32 outputs of the layout / state kernels
(tests/test_ops_gpu.py).  The fp32 bicubic output keeps its max-abs 2e-5 (BICUBIC_F32_ABS, on values in [0, 1]) next to the bound:
a whole-tensor 1e-6 is below what term 2 alone allows at a source position near 60 (half an fp32 ulp of it is 1.9e-6).

CPU emulations (numpy fp32, emu_*): the kernels' arithmetic in the kernels' order - cubic_taps in fp32 Horner form, the explicit
fused-multiply-add pattern of bicubic_in (a product plus addend in fp64 rounded once to fp32), the plain loop of bicubic_out, rintf,
the 16-bit pack (torch's cast) - with switches for the mutations of MUTATIONS.
"""
import zlib

import numpy as np
import torch

from conv_reference import ABS_OUT, U_OUT, compare  # noqa: F401  (compare: re-exported)
from norm_reference import DTYPES, REL_TOL, out_bound, rel_l2, worst  # noqa: F401  (re-exported)
import boundary_cases as T

U32 = 2.0 ** -24
REL_TOL_F32 = 1e-6
TIE_SHARE_MAX = 0.03
BICUBIC_F32_ABS = 2e-5
A_CUBIC = -0.75
DW_OUTER, DW_INNER = 40 * U32, 8 * U32
f32 = np.float32


def r32(v):
    """A Python float as the C ABI passes it: rounded to fp32."""
    return float(np.float32(v))


def gen_of(cid, device="cpu"):
    return torch.Generator(device=device).manual_seed(zlib.crc32(cid.encode()))


def bits16(t):
    return t.view(torch.int16)


# ---- layout, casts ------------------------------------------------------------------------------------------------------------------
def layout_in_inputs(c, device="cpu"):
    return torch.rand(c["N"], c["C"], c["H"], c["W"], generator=gen_of(c["id"], device), device=device) * 1.5 - 0.25


def layout_in_reference(x, mul, add, dt):
    """x [N,C,H,W] fp32 -> (ref, bnd) [N,H,W,C]."""
    p = x.double().permute(0, 2, 3, 1) * r32(mul)
    ref = p + r32(add)
    return ref, out_bound(ref, 2 * U32 * (p.abs() + abs(r32(add))) if (mul, add) != (1.0, 0.0) else torch.zeros_like(ref), dt)


def layout_out_inputs(c, dt, device="cpu"):
    x = torch.randn(c["N"], c["H"], c["W"], c["ld"], generator=gen_of(c["id"], device), device=device)
    x[..., c["C"]:] = float("nan")
    return x if c["f32"] else x.to(dt)


def layout_out_reference(x, C, mul, add):
    """x [N,H,W,ld] -> (ref, bnd) [N,C,H,W], fp32 output."""
    p = x[..., :C].double().permute(0, 3, 1, 2) * r32(mul)
    return p + r32(add), 2 * U32 * (p.abs() + abs(r32(add)))


def cast_inputs(c, dt, device="cpu"):
    g = gen_of(c["id"], device)
    x = torch.randn(c["M"], c["ld"], generator=g, device=device) * 3
    if c["kind"] == "ties":
        n = c["M"] * c["C"]
        v = (torch.randn(n, generator=g, device=device) * torch.tensor([1.0, 37.0, 1e-3, 300.0], device=device).repeat(n // 4)).to(dt)
        up = (bits16(v) + 1).view(dt)                                  # the neighbour of larger magnitude
        mid = ((v.double() + up.double()) / 2).float()                 # exact in fp32: one more mantissa bit than the 16-bit type has
        extra = torch.tensor([65520.0, -65520.0, 65519.996, 65536.0, 1e5, -7e4, 3.0e38, -1e30,                    # beyond +-65504
                              3e-6, -2.0 ** -24 * 1.5, 2.0 ** -25, -2.0 ** -25, 2.0 ** -24 * 2.5, 1e-8, 6.0e-8, -5.9e-8],  # fp16 subnormals
                             device=device)
        mid[:extra.numel()] = extra
        x[:, :c["C"]] = mid.view(c["M"], c["C"])
    x[:, c["C"]:] = float("nan")
    return x


def cast_reference(x, C, mul, dt):
    p = x[:, :C].double() * r32(mul)
    return p, out_bound(p, torch.zeros_like(p) if mul == 1.0 else U32 * p.abs(), dt)


# ---- vae_sample, add_noise, ddim_step ------------------------------------------------------------------------------------------------
def vae_inputs(c, device="cpu"):
    g = gen_of(c["id"], device)
    N, HW, Cl, ld = c["N"], c["HW"], c["Clat"], c["ld"]
    mom = torch.full((N * HW, ld), float("nan"), device=device)
    mom[:, :Cl] = torch.randn(N * HW, Cl, generator=g, device=device)
    lv = torch.rand(N * HW * Cl, generator=g, device=device) * 65 - 40                 # -40 .. 25: beyond both clamp ends
    edge = torch.tensor([-30.0, 20.0, -40.0, 25.0], device=device)
    lv[:4] = edge
    mom[:, Cl:2 * Cl] = lv.view(N * HW, Cl)
    noise = torch.randn(N, Cl, HW, generator=g, device=device)
    return mom, noise


def vae_reference(mom, noise, c, scale):
    N, HW, Cl = c["N"], c["HW"], c["Clat"]
    mean = mom[:, :Cl].double().view(N, HW, Cl)
    a = 0.5 * mom[:, Cl:2 * Cl].double().view(N, HW, Cl).clamp(-30, 20)
    Tm = torch.exp(a) * noise.double().permute(0, 2, 1)
    s = r32(scale)
    ref = (mean + Tm) * s
    E = abs(s) * (Tm.abs() * ((a.abs() + 2) * U32 + U32) + U32 * (mean.abs() + Tm.abs())) + U32 * ref.abs()
    return ref.view(N * HW, Cl), E.view(N * HW, Cl)


def state_inputs(c, ld_b, b_nchw, device="cpu"):
    """(a [M,Cpad] fp32 with NaN padding channels, b: noise [N,Clat,HW] or eps [M,ld_b] with NaN padding columns)."""
    g = gen_of(c["id"], device)
    M, Cl = c["N"] * c["HW"], c["Clat"]
    a = torch.full((M, c["Cpad"]), float("nan"), device=device)
    a[:, :Cl] = torch.randn(M, Cl, generator=g, device=device)
    if b_nchw:
        return a, torch.randn(c["N"], Cl, c["HW"], generator=g, device=device)
    b = torch.full((M, ld_b), float("nan"), device=device)
    b[:, :Cl] = torch.randn(M, Cl, generator=g, device=device)
    return a, b


def axpby_reference(a, b, ca, cb):
    """ca a + cb b on [M,Clat] fp64 views -> (ref, E)."""
    p, q = a.double() * r32(ca), b.double() * r32(cb)
    return p + q, 2 * U32 * (p.abs() + q.abs())


# ---- tiles -----------------------------------------------------------------------------------------------------------------------------
PROBE_W, PROBE_EPS = [0.25, 0.25, 0.5], [2.0 ** 26, 4.0, -2.0 ** 25]     # 2^24 + 1 - 2^24 = 1; ascending in fp32: 2^24 (+ 1 is lost to the tie) - 2^24 = 0


def tile_probe(c):
    """(y, x, [k...]) of the order probe: the first pixel covered by exactly 3 valid tiles of a small case with synthetic weights, or None."""
    if c["plan"] or "op" in c:
        return None
    cov = T.tile_cover(c)
    for y in range(c["LH"]):
        for x in range(c["LW"]):
            if cov[y][x] == 3:
                ks = [k for k, (y0, x0) in enumerate(c["origins"]) if T.tile_valid(c, k) and y0 <= y < y0 + c["th"] and x0 <= x < x0 + c["tw"]]
                return y, x, ks
    return None


def tile_inputs(c, device="cpu"):
    """z [N,LH,LW,Cpad] fp32 (zero padding channels, as the state always has), eps [N*T,th,tw,ld_eps] (NaN padding columns; ALL NaN for
    a tile that must be skipped), wn [T,th,tw], origins int32 [T,2]."""
    g = gen_of(c["id"], device)
    N, LH, LW, th, tw, Cl, Cp, le = c["N"], c["LH"], c["LW"], c["th"], c["tw"], c["Clat"], c["Cpad"], c["ld_eps"]
    nt = len(c["origins"])
    z = torch.zeros(N, LH, LW, Cp, device=device)
    z[..., :Cl] = torch.randn(N, LH, LW, Cl, generator=g, device=device)
    eps = torch.full((N, nt, th, tw, le), float("nan"), device=device)
    valid = [T.tile_valid(c, k) for k in range(nt)]
    for k in range(nt):
        if valid[k]:
            eps[:, k, :, :, :Cl] = torch.randn(N, th, tw, Cl, generator=g, device=device)
    if c["plan"]:
        from unirestore_amd.tiling import _gauss
        w = torch.from_numpy(np.outer(_gauss(th), _gauss(tw))).to(device)[None].repeat(nt, 1, 1)
    else:
        w = (torch.rand(nt, th, tw, generator=g, device=device) + 0.25).double()
    acc = torch.zeros(LH, LW, dtype=torch.float64, device=device)
    for k, (y0, x0) in enumerate(c["origins"]):
        if valid[k]:
            acc[y0:y0 + th, x0:x0 + tw] += w[k]
    wn = torch.ones(nt, th, tw, dtype=torch.float64, device=device)          # a skipped tile's weights are never read: 1.0 would show
    for k, (y0, x0) in enumerate(c["origins"]):
        if valid[k]:
            wn[k] = w[k] / acc[y0:y0 + th, x0:x0 + tw]
    wn = wn.float()
    probe = tile_probe(c)
    if probe is not None:
        y, x, ks = probe
        for k, wk, ek in zip(ks, PROBE_W, PROBE_EPS):
            y0, x0 = c["origins"][k]
            wn[k, y - y0, x - x0] = wk
            eps[0, k, y - y0, x - x0, 0] = ek
        z[0, y, x, 0] = 0.0
    return z, eps.view(N * nt, th, tw, le), wn, torch.tensor(c["origins"], dtype=torch.int32, device=device)


def gather_reference(z, c, dt):
    """[N*T,th,tw,Cpad] dt: the exact expected tile batch."""
    N, th, tw = c["N"], c["th"], c["tw"]
    nt = len(c["origins"])
    out = torch.zeros(N, nt, th, tw, c["Cpad"], dtype=dt, device=z.device)
    for k, (y0, x0) in enumerate(c["origins"]):
        if T.tile_valid(c, k):
            out[:, k] = z[:, y0:y0 + th, x0:x0 + tw].to(dt)
    return out.view(N * nt, th, tw, c["Cpad"])


def blend_reference(z, eps, wn, c, c_x, c_e):
    """-> (ref, E, the 8 u bound of tests/test_tiling_gpu.py) [N,LH,LW,Clat] fp64."""
    N, LH, LW, th, tw, Cl = c["N"], c["LH"], c["LW"], c["th"], c["tw"], c["Clat"]
    nt = len(c["origins"])
    e64 = torch.zeros(N, LH, LW, Cl, dtype=torch.float64, device=z.device)
    mag, K = torch.zeros_like(e64), torch.zeros(LH, LW, dtype=torch.float64, device=z.device)
    ev = eps.double().view(N, nt, th, tw, -1)[..., :Cl]
    for k, (y0, x0) in enumerate(c["origins"]):
        if T.tile_valid(c, k):
            t = wn[k].double()[None, :, :, None] * ev[:, k]
            e64[:, y0:y0 + th, x0:x0 + tw] += t
            mag[:, y0:y0 + th, x0:x0 + tw] += t.abs()
            K[y0:y0 + th, x0:x0 + tw] += 1
    cx, ce = r32(c_x), r32(c_e)
    z64 = z[..., :Cl].double()
    return (cx * z64 + ce * e64, 2 * U32 * abs(cx) * z64.abs() + (K[None, :, :, None] + 2) * U32 * abs(ce) * mag,
            8 * U32 * (abs(cx) * z64.abs() + abs(ce) * mag) + 1e-30)


# ---- bicubic ---------------------------------------------------------------------------------------------------------------------------
def reflect(o, size):
    return torch.where(o < size, o, 2 * (size - 1) - o)


def cubic_axis(d, in_size, out_size):
    """d int64 [P] -> idx [P,4] long, w, |dw/dt| [P,4], dt [P], dw_abs [4] (fp64): the taps of one axis and the terms 2 and 3 of the bound."""
    j = torch.arange(4, device=d.device)
    A = A_CUBIC
    if in_size == out_size:                         # scale = 1: real = dst, t = 0, weights (0, 1, 0, 0), all exact in fp32
        fl, t, real, exact = d.double(), torch.zeros(d.numel(), dtype=torch.float64, device=d.device), d.double(), True
    else:
        scale = float(f32(in_size) / f32(out_size))
        real = scale * (d.double() + 0.5) - 0.5
        fl = torch.floor(real)
        t, exact = real - fl, False
    idx = (fl.long()[:, None] + j - 1).clamp(0, in_size - 1)
    s = 1 - t
    y0, y3 = t + 1, s + 1
    outer = lambda y: ((A * y - 5 * A) * y + 8 * A) * y - 4 * A
    inner = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    d_outer = lambda y: 3 * A * y * y - 10 * A * y + 8 * A
    d_inner = lambda x: 3 * (A + 2) * x * x - 2 * (A + 3) * x
    w = torch.stack([outer(y0), inner(t), inner(s), outer(y3)], 1)
    dw = torch.stack([d_outer(y0), d_inner(t), d_inner(s), d_outer(y3)], 1).abs()
    dt = torch.zeros_like(t) if exact else U32 * (real.abs() + 1) + U32
    ew = torch.tensor([0.0] * 4 if exact else [DW_OUTER, DW_INNER, DW_INNER, DW_OUTER], dtype=torch.float64, device=d.device)
    return idx, w, dw, dt, ew


def bicubic_eval(S, M, n, sy, sx, in_hw, out_hw, bad=None):
    """sum over the taps at the output positions (n, sy, sx) [P] of an image batch S [N,C,SH,SW] (fp64; M >= |S| the magnitudes; the
    window in_hw = (H, W) of it is resized to out_hw).  -> ref [P,C], S1 [P,C] (sum |w_y||w_x| M), T23 [P,C] (terms 2 + 3),
    touched [P,C] bool (any tap's sample marked in `bad`)."""
    if in_hw == out_hw:
        g, m = S[n, :, sy, sx], M[n, :, sy, sx]
        return g, m, torch.zeros_like(g), (bad[n, :, sy, sx] if bad is not None else None)
    iy, wy, dwy, dty, ewy = cubic_axis(sy, in_hw[0], out_hw[0])
    ix, wx, dwx, dtx, ewx = cubic_axis(sx, in_hw[1], out_hw[1])
    I = (n[:, None, None], slice(None), iy[:, :, None], ix[:, None, :])
    g, m = S[I], M[I]                                                               # [P,4,4,C]
    ay, ax = wy.abs()[:, :, None], wx.abs()[:, None, :]
    sm = lambda W: (W[..., None] * m).sum((1, 2))
    ref = ((wy[:, :, None] * wx[:, None, :])[..., None] * g).sum((1, 2))
    t23 = dty[:, None] * sm(dwy[:, :, None] * ax) + dtx[:, None] * sm(ay * dwx[:, None, :]) + sm(ewy[None, :, None] * ax + ay * ewx[None, None, :])
    return ref, sm(ay * ax), t23, (bad[I].any(1).any(1) if bad is not None else None)


def pixels(N, OH, OW, device, subset=None):
    i = torch.arange(N * OH * OW, device=device) if subset is None else subset
    return i // (OH * OW), (i // OW) % OH, i % OW


def resize_in_inputs(c, device="cpu"):
    return torch.rand(c["N"], c["C"], c["H"], c["W"], generator=gen_of(c["id"], device), device=device)


def resize_in_reference(img, c, dt, subset=None, pre_u=0):
    """img [N,C,H,W] (fp32 pixels, or fp64 code / 255 with pre_u = 1) -> (ref, bnd) [P,C] over all output pixels or `subset`."""
    RH, RW = c["RH"], c["RW"]
    n, oy, ox = pixels(img.shape[0], RH + c["PH"], RW + c["PW"], img.device, subset)
    S = img.double()
    v, S1, t23, _ = bicubic_eval(S, S.abs(), n, reflect(oy, RH), reflect(ox, RW), (c["H"], c["W"]), (RH, RW))
    mul, add = r32(c["mul"]), r32(c["add"])
    ref = v * mul + add
    if (c["H"], c["W"]) == (RH, RW):
        E = (2 + pre_u) * U32 * ((v * mul).abs() + abs(add))
    else:
        E = abs(mul) * ((10 + pre_u) * U32 * S1 + t23) + 2 * U32 * ((v * mul).abs() + abs(add))
    return ref, out_bound(ref, E, dt)


def planted_ties(c):
    """[(k, s)] with s an fp32 value in [0.5, 1) and fl32(255 s) == k + 0.5 exactly, for the no-resize fp32 quantised cases of
    RESIZE_OUT_CASES (eight of them: they sit in the tie zone by construction and count towards its 3 %); [] for any other case."""
    if not (c.get("special", True) is False and c["f32"] and c["quantize"] and (c["CH"], c["CW"]) == (c["OH"], c["OW"]) and
            (c["mul"], c["add"]) == (0.5, 0.5)):
        return []
    out = []
    for k in range(128, 254):
        s = f32(f32(k + 0.5) / f32(255))
        if f32(s * f32(255)) == f32(k + 0.5) and f32(f32(2) * s - f32(1)) * f32(0.5) + f32(0.5) == s:
            out.append((k, float(s)))
    return out[:8]


def resize_out_inputs(c, dt, device="cpu"):
    """x [N,XH,XW,ld]: NaN outside the crop window and in the columns [C, ld); inside, values that land in [0, 1] after mul, add."""
    g = gen_of(c["id"], device)
    N, C, CH, CW = c["N"], c["C"], c["CH"], c["CW"]
    x = torch.full((N, c["XH"], c["XW"], c["ld"]), float("nan"), device=device)
    s = torch.rand(N, CH, CW, C, generator=g, device=device) * 1.1 - 0.05           # a little beyond both clamp ends
    x[:, :CH, :CW, :C] = (s - r32(c["add"])) / r32(c["mul"])
    if c["special"]:
        val = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf"), "+1e30": 1e30, "-1e30": -1e30, "3e38": 3e38}
        for name, (n, ch, y, xx) in T.SPECIAL_POS.items():
            x[n, y, xx, ch] = val[name]
    for i, (k, sv) in enumerate(planted_ties(c)):
        x[0, 0, i, 0] = 2 * sv - 1
    return x if c["f32"] else x.to(dt)


def resize_out_reference(x, c, subset=None):
    """-> dict(ref, E [P,C] of the fp32 value before quantisation; nonfinite [P,C] bool)."""
    mul, add = r32(c["mul"]), r32(c["add"])
    xw = x[..., :c["C"]].float().permute(0, 3, 1, 2)
    bad = ~torch.isfinite(xw * f32(mul) + f32(add))                                 # the SAMPLE as an fp32 value
    xd = torch.where(bad, torch.zeros_like(xw), xw).double()
    S, M = xd * mul + add, (xd * mul).abs() + abs(add)
    n, oy, ox = pixels(x.shape[0], c["OH"], c["OW"], x.device, subset)
    ref, S1, t23, touched = bicubic_eval(S, M, n, oy, ox, (c["CH"], c["CW"]), (c["OH"], c["OW"]), bad)
    E = 2 * U32 * S1 if (c["CH"], c["CW"]) == (c["OH"], c["OW"]) else 12 * U32 * S1 + t23
    return dict(ref=ref, E=E, nonfinite=touched)


def quant_reference(ref, E):
    """-> (code fp64 [..] = clamp(round_half_even(255 ref)), tie [..] bool: within E_q of a half-integer of [0.5, 254.5])."""
    v = 255.0 * ref
    Eq = 255.0 * E + U32 * v.abs()
    h = (torch.floor(v) + 0.5).clamp(0.5, 254.5)
    return torch.round(v).clamp(0, 255), (v - h).abs() <= Eq


def check_codes(code, ref, E, what, nonfinite=None):
    """code: what the kernel stored (fp64 code values; NaN allowed only where `nonfinite`).  Returns the share of elements in the tie zone."""
    want, tie = quant_reference(ref, E)
    live = torch.ones_like(tie) if nonfinite is None else ~nonfinite
    if nonfinite is not None:
        assert torch.equal(torch.isnan(code), nonfinite), what + ": NaN must leave exactly where the taps touch a non-finite sample"
    diff = torch.where(live, (code - want).abs(), torch.zeros_like(want))
    bad = live & (((diff != 0) & ~tie) | (diff > 1))
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} codes wrong outside the tie zone - {i}: got {float(code[i])} want {float(want[i])} "
                             f"(255 ref = {255 * float(ref[i]):.6f})")
    return float((tie & live).double().mean())


def ragged_inputs(cv, device="cpu"):
    """src uint8 [N, slot_bytes] (stale pattern 0xA5 behind each image), images as [1,3,H,W] fp64 code / 255 lists."""
    g = gen_of(cv["id"], device)
    slot = 3 * cv["CH"] * cv["CW"] + cv["slack"]
    src = torch.full((len(cv["geom"]), slot), 0xA5, dtype=torch.uint8, device=device)
    for n, (H, W, _, _) in enumerate(cv["geom"]):
        src[n, :H * W * 3] = torch.randint(0, 256, (H * W * 3,), generator=g, device=device, dtype=torch.int32).to(torch.uint8)
    return src, slot


def ragged_image(src, n, H, W):
    """slot n of src as [1,3,H,W] fp64 code values."""
    return src[n, :H * W * 3].view(H, W, 3).permute(2, 0, 1)[None].double()


def egress_inputs(cv, dt, f32in, device="cpu", nan_image=None):
    """x [N,CH,CW,8]: per image, values landing in [0, 1] inside its window [0:RH, 0:RW], NaN elsewhere and in the columns [3, 8)."""
    g = gen_of(cv["id"] + "_x", device)
    N = len(cv["geom"])
    x = torch.full((N, cv["CH"], cv["CW"], 8), float("nan"), device=device)
    for n, (_, _, RH, RW) in enumerate(cv["geom"]):
        x[n, :RH, :RW, :3] = (torch.rand(RH, RW, 3, generator=g, device=device) * 1.1 - 0.05 - 0.5) / 0.5
    if nan_image is not None:
        x[nan_image, 1, 1, 1] = float("nan")
    return x if f32in else x.to(dt)


def egress_case(cv, n):
    """Image n of a ragged canvas as an ur_image_unpad_resize_nchw case."""
    H, W, RH, RW = cv["geom"][n]
    return dict(N=1, C=3, XH=cv["CH"], XW=cv["CW"], ld=8, CH=RH, CW=RW, OH=H, OW=W, mul=0.5, add=0.5, quantize=1)


def ingest_case(cv, n):
    H, W, RH, RW = cv["geom"][n]
    return dict(N=1, C=3, H=H, W=W, RH=RH, RW=RW, PH=cv["CH"] - RH, PW=cv["CW"] - RW, Cpad=8, mul=2.0, add=-1.0)


# ---- CPU emulations (numpy fp32) -------------------------------------------------------------------------------------------------------
def pack(v, dt):
    """fp32 numpy -> 16-bit torch tensor (round to nearest even, overflow to inf in fp16)."""
    return torch.from_numpy(np.ascontiguousarray(v, dtype=f32)).to(dt)


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def emu_taps(d, in_size, out_size, mut=()):
    """cubic_taps of the kernel: d int [P] -> idx [P,4], w [P,4] fp32."""
    scale = f32(out_size) / f32(in_size) if "scale_inverted" in mut else f32(in_size) / f32(out_size)
    if "align_corners" in mut:
        real = (f32(in_size - 1) / f32(max(out_size - 1, 1))) * d.astype(f32)
    else:
        real = scale * (d.astype(f32) + f32(0.5)) - f32(0.5)
    if "src_clamped" in mut:
        real = np.maximum(real, f32(0))
    fl = np.floor(real)
    t = np.clip(real - fl, f32(0), f32(1)).astype(f32)
    A = f32(-0.5 if "cubic_a_half" in mut else -0.75)
    x1, x2, one = t, f32(1) - t, f32(1)
    outer = lambda y: ((A * y - f32(5) * A) * y + f32(8) * A) * y - f32(4) * A
    inner = lambda x: ((A + f32(2)) * x - (A + f32(3))) * x * x + one
    w = np.stack([outer(x1 + one), inner(x1), inner(x2), outer(x2 + one)], 1).astype(f32)
    idx = np.clip(fl.astype(np.int64)[:, None] + np.arange(4) - 1, 0, in_size if "tap_clamp_in_size" in mut else in_size - 1)
    return idx, w


def _flat_read(flat, off):
    """Read a flat fp32 array at `off`, NaN past its end (what a tap index clamped one too far may reach)."""
    ok = off < flat.size
    return np.where(ok, flat[np.minimum(off, flat.size - 1)], f32("nan")).astype(f32)


def emu_resize_in(img, c, mut=(), sample_div=False):
    """image_resize_pad_kernel / image_u8_ingest_kernel: img [N,C,H,W] fp32 pixels (or code values with sample_div) -> fp32 [N,OH,OW,C]
    before the 16-bit pack."""
    N, C, H, W = img.shape
    RH, RW, OH, OW = c["RH"], c["RW"], c["RH"] + c["PH"], c["RW"] + c["PW"]
    mul, add = f32(c["mul"]), f32(c["add"])
    px = (img.astype(f32) / f32(255)).astype(f32) if sample_div else img.astype(f32)
    i = np.arange(N * OH * OW)
    n, oy, ox = i // (OH * OW), (i // OW) % OH, i % OW
    refl = (lambda o, s: np.where(o < s, o, 2 * s - 1 - o)) if "reflect_symmetric" in mut else (lambda o, s: np.where(o < s, o, 2 * (s - 1) - o))
    ry, rx = refl(oy, RH), refl(ox, RW)
    out = np.zeros((N * OH * OW, C), f32)
    flat = px.reshape(-1)
    if (H, W) == (RH, RW):
        for ch in range(C):
            out[:, ch] = px[n, ch, ry, rx] * mul + add
        return out.reshape(N, OH, OW, C)
    iy, wy = emu_taps(ry, H, RH, mut)
    ix, wx = emu_taps(rx, W, RW, mut)
    if "weights_swapped" in mut:
        wy, wx = wx, wy
    for ch in range(C):
        at = lambda a, b: _flat_read(flat, ((n * C + ch) * H + iy[:, a]) * W + ix[:, b])
        row = []
        for a in range(4):
            head = fma(wx[:, 2], at(a, 2), fma(wx[:, 0], at(a, 0), wx[:, 1] * at(a, 1)))
            row.append(head + wx[:, 3] * at(a, 3) if a < 3 else fma(wx[:, 3], at(a, 3), head))
        v = fma(wy[:, 3], row[3], fma(wy[:, 2], row[2], fma(wy[:, 1], row[1], fma(wy[:, 0], row[0], np.zeros_like(row[0])))))
        out[:, ch] = v * mul + add
    return out.reshape(N, OH, OW, C)


def emu_resize_out(x, c, mut=()):
    """image_unpad_resize_kernel / image_u8_egress_kernel: x [N,XH,XW,ld] (any float type, widened exactly) -> fp32 [N,C,OH,OW]; with
    quantize the value code / 255, NaN for a non-finite sample."""
    x = x.float().numpy()
    N, XH, XW, ld = x.shape
    C, OH, OW = c["C"], c["OH"], c["OW"]
    CH, CW = (XH, XW) if "crop_ignored" in mut else (c["CH"], c["CW"])
    mul, add = f32(c["mul"]), f32(c["add"])
    i = np.arange(N * OH * OW)
    n, oy, ox = i // (OH * OW), (i // OW) % OH, i % OW
    resize = (OH, OW) != (CH, CW)
    if resize:
        iy, wy = emu_taps(oy, CH, OH, mut)
        ix, wx = emu_taps(ox, CW, OW, mut)
        if "weights_swapped" in mut:
            wy, wx = wx, wy
    else:
        iy, ix = oy[:, None], ox[:, None]
        wy = wx = np.ones((i.size, 1), f32)
    taps = 4 if resize else 1
    flat = x.reshape(-1)
    out = np.zeros((N, C, OH * OW), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for ch in range(C):
            v = np.zeros(i.size, f32)
            for a in range(taps):
                rowv = np.zeros(i.size, f32)
                for b in range(taps):
                    s = _flat_read(flat, ((n * XH + iy[:, a]) * XW + ix[:, b]) * ld + ch)
                    rowv = rowv + wx[:, b] * (s if "muladd_after" in mut else s * mul + add)
                v = v + wy[:, a] * rowv
            if "muladd_after" in mut:
                v = v * mul + add
            if c["quantize"]:
                q = np.floor(v * f32(255) + f32(0.5)) if "round_half_up" in mut else np.rint(v * f32(255))
                v = np.where(np.abs(v) <= f32(3.0e38), np.clip(q, 0, 255).astype(f32) / f32(255), f32("nan")).astype(f32)
            out[:, ch] = v.reshape(N, OH * OW)
    return torch.from_numpy(out.reshape(N, C, OH, OW))


def emu_layout_in(x, mul, add):
    return (x.numpy().transpose(0, 2, 3, 1) * f32(mul) + f32(add)).astype(f32)


def emu_layout_out(x, C, mul, add):
    return torch.from_numpy((x[..., :C].float().numpy().transpose(0, 3, 1, 2) * f32(mul) + f32(add)).astype(f32))


def emu_cast(x, C, mul):
    with np.errstate(over="ignore"):
        return (x[:, :C].numpy() * f32(mul)).astype(f32)


def emu_vae(mom, noise, c, scale, mut=()):
    N, HW, Cl = c["N"], c["HW"], c["Clat"]
    ld = c["Cpad"] if "ld_as_cpad" in mut else c["ld"]
    flat = mom.numpy().reshape(-1)
    row = np.arange(N * HW)[:, None] * ld + np.arange(Cl)[None]
    mean, lv = _flat_read(flat, row), _flat_read(flat, row + Cl)
    lo = f32(-20 if "logvar_clamp_20" in mut else -30)
    lv = np.minimum(np.maximum(lv, lo), f32(20))
    nz = noise.numpy()
    nz = nz.reshape(N, HW, Cl) if "noise_nhwc" in mut else nz.transpose(0, 2, 1)
    ex = np.exp((lv if "exp_lv" in mut else f32(0.5) * lv).astype(f32)).astype(f32)
    return ((mean + ex * nz.reshape(N * HW, Cl)) * f32(scale)).astype(f32)


def emu_axpby(a, b, ca, cb, c, b_nchw, ld_b=None, mut=()):
    """add_noise / ddim_step -> fp32 state [M,Cpad] (padding channels zero)."""
    N, HW, Cl, Cp = c["N"], c["HW"], c["Clat"], c["Cpad"]
    an = a.numpy()
    if b_nchw:
        bn = b.numpy()
        bn = bn.reshape(N, HW, Cl) if "noise_nhwc" in mut else bn.transpose(0, 2, 1)
        bn = bn.reshape(N * HW, Cl)
    else:
        ld = Cp if "ld_as_cpad" in mut else ld_b
        bn = _flat_read(b.numpy().reshape(-1), np.arange(N * HW)[:, None] * ld + np.arange(Cl)[None])
    out = an.copy() if "zt_padding_passthrough" in mut else np.zeros_like(an)
    out[:, :Cl] = f32(ca) * an[:, :Cl] + f32(cb) * bn
    return out


def emu_blend(z, eps, wn, c, c_x, c_e, mut=()):
    """-> (state fp32 [N,LH,LW,Cpad], written [N*T,th,tw] bool: the slots the kernel writes)."""
    N, LH, LW, th, tw, Cl, Cp = c["N"], c["LH"], c["LW"], c["th"], c["tw"], c["Clat"], c["Cpad"]
    nt = len(c["origins"])
    zn, en, wnn = z.numpy(), eps.numpy().reshape(N, nt, th, tw, -1), wn.numpy()
    acc = np.zeros((N, LH, LW, Cl), f32)
    written = np.zeros((N, nt, th, tw), bool)
    order = range(nt - 1, -1, -1) if "tiles_descending_k" in mut else range(nt)
    with np.errstate(invalid="ignore"):
        for k in order:
            y0, x0 = c["origins"][k]
            ok = T.tile_valid(c, k) if "blend_no_negative_skip" not in mut else (y0 + th <= LH and x0 + tw <= LW)
            if not ok:
                continue
            ya, yb, xa, xb = max(y0, 0), min(y0 + th, LH), max(x0, 0), min(x0 + tw, LW)
            sl = (slice(None), slice(ya, yb), slice(xa, xb))
            tl = (slice(ya - y0, yb - y0), slice(xa - x0, xb - x0))
            acc[sl] = acc[sl] + wnn[k][tl][None, :, :, None] * en[:, k][(slice(None),) + tl][..., :Cl]
            written[:, k][(slice(None),) + tl] = True
        out = np.zeros_like(zn)
        out[..., :Cl] = f32(c_x) * zn[..., :Cl] + f32(c_e) * acc
    return out, written.reshape(N * nt, th, tw)


# ---- mutations: name -> (family, what it is) ----------------------------------------------------------------------------------------------
MUTATIONS = {
    "cubic_a_half": ("resize", "A = -0.5 instead of -0.75"),
    "align_corners": ("resize", "source index computed as for align_corners=True"),
    "src_clamped": ("resize", "source index clamped at 0 before the floor"),
    "tap_clamp_in_size": ("resize", "tap index clamped to in_size instead of in_size - 1"),
    "reflect_symmetric": ("resize_in", "reflect as 2 size - 1 - o (symmetric pad)"),
    "scale_inverted": ("resize", "scale taken as out / in"),
    "weights_swapped": ("resize", "x and y weights swapped"),
    "crop_ignored": ("resize_out", "crop ignored: XH, XW used as CH, CW"),
    "muladd_after": ("resize_out", "mul, add applied after the interpolation instead of to the samples"),
    "round_half_up": ("resize_out", "round-half-up instead of half-even"),
    "logvar_clamp_20": ("vae", "logvar clamped to [-20, 20]"),
    "exp_lv": ("vae", "exp(lv) instead of exp(0.5 lv)"),
    "noise_nhwc": ("noise", "noise indexed NHWC"),
    "ld_as_cpad": ("ld", "ld taken as Cpad"),
    "tiles_descending_k": ("tiles", "tiles blended in descending k"),
    "blend_no_negative_skip": ("tiles", "blend not skipping a negative origin (the parent's behaviour)"),
    "zt_padding_passthrough": ("state", "padding channels of zt passed through"),
}
