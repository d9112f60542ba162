"""fp64 reference and per-element bound of the conv / GEMM launcher parity matrix (tests/test_conv_launchers_gpu.py).

Every output element of a launch must satisfy

    |y - ref| <= u_out * |ref| + C * sqrt(K) * 2^-24 * A + eps_act + abs_out

  * ref: fp64 torch on the same 16-bit-rounded inputs (and fp32 bias / statistics values) the kernel reads;
  * u_out: unit roundoff of the stored output, 2^-8 (bf16), 2^-11 (fp16), 2^-24 (fp32); abs_out = 2^-24 for fp16 outputs (half the
    spacing of the fp16 subnormals is 2^-25: the relative term vanishes there), else 0;
  * A: the same launch on |x| and |w| in fp64, plus |bias|, propagated through the epilogue to first order: |gelu'| <= 1.13,
    |silu'| <= 1.1, the product rule for GEGLU (|gelu(g)| A_a + |a| 1.13 A_g) and GATE (|g| A_a + |a| A_g), times |out_scale|,
    plus |residual|; with LayerNorm folding, rstd * (A + |mean * colsum|) before the bias;
  * eps_act: the epilogue's own approximation (csrc/common.h): GELU 2.6e-5 absolute (|a| 2.6e-5 in GEGLU; the fit's largest error
    is 2.52e-5 at x = 1.29 - relative to |x| it reaches 5.0e-5 near x = -0.43, so a bound proportional to |x| would be wrong), SiLU
    2^-20 |z|;
  * C = 4, fixed for every case (fp32 accumulation of K exact products: the error of a sum grows like sqrt(K) unit roundoffs of
    the sum of magnitudes; C leaves room for the order the MFMA and split-K reduce pick).  Never tuned per case.

With a GroupNorm prologue (gn_ab) the loader rounds act(a x + b) to the 16-bit type.  The reference rounds its own fp32 value the same
way; where that value lies within 2^-20 (relative) of a rounding boundary - the kernel's fast exp / reciprocal may land on either
side - either neighbour is right, and the bound adds the same conv over those elements' spacing and |w| (times max |act'|).

The statistics planes (GroupNorm partials, row sums) are checked per (image, channel) / per row against fp64 sums of the kernel's
own 16-bit output with the same C: |s - ref| <= C * sqrt(n) * 2^-24 * sum|terms| (n = terms summed).  NaN never satisfies a bound.
"""
import math

import torch
import torch.nn.functional as F

C_BOUND = 4.0
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
ABS_OUT = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -24, torch.float32: 0.0}
GELU_D, SILU_D, GELU_EPS, SILU_EPS = 1.13, 1.1, 2.6e-5, 2.0 ** -20
NONE, SILU, GELU, GEGLU, GATE = 0, 1, 2, 3, 4


ACT_D = {NONE: 1.0, SILU: SILU_D, GELU: GELU_D}


def round_ambiguous(v, dtype):
    """fp32 v -> (v rounded to dtype, in fp64; the spacing where v +- 2^-20 |v| rounds to two different values, else 0)."""
    d = v.abs() * 2.0 ** -20
    lo, hi = (v - d).to(dtype).double(), (v + d).to(dtype).double()
    return v.to(dtype).double(), (hi - lo).abs()


def conv_nhwc(x, w, stride=1, pad=(0, 0), OH=None, OW=None):
    """x [N,H,W,C], w [Cout,KH,KW,C] (fp64) -> [N*OH*OW, Cout]: cross-correlation with zero padding pad = (top, left); the bottom /
    right padding is whatever OH / OW reach (as the kernels' loaders read zeros outside the image)."""
    N, H, W, C = x.shape
    Cout, KH, KW, _ = w.shape
    OH = (H + 2 * pad[0] - KH) // stride + 1 if OH is None else OH
    OW = (W + 2 * pad[1] - KW) // stride + 1 if OW is None else OW
    hp, wp = (OH - 1) * stride + KH, (OW - 1) * stride + KW
    xp = x.new_zeros(N, max(hp, pad[0] + H), max(wp, pad[1] + W), C)
    xp[:, pad[0]:pad[0] + H, pad[1]:pad[1] + W] = x
    acc = x.new_zeros(N * OH * OW, Cout)
    for kh in range(KH):
        for kw in range(KW):
            xs = xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]
            acc += xs.reshape(-1, C) @ w[:, kh, kw, :].t()
    return acc


def epilogue(acc, A, act=NONE, bias=None, out_scale=1.0, res=None, ln=None):
    """fp64 epilogue of the GEMM N space acc [M, Cout] (and its magnitude A) -> (ref, A_out, eps_act) in output columns.
    bias: [M, Cout] rows (already expanded per image); ln: (mean [M], rstd [M], colsum [Cout]); res: [M, Cout_out]."""
    z, Az = acc, A
    if ln is not None:
        mean, rstd, colsum = ln
        mc = mean[:, None] * colsum[None, :]
        z, Az = rstd[:, None] * (acc - mc), rstd[:, None] * (A + mc.abs())
    if bias is not None:
        z, Az = z + bias, Az + bias.abs()
    if act in (GEGLU, GATE):
        M, n = z.shape
        zz, AA = z.view(M, n // 64, 2, 32), Az.view(M, n // 64, 2, 32)
        a, g = zz[:, :, 0].reshape(M, n // 2), zz[:, :, 1].reshape(M, n // 2)
        Aa, Ag = AA[:, :, 0].reshape(M, n // 2), AA[:, :, 1].reshape(M, n // 2)
        if act == GEGLU:
            phi = F.gelu(g)
            out, Aout, eps = a * phi, phi.abs() * Aa + a.abs() * GELU_D * Ag, a.abs() * GELU_EPS
        else:
            out, Aout, eps = a * g, g.abs() * Aa + a.abs() * Ag, torch.zeros_like(a)
    elif act == SILU:
        out, Aout, eps = F.silu(z), SILU_D * Az, SILU_EPS * z.abs()
    elif act == GELU:
        out, Aout, eps = F.gelu(z), GELU_D * Az, GELU_EPS * torch.ones_like(z)
    else:
        out, Aout, eps = z, Az, torch.zeros_like(z)
    s = abs(out_scale)
    out, Aout, eps = out * out_scale, Aout * s, eps * s
    if res is not None:
        out, Aout = out + res, Aout + res.abs()
    return out, Aout, eps


def bound(ref, A, eps, K, out_dtype):
    return U_OUT[out_dtype] * ref.abs() + C_BOUND * math.sqrt(K) * 2.0 ** -24 * A + eps + ABS_OUT[out_dtype]


def compare(y, ref, bnd, what=""):
    """Element-wise |y - ref| <= bnd (fp64 tensors of one shape).  Returns max |y - ref| / bnd (0 where both are 0); raises
    AssertionError naming the first violations (a NaN anywhere is one)."""
    err = (y - ref).abs()
    ok = err <= bnd
    if not bool(ok.all()):
        bad = (~ok).nonzero()[:6].tolist()
        det = "; ".join(f"{tuple(i)}: got {float(y[tuple(i)]):.6g} ref {float(ref[tuple(i)]):.6g} bound {float(bnd[tuple(i)]):.3g}"
                        for i in bad)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside the bound - {det}")
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.zeros_like(err))
    return float(ratio.max()) if ratio.numel() else 0.0


def compare_sums(got_s, got_q, terms, n, what=""):
    """Statistics plane check: got_s / got_q = summed (sum, sum of squares) over the last dim of `terms` (fp64 kernel output values,
    n of them per sum).  Returns the worst ratio."""
    k = C_BOUND * math.sqrt(n) * 2.0 ** -24
    r1 = compare(got_s, terms.sum(-1), k * terms.abs().sum(-1), what + " sum")
    r2 = compare(got_q, (terms * terms).sum(-1), k * (terms * terms).sum(-1), what + " sum of squares")
    return max(r1, r2)
