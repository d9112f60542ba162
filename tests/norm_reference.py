"""fp64 references, per-element bounds and CPU emulations of the norm / per-channel kernel parity matrix
(tests/test_norm_launchers_gpu.py, tests/test_norm_reference_cpu.py; the cases are tests/norm_cases.py).

Every reference is fp64 torch on the 16-bit inputs as stored (fp32 parameters as stored); GroupNorm and LayerNorm use the two-pass
variance.  The references run on whatever device their inputs are on.  NaN never satisfies a bound.

Notation: u = 2^-24 (fp32 unit roundoff), u_out = 2^-8 / 2^-11 (bf16 / fp16), abs_out = 2^-24 for fp16 outputs (its subnormal spacing:
the relative term vanishes there), both from conv_reference.  A kernel that computes an fp32 value v' with |v' - ref| <= E and then
rounds it stores y with

    |y - ref| <= u_out |ref| + (1 + u_out) E + abs_out                                                          (OUT)

and every family below only has to state its E.  K = 4 is conv_reference's C: an fp32 sum of n terms is allowed K sqrt(n) u sum|terms|.
That term is STATISTICAL: under the usual model of independent roundings, recursive summation of n terms of one sign has a standard
deviation of about u sum|terms| sqrt(n) / 3, so K = 4 is 12 sigma (more for mixed signs and for the kernels' shorter chains); the
worst case (n - 1) u sum|terms| is never approached.  Where n <= 10 (dwconv) the worst-case bound itself is used.  No constant below
was fitted to a GPU result.

GroupNorm (csrc/norms.hip: gn_stats_kernel -> gn_finalize_kernel -> gn_apply*_kernel).  For group g of image n with cnt = cpg HW
elements, fp64 two-pass mean m and variance v, E1 = mean|x|, E2 = mean x^2 = v + m^2:
  planes   x^2 of a 16-bit value is exact in fp32, so both planes are fp32 sums of exact terms.  Their sum over p per (image, channel)
           against the fp64 sums of the input - independent of the partition:
               |S - sum x| <= k sum|x|,  |Q - sum x^2| <= k sum x^2,   k = K sqrt(HW) u.
  moments  finalize adds the partials in fp64 (k64 = 2^-44: up to 512 roundings of 2^-53 per sum; per thread and tree together stay far below):  dm = (k + k64) E1,
               dv = (k + k64) E2 + 2 |m| dm + dm^2          <- var = Q/cnt - mean^2: the error scales with v + m^2, not with v.
           rstd' = rsqrtf(max((float)var', 0) + eps) with var' in [v - dv, v + dv]:
               rho = max( sqrt((v + eps) / (max(v - dv, 0) + eps)) - 1,  1 - sqrt((v + eps) / (v + dv + eps)) ) + 6 u
           (exact in dv, not first order - a constant group has v = 0; 6 u: the cast of var and the add are u / 2 each on rstd,
           v_rsq_f32 is 1 ulp = 2 u, the product with gamma u, and 2 u of margin for a fused or unfused mean * a).
  ab       a = rstd gamma, b = beta - m a:   da = |a| rho,   db = |m| da + (|a| + da) dm + 3 u (|beta| + |m a|).
  mean_out |mean' - m| <= dm + u |m|.
  output   a' x + b' - (a x + b) = da (x - m) - a' dm + roundings, so before the activation
               E = |x - m| da + (|a| + da) dm + 3 u (|beta| + |m a|) + 2 u (|a x| + |b|)
           - that is |y - beta| drstd/rstd + |a| dmean plus the fp32 evaluation of a x + b, where |b| ~ |m a| is much larger than |y|
           in an offset group.  SiLU: E <- 1.1 E + 2^-20 |z| (conv_reference's activation term).  Then (OUT).
  Producer-side planes (ur_groupnorm_nhwc with pre1 / pre2) are fp32 roundings of exact sums: inside the same k.  Planes that ARE the
  input (finalize alone): k = 0 and the reference is the fp64 value of the same formula.

LayerNorm (ln_rows_kernel: fp32 two-pass in registers, one wave per row).  E1 = mean|x| of the row:
               dm = K sqrt(C) u E1 + u |m|,   dv = dm^2 + (K sqrt(C) + 4) u (v + dm^2)       (sum (x - m')^2 = C v + C dm^2)
           rho as above from (v, dv), and for y = (x - m) rstd gamma + beta
               E = |gamma| rstd (1 + rho) dm + |y - beta| (rho + 4 u) + u |y|.
           The masked lanes of the last vector slot contribute 0 to both sums; a kernel that lets them add m^2 breaks dv by m^2.

Row softmax (softmax_rows_kernel: fp32 scores, __expf, 4 wave partial sums, 1 / l).  x = s - max (exact in fp64):
               e(x) = (3 |x| + 2) u      (fl(s - m): |x| u on the exponent; x * log2(e) and the constant's own rounding: 2 |x| u; v_exp_f32 1 ulp)
               dl = sum_i p_i e(x_i) + K sqrt(cols) u
               E = p (e(x) + dl + 3 u) + 2^-125     (3 u: the division and the product; 2^-125: the native exp and the product may flush
                                                     results below the fp32 normal range, 2^-126, to zero)
           then (OUT).  Columns [cols, ldp) must be zero bits (checked by the tests, not by the bound).

TFA prompt update (tfa_prompt_kernel: expf, IEEE division, tanhf; fp32 output): per softmax e(x) = (|x| + 2) u (expf is 1 ulp on the
           rounded argument), dl as above with D terms, tanhf 2 ulp = 4 u:
               E = |f cond| (e_f + dl_f + 2 u) + |i c| (e_i + dl_i + 6 u) + u |upd| + 2^-125.

linear_f32 (one wave per column, lane-strided fp32 sums + butterfly).  A = sum_k |w||x| + |bias|:
               E = (K sqrt(Kg) + 1) u A, then SiLU 1.1 E + 2^-20 |z|, GELU 1.13 E + 2.6e-5, tanh E + 4 u |tanh z|, ReLU E; + u |ref|.

dwconv (bias + 9 taps in fp32, fixed order):  A = |bias| + sum |x||w|,  E = 11 u A (worst case of 10 terms with rounded products);
           SimpleGate a0 * a1: E = |a1| E0 + |a0| E1 + E0 E1 + u |a0 a1|.  Then (OUT).
scale_channels x s (+ r): E = u |x s| (+ u (|x s| + |r|)).   axpy a + b s: E = 2 u (|a| + |b s|).
spade n (1 + g) + b (+ r): E = 3 u (|n| (1 + |g|) + |b| + |r|).   vec_mul_group: E = u |ref| (fp32 output).  Then (OUT).
The fan-out kernels must give the bits of the single-task kernels (checked as such) and are inside the same bounds.

CPU emulations (numpy fp32, emu_*): the kernels' arithmetic in the kernels' order where the order matters - per-thread pixel rows and
the row-order LDS sum of the statistics pass, E[x^2] - mean^2 from fp32 partials added in fp64, rsqrt in fp32, the masked lanes and the
butterfly of LayerNorm, the four wave sums of the softmax, the 16-bit pack - with switches for the mutations of MUTATIONS.
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from conv_reference import ABS_OUT, GELU_D, GELU_EPS, SILU_D, SILU_EPS, U_OUT, compare  # noqa: F401  (compare: re-exported)
import norm_cases as T

U32 = 2.0 ** -24
K64 = 2.0 ** -44
K_SUM = 4.0
FTZ = 2.0 ** -125
EPS = 1e-5
REL_TOL = {torch.bfloat16: 3e-3, torch.float16: 4e-4}           # the whole-tensor tolerance of tests/test_ops_gpu.py
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def out_bound(ref, E, dt):
    """(OUT).  dt = torch.float32: an fp32 result whose own rounding is part of E."""
    if dt == torch.float32:
        return E
    return U_OUT[dt] * ref.abs() + (1 + U_OUT[dt]) * E + ABS_OUT[dt]


def gen_of(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------
def gn_inputs(c, dt):
    """(x1 [N,HW,C1] dt, x2 | None, gamma | None, beta | None) of a GN_CASES / NHWC_CASES row."""
    g = gen_of(c["id"])
    N, HW, C, G = c["N"], c["HW"], c["C1"] + c["C2"], c["G"]
    cpg = C // G
    grp = torch.arange(C) // cpg
    sigma = 0.5 + (grp % 3).double() * 0.75
    sign = 1.0 - 2.0 * (grp % 2).double()
    x = (torch.randn(N, HW, C, generator=g, dtype=torch.float64) + sign * float(c.get("offset", 0))) * sigma
    if c.get("const_group") is not None:
        n, gg = c["const_group"]
        x[n, :, gg * cpg:(gg + 1) * cpg] = 1.375
    x = x.to(dt)
    affine = c.get("affine", True)
    gamma = (1 + 0.5 * torch.randn(C, generator=g)) if affine else None
    beta = torch.randn(C, generator=g) if affine else None
    x1 = x[..., :c["C1"]].contiguous()
    x2 = x[..., c["C1"]:].contiguous() if c["C2"] else None
    return x1, x2, gamma, beta


def moment_bounds(m, v, E1, E2, k, eps):
    dm = (k + K64) * E1
    dv = (k + K64) * E2 + 2 * m.abs() * dm + dm * dm
    up = torch.sqrt((v + eps) / ((v - dv).clamp_min(0) + eps)) - 1
    lo = 1 - torch.sqrt((v + eps) / (v + dv + eps))
    return dm, dv, torch.maximum(up, lo) + 6 * U32


def gn_tables(m, v, E1, E2, k, gamma, beta, eps, cpg):
    """Group moments [N,G] -> per-channel reference and bounds: dict of a, b, da, db [N,C]; m_c, dm_c [N,C]; dm [N,G]."""
    dm, _, rho = moment_bounds(m, v, E1, E2, k, eps)
    rstd = 1 / torch.sqrt(v + eps)
    ex = lambda t: t.repeat_interleave(cpg, dim=1)
    C = m.shape[1] * cpg
    ga = gamma.double().to(m.device) if gamma is not None else torch.ones(C, dtype=torch.float64, device=m.device)
    be = beta.double().to(m.device) if beta is not None else torch.zeros(C, dtype=torch.float64, device=m.device)
    a = ex(rstd) * ga
    mc, dmc = ex(m), ex(dm)
    b = be - mc * a
    da = a.abs() * ex(rho)
    rnd_b = 3 * U32 * (be.abs() + (mc * a).abs())
    db = mc.abs() * da + (a.abs() + da) * dmc + rnd_b
    return dict(a=a, b=b, da=da, db=db, m=mc, dm=dmc, rnd_b=rnd_b, mean=m, dmean=dm + U32 * m.abs(), be=be)


def gn_reference(x1, x2, gamma, beta, G, silu, dt, eps=EPS):
    """fp64 GroupNorm(+SiLU) of cat(x1, x2) over [N,HW,C] and every bound: dict(y, y_bnd, ab, ab_bnd [N,2,C], mean, mean_bnd [N,G],
    S, S_bnd, Q, Q_bnd [N,C])."""
    x = (x1 if x2 is None else torch.cat([x1, x2], -1)).double()
    N, HW, C = x.shape
    cpg = C // G
    xg = x.view(N, HW, G, cpg)
    m = xg.mean((1, 3))
    v = ((xg - m[:, None, :, None]) ** 2).mean((1, 3))
    E1, E2 = xg.abs().mean((1, 3)), (xg * xg).mean((1, 3))
    k = K_SUM * math.sqrt(HW) * U32
    t = gn_tables(m, v, E1, E2, k, gamma, beta, eps, cpg)
    a, b = t["a"][:, None, :], t["b"][:, None, :]
    z = a * x + b
    E = (x - t["m"][:, None, :]).abs() * t["da"][:, None, :] + ((a.abs() + t["da"][:, None, :]) * t["dm"][:, None, :] + t["rnd_b"][:, None, :]) + \
        2 * U32 * ((a * x).abs() + b.abs())
    if silu:
        y, E = F.silu(z), SILU_D * E + SILU_EPS * z.abs()
    else:
        y = z
    return dict(y=y, y_bnd=out_bound(y, E, dt), ab=torch.stack([t["a"], t["b"]], 1), ab_bnd=torch.stack([t["da"], t["db"]], 1),
                mean=t["mean"], mean_bnd=t["dmean"], S=x.sum(1), S_bnd=k * x.abs().sum(1), Q=(x * x).sum(1), Q_bnd=k * (x * x).sum(1),
                chan_mean=x.mean(1), chan_mean_bnd=k * x.abs().mean(1) + U32 * x.mean(1).abs() + K64 * x.abs().mean(1))


def producer_planes(x, P):
    """fp32 partial planes [N,P,C,2] of x [N,HW,C] over P pixel chunks of ceil(HW / P) (the last may be short or EMPTY: zeros), as a
    producer's epilogue leaves them: exact sums rounded to fp32."""
    N, HW, C = x.shape
    ppb = (HW + P - 1) // P
    xd = x.double()
    out = torch.zeros(N, P, C, 2, dtype=torch.float64, device=x.device)
    for p in range(P):
        seg = xd[:, p * ppb:min(HW, (p + 1) * ppb)]
        out[:, p, :, 0], out[:, p, :, 1] = seg.sum(1), (seg * seg).sum(1)
    return out.float()


def finalize_inputs(c):
    """Synthetic planes of a FINALIZE_CASES row: (p1 [N,P1,C1,2], p2 | None, gamma | None, beta | None), fp32.  Each entry is the
    (sum, sum of squares) of HW / P pixels drawn around a per-channel mean, so every group variance is positive."""
    g = gen_of(c["id"])
    out = []
    for C, P in ((c["C1"], c["P1"]), (c["C2"], c["P2"])):
        if not C:
            out.append(None)
            continue
        assert c["HW"] % P == 0 or P in (3, 4, 5)
        npx = max(1, c["HW"] // P)
        x = torch.randn(c["N"], P, npx, C, generator=g, dtype=torch.float64) + 2.0 * torch.randn(C, generator=g, dtype=torch.float64)
        out.append(torch.stack([x.sum(2), (x * x).sum(2)], -1).float())
    Ct = c["C1"] + c["C2"]
    gamma = (1 + 0.5 * torch.randn(Ct, generator=g)) if c["affine"] else None
    beta = torch.randn(Ct, generator=g) if c["affine"] else None
    return out[0], out[1], gamma, beta


def finalize_reference(p1, p2, gamma, beta, G, HW, eps=EPS):
    """The planes ARE the input: fp64 value of the kernel's own formula, bounds with k = 0."""
    S = p1.double().sum(1) if p2 is None else torch.cat([p1.double().sum(1), p2.double().sum(1)], 1)       # [N,C,2]
    N, C, _ = S.shape
    cpg = C // G
    cnt = cpg * HW
    sg = S.view(N, G, cpg, 2).sum(2)
    m, E2 = sg[..., 0] / cnt, sg[..., 1] / cnt
    v = E2 - m * m
    t = gn_tables(m, v, torch.sqrt(E2), E2, 0.0, gamma, beta, eps, cpg)
    return dict(ab=torch.stack([t["a"], t["b"]], 1), ab_bnd=torch.stack([t["da"], t["db"]], 1), mean=t["mean"], mean_bnd=t["dmean"])


def worst(y, ref, bnd):
    """max |y - ref| / bnd without asserting (NaN -> inf)."""
    r = ((y.double() - ref).abs() / bnd.clamp_min(1e-300)).nan_to_num(nan=float("inf"))
    return float(r.max()) if r.numel() else 0.0


def gn_check(ref, y, planes, ab, mean, what):
    """Every quantity of a GroupNorm run against `ref` (gn_reference / finalize_reference), each in its own units.  y [N,HW,C] 16-bit |
    None, planes: list of [N,P,C_i,2] fp32 (one per source) | None, ab [N,2,C] | None, mean [N,G] | None.  Returns {name: worst ratio}."""
    out = {}
    if planes is not None:
        for i, pl in enumerate(planes):
            assert bool(torch.isfinite(pl).all()), what + f": a statistics plane of source {i + 1} holds a non-finite entry"
        S = torch.cat([pl.double().sum(1) for pl in planes], 1)
        out["planes"] = max(compare(S[..., 0], ref["S"], ref["S_bnd"], what + " plane sums"), compare(S[..., 1], ref["Q"], ref["Q_bnd"], what + " plane sums of squares"))
    if ab is not None:
        out["ab"] = compare(ab.double(), ref["ab"], ref["ab_bnd"], what + " ab")
    if mean is not None:
        out["mean_out"] = compare(mean.double(), ref["mean"], ref["mean_bnd"], what + " mean_out")
    if y is not None:
        out["y"] = compare(y.double(), ref["y"], ref["y_bnd"], what + " y")
    return out


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
def ln_inputs(c, dt):
    g = gen_of(c["id"])
    rows, C = c["rows"], c["C"]
    sign = 1.0 - 2.0 * (torch.arange(rows) % 2).double()
    sigma = 0.5 + (torch.arange(rows) % 3).double() * 0.75
    x = (torch.randn(rows, C, generator=g, dtype=torch.float64) + (sign * float(c["offset"]))[:, None]) * sigma[:, None]
    if c["const_row"] is not None and c["const_row"] < rows:
        x[c["const_row"]] = 0.3
    gamma = (1 + 0.5 * torch.randn(C, generator=g)) if c["gamma"] else None
    beta = torch.randn(C, generator=g) if c["beta"] else None
    return x.to(dt), gamma, beta


def ln_reference(x, gamma, beta, dt, eps=EPS):
    x = x.double()
    C = x.shape[1]
    m = x.mean(1, keepdim=True)
    v = ((x - m) ** 2).mean(1, keepdim=True)
    dm = K_SUM * math.sqrt(C) * U32 * x.abs().mean(1, keepdim=True) + U32 * m.abs()
    dv = dm * dm + (K_SUM * math.sqrt(C) + 4) * U32 * (v + dm * dm)
    up = torch.sqrt((v + eps) / ((v - dv).clamp_min(0) + eps)) - 1
    lo = 1 - torch.sqrt((v + eps) / (v + dv + eps))
    rho = torch.maximum(up, lo) + 6 * U32
    rstd = 1 / torch.sqrt(v + eps)
    ga = gamma.double().to(x.device) if gamma is not None else torch.ones(C, dtype=torch.float64, device=x.device)
    be = beta.double().to(x.device) if beta is not None else torch.zeros(C, dtype=torch.float64, device=x.device)
    y = (x - m) * rstd * ga + be
    E = ga.abs() * rstd * (1 + rho) * dm + (y - be).abs() * (rho + 4 * U32) + U32 * y.abs()
    return y, out_bound(y, E, dt)


# ---- row softmax -------------------------------------------------------------------------------------------------------------------
def softmax_inputs(c):
    g = gen_of(c["id"])
    s = torch.randn(c["rows"], c["cols"], generator=g) * c["std"]
    if c["kind"] == "subnormal":                    # one dominant score; the others 10.5 .. 16 below it: p in 2^-23 .. 2^-15, fp16 subnormals
        s[0] = -10.5 - 5.5 * torch.rand(c["cols"], generator=g)
        s[0, 5] = 0.0
    return s


def _softmax_terms(s, arg_u, n):
    """fp64 softmax over the last dim and its relative error: e(x) = (arg_u |x| + 2) u per exponential, dl of the row sum."""
    s = s.double()
    x = s - s.max(-1, keepdim=True).values
    e = torch.exp(x)
    p = e / e.sum(-1, keepdim=True)
    ex = (arg_u * x.abs() + 2) * U32
    dl = (p * ex).sum(-1, keepdim=True) + K_SUM * math.sqrt(n) * U32
    return p, ex, dl


def softmax_reference(s, dt):
    p, ex, dl = _softmax_terms(s, 3.0, s.shape[-1])
    return p, out_bound(p, p * (ex + dl + 3 * U32) + FTZ, dt)


# ---- TFA prompt update -------------------------------------------------------------------------------------------------------------
def tfa_inputs(c, rows_cond=None):
    g = gen_of(c["id"])
    B, T_, D = c["B"], c["T"], c["D"]
    pooled = torch.randn(B, 3, T_ * D, generator=g) * 2
    cond = torch.randn(B if rows_cond is None else rows_cond, T_, D, generator=g)
    return pooled, cond


def tfa_reference(pooled, cond, T_, D):
    """pooled [B,3,T*D], cond [B,T,D] (already expanded to the rows of the output) -> (upd [B,T,D] fp64, bound)."""
    B = pooled.shape[0]
    pf, pi, pc = (pooled[:, j].reshape(B, T_, D) for j in range(3))
    f, ef, dlf = _softmax_terms(pf, 1.0, D)
    i, ei, dli = _softmax_terms(pi, 1.0, D)
    c = torch.tanh(pc.double())
    cond = cond.double()
    upd = f * cond + i * c
    E = (f * cond).abs() * (ef + dlf + 2 * U32) + (i * c).abs() * (ei + dli + 6 * U32) + U32 * upd.abs() + FTZ
    return upd, E


# ---- linear_f32 --------------------------------------------------------------------------------------------------------------------
def linear_inputs(c):
    g = gen_of(c["id"])
    M, N, K, G = c["M"], c["N"], c["K"], c["groups"]
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K // G, generator=g) / math.sqrt(K // G)
    b = torch.randn(N, generator=g) if c["bias"] else None
    return x, w, b


def linear_reference(x, w, b, groups, act):
    M, K = x.shape
    N, Kg = w.shape
    Ng = N // groups
    xd, wd = x.double(), w.double()
    z = torch.cat([xd[:, g * Kg:(g + 1) * Kg] @ wd[g * Ng:(g + 1) * Ng].t() for g in range(groups)], 1)
    A = torch.cat([xd[:, g * Kg:(g + 1) * Kg].abs() @ wd[g * Ng:(g + 1) * Ng].abs().t() for g in range(groups)], 1)
    if b is not None:
        z, A = z + b.double(), A + b.double().abs()
    E = (K_SUM * math.sqrt(Kg) + 1) * U32 * A
    if act == T.ACT_SILU:
        y, E = F.silu(z), SILU_D * E + SILU_EPS * z.abs()
    elif act == T.ACT_GELU:
        y, E = F.gelu(z), GELU_D * E + GELU_EPS
    elif act == T.ACT_TANH:
        y = torch.tanh(z)
        E = E + 4 * U32 * y.abs()
    elif act == T.ACT_RELU:
        y = z.clamp_min(0)
    else:
        y = z
    return y, E + U32 * y.abs()


# ---- depthwise 3x3 -----------------------------------------------------------------------------------------------------------------
def dwconv_inputs(c, dt, device="cpu"):
    g = torch.Generator(device=device).manual_seed(zlib.crc32(c["id"].encode()))
    N, H, W, C = c["N"], c["H"], c["W"], c["C"]
    x = torch.randn(N, H, W, C, generator=g, device=device)
    x += 3.0 * (torch.arange(N, device=device).float()[:, None, None, None] + 1)       # a tap that reaches into the neighbouring image shows
    w = torch.randn(9, C, generator=g, device=device)
    b = torch.randn(C, generator=g, device=device)
    return x.to(dt), w, b


def dwconv_reference(x, w, b, gate, dt):
    """Plain shifted multiply-adds (no library convolution) in fp64 on x's device."""
    N, H, W, C = x.shape
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    wd = w.double()
    o = b.double().expand(N, H, W, C).clone()
    A = b.double().abs().expand(N, H, W, C).clone()
    for dy in range(3):
        for dx in range(3):
            t = xp[:, dy:dy + H, dx:dx + W] * wd[dy * 3 + dx]
            o += t
            A += t.abs()
    del xp
    E = 11 * U32 * A
    if gate:
        h = C // 2
        o0, o1, E0, E1 = o[..., :h], o[..., h:], E[..., :h], E[..., h:]
        o, E = o0 * o1, o1.abs() * E0 + o0.abs() * E1 + E0 * E1 + U32 * (o0 * o1).abs()
    return o, out_bound(o, E, dt)


# ---- per-channel elementwise -------------------------------------------------------------------------------------------------------
def scale_reference(x, s, r, dt):
    """x [N,HW,C], s [N,C] fp32, r | None."""
    t = x.double() * s.double()[:, None, :]
    E = U32 * t.abs()
    y = t
    if r is not None:
        y = t + r.double()
        E = E + U32 * (t.abs() + r.double().abs())
    return y, out_bound(y, E, dt)


def axpy_reference(a, b, s, dt):
    t = b.double() * s.double()
    y = a.double() + t
    return y, out_bound(y, 2 * U32 * (a.double().abs() + t.abs()), dt)


def spade_reference(n, gb, C, r, dt):
    """n [rows,C], gb [rows,ldgb] (gamma | beta | padding), r | None."""
    nd, g, b = n.double(), gb[:, :C].double(), gb[:, C:2 * C].double()
    y = nd * (1 + g) + b
    A = nd.abs() * (1 + g.abs()) + b.abs()
    if r is not None:
        y, A = y + r.double(), A + r.double().abs()
    return y, out_bound(y, 3 * U32 * A, dt)


def vmg_reference(a, b, G):
    N, C = a.shape
    y = a.double() * b.double().repeat_interleave(C // G, dim=1)
    return y, U32 * y.abs() + FTZ


# ---- CPU emulations (numpy fp32) ---------------------------------------------------------------------------------------------------
f32 = np.float32


def _np(t):
    return t.float().numpy().astype(f32)


def pack16(a, dt):
    """numpy fp32 -> the 16-bit type (round to nearest even), as a torch tensor of dt."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dt)


def emu_gn_stats(x, count_clamped=False):
    """gn_stats_kernel: x fp32 [N,HW,C] -> planes fp32 [N,P,C,2].  Thread (r, channel) adds pixel rows p_begin + r + j R in order, four
    loads in flight with the row index clamped to the chunk; one thread per channel then adds the R rows in row order.
    count_clamped: the `break` behind the clamped loads is missing - the duplicate last pixel of a short chunk is counted."""
    N, HW, C = x.shape
    cvs, slabs, R, chunks, ppb, _ = T.gn_geom(N, HW, C, 8)
    part = np.zeros((N, chunks, C, 2), f32)
    rr = np.arange(R)
    for p in range(chunks):
        b, e = p * ppb, min(HW, (p + 1) * ppb)
        s, q = np.zeros((N, R, C), f32), np.zeros((N, R, C), f32)
        for p0 in range(b, e, 4 * R):
            active = (p0 + rr) < e
            for u in range(4):
                rows = p0 + u * R + rr
                take = (rows < e) | (active if count_clamped else False)
                f = x[:, np.minimum(rows, e - 1), :] * take[None, :, None].astype(f32)
                s += f
                q += f * f
        a, c2 = np.zeros((N, C), f32), np.zeros((N, C), f32)
        for r in range(R):
            a += s[:, r]
            c2 += q[:, r]
        part[:, p, :, 0], part[:, p, :, 1] = a, c2
    return part


def emu_gn_finalize(p1, p2, gamma, beta, G, HW, eps=EPS, drop_last=False, stride_c1=False, first_channel_group=False):
    """gn_finalize_kernel: fp32 planes -> (ab fp32 [N,2,C], mean fp32 [N,G]): fp64 sums, var = Q/cnt - mean^2, rsqrt in fp32.
    drop_last: the last partial of every source is left out.  stride_c1: source-2 partials indexed with the source-1 channel stride.
    first_channel_group: a 16-byte vector's (a, b) use the statistics of the group of its first channel."""
    N, P1, C1, _ = p1.shape
    C2 = 0 if p2 is None else p2.shape[2]
    C, cpg = C1 + C2, (C1 + C2) // G
    s1 = p1[:, :P1 - 1 if drop_last else P1].astype(np.float64).sum(1)
    if p2 is not None:
        P2 = p2.shape[1]
        if stride_c1:
            flat = p2.reshape(N, -1)
            idx = ((np.arange(P2)[:, None] * C1 + np.arange(C2)[None, :]) * 2) % (flat.shape[1] - 1)
            src = np.stack([flat[:, idx], flat[:, idx + 1]], -1)                # [N,P2,C2,2]
        else:
            src = p2
        s1 = np.concatenate([s1, src[:, :P2 - 1 if drop_last else P2].astype(np.float64).sum(1)], 1)
    sg = s1.reshape(N, G, cpg, 2).sum(2)
    inv = 1.0 / (cpg * HW)
    mean = sg[..., 0] * inv
    var = sg[..., 1] * inv - mean * mean
    rstd = (f32(1) / np.sqrt(np.maximum(var.astype(f32), f32(0)) + f32(eps))).astype(f32)
    ch = np.arange(C)
    grp = ((ch // 8) * 8) // cpg if first_channel_group else ch // cpg
    ga = np.ones(C, f32) if gamma is None else _np(gamma)
    be = np.zeros(C, f32) if beta is None else _np(beta)
    a = (rstd[:, grp] * ga[None, :]).astype(f32)
    b = (be[None, :] - mean.astype(f32)[:, grp] * a).astype(f32)
    return np.stack([a, b], 1), mean.astype(f32)


def emu_gn_apply(x, ab, silu, dt):
    """gn_apply_body: y = act(a x + b) in fp32, packed to dt.  x fp32 [N,HW,C], ab [N,2,C]."""
    o = (x * ab[:, 0][:, None, :]).astype(f32) + ab[:, 1][:, None, :]
    if silu:
        with np.errstate(over="ignore"):                         # exp(-o) = inf for o < -88: o / inf = -0, as in the kernel
            o = (o / (f32(1) + np.exp(-o, dtype=f32))).astype(f32)
    return pack16(o, dt)


def emu_groupnorm(x1, x2, gamma, beta, G, silu, dt, mutation=None):
    """The whole path on 16-bit tensors: (y dt, planes1, planes2 | None, ab, mean)."""
    a1 = _np(x1)
    a2 = None if x2 is None else _np(x2)
    pl1 = emu_gn_stats(a1, count_clamped=mutation == "clamped_pixel_counted")
    pl2 = None if a2 is None else emu_gn_stats(a2, count_clamped=mutation == "clamped_pixel_counted")
    ab, mean = emu_gn_finalize(pl1, pl2, gamma, beta, G, x1.shape[1], drop_last=mutation == "last_partial_dropped",
                               stride_c1=mutation == "source2_stride_c1", first_channel_group=mutation == "vector_first_channel_group")
    x = a1 if a2 is None else np.concatenate([a1, a2], -1)
    return emu_gn_apply(x, ab, silu, dt), pl1, pl2, ab, mean


def _butterfly(v):
    """wave_sum: 6 xor-shuffle steps over the last axis (64 lanes); every lane ends with the same total."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ o]).astype(f32)
    return v[..., 0]


def emu_layernorm(x, gamma, beta, dt, eps=EPS, masked_lanes_add_mean2=False):
    """ln_rows_kernel: lane l owns vectors l, l + 64, ...; per-lane sums in (j, e) order, butterfly, exact two-pass variance.
    masked_lanes_add_mean2: the variance loop is not masked - every dead lane element adds (0 - mean)^2."""
    xs = _np(x)
    rows, C = xs.shape
    vpl = (C // 8 + 63) // 64
    pad = np.zeros((rows, vpl * 512), f32)
    pad[:, :C] = xs
    f = pad.reshape(rows, vpl, 64, 8)
    live = (np.arange(vpl * 512) < C).reshape(vpl, 64, 8)
    s = np.zeros((rows, 64), f32)
    for j in range(vpl):
        for e in range(8):
            s += f[:, j, :, e]
    mean = (_butterfly(s) / f32(C)).astype(f32)
    q = np.zeros((rows, 64), f32)
    for j in range(vpl):
        for e in range(8):
            d = (f[:, j, :, e] - mean[:, None]).astype(f32)
            if not masked_lanes_add_mean2:
                d = d * live[j, :, e][None, :].astype(f32)
            q += d * d
    rstd = (f32(1) / np.sqrt(_butterfly(q) / f32(C) + f32(eps))).astype(f32)
    ga = np.ones(C, f32) if gamma is None else _np(gamma)
    be = np.zeros(C, f32) if beta is None else _np(beta)
    o = ((xs - mean[:, None]) * rstd[:, None]).astype(f32) * ga[None, :] + be[None, :]
    return pack16(o, dt)


def emu_softmax(s, dt, three_waves=False):
    """softmax_rows_kernel: thread t adds exp(s[t + 256 j] - m) in order, one butterfly per wave, ((w0 + w1) + w2) + w3, p = e * (1 / l).
    three_waves: the row sum leaves out the fourth wave."""
    s = s.numpy().astype(f32)
    rows, cols = s.shape
    m = s.max(1, keepdims=True)
    e = np.exp((s - m).astype(f32), dtype=f32)
    trips = (cols + 255) // 256
    pad = np.zeros((rows, trips * 256), f32)
    pad[:, :cols] = e
    l = np.zeros((rows, 256), f32)
    for j in range(trips):
        l += pad[:, j * 256:(j + 1) * 256]
    w = _butterfly(l.reshape(rows, 4, 64))
    tot = ((w[:, 0] + w[:, 1]).astype(f32) + w[:, 2]).astype(f32)
    if not three_waves:
        tot = (tot + w[:, 3]).astype(f32)
    inv = (f32(1) / tot).astype(f32)
    return pack16(e * inv[:, None], dt)


def emu_tfa(pooled, cond, T_, D):
    B = pooled.shape[0]
    p = pooled.numpy().astype(f32).reshape(B, 3, T_, D)

    def sm_(a):
        e = np.exp((a - a.max(-1, keepdims=True)).astype(f32), dtype=f32)
        return (e / e.sum(-1, keepdims=True, dtype=f32)).astype(f32)
    return torch.from_numpy((sm_(p[:, 0]) * cond.numpy().astype(f32) + sm_(p[:, 1]) * np.tanh(p[:, 2], dtype=f32)).astype(f32))


def emu_linear(x, w, b, groups, act):
    """linear_f32_kernel: lane l adds k = l, l + 64, ... in order, butterfly over the 64 lanes, bias, activation (exact functions)."""
    x, w = x.numpy().astype(f32), w.numpy().astype(f32)
    M, K = x.shape
    N, Kg = w.shape
    Ng = N // groups
    y = np.zeros((M, N), f32)
    steps = (Kg + 63) // 64
    for g in range(groups):
        xs = np.zeros((M, steps * 64), f32)
        xs[:, :Kg] = x[:, g * Kg:(g + 1) * Kg]
        ws = np.zeros((Ng, steps * 64), f32)
        ws[:, :Kg] = w[g * Ng:(g + 1) * Ng]
        acc = np.zeros((M, Ng, 64), f32)
        for j in range(steps):
            acc += xs[:, None, j * 64:(j + 1) * 64] * ws[None, :, j * 64:(j + 1) * 64]
        y[:, g * Ng:(g + 1) * Ng] = _butterfly(acc)
    if b is not None:
        y = y + b.numpy().astype(f32)[None, :]
    t = torch.from_numpy(y.astype(f32))
    return {T.ACT_SILU: F.silu, T.ACT_GELU: F.gelu, T.ACT_TANH: torch.tanh, T.ACT_RELU: torch.relu}.get(act, lambda v: v)(t)


def emu_dwconv(x, w, b, gate, dt):
    xs, ws, bs = _np(x), w.numpy().astype(f32), b.numpy().astype(f32)
    N, H, W, C = xs.shape
    xp = np.zeros((N, H + 2, W + 2, C), f32)
    xp[:, 1:H + 1, 1:W + 1] = xs
    o = np.broadcast_to(bs, (N, H, W, C)).astype(f32).copy()
    for dy in range(3):
        for dx in range(3):
            o += xp[:, dy:dy + H, dx:dx + W] * ws[dy * 3 + dx]
    if gate:
        o = o[..., :C // 2] * o[..., C // 2:]
    return pack16(o, dt)


def emu_scale(x, s, r, dt):
    o = _np(x) * s.numpy().astype(f32)[:, None, :]
    return pack16(o if r is None else o + _np(r), dt)


def emu_axpy(a, b, s, dt):
    return pack16(_np(a) + _np(b) * s.numpy().astype(f32), dt)


def emu_spade(n, gb, C, r, dt):
    o = _np(n) * (f32(1) + _np(gb[:, :C])) + _np(gb[:, C:2 * C])
    return pack16(o if r is None else o + _np(r), dt)


def emu_vmg(a, b, G):
    return torch.from_numpy(a.numpy().astype(f32) * np.repeat(b.numpy().astype(f32), a.shape[1] // G, axis=1))


# name -> (family, what a wrong kernel would do)
MUTATIONS = {
    "vector_first_channel_group": ("groupnorm", "a 16-byte vector's (a, b) taken from the group of its first channel only (cpg < 8, cpg = 10)"),
    "last_partial_dropped": ("groupnorm", "finalize leaves out the last partial chunk"),
    "source2_stride_c1": ("groupnorm", "source-2 partials indexed with the source-1 channel stride"),
    "clamped_pixel_counted": ("groupnorm", "the clamped duplicate pixel of a short chunk counted in the statistics"),
    "masked_lanes_add_mean2": ("layernorm", "LayerNorm's masked lanes add mean^2 to the variance (C = 520, 1544)"),
    "three_waves": ("softmax", "the softmax row sum taken from three of the four waves"),
}
