"""fp64 reference, per-element bound and CPU emulation of the attention parity matrix (tests/test_attention_launchers_gpu.py).

Reference: fp64 torch on the 16-bit-rounded q, k, v the kernel reads, in the exp2 domain the kernels work in:
    s_k = c q.k,  c = fp32(scale * log2(e)),  w_k = 2^(s_k - max s) / sum,  ref = sum_k w_k v_k.
Where the ping-pong kernel runs and c != 1 it multiplies the 16-bit q by c in fp32 and rounds it to 16 bits a second time
(include/unirestore_hip.h, "Scale convention"): the reference then uses q' = round16(fp32(q) * c) and c = 1.  Everywhere else q is
used as given.

Bound: with A = sum w|v|, Q2 = sqrt(sum w^2 v^2), W2 = sqrt(sum w^2), every output element must satisfy

    |o - ref| <= u_out |ref| + abs_out + C u_P (Q2 + W2 |ref|) + (C sqrt(Tk) 2^-24 + 2 eps_s) A + E_sub

  * u_out |ref| + abs_out: the one rounding of the stored 16-bit output (tests/conv_reference.py U_OUT, ABS_OUT);
  * C u_P (Q2 + W2 |ref|): P is a 16-bit MFMA operand, u_P = u_out of the type.  Every p_k carries an independent relative rounding
    error <= u_P: the numerator sum p_k v_k moves by a random walk over the terms, u_P sqrt(sum p^2 v^2), and so does the row sum
    where it is taken from the rounded P (ping-pong kernel; the 128-query and d = 512 kernels sum the unrounded fp32 p, for them
    the W2 term is slack).  Divided by the row sum these are u_P Q2 and u_P W2 |ref|.  The stale reference maximum (p up to 2^8 or
    2^14) scales numerator and row sum alike and drops out;
  * E_sub = sum_k min(w_k, abs_P w_max) (|v_k| + |ref|), abs_P = 2^-25 (fp16), 2^-134 (bf16): the relative model of the line above
    holds for NORMAL 16-bit numbers only.  An fp16 p_k below 2^-14 is a subnormal (spacing 2^-24): its rounding error is up to
    2^-25 ABSOLUTE, and below 2^-25 it becomes 0 (error p_k).  p is taken against a reference maximum that is never above the
    row's true maximum, so the row sum is >= 1 in the units of p and an absolute error e of p_k is an error <= e w_max of w_k;
    tiles rounded against an older, lower reference are scaled DOWN by the later rescale (and by the combine kernel's weights).
    These errors are one-sided where p is flushed, so they are summed, not random-walked.  For ordinary rows the term is
    ~2^-25 w_max Tk |v|, a few per cent of u_out |ref|; it matters where one key takes nearly all the weight (w_max ~ 1) and its
    v is small - found on the MI355X by the split_jump inputs in fp16 (13 of 8.4 M elements at up to 3.0 x the bound without the
    term; bf16 0.52) and reproduced by emulate() on the "dominant" input kind, which
    tests/test_attention_plan_cpu.py keeps as the proof that the term is needed.  In bf16 it is ~0;
  * C sqrt(Tk) 2^-24 A: fp32 accumulation of Tk products p_k v_k and of the row sum, as for a GEMM of depth Tk (conv_reference.py);
  * 2 eps_s A: a score error delta_k (exp2 domain, |delta_k| <= eps_s) moves w_k by the factor 2^delta_k and the row sum by at most
    2^eps_s: |d o| <= ln 2 eps_s (sum w|v| + |ref|) <= 2 ln 2 eps_s A < 2 eps_s A;
  * C = 4 (conv_reference.C_BOUND), fixed for every case and kernel, never tuned; no constant is fitted to a kernel's output.

eps_s, the score error in the exp2 domain, from the kernels' arithmetic (csrc/attention.hip, attention512.hip, attention_pp.hip):
  (1) s = q.k: D exact products of 16-bit values accumulated in fp32 by the MFMA: C sqrt(D) 2^-24 A_s with
      A_s = c max_k sum_d |q_d k_d| (the ping-pong kernel starts the accumulator at -m instead of 0: |m| <= max|s| <= A_s, inside C);
  (2) the exponent's argument.  The 128-query and d = 512 kernels form t = fma(s, c, -(m c)): m c is rounded to fp32 once per tile
      (<= 2^-24 R with R = max_k |s_k|: the SAME error for every key of a tile, but tiles before and after a reference change see
      different ones, so it does not cancel in the normalisation) and the fma rounds once (<= 2^-24 |t|, |t| <= 2 R + 14: the row's
      score range below the reference, the 2^14 head-room of the deferred rescale above it).  The rescale factor 2^((m_old - m_new) c)
      has the same two roundings on a smaller argument.  Together <= 2^-24 (3 R + 14).  The ping-pong kernel has t in the
      accumulator already; its share of (2) is slack;
  (3) v_exp_f32 is accurate to 1 ulp: a relative error 2^-23 of p, which is a score error 2^-23 / ln 2 < 3 * 2^-24.
      eps_s = 2^-24 (C sqrt(D) A_s + 3 R + 17).

compare() checks every element and names the first violating (batch, query, head, channel); NaN never satisfies the bound.  The
whole-tensor rel-L2 tolerances stay the project's (REL_TOL: 6e-3 / 8e-4 = 2 x the GEMM tolerance, tests/test_ops_gpu.py), checked
in addition.

emulate() is the throw-away model the bound was tried on, kept so that tests/test_attention_plan_cpu.py re-establishes it on the CPU:
64-key tiles, fp32 scores and accumulators, P rounded to 16 bits against a stale reference maximum with 2^8 or 2^14 head-room,
the row sum taken from the rounded P.
"""
import math

import torch

from conv_reference import ABS_OUT, C_BOUND, U_OUT

LOG2E = 1.4426950408889634
REL_TOL = {torch.bfloat16: 6e-3, torch.float16: 8e-4}
ABS_P = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}      # half the spacing of the type's subnormals
KINDS = ("randn", "v2", "peaked", "jumps", "negative", "split_jump", "spike", "dominant")


def scale_of(scale, D):
    """The `scale` argument of ur_attention_fwd_ws for a case's scale convention."""
    return {"folded": math.log(2.0), "passed": 1.0 / math.sqrt(D), "one": 1.0}[scale]


def c_of(scale):
    """scale * log2(e) as the launch computes it: (float)((double)(float)scale * log2(e))."""
    f32 = torch.tensor(scale, dtype=torch.float32)
    return float((f32.double() * LOG2E).float())


def inputs(kind, scale, B, H, Tq, Tk, D, dt, gen, nb=None):
    """Logical q [B][Tq][C], k, v [nb][Tk][C] of an input kind: fp32 values already rounded to dt (CPU)."""
    C = H * D
    nb = B if nb is None else nb
    q = torch.randn(B, Tq, C, generator=gen)
    k = torch.randn(nb, Tk, C, generator=gen)
    v = torch.randn(nb, Tk, C, generator=gen)
    if kind == "v2":
        v += 2
    elif kind == "peaked":
        q *= 4
    elif kind == "jumps":         # tests/test_attention_pp_gpu.py test_pp_attention_online_softmax_slow_path
        k[0, (3 * 64 + 7) % Tk, :D] = q[0, 5 % Tq, :D] * 6            # row 5, head 0: score ~ 6 |q|^2 / 8 ~ 48
        k[0, (9 * 64 + 1) % Tk, :D] = q[0, 5 % Tq, :D] * 12           # again, higher, later
        k[0, Tk - 1, C - D:] = q[0, 300 % Tq, C - D:] * 30            # last head: ~ 240 in the last tile
        q[0, 700 % Tq, :D] *= 40                                       # a row with a wide score range from tile 0 on
    elif kind == "negative":      # test_pp_attention_all_scores_far_below_zero: q.k = -20 |base|^2 for every key
        base = torch.randn(1, 1, C, generator=gen)
        q = base + 0.01 * q
        k = -20 * base + 0.01 * k
    elif kind == "split_jump":    # test_pp_attention_key_split_last_round: a jump inside the SECOND key half, + one in a split tile
        b0 = min(3, B - 1)
        k[b0 % nb, 700 % Tk, :D] = q[b0, 40 % Tq, :D] * 9
        k[(B - 1) % nb, 700 % Tk, C - D:] = q[B - 1, (Tq - 40) % Tq, C - D:] * 9
    elif kind == "spike":         # tests/test_ops_gpu.py test_attention_softmax_spike
        k[0, 200 % Tk] = q[0, 5 % Tq] * 8
    elif kind == "dominant":      # one key takes nearly all the weight of every row (batch 0, head 0) and its v is tiny: the other
        base = torch.randn(D, generator=gen)      # keys sit ~20 below it in the exp2 domain, where an fp16 P is a subnormal
        q[0, :, :D] = 0.3 * q[0, :, :D] + base
        k[0, 700 % Tk, :D] = base * (14 / math.sqrt(D))
        v[0, 700 % Tk, :D] *= 2.0 ** -15
    elif kind != "randn":
        raise ValueError(kind)
    if scale == "folded":         # modules/nn.py Q_FOLD: the factor enters BEFORE the one rounding of q
        q = q * (LOG2E / math.sqrt(D))
    return tuple(t.to(dt).float() for t in (q, k, v))


def _q_as_the_kernel_uses_it(q, dt, c, pingpong):
    """(q, c) of the scores s = c q.k: the ping-pong kernel folds c != 1 into q with a second 16-bit rounding; else unchanged."""
    if pingpong and c != 1.0:
        q = (q.float() * torch.tensor(c, dtype=torch.float32, device=q.device)).to(dt).float()
        c = 1.0
    return q, c


def reference(q, k, v, H, D, scale, dt, pingpong, elems=1 << 24, e_sub=True):
    """q [B][Tq][C], k / v [nb][Tk][C] (nb = B or 1; fp32 values of dt numbers, any device) -> (ref, bound) fp64 [B][Tq][C].
    Query chunks of <= elems / Tk rows keep the fp64 score block bounded (T = 16384 fits).  e_sub=False leaves E_sub out of the
    bound (only to show that it is needed)."""
    B, Tq, C = q.shape
    nb, Tk, _ = k.shape
    q, c = _q_as_the_kernel_uses_it(q, dt, c_of(scale), pingpong)
    u, ab = U_OUT[dt], ABS_OUT[dt]
    ref = torch.empty(B, Tq, C, dtype=torch.float64, device=q.device)
    bnd = torch.empty_like(ref)
    rows = max(1, elems // Tk)
    for b in range(B):
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            kh, vh = k[b % nb, :, sl].double(), v[b % nb, :, sl].double()
            kha, vha, vh2 = kh.abs().t().contiguous(), vh.abs(), vh * vh
            kht = kh.t().contiguous()
            for r0 in range(0, Tq, rows):
                qh = q[b, r0:r0 + rows, sl].double()
                s = (qh @ kht) * c
                R = s.abs().amax(1)
                A_s = (qh.abs() @ kha).amax(1) * c
                s -= s.amax(1, keepdim=True)
                w = torch.exp2(s)
                w /= w.sum(1, keepdim=True)
                o = w @ vh
                A = w @ vha
                wc = torch.minimum(w, w.amax(1, keepdim=True) * (ABS_P[dt] if e_sub else 0.0))
                sub = wc @ vha + wc.sum(1, keepdim=True) * o.abs()
                del wc
                w *= w
                Q2 = (w @ vh2).sqrt()
                W2 = w.sum(1, keepdim=True).sqrt()
                eps_s = 2.0 ** -24 * (C_BOUND * math.sqrt(D) * A_s + 3 * R + 17)
                ref[b, r0:r0 + rows, sl] = o
                bnd[b, r0:r0 + rows, sl] = u * o.abs() + ab + C_BOUND * u * (Q2 + W2 * o.abs()) + \
                    (C_BOUND * math.sqrt(Tk) * 2.0 ** -24 + 2 * eps_s[:, None]) * A + sub
    return ref, bnd


def compare(o, ref, bnd, H, D, what=""):
    """Element-wise |o - ref| <= bnd (fp64 [B][Tq][H*D]).  Returns max |o - ref| / bnd; raises AssertionError naming the first
    violating (batch, query, head, channel) - a NaN anywhere is one."""
    err = (o - ref).abs()
    ok = err <= bnd
    if not bool(ok.all()):
        bad = (~ok).nonzero()[:6].tolist()
        det = "; ".join(f"(batch {b}, query {t}, head {ch // D}, channel {ch % D}): got {float(o[b, t, ch]):.6g} ref {float(ref[b, t, ch]):.6g} "
                        f"bound {float(bnd[b, t, ch]):.3g}" for b, t, ch in bad)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside the bound - {det}")
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.zeros_like(err))
    return float(ratio.max()) if ratio.numel() else 0.0


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def emulate(q, k, v, H, D, scale, dt, headroom, pingpong):
    """The kernels' arithmetic on the CPU (see the module docstring): fp32 [B][Tq][C] values of dt numbers."""
    B, Tq, C = q.shape
    nb, Tk, _ = k.shape
    q, c = _q_as_the_kernel_uses_it(q, dt, c_of(scale), pingpong)
    c = torch.tensor(c, dtype=torch.float32)
    out = torch.empty(B, Tq, C)
    for b in range(B):
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            qh, kh, vh = q[b, :, sl], k[b % nb, :, sl], v[b % nb, :, sl]
            m = torch.full((Tq,), -1e30)
            l = torch.zeros(Tq)
            acc = torch.zeros(Tq, D)
            for t0 in range(0, Tk, 64):
                s = (qh @ kh[t0:t0 + 64].t()) * c                       # fp32 scores, exp2 domain
                mx = s.amax(1)
                m_new = torch.where(mx - m > headroom, torch.maximum(m, mx), m)
                alpha = torch.exp2(m - m_new)
                l, acc, m = l * alpha, acc * alpha[:, None], m_new
                p = torch.exp2(s - m[:, None]).to(dt).float()             # the 16-bit MFMA operand
                l = l + p.sum(1)                                          # row sum from the rounded P
                acc = acc + p @ vh[t0:t0 + 64]
            out[b, :, sl] = acc / l[:, None]
    return out.to(dt).float()
