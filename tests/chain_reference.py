"""Stream decoder, staged fp64 reference, per-element bound and CPU emulation of the fused-chain parity matrix
(tests/test_chain_launchers_gpu.py, tests/test_chain_stream_cpu.py; cases: tests/chain_cases.py; kernels: csrc/tchain.hip).

Decoder
-------
decode(kind, stream, dt, ...) reads a packed weight stream the way the KERNEL reads it, not by inverting the packer
(unirestore_amd/chain.py lds_block / perm_rows): two independent statements of the layout that must agree.
  * a tile is 40960 weight bytes + 4096 aux bytes; a weight block is [rows][128 B];
  * TChain::init: the lane of MFMA row j reads k-step s (k = 16 s + 8 h .. + 7) at byte j * 128 + (((2 s + h) ^ ((j >> 1) & 7)) << 4),
    so element (row r, k) sits at r * 128 + (((k >> 3) ^ ((r >> 1) & 7)) << 4) + 2 (k & 7);
  * the 32x32 MFMA accumulator register e of lane half h is row 8 (e >> 2) + 4 h + (e & 3), and the chain packs registers 8 u .. 8 u + 7
    as the CONSECUTIVE channels 16 u + 8 h .. + 7 of the next stage's B operand: channel c of a 32-row block therefore lives in MFMA
    row (c & 3) | ((c >> 3) & 1) << 2 | ((c >> 2) & 1) << 3 | (c & 16);
  * aux vectors (aux_base = tile + 40960 + 32 h, fragment offsets 128 f + 64 u bytes) are in natural channel order: a bias-only stage
    has its bias at floats 0.. of its LAST tile (aux_vec4), a LayerNorm-folded stage bias' at 0.. and column sums at 512.. (aux_bc),
    an FF1 tile ba | bg | colsum a | colsum g at floats 0 / 32 / 64 / 96 (aux_ff1);
  * stream order as documented above each kernel: an N = 320 stage is K / 64 tiles of [320][128 B]; an FF1-shaped tile is 5 blocks
    (k tiles) of [32 a rows | 32 g rows] at 8192 kb (+ 4096 for g); FF is (FF1 tile, FF1 tile, FF2 tile) per 64 hidden units; a TAIL
    head is (to_q2 tile, K_h [96][128 B] at 0 + V^T_h as two [64][128 B] blocks at 12288 / 20480, to_out2 k tile).
decode also returns the mask of 16-bit words the layout uses; the rest of a packed stream must be zero.

Staged reference
----------------
reference(kind, dec, inp, ...) runs the chain in fp64 on the decoded 16-bit weights and the 16-bit-rounded inputs, and rounds every
intermediate to the 16-bit type exactly where the kernel packs it: the GroupNorm-affine input, h0 and q / k / v of HEAD; s, the GELU
output and the result of CSCE; the GEGLU hidden units; h1, q2, the unnormalised P (against the row maximum over the real keys), o2
after * 1 / l, h2, h3 and y of TAIL.  Row statistics are two-pass on the rounded values (row_stats).

Bound
-----
Every stage computes z (before its rounding) from 16-bit operands.  With the kernel's operands equal to the reference's,
    |z_kernel - z_ref| <= b_own = C sqrt(K) 2^-24 M + eps_act,      C = 4 (conv_reference.C_BOUND), K = the stage's GEMM depth,
  * M = |x| . |W| + |bias| for a bias stage (conv_reference.py: fp32 accumulation of K exact products);
  * M = rstd (A + m_abs |colsum|) + |bias'| for a LayerNorm-folded stage, A = |x| . |W'|, m_abs = mean |x| >= |mean|: the fold
    rstd * (acc - mean * colsum) + bias' cancels when |mean| >> std, and the fp32 error of acc, of mean (<= sqrt(K) 2^-24 m_abs) and of
    the two fmas is relative to the cancelling magnitudes, not to the result.  rstd itself (two-pass variance, rsqrt) has a relative
    error <= C sqrt(K) 2^-24, which enters on |z - bias'|: one more term S = C sqrt(K) 2^-24 rstd |acc - mean colsum|;
  * GELU (csrc/common.h gelu_f): b -> 1.13 b + 2.6e-5; GEGLU a * gelu(g): |gelu(g)| b_a + |a| (1.13 b_g + 2.6e-5)
    (conv_reference.GELU_D, GELU_EPS);
  * the GroupNorm affine of HEAD is one fp32 fma: 2^-24 |a x + b|.
Intermediate roundings that can go either way.  The kernel rounds z_kernel to 16 bits, the reference z_ref.  Where both round to the
same number the stage hands NO error on; where a rounding boundary lies between them the two 16-bit values differ by a whole
spacing, however small |z_kernel - z_ref| is.  Val.var is the modelled VARIANCE, per element, of (the kernel's 16-bit value - the
reference's): E[delta^2] under the model below, 0 for inputs.
  * Flip model (_rnd, _FLIP_X, _FLIP_W).  The stage bound b is read as C standard deviations: e = z_kernel - z_ref is taken as
    Gaussian with sigma = b / C.  (b_own is C times a sqrt(K) 2^-24 random-walk estimate to begin with; the kernel's real error is
    smaller than that sigma, which only lowers its chance of crossing.)  A boundary at distance g from z_ref is crossed with
    probability Phi(-g / sigma).  _rnd evaluates var = sum_j w_j [(round(z + x_j sigma) - round z)^2 + (round(z - x_j sigma) - round z)^2]
    on the grid x_j = 0.5, 1, .. 4 with one-sided masses w_j = Phi(x_j) - Phi(x_j - 0.5), the last one the whole tail beyond 3.5.
    For a boundary at g the grid points that see it are x_j >= g / sigma, and their masses add up to 1 - Phi(x_j* - 0.5) with
    x_j* - 0.5 < g / sigma: never less than the true probability, so the grid is conservative.  Nothing is evaluated beyond
    4 sigma = b: an element whose nearest boundary is further than its own derived stage bound is not ambiguous and carries 0 (the
    window is the derived b, not a fixed relative one).  round() is the real conversion, so binade edges, fp16 subnormals and
    windows wider than one spacing are what they are.
  * Independence.  The flips of different elements are taken as independent and of either sign (each depends on where its own
    z_ref lies between two boundaries), so variances add through linear maps and nothing else is assumed about them.
  * Through a GEMM: var z_n = sum_k W_nk^2 var_k (_through).  Through a residual: var adds.  Through GELU: x 1.13^2.
  * Through LayerNorm statistics, to first order: d mean = sum_k delta_k / K has variance sum var_k / K^2 and moves z by
    rstd |colsum| d mean; d rstd = -rstd^3 sum_k (x_k - mean) delta_k / K has variance rstd^6 sum (x_k - mean)^2 var_k / K^2 and moves
    z by |acc - mean colsum| d rstd; together with rstd sqrt(sum W'^2 var) these three are added as magnitudes (_LN.dmean, _LN.drstd).
  * C is applied ONCE per stage: b = b_own + C sqrt(propagated variance), and the output bound of a launch is
        |y - z_ref| <= u_out |z_ref| + abs_out + b                                              (conv_reference.U_OUT, ABS_OUT).
Why not the plainer forms.  Letting every ambiguous element carry one whole spacing d - worst case sum |W| d, or the random walk
C sqrt(sum W^2 d^2) - is admissible but does not close on a chain: with the window b = C sigma a fraction f of the inputs being
ambiguous makes the consumer's bound ~8 sqrt(f) of ITS spacing (320 inputs, |W| ~ 320^-1/2, C = 4, d = 2 u |x|), which is > f for
every f < 1: after three stages every element is ambiguous, then the windows exceed a spacing and the bound grows 4-8 x per stage
(17 700 output ulps at tail_tk77; MLP, HEAD and CSCE, one or two roundings deep, were unaffected).  The whole-spacing forms count an
element whose boundary sits at 3.9 sigma like one at 0; the flip model counts it with its probability, 5e-5.  It also is what
happens: a flip turns an error of 1e-4 spacings into a whole one, so kernel and staged reference drift apart like the square root
per stage until they differ by independent roundings.
WHAT KIND OF BOUND THIS IS.  A 4-sigma statistical bound, not a worst-case one: b_own already is (C sqrt(K) 2^-24 against the worst
case K 2^-24), and the ambiguity term now is too.  A correct kernel may leave it with the probability of a 4-sigma event per
element; nothing proves it cannot.  It rests on two observations: emulate() - fp32 in another summation order, so with flips of its
own - stays inside it on every case and type (tests/test_chain_stream_cpu.py, worst ratio 0.99 where the output rounding alone
reaches u_out |ref|, 0.78 on TAIL), and so does the kernel on the GPU.  The worst-case sum over ambiguous elements
remains the admissible fallback if either ever fails for a reason that is not a bug.
TAIL's cross-attention (one pass over tk <= 80 keys, true row maximum, row sum l from the UNROUNDED fp32 p, o = (sum P16 v) / l) is
two more stages of the same kind, with the terms of attention_reference.py specialised to them:
  * scores in the exp2 domain carry eps_s = 2^-24 (C sqrt(64) A_s + 3 R + 17) as derived there (A_s = c max_k sum |q k|,
    R = max |c s|, c = fp32(scale) * fp32(log2 e)) plus dt_k = c C sqrt(sum_d K_kd^2 var q2_d) from the flips of q2 (variances as above);
  * P: the reference rounds p_k = 2^(t_k - t_max) to the 16-bit type where the kernel does, with the stage bound
    (ln 2 r_k + 2^-23) p_k, r_k = (eps_s + dt_k) + (eps_s + dt_max): both scores of the difference are uncertain.  The largest
    key's own p is 1 whatever its score; it carries r = max_j max(0, r_j - (t_max - t_j)), how far another key can get above it
    (0 where one key leads by more than the uncertainty: the rows of the "peaked" kind).
    This replaces the P-rounding term C u_P (Q2 + W2 |ref|) and E_sub of attention_reference: there the reference keeps P unrounded
    and every p_k carries u_P; here only the p_k that can round either way carry anything, and an fp16 subnormal p_k is rounded (or
    flushed) by the reference exactly as by the kernel.  (Kept as in attention_reference the term alone is 4 u_out |o| - Q2 ~ |o| for
    tk keys of similar weight - and every element of o2 becomes ambiguous.)  The W2 term is not needed: l is not taken from the
    rounded P;
  * o = (sum P16 v) / l: b_o = C sqrt(sum_k var P_k v_k^2) / l + C sqrt(tk) 2^-24 A + (2^-22 + ln 2 sum_k w_k r_k) |o|,
    w = p / l, A = sum w |v|: the flips of P, the fp32 accumulation, v_rcp_f32 (1 ulp) and its product, and the score error in l.
No constant is fitted to a kernel's output.  NaN never satisfies the bound (conv_reference.compare).

GroupNorm partial planes are checked with conv_reference.compare_sums per (image, part, channel) against fp64 sums of the kernel's own
16-bit y over that part's 128 tokens.  HEAD's q / k / v are additionally checked against the fp64 fold of the kernel's own h0
(reference_from_h0: no ambiguity term).

emulate(kind, dec, inp, ...) mirrors the kernel in fp32 on the decoded stream: 16-bit packs at the same points, gelu_f written
out, two-pass statistics, the masked softmax.  fault= names one of the mutations tests/test_chain_stream_cpu.py proves the bound
sharp against.
"""
import math
import zlib

import torch
import torch.nn.functional as F

import chain_cases as T
from conv_reference import ABS_OUT, C_BOUND, GELU_D, GELU_EPS, U_OUT
from attention_reference import ABS_P, LOG2E, REL_TOL, rel_l2  # noqa: F401  (REL_TOL, rel_l2: used by the tests)

TILE_W, TILE_AUX = 40960, 4096
TILE = TILE_W + TILE_AUX
C = T.C
LN_EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------------ decoder
def _mfma_row(c):
    """MFMA row of a 32-row block that holds channel c (accumulator layout of v_mfma_f32_32x32x16, see the module docstring)"""
    return (c & 3) | (((c >> 3) & 1) << 2) | (((c >> 2) & 1) << 3) | (c & 16)


def _block_bytes(rows):
    """[rows][64] byte offsets inside a [rows][128 B] block of element (channel n, k)"""
    n = torch.arange(rows)
    r = (n & ~31) | _mfma_row(n & 31)
    k = torch.arange(64)
    return r[:, None] * 128 + (((k[None, :] >> 3) ^ ((r[:, None] >> 1) & 7)) << 4) + 2 * (k[None, :] & 7)


class _Reader:
    def __init__(self, stream, dt):
        assert stream.dtype == torch.uint8 and stream.device.type == "cpu" and stream.numel() % TILE == 0
        self.w16 = stream.view(torch.int16)
        self.f32 = stream.view(torch.float32)
        self.dt = dt
        self.used = torch.zeros(self.w16.numel(), dtype=torch.bool)

    def block(self, tile, off, rows):
        """fp64 [rows][64] of the block at byte `off` of tile `tile`, natural channel order"""
        idx = (tile * TILE + off + _block_bytes(rows)) // 2
        self.used[idx] = True
        return self.w16[idx].view(self.dt).double()

    def vec(self, tile, at, n):
        """fp32 vector of n floats at float offset `at` of the tile's aux area"""
        i0 = (tile * TILE + TILE_W) // 4 + at
        self.used[2 * i0:2 * (i0 + n)] = True
        return self.f32[i0:i0 + n].clone()

    def gemm(self, t0, K, N=C):
        """N = 320 stage of depth K from tile t0: (W [N][K], first tile behind it)"""
        return torch.cat([self.block(t0 + kt, 0, N) for kt in range(K // 64)], 1), t0 + K // 64

    def ff1_tile(self, t):
        """FF1-shaped tile: (a rows [32][320], g rows [32][320])"""
        a = torch.cat([self.block(t, 8192 * kb, 32) for kb in range(C // 64)], 1)
        g = torch.cat([self.block(t, 8192 * kb + 4096, 32) for kb in range(C // 64)], 1)
        return a, g

    def ff(self, t0, hidden, d, p):
        """FeedForward(GEGLU) from tile t0 into d[p + ...]; returns the first tile behind it"""
        wa, wg, ba, bg, ca, cg, w2 = [], [], [], [], [], [], []
        t = t0
        for _ in range(hidden // 64):
            for _half in range(2):
                a, g = self.ff1_tile(t)
                wa.append(a), wg.append(g)
                ba.append(self.vec(t, 0, 32)), bg.append(self.vec(t, 32, 32)), ca.append(self.vec(t, 64, 32)), cg.append(self.vec(t, 96, 32))
                t += 1
            w2.append(self.block(t, 0, C))
            t += 1
        d[p + "ff1_w"] = torch.cat(wa + wg, 0)                  # [2 hidden][320]: value rows, then gate rows (diffusers GEGLU.chunk)
        d[p + "ff1_b"], d[p + "ff1_cs"] = torch.cat(ba + bg), torch.cat(ca + cg)
        d[p + "ff2_w"] = torch.cat(w2, 1)
        d[p + "ff2_b"] = self.vec(t - 1, 0, C)
        return t


def decode(kind, stream, dt, hidden=0):
    """packed stream (uint8, CPU) -> (dict of fp64 weight matrices [out][in] and fp32 vectors in natural order, bool mask over the
    stream's 16-bit words of those the layout uses)"""
    r = _Reader(stream, dt)
    d = {}

    def ln_stage(name, t0):
        d[name + "_w"], t1 = r.gemm(t0, C)
        d[name + "_b"], d[name + "_cs"] = r.vec(t1 - 1, 0, C), r.vec(t1 - 1, 512, C)
        return t1

    def bias_stage(name, t0, K=C):
        d[name + "_w"], t1 = r.gemm(t0, K)
        d[name + "_b"] = r.vec(t1 - 1, 0, C)
        return t1

    if kind == T.MLP:
        t = r.ff(0, hidden, d, "")
    elif kind == T.HEAD:
        t = bias_stage("in", 0)
        for n in ("q", "k", "v"):
            t = ln_stage(n, t)
    elif kind == T.CSCE:
        t = bias_stage("proj", 0, T.CCOND)
        t = bias_stage("t0", t)
        t = bias_stage("t2", t)
    elif kind == T.TAIL:
        t = bias_stage("o1", 0)
        qw, qb, qc, ks, vs, o2 = [], [], [], [], [], []
        for _hd in range(T.HEADS):
            a, g = r.ff1_tile(t)
            qw += [a, g]
            qb.append(r.vec(t, 0, 64)), qc.append(r.vec(t, 512, 64))
            ks.append(r.block(t + 1, 0, 96))                                                              # K_h [96 keys][64 d]
            vs.append(torch.cat([r.block(t + 1, 12288, 64), r.block(t + 1, 20480, 64)], 1))               # V^T_h [64 d][128 keys]
            o2.append(r.block(t + 2, 0, C))
            t += 3
        d["q2_w"], d["q2_b"], d["q2_cs"] = torch.cat(qw, 0), torch.cat(qb), torch.cat(qc)
        d["K"], d["VT"] = torch.stack(ks), torch.stack(vs)
        d["o2_w"], d["o2_b"] = torch.cat(o2, 1), r.vec(t - 1, 0, C)
        t = r.ff(t, hidden, d, "")
        t = bias_stage("out", t)
    else:
        raise ValueError(kind)
    assert t * TILE == stream.numel(), (t, stream.numel() // TILE)
    return d, r.used


# ------------------------------------------------------------------------------------------------------------------ inputs
def make(c, dt):
    """Master weights (fp32) and inputs (fp32 values of dt numbers) of case c, from a generator seeded by the case id."""
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    kind, k, n, hw, hid = c["kind"], c["kernel"], c["N"], c["hw"], c["hidden"]
    tt = n * hw
    m = {}
    lnp = lambda: (1 + 0.2 * r(C), 0.1 * r(C))
    if k in (T.MLP, T.TAIL):
        m["ff1_w"], m["ff1_b"] = r(2 * hid, C, sc=C ** -0.5), r(2 * hid, sc=0.1)
        m["ff2_w"], m["ff2_b"] = r(C, hid, sc=hid ** -0.5), r(C, sc=0.1)
        m["ln3_g"], m["ln3_b"] = lnp()
        if kind == "gelu_tail":                       # gate pre-activations spread over [-6, 6]
            m["ff1_b"][hid:] = torch.linspace(-6, 6, hid)[torch.randperm(hid, generator=g)]
    if k == T.MLP:
        m["x"] = r(tt, C) + 8.0 if kind == "offset" else r(tt, C, sc=1.5) + 0.3
    elif k == T.HEAD:
        m["in_w"], m["in_b"] = r(C, C, sc=C ** -0.5), r(C, sc=0.1)
        m["ln1_g"], m["ln1_b"] = lnp()
        for nm in ("q", "k", "v"):
            m[nm + "_w"] = r(C, C, sc=C ** -0.5)
        x = r(n, hw, C, sc=2.0) + 0.5
        a, b = 1 + 0.3 * r(n, C), 0.2 * r(n, C)
        if kind == "per_image":                       # scale of the inputs and of the affine differs 4 x from image to image
            s = torch.tensor([4.0 ** ((i % 3) - 1) for i in range(n)])
            x, a, b = x * s[:, None, None], a / s[:, None], b + 0.5 * torch.arange(n)[:, None]
        elif kind == "offset":                        # a large b: proj_in(b) = 16 in every channel, |mean h0| >> std h0 (proj_in
            m["in_w"] = torch.linalg.qr(r(C, C))[0].contiguous()      # orthogonal: that b stays ~16 and rounds to 16 bits harmlessly)
            b = b + torch.linalg.solve(m["in_w"].double(), torch.full((C,), 16.0, dtype=torch.float64)).float()[None, :]
        m["x"], m["ab"] = x.reshape(tt, C), torch.stack([a, b], 1).contiguous()
    elif k == T.TAIL:
        for nm in ("o1", "o2", "out"):
            m[nm + "_w"], m[nm + "_b"] = r(C, C, sc=C ** -0.5), r(C, sc=0.1)
        m["ln2_g"], m["ln2_b"] = lnp()
        m["q2_w"] = r(C, C, sc=C ** -0.5)
        m["k2_w"], m["v2_w"] = r(C, T.CROSS, sc=T.CROSS ** -0.5), r(C, T.CROSS, sc=T.CROSS ** -0.5)
        m["ctx"] = r(c["tk"], T.CROSS)
        if kind == "peaked":                          # one key takes the row: scores spread over tens of units of the exp2 domain
            m["q2_w"], m["ctx"] = m["q2_w"] * 8, m["ctx"] * 6
            m["v2_w"] = m["v2_w"] / 6
        m["o1"], m["h0"], m["xres"] = r(tt, C), r(tt, C, sc=1.5), r(tt, C, sc=2.0)
        if kind == "offset":
            m["h0"] = r(tt, C, sc=0.5) + 10.0
    elif k == T.CSCE:
        for nm, kk in (("proj", T.CCOND), ("t0", C), ("t2", C)):
            m[nm + "_w"], m[nm + "_b"] = r(C, kk, sc=kk ** -0.5), r(C, sc=0.1)
        if kind == "gelu_tail":
            m["t0_b"] = torch.linspace(-6, 6, C)[torch.randperm(C, generator=g)]
        m["x"], m["cond"] = r(tt, C, sc=1.5), r(tt, T.CCOND)
    for nm in ("x", "cond", "o1", "h0", "xres"):
        if nm in m:
            m[nm] = m[nm].to(dt).float()
    return m


def pack(c, m, dt, dev="cpu"):
    """the case's weight stream through the project's packers"""
    from unirestore_amd import chain
    k = c["kernel"]
    if k == T.MLP:
        return chain.pack_mlp(m["ff1_w"], m["ff1_b"], m["ff2_w"], m["ff2_b"], m["ln3_g"], m["ln3_b"], dev, dt)
    if k == T.HEAD:
        return chain.pack_head(m["in_w"], m["in_b"], m["q_w"], m["k_w"], m["v_w"], m["ln1_g"], m["ln1_b"], dev, dt)
    if k == T.TAIL:
        return chain.pack_tail(m["o1_w"], m["o1_b"], m["q2_w"], m["ln2_g"], m["ln2_b"], m["k2_w"], m["v2_w"], m["ctx"], m["o2_w"], m["o2_b"],
                               m["ff1_w"], m["ff1_b"], m["ff2_w"], m["ff2_b"], m["ln3_g"], m["ln3_b"], m["out_w"], m["out_b"], T.HEADS, dev, dt)
    return chain.pack_csce(m["proj_w"], m["proj_b"], m["t0_w"], m["t0_b"], m["t2_w"], m["t2_b"], dev, dt)


def inputs_of(c, m):
    """the launch inputs of make()'s dict"""
    return {nm: m[nm] for nm in {T.MLP: ("x",), T.HEAD: ("x", "ab"), T.TAIL: ("o1", "h0", "xres"), T.CSCE: ("x", "cond")}[c["kernel"]]}


def c_of(scale):
    """attn_scale * log2(e) as the launcher computes it: a float product of two floats"""
    return float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------ reference
class Val:
    """A 16-bit intermediate of the reference: v = its fp64 value, var = the modelled variance, per element, of (the kernel's 16-bit
    value - v): 0 where both round alike for certain."""
    def __init__(self, v, var=None):
        self.v, self.var = v, torch.zeros_like(v) if var is None else var


# one-sided Gaussian masses of the flip model: a boundary at distance g from z_ref is crossed with probability Phi(-g / sigma); the
# grid point x_j carries the mass of (x_j - 0.5, x_j], the last one the whole tail, so that the sum over x_j >= g / sigma is never
# below that probability.  Nothing beyond 4 sigma = b: an element whose boundary is further than its stage bound is not ambiguous.
_FLIP_X = [0.5 * j for j in range(1, 9)]
_PHI = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))
_FLIP_W = [(_PHI(x) - _PHI(x - 0.5)) if x < 4.0 else (1.0 - _PHI(x - 0.5)) for x in _FLIP_X]


def _rnd(z, b, dt):
    """round the stage output z (bound b) where the kernel packs it"""
    v = z.to(dt).double()
    sigma = b / C_BOUND
    var = torch.zeros_like(z)
    for x, w in zip(_FLIP_X, _FLIP_W):
        var += w * (((z + x * sigma).to(dt).double() - v) ** 2 + ((z - x * sigma).to(dt).double() - v) ** 2)
    return Val(v, var)


def _kc(K):
    return C_BOUND * math.sqrt(K) * 2.0 ** -24


def _through(var, w):
    """variance of sum_k W_nk delta_k for independent delta of variance var [T][K], W [N][K]"""
    return var @ (w * w).t()


def _bias_stage(x, w, bias, res=None, gelu=False):
    """z = act(x W^T + bias) + res -> (z, b)"""
    bias = bias.double()
    z = x.v @ w.t() + bias
    b = _kc(w.shape[1]) * (x.v.abs() @ w.abs().t() + bias.abs())
    pv = _through(x.var, w)
    if gelu:
        z, b, pv = F.gelu(z), GELU_D * b + GELU_EPS, GELU_D ** 2 * pv
    if res is not None:
        z, pv = z + res.v, pv + res.var
    return z, b + C_BOUND * pv.sqrt()


class _LN:
    """two-pass statistics of a rounded row and the LayerNorm-folded stage over it"""
    def __init__(self, x):
        self.x = x
        self.mean = x.v.mean(1, keepdim=True)
        self.cen = x.v - self.mean
        self.rstd = (self.cen.pow(2).mean(1, keepdim=True) + LN_EPS).rsqrt()
        self.mabs = x.v.abs().mean(1, keepdim=True)
        K = x.v.shape[1]
        self.dmean = C_BOUND * x.var.sum(1, keepdim=True).sqrt() / K
        self.drstd = self.rstd ** 3 * C_BOUND * (self.cen.pow(2) * x.var).sum(1, keepdim=True).sqrt() / K

    def ratio(self):
        """|mean| / std per token"""
        return (self.mean.abs() * self.rstd).squeeze(1)

    def fold(self, w, bias, cs):
        bias, cs = bias.double(), cs.double()
        x = self.x
        acc = x.v @ w.t()
        core = acc - self.mean * cs
        z = self.rstd * core + bias
        kc = _kc(w.shape[1])
        b = kc * (self.rstd * (x.v.abs() @ w.abs().t() + self.mabs * cs.abs()) + bias.abs()) + kc * self.rstd * core.abs()
        b = b + self.rstd * C_BOUND * _through(x.var, w).sqrt() + self.rstd * cs.abs() * self.dmean + core.abs() * self.drstd
        return z, b


def _geglu(ln, d, dt):
    h = d["ff1_w"].shape[0] // 2
    za, ba = ln.fold(d["ff1_w"][:h], d["ff1_b"][:h], d["ff1_cs"][:h])
    zg, bg = ln.fold(d["ff1_w"][h:], d["ff1_b"][h:], d["ff1_cs"][h:])
    phi = F.gelu(zg)
    return _rnd(za * phi, phi.abs() * ba + za.abs() * (GELU_D * bg + GELU_EPS), dt), zg


def _out(z, b, dt):
    return z, U_OUT[dt] * z.abs() + ABS_OUT[dt] + b


def reference(c, dec, inp, dt):
    """-> ({output name: (ref, bound)} fp64 [T][320], info: properties of the staged run the CPU test asserts on)"""
    k = c["kernel"]
    dev = next(iter(inp.values())).device
    d = {n: v.to(dev) for n, v in dec.items()}
    I = {n: Val(v.double()) for n, v in inp.items() if n != "ab"}
    info = {"ln_ratio": [], "gate": None}
    out = {}
    if k == T.MLP:
        ln = _LN(I["x"])
        info["ln_ratio"].append(ln.ratio())
        hid, info["gate"] = _geglu(ln, d, dt)
        out["y"] = _out(*_bias_stage(hid, d["ff2_w"], d["ff2_b"], I["x"]), dt)
    elif k == T.CSCE:
        s = _rnd(*_bias_stage(I["cond"], d["proj_w"], d["proj_b"], I["x"]), dt)
        info["gate"] = s.v @ d["t0_w"].t() + d["t0_b"].double()
        h = _rnd(*_bias_stage(s, d["t0_w"], d["t0_b"], gelu=True), dt)
        out["y"] = _out(*_bias_stage(h, d["t2_w"], d["t2_b"], s), dt)
    elif k == T.HEAD:
        ab = inp["ab"].double().repeat_interleave(c["hw"], 0)                 # [T][2][C]
        z = I["x"].v * ab[:, 0] + ab[:, 1]
        xn = _rnd(z, 2.0 ** -24 * z.abs(), dt)
        z, b = _bias_stage(xn, d["in_w"], d["in_b"])
        out["h0"] = _out(z, b, dt)
        ln = _LN(_rnd(z, b, dt))
        info["ln_ratio"].append(ln.ratio())
        for n in ("q", "k", "v"):
            out[n] = _out(*ln.fold(d[n + "_w"], d[n + "_b"], d[n + "_cs"]), dt)
    elif k == T.TAIL:
        h1 = _rnd(*_bias_stage(I["o1"], d["o1_w"], d["o1_b"], I["h0"]), dt)
        ln = _LN(h1)
        info["ln_ratio"].append(ln.ratio())
        q2 = _rnd(*ln.fold(d["q2_w"], d["q2_b"], d["q2_cs"]), dt)
        o2 = _attention(q2, d, c["tk"], c["scale"], dt, info)
        h2 = _rnd(*_bias_stage(o2, d["o2_w"], d["o2_b"], h1), dt)
        ln = _LN(h2)
        info["ln_ratio"].append(ln.ratio())
        hid, info["gate"] = _geglu(ln, d, dt)
        h3 = _rnd(*_bias_stage(hid, d["ff2_w"], d["ff2_b"], h2), dt)
        out["y"] = _out(*_bias_stage(h3, d["out_w"], d["out_b"], I["xres"]), dt)
    return out, info


def _attention(q2, d, tk, scale, dt, info):
    """cross-attention over the baked context, head by head -> o2 (Val [T][320])"""
    cc = c_of(scale)
    vs, ds, wmax, psub = [], [], [], []
    for hd in range(T.HEADS):
        sl = slice(64 * hd, 64 * hd + 64)
        q, qd = q2.v[:, sl], q2.var[:, sl]
        K, V = d["K"][hd, :tk], d["VT"][hd, :, :tk].t()                        # [tk][64] each
        t = cc * (q @ K.t())
        R = t.abs().amax(1, keepdim=True)
        A_s = cc * (q.abs() @ K.abs().t()).amax(1, keepdim=True)
        p = torch.exp2(t - t.amax(1, keepdim=True))
        l = p.sum(1, keepdim=True)
        w = p / l
        eps_s = 2.0 ** -24 * (C_BOUND * 8.0 * A_s + 3 * R + 17)
        dts = eps_s + cc * C_BOUND * _through(qd, K).sqrt()                      # [T][tk] score uncertainty, exp2 domain
        # p_k = 2^(t_k - t_max): uncertain by both scores - except the largest key itself, whose p is 1 whatever its score, unless
        # another key can overtake it (then by how far that key can get above it)
        tmax, kmax = t.max(1, keepdim=True)
        rel = dts + dts.gather(1, kmax)
        over = (rel - (tmax - t)).clamp_min(0.0).scatter(1, kmax, 0.0).amax(1, keepdim=True)
        rel = rel.scatter(1, kmax, over)
        p16 = _rnd(p, (math.log(2.0) * rel + 2.0 ** -23) * p, dt)              # P as the MFMA operand, with its flips
        o = (p16.v @ V) / l
        A = w @ V.abs()
        b = C_BOUND * _through(p16.var, V.t()).sqrt() / l + C_BOUND * math.sqrt(tk) * 2.0 ** -24 * A + \
            (2.0 ** -22 + math.log(2.0) * (w * rel).sum(1, keepdim=True)) * o.abs()
        r = _rnd(o, b, dt)
        vs.append(r.v), ds.append(r.var)
        wmax.append(w.amax(1))
        psub.append(((p > 0) & (p < 2.0 ** -14)).any(1))
    info["w_max"], info["p_subnormal"] = torch.stack(wmax, 1), torch.stack(psub, 1)       # [T][heads]
    return Val(torch.cat(vs, 1), torch.cat(ds, 1))


def reference_from_h0(dec, h0_kernel, dt):
    """HEAD's q / k / v from the kernel's OWN stored h0 (fp64 values of its 16-bit numbers): {name: (ref, bound)}, no ambiguity term"""
    d = {n: v.to(h0_kernel.device) for n, v in dec.items()}
    ln = _LN(Val(h0_kernel))
    return {n: _out(*ln.fold(d[n + "_w"], d[n + "_b"], d[n + "_cs"]), dt) for n in ("q", "k", "v")}


def gn_terms(y, c):
    """kernel output y [T][320] -> fp64 [N][parts][320][128]: the terms of every partial-plane sum, summed over the last dim"""
    return y.double().view(c["N"], c["hw"] // T.TOK, T.TOK, C).transpose(2, 3)


# ------------------------------------------------------------------------------------------------------------------ emulation
FAULTS = ("colsum_unrounded", "no_swap23", "key_mask", "no_bias", "neighbour_image", "ktile_scale")


def _gelu_f(x):
    """csrc/common.h gelu_f in fp32"""
    xc = x.clamp(-8.0, 8.0)
    t = xc * xc
    pz = 1.0142631e-3 * t - 0.10677573
    pz = pz * t - 2.3011214
    return x / (1.0 + torch.exp2(pz * xc))


def _stats32(x, eps=LN_EPS):
    mean = x.sum(1, keepdim=True) * (1.0 / x.shape[1])
    q = ((x - mean) ** 2).sum(1, keepdim=True) * (1.0 / x.shape[1])
    return mean, torch.rsqrt(q + eps)


def _fold32(x, st, w, b, cs):
    mean, rstd = st
    return rstd * (x @ w.t()) + (-(mean * rstd) * cs + b)


def _faulty(dec, fault):
    """the decoded stream with a weight-level mutation applied (fp32 copies)"""
    d = {n: v.float().clone() for n, v in dec.items()}
    if fault is None:
        return d
    name = fault[0]
    assert name in FAULTS
    if name == "colsum_unrounded":                    # (name, stage, column sums of the unrounded w * gamma)
        d[fault[1] + "_cs"] = fault[2].float()
    elif name == "no_swap23":                         # (name, stage, 32-row block): rows in plain MFMA order
        w, blk = d[fault[1] + "_w"], fault[2]
        src = torch.tensor([_mfma_row(i) for i in range(32)]) + 32 * blk
        w[32 * blk:32 * blk + 32] = w[src].clone()
    elif name == "no_bias":                           # (name, stage)
        d[fault[1] + "_b"].zero_()
    elif name == "ktile_scale":                       # (name, stage, k tile, factor)
        d[fault[1] + "_w"][:, 64 * fault[2]:64 * fault[2] + 64] *= fault[3]
    return d


def emulate(c, dec, inp, dt, fault=None):
    """the kernel's arithmetic in fp32 on the CPU -> {output name: fp32 values of dt numbers [T][320]} (+ "gn_part" [N][parts][320][2])"""
    k = c["kernel"]
    d = _faulty(dec, fault)
    fname = fault[0] if fault else None
    r16 = lambda z: z.to(dt).float()
    lin = lambda x, n: x @ d[n + "_w"].t() + d[n + "_b"]
    out = {}

    def ff(x):
        st = _stats32(x)
        h = d["ff1_w"].shape[0] // 2
        p = _fold32(x, st, d["ff1_w"], d["ff1_b"], d["ff1_cs"])
        return r16(p[:, :h] * _gelu_f(p[:, h:])) @ d["ff2_w"].t() + d["ff2_b"]

    if k == T.MLP:
        out["y"] = r16(ff(inp["x"]) + inp["x"])
    elif k == T.CSCE:
        s = r16(lin(inp["cond"], "proj") + inp["x"])
        h = r16(_gelu_f(lin(s, "t0")))
        out["y"] = r16(lin(h, "t2") + s)
    elif k == T.HEAD:
        ab = inp["ab"]
        if fname == "neighbour_image":
            ab = ab.roll(-1, 0)
        ab = ab.repeat_interleave(c["hw"], 0)
        xn = r16(torch.addcmul(ab[:, 1], inp["x"], ab[:, 0]))
        out["h0"] = h0 = r16(lin(xn, "in"))
        st = _stats32(h0)
        for n in ("q", "k", "v"):
            out[n] = r16(_fold32(h0, st, d[n + "_w"], d[n + "_b"], d[n + "_cs"]))
    elif k == T.TAIL:
        tk = c["tk"]
        h1 = r16(lin(inp["o1"], "o1") + inp["h0"])
        q2 = r16(_fold32(h1, _stats32(h1), d["q2_w"], d["q2_b"], d["q2_cs"]))
        cc = torch.tensor(c_of(c["scale"]), dtype=torch.float32)
        real = torch.arange(96) < tk
        if fname == "key_mask":
            real[tk - 1], real[tk] = False, True
        o2 = []
        for hd in range(T.HEADS):
            s = q2[:, 64 * hd:64 * hd + 64] @ d["K"][hd].t()                     # [T][96]
            mx = s.masked_fill(~real, float("-inf")).amax(1, keepdim=True)
            p = torch.where(real, torch.exp2(s * cc - mx * cc), torch.zeros(()))
            l = p.sum(1, keepdim=True)
            o2.append(r16((r16(p)[:, :80] @ d["VT"][hd][:, :80].t()) * (1.0 / l)))
        h2 = r16(torch.cat(o2, 1) @ d["o2_w"].t() + d["o2_b"] + h1)
        h3 = r16(ff(h2) + h2)
        out["y"] = r16(lin(h3, "out") + inp["xres"])
    if k in (T.TAIL, T.CSCE):
        t = out["y"].view(c["N"], c["hw"] // T.TOK, T.TOK, C)
        out["gn_part"] = torch.stack([t.sum(2), (t * t).sum(2)], -1)
    return out
