"""Case table of the norm / per-channel kernel parity matrix (tests/test_norm_launchers_gpu.py): every export of csrc/norms.hip and
the per-channel block of csrc/elementwise.hip.  Importable without torch: tests/test_norm_reference_cpu.py checks the geometry
mirror against the library, asserts that every property of PROPERTIES is held by at least one launched case, and runs the refusal
table (host only, placeholder pointers).

Rows are plain dicts.  Every 16-bit case runs in bf16 and fp16.

GroupNorm rows: N, HW (flat), C1, C2 (0: one source), G, silu, affine (False: gamma = beta = NULL), offset (per-group |mean| in
standard deviations, alternating sign from group to group), const_group (a (image, group) pair that holds one constant), avgpool
(also run ur_avgpool_hw on source 1), and the EXPECTED partition as literals: P (ur_groupnorm_stats_parts of source 1) and P2 (of
source 2) - a case whose partition moves fails on the CPU before anything is launched.
"""

P = 1 << 20                      # placeholder pointer of the host-only refusal table (16-byte aligned, never dereferenced)
UR_E_INVALID = -1
BF16, F16 = 0, 1


# ---- mirror of gn_geom (csrc/norms.hip) -------------------------------------------------------------------------------------------
def gn_geom(N, HW, C, ppt):
    """(cvs, slabs, R, chunks, ppb, last): channel vectors per slab, slabs, pixel rows per workgroup, pixel chunks, pixels per chunk,
    pixels of the last chunk.  ppt = 8 is the statistics pass, ppt = 2 the apply pass; maps of HW <= 64 use at most 2."""
    cv = C // 8
    cvs = min(cv, 32)
    while cv % cvs:
        cvs -= 1
    slabs, R = cv // cvs, 256 // cvs
    want = max(1, 2048 // (N * slabs))
    eff = min(ppt, 2) if HW <= 64 else ppt
    chunks = min(want, max(1, HW // (eff * R)))
    ppb = (HW + chunks - 1) // chunks
    chunks = (HW + ppb - 1) // ppb
    return cvs, slabs, R, chunks, ppb, HW - (chunks - 1) * ppb


def stats_parts(N, HW, C):
    return gn_geom(N, HW, C, 8)[3]


def ws_bytes(N, HW, C):
    return N * stats_parts(N, HW, C) * C * 2 * 4


def gn(cid, N, HW, C1, C2, G, P, P2=0, *, silu=0, affine=True, offset=0, const_group=None, avgpool=False):
    return dict(id=cid, N=N, HW=HW, C1=C1, C2=C2, G=G, P=P, P2=P2, silu=silu, affine=affine, offset=offset, const_group=const_group,
                avgpool=avgpool)


GN_CASES = [
    # cvs = 20 does not divide 256 (16 idle threads), 2 slabs, cpg = 10: a 16-byte vector spans two groups
    gn("gn_c320_off0", 2, 256, 320, 0, 32, 2, silu=1, const_group=(1, 3), avgpool=True),
    gn("gn_c320_off6", 2, 256, 320, 0, 32, 2, offset=6),
    gn("gn_c320_off30", 2, 256, 320, 0, 32, 2, silu=1, offset=30),
    # cpg = 4 < 8; statistics chunk 341 > 4R = 128 (second trip of the unrolled loop), last chunk 339; apply last chunk 55
    gn("gn_hw1021_cpg4", 1, 1021, 64, 0, 16, 3, offset=6, avgpool=True),
    gn("gn_instnorm", 2, 64, 64, 0, 64, 1, affine=False),
    gn("gn_hw16_c2560", 1, 16, 2560, 0, 32, 1, silu=1),
    # C / 8 = 37 is prime: cvs = 1, R = 256, 37 slabs, 300 pixels > R
    gn("gn_prime_cv37", 1, 300, 296, 0, 8, 1, silu=1, avgpool=True),
    # two sources: cpg = 6, group 21 = channels 126..131 straddles C1 = 128
    gn("gn_cat_128_64", 2, 64, 128, 64, 32, 2, 1, silu=1, offset=6),
    # the UNet's ratio: cpg = 60 (group 21 straddles), cvs 32 / 20, apply chunks 4 / 2
    gn("gn_cat_1280_640", 1, 64, 1280, 640, 32, 4, 2, silu=1),
    # 19 x 19: apply chunks of 25 pixels, the last has 11 < R = 12; statistics chunks 121, 121, 119
    gn("gn_hw361_short_apply", 1, 361, 320, 0, 32, 3),
    # the whole path with the 256-thread finalize: cpg * P = 10 * 104 = 1040 > 1024; last statistics chunk 9 < R = 12
    gn("gn_hw10000", 1, 10000, 320, 0, 32, 104, silu=1),
]

# ---- finalize alone, on synthetic fp32 planes: N, HW, C1, P1, C2, P2, G, which outputs, affine ------------------------------------
def fin(cid, N, HW, C1, P1, C2, P2, G, outs, affine=True):
    return dict(id=cid, N=N, HW=HW, C1=C1, P1=P1, C2=C2, P2=P2, G=G, outs=outs, affine=affine)


FINALIZE_CASES = [
    fin("fin_p130_p7_straddle", 2, 910, 16, 130, 8, 7, 4, "both"),        # cpg = 6: group 2 = channels 12..17 straddles; 780 entries
    fin("fin_p130_p7_wide", 1, 910, 40, 130, 24, 7, 4, "ab"),             # cpg = 16: 2080 entries, 256 threads, P1 != P2, straddle
    fin("fin_cpg256_one_wave", 1, 64, 512, 4, 0, 0, 2, "both"),           # cpg = 256 > 64 lanes with one wave (1024 entries)
    fin("fin_cpg512_p3", 1, 64, 512, 3, 0, 0, 1, "ab"),                   # cpg = 512 > 256 threads (1536 entries)
    fin("fin_cpg1", 2, 50, 24, 5, 0, 0, 24, "both", affine=False),        # cpg = 1, null gamma / beta
    fin("fin_mean_only", 2, 50, 24, 5, 0, 0, 24, "mean"),
]

# ---- ur_groupnorm_nhwc: which sources come with producer-side planes (parts: the producer's own P, not ur_groupnorm_stats_parts) ----
NHWC_CASES = [
    dict(id="nhwc_pre1_ws2", N=2, HW=64, C1=128, C2=64, G=32, silu=1, pre=(5, 0)),
    dict(id="nhwc_pre_both", N=2, HW=64, C1=128, C2=64, G=32, silu=0, pre=(5, 3)),
    dict(id="nhwc_pre_none", N=2, HW=64, C1=128, C2=64, G=32, silu=1, pre=(0, 0)),
    dict(id="nhwc_single", N=1, HW=361, C1=320, C2=0, G=32, silu=1, pre=(0, 0)),
]

# ---- LayerNorm: rows, C, gamma, beta, offset (|row mean| in standard deviations), const_row ---------------------------------------
def ln(rows, C, gamma=True, beta=True, offset=0, const_row=None):
    return dict(id=f"ln_r{rows}_c{C}" + ("" if gamma else "_nogamma") + ("" if beta else "_nobeta") + (f"_off{offset}" if offset else ""),
                rows=rows, C=C, gamma=gamma, beta=beta, offset=offset, const_row=const_row)


LN_CASES = [ln(1, 8), ln(15, 64, offset=6), ln(16, 320, gamma=False), ln(17, 512, beta=False), ln(33, 520, offset=30, const_row=7), ln(5, 1280),
            ln(4, 1536, offset=6), ln(3, 1544, offset=30), ln(2, 2048), ln(33, 520, gamma=False, beta=False)]

# ---- row softmax: rows, cols, ldp, standard deviation of the scores; kind "subnormal": fp16 probabilities below 2^-14 ---------------
def sm(rows, cols, ldp, std, kind="randn"):
    return dict(id=f"sm_{rows}x{cols}_ld{ldp}_s{std}" + ("" if kind == "randn" else "_" + kind), rows=rows, cols=cols, ldp=ldp, std=std, kind=kind)


SOFTMAX_CASES = [sm(3, 1, 8, 1), sm(2, 77, 77, 4), sm(2, 77, 80, 30), sm(5, 255, 256, 1), sm(4, 256, 256, 4), sm(3, 257, 264, 30),
                 sm(2, 333, 336, 4), sm(2, 1029, 1032, 1), sm(2, 1029, 1032, 30), sm(2, 333, 336, 1, kind="subnormal")]

# ---- depthwise 3x3: N, H, W, C, gate -----------------------------------------------------------------------------------------------
DWCONV_CASES = [dict(id=f"dw_n{n}_{h}x{w}_c{c}_g{g}", N=n, H=h, W=w, C=c, gate=g)
                for n, h, w, c, g in [(2, 1, 1, 8, 0), (1, 3, 4, 16, 1), (2, 5, 8, 64, 1), (2, 9, 11, 64, 0), (2, 9, 11, 64, 1), (1, 1, 12, 8, 0),
                                      (1, 6, 1, 8, 0), (3, 4, 5, 24, 0)]]

# ---- scale_channels (N, HW, C, residual) and its fan-out (K, with s or s = NULL) ---------------------------------------------------
SCALE_CASES = [dict(id=f"scale_n{n}_hw{hw}_c{c}_r{r}", N=n, HW=hw, C=c, res=r) for n, hw, c, r in [(1, 7, 8, 0), (3, 7, 8, 1), (1, 5, 320, 1), (3, 5, 320, 0)]]
FANOUT_CASES = [dict(id=f"fanout_b{b}_k{k}_c{c}_s{s}", B=b, K=k, HW=hw, C=c, s=s)
                for b, k, hw, c, s in [(1, 1, 7, 8, 1), (3, 3, 5, 320, 1), (2, 8, 7, 8, 1), (2, 3, 5, 320, 0), (1, 8, 7, 8, 0)]]

# ---- axpy_channels (rows, C) and spade_modulate (rows, C, ldgb - 2C, residual) -----------------------------------------------------
AXPY_CASES = [dict(id=f"axpy_r{r}_c{c}", rows=r, C=c) for r, c in [(1, 8), (5, 8), (1, 320), (7, 320)]]
SPADE_CASES = [dict(id=f"spade_r{r}_c{c}_pad{p}_res{s}", rows=r, C=c, pad=p, res=s)
               for r, c, p, s in [(1, 8, 0, 0), (1, 8, 8, 1), (5, 320, 0, 1), (5, 320, 8, 0), (1, 320, 8, 1)]]

# ---- linear_f32: M, N, K, groups, act (capi UR_ACT_* values), bias -----------------------------------------------------------------
ACT_NONE, ACT_SILU, ACT_GELU, ACT_TANH, ACT_RELU = 0, 1, 2, 5, 6
LINEAR_CASES = [dict(id=f"lin_m{m}_n{n}_k{k}_g{g}_a{a}_b{b}", M=m, N=n, K=k, groups=g, act=a, bias=b)
                for m, n, k, g, a in [(1, 1, 1, 1, ACT_NONE), (9, 5, 257, 1, ACT_GELU), (50, 1280, 320, 1, ACT_SILU), (17, 8, 1280, 1, ACT_TANH),
                                      (5, 96, 96, 4, ACT_NONE), (8, 6, 520, 2, ACT_RELU)] for b in (1, 0)]

# ---- tfa_prompt_update: B, T, D; fan-out: K, cond_per_row --------------------------------------------------------------------------
TFA_CASES = [dict(id=f"tfa_b{b}_t{t}_d{d}", B=b, T=t, D=d) for b, t, d in [(2, 2, 48), (1, 1, 256), (2, 3, 300), (1, 4, 768)]]
TFA_FANOUT_CASES = [dict(id=f"tfa_fan_b{b}_k{k}_t{t}_d{d}_cpr{c}", B=b, K=k, T=t, D=d, cpr=c)
                    for b, k, t, d, c in [(2, 1, 2, 48, 0), (2, 3, 3, 300, 0), (2, 3, 3, 300, 1), (1, 1, 1, 256, 1)]]

VMG_CASES = [dict(id=f"vmg_n{n}_c{c}_g{g}", N=n, C=c, G=g) for n, c, g in [(2, 64, 4), (1, 8, 8), (3, 96, 1)]]

# ---- second trip through the grid-stride loop: nblocks() caps the grid at 8192 blocks of 256 threads -------------------------------
GRID_THREADS = 8192 * 256
BIG_CASES = [
    dict(id="big_scale", op="scale", N=2, HW=16400, C=512, res=1),                     # 2 * 16400 * 64 = 2,099,200 vectors
    dict(id="big_axpy", op="axpy", rows=32800, C=512),
    dict(id="big_spade", op="spade", rows=32800, C=512, pad=8, res=1),
    dict(id="big_dwconv_pixel", op="dwconv", N=1, H=182, W=181, C=512),         # W % 4 = 1: 182 * 181 * 64 = 2,108,288 threads
    dict(id="big_dwconv_strip", op="dwconv", N=1, H=364, W=364, C=512),         # 364 * 91 * 64 = 2,119,936 threads of four pixels
]


def big_threads(c):
    if c["op"] == "scale":
        return c["N"] * c["HW"] * c["C"] // 8
    if c["op"] in ("axpy", "spade"):
        return c["rows"] * c["C"] // 8
    px = c["N"] * c["H"] * c["W"] * c["C"] // 8
    return px // 4 if c["W"] % 4 == 0 else px


# ---- properties the table must hold (each by at least one launched case) -----------------------------------------------------------
def _g(c, ppt, src=1):
    return gn_geom(c["N"], c["HW"], c["C1"] if src == 1 else c["C2"], ppt)


def _cpg(c):
    return (c["C1"] + c["C2"]) // c["G"]


def _straddles(c):
    return c["C2"] > 0 and c["C1"] % _cpg(c) != 0


def _fin_entries(c):
    return ((c["C1"] + c["C2"]) // c["G"]) * max(c["P1"], c["P2"])


GN_PROPERTIES = {
    "cvs does not divide 256, slabs > 1, cpg not a multiple of 8": lambda c: 256 % _g(c, 8)[0] != 0 and _g(c, 8)[1] > 1 and _cpg(c) % 8 != 0,
    "cpg < 8": lambda c: _cpg(c) < 8,
    "statistics chunk longer than 4R with a short last chunk": lambda c: _g(c, 8)[4] > 4 * _g(c, 8)[2] and _g(c, 8)[5] < _g(c, 8)[4],
    "last statistics chunk shorter than R": lambda c: _g(c, 8)[3] > 1 and _g(c, 8)[5] < _g(c, 8)[2],
    "instance norm with null gamma and beta": lambda c: c["G"] == c["C1"] + c["C2"] and not c["affine"],
    "HW <= 64 with many slabs": lambda c: c["HW"] <= 64 and _g(c, 8)[1] >= 8,
    "prime C/8: cvs = 1, R = 256, pixels past the first R": lambda c: _g(c, 8)[0] == 1 and c["HW"] > 256,
    "two sources with a straddling group": _straddles,
    "two sources with chunks1 != chunks2 and cvs1 != cvs2 in the apply pass":
        lambda c: c["C2"] > 0 and _g(c, 2, 1)[3] != _g(c, 2, 2)[3] and _g(c, 2, 1)[0] != _g(c, 2, 2)[0],
    "last apply chunk shorter than R": lambda c: _g(c, 2)[3] > 1 and _g(c, 2)[5] < _g(c, 2)[2],
    "statistics and apply partitions differ": lambda c: _g(c, 8)[3] != _g(c, 2)[3],
    "SiLU on": lambda c: c["silu"] == 1,
    "SiLU off": lambda c: c["silu"] == 0,
    "group means of 0 standard deviations": lambda c: c["offset"] == 0,
    "group means of 6 standard deviations": lambda c: c["offset"] == 6,
    "group means of 30 standard deviations": lambda c: c["offset"] == 30,
    "one constant group": lambda c: c["const_group"] is not None,
    "whole path with cpg * P > 1024": lambda c: _cpg(c) * c["P"] > 1024,
}
FINALIZE_PROPERTIES = {
    "P1 = 130, P2 = 7 with a straddling group": lambda c: (c["P1"], c["P2"]) == (130, 7) and c["C1"] % ((c["C1"] + c["C2"]) // c["G"]) != 0,
    "entries <= 1024 (one wave)": lambda c: _fin_entries(c) <= 1024,
    "entries > 1024 (256 threads)": lambda c: _fin_entries(c) > 1024,
    "cpg = 256 with one wave": lambda c: c["C1"] // c["G"] == 256 and _fin_entries(c) <= 1024,
    "cpg > 256 threads": lambda c: (c["C1"] + c["C2"]) // c["G"] > 256 and _fin_entries(c) > 1024,
    "cpg = 1": lambda c: (c["C1"] + c["C2"]) // c["G"] == 1,
    "mean_out only": lambda c: c["outs"] == "mean",
    "ab only": lambda c: c["outs"] == "ab",
    "ab and mean_out": lambda c: c["outs"] == "both",
    "null gamma and beta": lambda c: not c["affine"],
}
NHWC_PROPERTIES = {
    "pre1 given, x2 through the ws scratch": lambda c: c["pre"][0] > 0 and c["C2"] > 0 and c["pre"][1] == 0,
    "both planes given": lambda c: c["pre"][0] > 0 and c["pre"][1] > 0,
    "neither plane given": lambda c: c["pre"] == (0, 0) and c["C2"] > 0,
    "producer planes whose P is not ur_groupnorm_stats_parts": lambda c: c["pre"][0] > 0 and c["pre"][0] != stats_parts(c["N"], c["HW"], c["C1"]),
}
LN_PROPERTIES = {
    "C = 8 (one live lane)": lambda c: c["C"] == 8,
    "C = 512 (exactly 64 vectors)": lambda c: c["C"] == 512,
    "last VPL slot with one live lane": lambda c: (c["C"] // 8) % 64 == 1,
    "C = 2048 (the cap)": lambda c: c["C"] == 2048,
    "rows = 1": lambda c: c["rows"] == 1,
    "rows = 15": lambda c: c["rows"] == 15,
    "rows = 17": lambda c: c["rows"] == 17,
    "null gamma": lambda c: not c["gamma"],
    "null beta": lambda c: not c["beta"],
    "row means of 6 standard deviations": lambda c: c["offset"] == 6,
    "row means of 30 standard deviations": lambda c: c["offset"] == 30,
    "one constant row": lambda c: c["const_row"] is not None,
    "VPL = 1": lambda c: c["C"] <= 512,
    "VPL = 2": lambda c: 512 < c["C"] <= 1024,
    "VPL = 3": lambda c: 1024 < c["C"] <= 1536,
    "VPL = 4": lambda c: 1536 < c["C"],
}
SOFTMAX_PROPERTIES = {
    "cols = 1": lambda c: c["cols"] == 1,
    "cols < 64 .. 256: waves with no element": lambda c: c["cols"] < 192,
    "cols = 255": lambda c: c["cols"] == 255,
    "cols = 256": lambda c: c["cols"] == 256,
    "cols = 257": lambda c: c["cols"] == 257,
    "ldp == cols": lambda c: c["ldp"] == c["cols"],
    "ldp > cols": lambda c: c["ldp"] > c["cols"],
    "several trips per thread": lambda c: c["cols"] > 1024,
    "std 1": lambda c: c["std"] == 1,
    "std 4": lambda c: c["std"] == 4,
    "std 30 (peaked rows, exact zeros)": lambda c: c["std"] == 30,
    "fp16 subnormal probabilities": lambda c: c["kind"] == "subnormal",
}
DWCONV_PROPERTIES = {
    "strip kernel (W % 4 == 0)": lambda c: c["W"] % 4 == 0,
    "one-pixel kernel": lambda c: c["W"] % 4 != 0,
    "H = 1": lambda c: c["H"] == 1,
    "W = 1": lambda c: c["W"] == 1,
    "W = 4": lambda c: c["W"] == 4,
    "image boundary inside a batch, strip": lambda c: c["N"] > 1 and c["W"] % 4 == 0 and c["H"] > 1,
    "image boundary inside a batch, one-pixel": lambda c: c["N"] > 1 and c["W"] % 4 != 0 and c["H"] > 1,
    "gate with the strip kernel": lambda c: c["gate"] and c["W"] % 4 == 0,
    "gate with the one-pixel kernel": lambda c: c["gate"] and c["W"] % 4 != 0,
}
LINEAR_PROPERTIES = {
    "M > 8": lambda c: c["M"] > 8,
    "Kg > 256": lambda c: c["K"] // c["groups"] > 256,
    "N % 4 != 0": lambda c: c["N"] % 4 != 0,
    "GELU": lambda c: c["act"] == ACT_GELU,
    "TANH": lambda c: c["act"] == ACT_TANH,
    "RELU": lambda c: c["act"] == ACT_RELU,
    "SILU": lambda c: c["act"] == ACT_SILU,
    "groups > 1": lambda c: c["groups"] > 1,
    "no bias": lambda c: not c["bias"],
}
BIG_PROPERTIES = {
    "second trip: scale_channels": lambda c: c["op"] == "scale" and big_threads(c) > GRID_THREADS,
    "second trip: axpy_channels": lambda c: c["op"] == "axpy" and big_threads(c) > GRID_THREADS,
    "second trip: spade_modulate": lambda c: c["op"] == "spade" and big_threads(c) > GRID_THREADS,
    "second trip: one-pixel dwconv": lambda c: c["op"] == "dwconv" and c["W"] % 4 != 0 and big_threads(c) > GRID_THREADS,
    "second trip: strip dwconv": lambda c: c["op"] == "dwconv" and c["W"] % 4 == 0 and big_threads(c) > GRID_THREADS,
}
PROPERTIES = [(GN_CASES, GN_PROPERTIES), (FINALIZE_CASES, FINALIZE_PROPERTIES), (NHWC_CASES, NHWC_PROPERTIES), (LN_CASES, LN_PROPERTIES),
              (SOFTMAX_CASES, SOFTMAX_PROPERTIES), (DWCONV_CASES, DWCONV_PROPERTIES), (LINEAR_CASES, LINEAR_PROPERTIES), (BIG_CASES, BIG_PROPERTIES)]


# ---- refusal table: one row per check.  (function, argument tuple) must return UR_E_INVALID before anything is launched -------------
# Each row is a valid call with ONE thing wrong.  A row may exist only for a condition the entry point refuses before any launch
# (read in csrc/norms.hip / csrc/elementwise.hip): the pointers are placeholders.
_GOOD = {
    "ur_groupnorm_stats": dict(x=P, part=P, N=1, HW=64, C=64, dtype=BF16, stream=None),
    "ur_instnorm_stats": dict(x=P, part=P, N=1, HW=64, C=64, dtype=BF16, stream=None),
    "ur_groupnorm_finalize": dict(part1=P, parts1=2, C1=64, part2=None, parts2=0, C2=0, gamma=P, beta=P, N=1, HW=64, G=8, eps=1e-5, ab=P, mean_out=None,
                                  stream=None),
    "ur_groupnorm_apply_act": dict(x=P, x2=None, y=P, ab=P, N=1, HW=64, C1=64, C2=0, silu=0, dtype=BF16, stream=None),
    "ur_groupnorm_nhwc": dict(x=P, x2=None, y=P, gamma=P, beta=P, N=1, HW=64, C1=64, C2=0, G=8, eps=1e-5, silu=0, ws=P, ab=P, pre1=None, parts1=0,
                              pre2=None, parts2=0, dtype=BF16, stream=None),
    "ur_avgpool_hw": dict(x=P, out=P, N=1, HW=64, C=64, ws=P, dtype=BF16, stream=None),
    "ur_layernorm_rows": dict(x=P, y=P, gamma=P, beta=P, rows=4, C=64, eps=1e-5, dtype=BF16, stream=None),
    "ur_softmax_rows_f32": dict(s=P, p=P, rows=4, cols=77, ldp=80, dtype=BF16, stream=None),
    "ur_dwconv3x3_nhwc": dict(x=P, w=P, bias=P, y=P, N=1, H=4, W=4, C=16, gate=0, dtype=BF16, stream=None),
    "ur_scale_channels": dict(x=P, s=P, res=None, y=P, N=1, HW=4, C=16, dtype=BF16, stream=None),
    "ur_scale_channels_fanout": dict(x=P, s=P, y=P, B=1, K=2, HW=4, C=16, dtype=BF16, stream=None),
    "ur_axpy_channels": dict(a=P, b=P, s=P, y=P, rows=4, C=16, dtype=BF16, stream=None),
    "ur_spade_modulate": dict(n=P, gb=P, ldgb=32, res=None, y=P, rows=4, C=16, dtype=BF16, stream=None),
    "ur_linear_f32": dict(x=P, w=P, bias=None, y=P, M=2, N=8, K=8, groups=2, act=0, stream=None),
    "ur_tfa_prompt_update": dict(pooled=P, cond=P, upd=P, B=1, T=2, D=48, stream=None),
    "ur_tfa_prompt_update_fanout": dict(pooled=P, cond=P, upd=P, B=1, K=2, T=2, D=48, cpr=0, stream=None),
    "ur_vec_mul_group": dict(a=P, b=P, out=P, N=2, C=64, G=4, stream=None),
}
_BAD = {
    "ur_groupnorm_stats": [dict(x=None), dict(part=None), dict(N=0), dict(HW=0), dict(C=0), dict(C=12), dict(N=-1), dict(dtype=7)],
    "ur_instnorm_stats": [dict(C=0), dict(dtype=2)],
    "ur_groupnorm_finalize": [dict(part1=None), dict(parts1=0), dict(C1=0), dict(part2=P, parts2=0, C2=64), dict(part2=P, parts2=2, C2=0), dict(G=0),
                              dict(G=-4), dict(G=7), dict(N=0), dict(HW=0), dict(ab=None, mean_out=None)],
    "ur_groupnorm_apply_act": [dict(x=None), dict(y=None), dict(ab=None), dict(N=0), dict(HW=0), dict(C1=0), dict(C1=-8), dict(C1=12),
                               dict(x2=P, C2=0), dict(x2=P, C2=12), dict(dtype=7)],
    "ur_groupnorm_nhwc": [dict(x=None), dict(y=None), dict(ab=None), dict(N=0), dict(HW=0), dict(C1=0), dict(C1=12), dict(x2=P, C2=0), dict(x2=P, C2=12),
                          dict(G=0), dict(G=7), dict(dtype=7), dict(ws=None), dict(x2=P, C2=64, pre1=P, parts1=2, ws=None), dict(pre1=P, parts1=0)],
    "ur_avgpool_hw": [dict(x=None), dict(out=None), dict(ws=None), dict(N=0), dict(HW=0), dict(C=0), dict(C=12), dict(dtype=7)],
    "ur_layernorm_rows": [dict(x=None), dict(y=None), dict(rows=0), dict(C=0), dict(C=-8), dict(C=12), dict(C=2056), dict(dtype=7)],
    "ur_softmax_rows_f32": [dict(s=None), dict(p=None), dict(rows=0), dict(cols=0), dict(ldp=76), dict(dtype=7), dict(dtype=-1)],
    "ur_dwconv3x3_nhwc": [dict(x=None), dict(w=None), dict(bias=None), dict(y=None), dict(N=0), dict(H=0), dict(W=0), dict(C=0), dict(C=12),
                          dict(C=8, gate=1), dict(dtype=7)],
    "ur_scale_channels": [dict(x=None), dict(s=None), dict(y=None), dict(N=0), dict(HW=0), dict(C=0), dict(C=12), dict(dtype=7)],
    "ur_scale_channels_fanout": [dict(x=None), dict(y=None), dict(B=0), dict(HW=0), dict(C=0), dict(C=12), dict(K=0), dict(K=9), dict(dtype=7)],
    "ur_axpy_channels": [dict(a=None), dict(b=None), dict(s=None), dict(y=None), dict(rows=0), dict(C=0), dict(C=12), dict(dtype=7)],
    "ur_spade_modulate": [dict(n=None), dict(gb=None), dict(y=None), dict(rows=0), dict(C=0), dict(C=12, ldgb=24), dict(ldgb=24), dict(ldgb=36), dict(dtype=7)],
    "ur_linear_f32": [dict(x=None), dict(w=None), dict(y=None), dict(M=0), dict(N=0), dict(K=0), dict(groups=0), dict(N=7), dict(K=7)],
    "ur_tfa_prompt_update": [dict(pooled=None), dict(cond=None), dict(upd=None), dict(B=0), dict(T=0), dict(D=0)],
    "ur_tfa_prompt_update_fanout": [dict(pooled=None), dict(cond=None), dict(upd=None), dict(B=0), dict(K=0), dict(T=0), dict(D=0),
                                    dict(B=1 << 12, K=1 << 10, T=1 << 9)],
    "ur_vec_mul_group": [dict(a=None), dict(b=None), dict(out=None), dict(N=0), dict(C=0), dict(G=0), dict(G=-4), dict(G=5), dict(N=1 << 16, C=1 << 16, G=4)],
}


def refusals():
    """[(id, function name, argument tuple)]"""
    rows = []
    for fn, bads in _BAD.items():
        for bad in bads:
            assert set(bad) <= set(_GOOD[fn]), (fn, bad)
            args = dict(_GOOD[fn], **bad)
            rows.append((fn[3:] + ":" + ",".join(f"{k}={'NULL' if v is None else v}" for k, v in bad.items()), fn, tuple(args.values())))
    return rows


# the size queries: (function, arguments, expected)
QUERY_REFUSALS = [("ur_groupnorm_stats_parts", (0, 64, 64), UR_E_INVALID), ("ur_groupnorm_stats_parts", (1, 0, 64), UR_E_INVALID),
                  ("ur_groupnorm_stats_parts", (1, 64, 0), UR_E_INVALID), ("ur_groupnorm_stats_parts", (1, 64, 12), UR_E_INVALID)]
