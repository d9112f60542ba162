"""Case table of the attention parity matrix (tests/test_attention_launchers_gpu.py).  Importable without torch: the CPU gate in
tests/test_attention_plan_cpu.py plans every case on the host (ur_attention_plan_launch) and checks that each case plans to the
kernel, n_full and n_split it names at each of its workspace variants, and that the table reaches every kernel and three key splits.

A case is one ur_attention_fwd_ws geometry (B, H, Tq, Tk, D), the memory layout of its operands, its scale convention, its input
kind and, per workspace variant, the EXPECTED plan as literals (never computed from the dispatcher's rule):

  layout   "packed"    q | k | (unused) in one [B][T][3C] tensor as the fused QKV GEMM writes them (ldq = ldk = 3C, Tq == Tk)
           "separate"  q [B][Tq][C] and k [B][Tk][C] (the chain layout)
           "kv"        q [B][Tq][C], k the first C columns of a [.][Tk][2C] tensor (K | V from one GEMM: ldk = 2C)
  shared   one context for the batch: bs_k = bs_vt = 0 (cross-attention over the constant prompt embedding)
  ldvt     leading dimension of V^T (columns [Tk, ldvt) are zero by the header's contract); None: Tk rounded up to 8
  ldo_pad  ldo = H * D + ldo_pad
  scale    "folded": scale = ln 2, q arrives multiplied by log2(e) / sqrt(D) before its rounding (modules/nn.py Q_FOLD);
           "passed": scale = 1 / sqrt(D); "one": scale = 1
  kind     "randn"; "v2" (V + 2: a wrong row sum shows against |ref| ~ 2); "peaked" (q x 4); "jumps", "negative", "split_jump",
           "spike": the reference-jump constructions of tests/test_attention_pp_gpu.py and tests/test_ops_gpu.py; "dominant": one key
           with nearly all the weight and a tiny v (fp16 subnormal P) - all built by attention_reference.inputs()
  plans    workspace variant -> (kernel name, n_full, n_split).  Variants: "exact" (ur_attention_workspace_bytes), "short" (16 bytes
           less: the split must be refused), "none" (ws = NULL).  Cases whose shape has no split carry "none" only.
  ws_tiles what ur_attention_workspace_bytes sizes the workspace for (it knows the shape, not the dispatch)
  launch   False: planned on the host only, never launched
  off      plan-only cases: byte offsets of the placeholder pointers, {"q" | "k" | "vt" | "o": bytes} (a view that starts off a 16-byte
           boundary; never launched - the launched buffers are whole allocations)
  bs_extra plan-only cases: elements added to a batch stride, {"q" | "k" | "vt": elements} (a batch stride that is not a multiple of
           16 bytes)
"""

K64, K128, K512, PP = "attn_q128_d64", "attn_q128_d128", "attn_d512", "attn_pp64"
KERNELS = (K64, K128, K512, PP)
GUARD = 3                        # guard rows behind Tq / Tk / H*D inside every batch stride
P = 1 << 20                      # placeholder pointer of the host-only plan (16-byte aligned)


def pp(n_full, n_split=0):
    return (PP, n_full, n_split)


def case(cid, B, H, Tq, Tk, D, plans, *, layout="separate", shared=False, ldvt=None, ldo_pad=8, scale="passed", kind="randn",
         ws_tiles=0, launch=True, off=None, bs_extra=None):
    if not isinstance(plans, dict):
        plans = {"none": plans}
    plans = {k: (v if isinstance(v, tuple) else (v, 0, 0)) for k, v in plans.items()}
    assert layout in ("packed", "separate", "kv") and (layout != "packed" or (Tq == Tk and not shared))
    assert not launch or not (off or bs_extra), "misaligned views are planned on the host only"
    return dict(id=cid, B=B, H=H, Tq=Tq, Tk=Tk, D=D, layout=layout, shared=shared, ldvt=(Tk + 7) // 8 * 8 if ldvt is None else ldvt,
                ldo_pad=ldo_pad, scale=scale, kind=kind, plans=plans, ws_tiles=ws_tiles, launch=launch, off=dict(off or {}), bs_extra=dict(bs_extra or {}))


def cross(cid, B, H, Tq, **kw):
    """Production cross-attention (modules/nn.py CrossAttention.run_cross): 77 keys, ldvt = 80, K | V packed, one context."""
    return case(cid, B, H, Tq, 77, 64, K64, layout="kv", shared=True, ldvt=80, **kw)


CASES = [
    # ---- ping-pong kernel: every residue of the 4-tile unrolled loop (Tk / 64 = 4, 8, 12, 16) ----------------------------------
    case("pp_t256_b1h1", 1, 1, 256, 256, 64, pp(1), layout="packed", scale="folded"),                   # n_full % 8 != 0: plain tile order
    case("pp_t512_b2h5", 2, 5, 512, 512, 64, pp(20), layout="packed", kind="v2", ldo_pad=0),
    case("pp_t768_b1h2", 1, 2, 768, 768, 64, pp(6), ldo_pad=4),
    case("pp_t1024_b2h4", 2, 4, 1024, 1024, 64, pp(32), layout="packed", scale="folded", kind="peaked"),      # n_full % 8 == 0: XCD order
    # production self-attention shapes
    case("pp_chain_b8h5_t4096", 8, 5, 4096, 4096, 64, {"exact": pp(512, 128), "short": pp(640), "none": pp(640)}, scale="folded",
         ws_tiles=128),
    case("pp_b8h10_t1024", 8, 10, 1024, 1024, 64, {"exact": pp(256, 64), "short": K64, "none": K64}, layout="packed", scale="folded",
         kind="v2", ws_tiles=64),                                                                                 # 320 tiles
    case("pp_b8h20_t256", 8, 20, 256, 256, 64, pp(160), layout="packed", scale="folded"),                     # Tk % 512 != 0: never split
    case("pp_b2h5_t16384", 2, 5, 16384, 16384, 64, {"exact": pp(512, 128), "short": pp(640), "none": pp(640)}, layout="packed",
         scale="folded", ws_tiles=128, ldo_pad=0),
    # split edges.  260 tiles: the shape has 4 remainder tiles (ur_attention_workspace_bytes sizes for them), but one full round plus
    # a half round of 8 workgroups fills 260 / 384 = 0.68 < 0.75 of its slots, so the fill rule keeps the 128-query kernel with or
    # without a workspace; the smallest launch that does run a 4-tile split is two full rounds + 4 (516 tiles).
    case("q64_b13h5_t1024_260", 13, 5, 1024, 1024, 64, {"exact": K64, "short": K64, "none": K64}, layout="packed", scale="folded",
         ws_tiles=4),
    # (ldo = H*D + 4: output rows that are 8-byte, not 16-byte, aligned - the least the dispatcher admits - under the ping-pong
    #  kernel's 8-byte stores, the combine kernel's 16-byte stores and, without the workspace, the 128-query kernel)
    case("pp_b43h3_t1024_516", 43, 3, 1024, 1024, 64, {"exact": pp(512, 4), "short": K64, "none": K64}, layout="packed", scale="folded",
         kind="split_jump", ws_tiles=4, ldo_pad=4),
    case("pp_b19h5_t1024_380", 19, 5, 1024, 1024, 64, {"exact": pp(256, 124), "short": K64, "none": K64}, layout="packed",
         scale="folded", ws_tiles=124, ldo_pad=0),
    case("q64_b76h5_t256_380", 76, 5, 256, 256, 64, K64, layout="packed", scale="folded"),                    # 380 < 384: two rounds too empty
    case("pp_b77h5_t256_385", 77, 5, 256, 256, 64, pp(385), layout="packed", scale="folded"),                 # 385 >= 384: ping-pong, unsplit
    case("pp_b32h5_t1024_split_jump", 32, 5, 1024, 1024, 64, {"exact": pp(512, 128), "none": pp(640)}, layout="packed",
         kind="split_jump", ws_tiles=128, ldo_pad=0),
    # Tq != Tk, shared context, the slow path of the online softmax
    case("pp_tq512_tk256", 2, 2, 512, 256, 64, pp(8)),
    case("pp_tq256_tk1024", 3, 2, 256, 1024, 64, pp(6), scale="folded", kind="jumps"),
    case("pp_shared_ctx", 4, 5, 512, 256, 64, pp(40), layout="kv", shared=True),
    case("pp_slow_path_jumps", 1, 2, 1024, 1024, 64, pp(8), layout="packed", scale="folded", kind="jumps"),
    case("pp_all_negative", 1, 1, 256, 256, 64, pp(1), scale="one", kind="negative"),
    case("pp_spike_t256", 1, 1, 256, 256, 64, pp(1), kind="spike", ldo_pad=0),
    case("pp_dominant_t1024", 2, 2, 1024, 1024, 64, pp(16), layout="packed", kind="dominant"),
    # ---- 128-query kernel, d = 64 -------------------------------------------------------------------------------------------------
    cross("q64_cross_b8h5_t4096", 8, 5, 4096),
    cross("q64_cross_b8h10_t1024", 8, 10, 1024, kind="v2"),
    cross("q64_cross_b8h20_t256", 8, 20, 256, kind="peaked", ldo_pad=0),
    cross("q64_cross_b8h20_t64", 8, 20, 64),
    case("q64_mid_b8h20_t64", 8, 20, 64, 64, 64, K64, layout="packed", scale="folded"),
    case("q64_tq1_tk1", 2, 2, 1, 1, 64, K64),
    case("q64_tq100_tk63", 2, 2, 100, 63, 64, K64, kind="v2"),
    case("q64_tq129_tk64", 2, 2, 129, 64, 64, K64, ldo_pad=0),
    case("q64_tq100_tk65", 2, 2, 100, 65, 64, K64, kind="peaked"),
    case("q64_tq129_tk200_ldvt264", 2, 2, 129, 200, 64, K64, ldvt=264, kind="spike"),
    case("q64_tq1_tk200", 1, 3, 1, 200, 64, K64, layout="kv"),
    case("q64_dominant_tq100_tk200", 2, 2, 100, 200, 64, K64, kind="dominant"),
    # shapes the ping-pong kernel refuses for a reason other than size
    case("q64_tq256_tk128", 2, 2, 256, 128, 64, K64, scale="folded"),                                          # Tk % 256 != 0
    case("q64_tq256_tk320", 1, 2, 256, 320, 64, K64, kind="jumps", scale="folded"),
    case("q64_tq384_tk256", 1, 2, 384, 256, 64, K64, kind="v2"),                                               # Tq % 256 != 0
    # plan only, never launched: q / k / V^T not 16-byte aligned, o not 8-byte aligned, a batch stride that is not a multiple of 16 bytes
    # (csrc/attention_params.h attn_pp_shape_ok: the hand-written loop reads whole 16-byte rows through unchecked buffer descriptors)
    case("q64_q_offset_8_bytes", 2, 2, 256, 256, 64, K64, launch=False, off={"q": 8}),
    case("q64_k_offset_8_bytes", 2, 2, 256, 256, 64, K64, launch=False, off={"k": 8}),
    case("q64_vt_offset_8_bytes", 2, 2, 256, 256, 64, K64, launch=False, off={"vt": 8}),
    case("q64_o_offset_4_bytes", 2, 2, 256, 256, 64, K64, launch=False, off={"o": 4}),
    case("pp_o_offset_8_bytes", 2, 2, 256, 256, 64, pp(4), launch=False, off={"o": 8}),                         # 8-byte aligned o is enough
    case("q64_bs_q_not_16_bytes", 2, 2, 256, 256, 64, K64, launch=False, bs_extra={"q": 4}),
    case("q64_bs_k_not_16_bytes", 2, 2, 256, 256, 64, K64, launch=False, bs_extra={"k": 4}),
    case("q64_bs_vt_not_16_bytes", 2, 2, 256, 256, 64, K64, launch=False, bs_extra={"vt": 4}),
    # ---- 128-query kernel, d = 128 ------------------------------------------------------------------------------------------------
    case("q128_b2h4_t64", 2, 4, 64, 64, 128, K128),
    case("q128_b2h4_tq256_tk77", 2, 4, 256, 77, 128, K128, kind="v2", layout="kv", shared=True, ldvt=80),
    case("q128_tq100_tk65", 1, 2, 100, 65, 128, K128, kind="peaked", ldo_pad=0),
    case("q128_tq300_tk200", 2, 2, 300, 200, 128, K128, kind="spike"),
    case("q128_dominant_tq64_tk256", 1, 2, 64, 256, 128, K128, kind="dominant"),
    # ---- d = 512 --------------------------------------------------------------------------------------------------------------------
    case("d512_b8h1_t4096", 8, 1, 4096, 4096, 512, K512, layout="packed"),
    case("d512_b1h1_t16384", 1, 1, 16384, 16384, 512, K512, ldo_pad=0),
    case("d512_tq100_tk200", 1, 1, 100, 200, 512, K512, kind="v2"),
    case("d512_h2_tq64_tk128", 1, 2, 64, 128, 512, K512, kind="peaked"),
    case("d512_b2_tq256_tk77", 2, 1, 256, 77, 512, K512, ldvt=80, layout="kv", shared=True),
    case("d512_spike_t256", 1, 1, 256, 256, 512, K512, kind="spike"),
    # (two batches of two heads, as the other "dominant" cases: the construction fills batch 0, head 0 with outputs of size 2^-15 |v|
    #  against an E_sub of ~2^-25 sqrt(Tk) - a tensor made of that head alone has a whole-tensor rel-L2 of that ratio, ~1e-3 in fp16,
    #  which says nothing about the kernel; the element bound is what checks those rows)
    case("d512_dominant_t256", 2, 2, 256, 256, 512, K512, kind="dominant", ldo_pad=0),
]
LAUNCHED = [c for c in CASES if c["launch"]]


def channels(c):
    return c["H"] * c["D"]


def geometry(c):
    """Leading dimensions, batch strides (elements) and allocation shapes of case c.  Every operand has GUARD rows behind its
    Tq / Tk / H*D rows inside the batch stride; a shared context is one block without a per-batch guard."""
    C, B, Tq, Tk = channels(c), c["B"], c["Tq"], c["Tk"]
    g = dict(C=C, ldvt=c["ldvt"], ldo=C + c["ldo_pad"])
    nb = 1 if c["shared"] else B
    if c["layout"] == "packed":
        g.update(ldq=3 * C, ldk=3 * C, q_shape=(B, Tq + GUARD, 3 * C), k_shape=None, k_col=C)
    else:
        ldk = 2 * C if c["layout"] == "kv" else C
        g.update(ldq=C, ldk=ldk, q_shape=(B, Tq + GUARD, C), k_shape=(nb, Tk + GUARD, ldk), k_col=0)
    ex = c["bs_extra"]
    g["bs_q"] = (Tq + GUARD) * g["ldq"] + ex.get("q", 0)
    g["bs_k"] = 0 if c["shared"] else (Tk + GUARD) * g["ldk"] + ex.get("k", 0)
    g["vt_shape"] = (nb, C + GUARD, c["ldvt"])
    g["bs_vt"] = 0 if c["shared"] else (C + GUARD) * c["ldvt"] + ex.get("vt", 0)
    g["o_shape"] = (B, Tq + GUARD, g["ldo"])
    g["bs_o"] = (Tq + GUARD) * g["ldo"]
    return g


def ws_bytes(c):
    return c["ws_tiles"] * 2 * 256 * 68 * 4


def ws_arg(c, variant):
    """(has workspace, ws_bytes passed) of a workspace variant."""
    return {"exact": (True, ws_bytes(c)), "short": (True, ws_bytes(c) - 16), "none": (False, 0)}[variant]


def plan_args(c, variant, q=None, k=None, vt=None, o=None, ws=None):
    """Argument tuple of ur_attention_plan_launch (pointers default to placeholders; the values matter only for alignment)."""
    g = geometry(c)
    has, nbytes = ws_arg(c, variant)
    off = c["off"]
    q = P + off.get("q", 0) if q is None else q
    k = (q + 2 * g["k_col"] if c["layout"] == "packed" else 2 * P + off.get("k", 0)) if k is None else k
    return (q, k, 3 * P + off.get("vt", 0) if vt is None else vt, 4 * P + off.get("o", 0) if o is None else o, c["B"], c["H"], c["Tq"], c["Tk"], c["D"], g["ldq"], g["ldk"],
            g["ldvt"], g["ldo"], g["bs_q"], g["bs_k"], g["bs_vt"], g["bs_o"], (5 * P if ws is None else ws) if has else None, nbytes)
