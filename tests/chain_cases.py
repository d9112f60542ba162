"""Case table of the fused-chain parity matrix (tests/test_chain_launchers_gpu.py, tests/test_chain_stream_cpu.py).  Importable
without torch.  The kernels are the token-stationary chains of csrc/tchain.hip behind the raw C ABI:

  MLP   ur_ff_geglu_fused             HEAD  ur_transformer_head_fused
  TAIL  ur_transformer_tail_fused     CSCE  ur_csce_fused

Every launched case has C = 320 and at most 1024 tokens, and runs in both 16-bit types.  A case is literal arguments:

  N, hw    images and tokens per image (T = N * hw; one workgroup = 128 tokens, so hw = 128 with N > 1 changes the image - GroupNorm
           affine row, V^T image stride, partial-plane slot - at every workgroup, and hw = 384 is no power of two)
  hidden   GEGLU hidden units (MLP, TAIL): the stream has 3 tiles per 64 of them.  64 / 128 / 192 give an MLP stream of 3 / 6 / 9 tiles
           around the 3-slot ring's prefetch depth of two tiles (shorter than, equal to and longer than it)
  tk       context tokens baked into the TAIL stream: the key mask is `key < tk - 8 * h` per lane half, keys sit in k-steps of 16 and
           score fragments of 64 + 32, so every tk around 8, 16 and 64, the production 77 and the limits 1 and 80 are there
  scale    attn_scale of TAIL
  ldx, ldy row strides of MLP's x and y (the other kernels take none)
  gn       "yes": gn_part given; "no": NULL; "both": launched both ways, y must agree bit for bit
  kind     input kind (tests/chain_reference.py make()): "randn", "offset", "peaked", "gelu_tail", "per_image"

REFUSALS are host-side argument checks: (id, kernel, overrides of a valid call, expected code).  The overrides are chosen so that a
wrongly ACCEPTED call would still stay inside the buffers the test allocates (test_chain_launchers_gpu.py sizes every buffer for
REFUSAL_T tokens of REFUSAL_LD elements and a full-length stream); the T * C >= 2^31 check is left out for that reason, and a NULL
pointer row also carries C = 256, which the next check refuses with the other code.
"""
MLP, HEAD, TAIL, CSCE = "mlp", "head", "tail", "csce"
KERNELS = (MLP, HEAD, TAIL, CSCE)
SYMBOL = {MLP: "ur_ff_geglu_fused", HEAD: "ur_transformer_head_fused", TAIL: "ur_transformer_tail_fused", CSCE: "ur_csce_fused"}
C, CCOND, HEADS, CROSS = 320, 256, 5, 96          # CROSS: width of the context the TAIL packer projects (any width packs alike)
TOK = 128                                          # tokens per workgroup
INVALID, UNSUPPORTED = -1, -2                      # UR_E_INVALID, UR_E_UNSUPPORTED (include/unirestore_hip.h)


def case(cid, kernel, N, hw, *, hidden=0, tk=0, scale=0.125, kind="randn", ldx=C, ldy=C, gn="yes"):
    assert kernel in KERNELS and hw % TOK == 0 and N * hw <= 1024 and gn in ("yes", "no", "both")
    return dict(id=cid, kernel=kernel, N=N, hw=hw, T=N * hw, hidden=hidden, tk=tk, scale=scale, kind=kind, ldx=ldx, ldy=ldy, gn=gn)


def ntiles(c):
    return {MLP: 3 * c["hidden"] // 64, HEAD: 20, TAIL: 25 + 3 * c["hidden"] // 64, CSCE: 14}[c["kernel"]]


CASES = [
    # ---- MLP: ring shorter than / equal to / longer than its prefetch depth, row strides, LayerNorm cancellation, GELU tail ----
    case("mlp_h64", MLP, 1, 128, hidden=64),
    case("mlp_h128", MLP, 1, 128, hidden=128),
    case("mlp_h192", MLP, 1, 128, hidden=192),
    case("mlp_h1280", MLP, 1, 128, hidden=1280),
    case("mlp_t384_ld", MLP, 1, 384, hidden=320, ldx=328, ldy=336),
    case("mlp_t256_offset", MLP, 1, 256, hidden=1280, kind="offset"),
    case("mlp_gelu_tail", MLP, 1, 128, hidden=128, kind="gelu_tail"),
    # ---- HEAD ---------------------------------------------------------------------------------------------------------------
    case("head_1x128", HEAD, 1, 128),
    case("head_3x128_per_image", HEAD, 3, 128, kind="per_image"),
    case("head_3x128_offset", HEAD, 3, 128, kind="offset"),
    case("head_2x384_offset", HEAD, 2, 384, kind="offset"),
    case("head_2x384", HEAD, 2, 384),
    case("head_1x1024", HEAD, 1, 1024),
    # ---- TAIL: every key-mask edge at the smallest shape ------------------------------------------------------------------------
    *[case(f"tail_tk{tk}", TAIL, 1, 128, hidden=128, tk=tk, gn="yes" if tk % 2 else "no")
      for tk in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 72, 77, 79, 80)],
    case("tail_h1280_tk77", TAIL, 1, 128, hidden=1280, tk=77, gn="both"),
    case("tail_h1280_tk80_offset", TAIL, 1, 128, hidden=1280, tk=80, kind="offset"),
    case("tail_3x128", TAIL, 3, 128, hidden=128, tk=77, gn="both"),
    case("tail_3x128_offset", TAIL, 3, 128, hidden=64, tk=9, kind="offset", scale=0.25),
    case("tail_2x384_scale4", TAIL, 2, 384, hidden=128, tk=77, scale=0.25),
    case("tail_2x384_peaked", TAIL, 2, 384, hidden=64, tk=77, kind="peaked", gn="both"),
    case("tail_1x128_peaked_tk65", TAIL, 1, 128, hidden=64, tk=65, kind="peaked", scale=0.25, gn="no"),
    # ---- CSCE ---------------------------------------------------------------------------------------------------------------
    case("csce_1x128", CSCE, 1, 128, gn="both"),
    case("csce_3x128_gelu_tail", CSCE, 3, 128, kind="gelu_tail"),
    case("csce_3x128", CSCE, 3, 128, gn="both"),
    case("csce_2x384", CSCE, 2, 384, gn="no"),
    case("csce_2x384_gelu_tail", CSCE, 2, 384, kind="gelu_tail", gn="both"),
]


def launch_ints(c):
    """the integer arguments of a launched case, keyed as VALID"""
    return dict(T=c["T"], hw=c["hw"], C=C, Ccond=CCOND, hidden=c["hidden"], heads=HEADS, tk=c["tk"], ldx=c["ldx"], ldy=c["ldy"])


def call_args(kernel, a, ptr, dtype, stream_bytes, handle=None, eps=1e-5, scale=0.125):
    """Argument tuple of the kernel's C entry point: a = the integer arguments (keys of VALID), ptr = {pointer name: address or None}
    ("gn_part" is optional), dtype = UR_DT_*."""
    p = lambda n: ptr.get(n)
    if kernel == MLP:
        return (p("x"), p("stream"), stream_bytes, p("y"), a["T"], a["C"], a["hidden"], a["ldx"], a["ldy"], eps, dtype, handle)
    if kernel == HEAD:
        return (p("x"), p("ab"), p("stream"), stream_bytes, p("h0"), p("q"), p("k"), p("vt"), a["T"], a["hw"], a["C"], eps, dtype, handle)
    if kernel == TAIL:
        return (p("o1"), p("h0"), p("xres"), p("stream"), stream_bytes, p("y"), p("gn_part"), a["T"], a["hw"], a["C"], a["hidden"],
                a["heads"], a["tk"], eps, scale, dtype, handle)
    return (p("x"), p("cond"), p("stream"), stream_bytes, p("y"), p("gn_part"), a["T"], a["hw"], a["C"], a["Ccond"], dtype, handle)


BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

# ---- refusals ------------------------------------------------------------------------------------------------------------------
REFUSAL_T, REFUSAL_LD, REFUSAL_HIDDEN = 256, 336, 128       # every buffer of a refusal call holds REFUSAL_T rows of REFUSAL_LD
# a valid call per kernel (never launched as such); `short` = bytes taken off stream_bytes; null = the pointer argument passed as NULL
VALID = {
    MLP: dict(T=128, C=C, hidden=REFUSAL_HIDDEN, ldx=C, ldy=C, short=0, null=None),
    HEAD: dict(T=256, hw=128, C=C, short=0, null=None),
    TAIL: dict(T=256, hw=128, C=C, hidden=REFUSAL_HIDDEN, heads=HEADS, tk=77, short=0, null=None),
    CSCE: dict(T=256, hw=128, C=C, Ccond=CCOND, short=0, null=None),
}
POINTERS = {MLP: ("x", "stream", "y"), HEAD: ("x", "ab", "stream", "h0", "q", "k", "vt"), TAIL: ("o1", "h0", "xres", "stream", "y"),
            CSCE: ("x", "cond", "stream", "y")}


def _ref(cid, kernel, code, **over):
    assert set(over) <= set(VALID[kernel])
    return (cid, kernel, over, code)


REFUSALS = [
    *[_ref(f"{k}_c256", k, UNSUPPORTED, C=256) for k in KERNELS],                 # C != 320 (smaller: a launch would read less)
    _ref("tail_heads4", TAIL, UNSUPPORTED, heads=4),
    _ref("tail_tk0", TAIL, UNSUPPORTED, tk=0),
    _ref("tail_tk81", TAIL, UNSUPPORTED, tk=81),
    _ref("csce_ccond128", CSCE, UNSUPPORTED, Ccond=128),
    *[_ref(f"{k}_t0", k, INVALID, T=0) for k in KERNELS],
    *[_ref(f"{k}_t100", k, INVALID, T=100, **({} if k == MLP else {"hw": 100})) for k in KERNELS],
    *[_ref(f"{k}_hw96", k, INVALID, T=192, hw=96) for k in (HEAD, TAIL, CSCE)],
    *[_ref(f"{k}_hw_not_dividing", k, INVALID, T=128, hw=256) for k in (HEAD, TAIL, CSCE)],
    *[_ref(f"{k}_hidden0", k, INVALID, hidden=0) for k in (MLP, TAIL)],
    *[_ref(f"{k}_hidden96", k, INVALID, hidden=96) for k in (MLP, TAIL)],
    _ref("mlp_ldx324", MLP, INVALID, ldx=324),
    _ref("mlp_ldy324", MLP, INVALID, ldy=324),
    _ref("mlp_ldx312", MLP, INVALID, ldx=312),
    _ref("mlp_ldy312", MLP, INVALID, ldy=312),
    *[_ref(f"{k}_stream_short", k, INVALID, short=1) for k in KERNELS],
    # NULL pointers: the pointer check comes first and answers INVALID.  C = 256 rides along, so that a call whose NULL got past a
    # broken check is still refused (as UNSUPPORTED: the row fails) and never launched with a NULL pointer
    *[_ref(f"{k}_null_{p}", k, INVALID, null=p, C=256) for k in KERNELS for p in POINTERS[k]],
]
assert len({r[0] for r in REFUSALS}) == len(REFUSALS)
REFUSAL_TILES = 25 + 3 * REFUSAL_HIDDEN // 64               # the longest stream a refusal row's valid call needs (TAIL)


def refusal_call(row, ptr, dtype, tile_bytes):
    """(symbol, argument tuple, expected code) of a refusal row; ptr = {name: address} of buffers sized as the module docstring says"""
    _, kernel, over, code = row
    a = dict(VALID[kernel], **over)
    nt = {MLP: 3 * REFUSAL_HIDDEN // 64, HEAD: 20, TAIL: REFUSAL_TILES, CSCE: 14}[kernel]
    ptr = {n: (None if n == a["null"] else v) for n, v in ptr.items()}
    return SYMBOL[kernel], call_args(kernel, a, ptr, dtype, nt * tile_bytes - a["short"]), code
