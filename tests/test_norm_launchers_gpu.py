"""Every export of csrc/norms.hip and the per-channel block of csrc/elementwise.hip against fp64, element by element (-m gpu, bf16 and
fp16): GroupNorm statistics / finalize / apply and the chained entry point, avgpool, LayerNorm, row softmax, depthwise 3x3, the
per-channel scale / axpy / SPADE kernels and their fan-outs, linear_f32, the TFA prompt update and vec_mul_group.

The cases are tests/norm_cases.py; the fp64 references and the per-element bounds, with their derivations, are
tests/norm_reference.py (the one statement of the bounds: this module only applies them).  tests/test_norm_reference_cpu.py holds the
host-side half: geometry, property coverage, refusals, the CPU emulation and the mutations.

Every call goes through the raw C ABI (capi.lib) and, for every case and dtype:
  * outputs, statistics planes, ab and mean_out live inside NaN-filled allocations with guard elements before and after them, which
    must come back bit-unchanged; every input sits inside a larger NaN-filled allocation too, so a read past its end reaches the
    output as NaN;
  * the case runs twice into fresh buffers: outputs and planes must be bit-identical;
  * every output element is checked against its bound, the whole tensor against the rel-L2 tolerance of tests/test_ops_gpu.py; no NaN
    may be left anywhere that should have been written (for the statistics: every one of the P planes).
The module sets no environment variables and starts no processes.  It prints the worst |y - ref| / bound per (kernel, dtype) at its end.
"""
import pytest
import torch

import norm_cases as T
import norm_reference as R

pytestmark = pytest.mark.gpu
DTYPES = R.DTYPES
GUARD = 64                      # guard elements before and after every buffer (a multiple of 16 bytes in every type)
WORST = {}                      # (kernel, dtype) -> largest |y - ref| / bound seen


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    yield c
    if WORST:
        print("\nlargest |y - ref| / bound per kernel:")
        for (name, dt), r in sorted(WORST.items()):
            print(f"  {name:28s} {dt}: {r:.3f}")


def _note(kernel, dtype, r):
    WORST[(kernel, dtype)] = max(WORST.get((kernel, dtype), 0.0), r)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class Buf:
    """`shape` elements of `dtype` inside a NaN-filled allocation with GUARD elements on either side."""

    def __init__(self, shape, dtype, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.raw = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.t = self.raw[GUARD:GUARD + n].view(*shape)
        if fill is not None:
            self.t.copy_(fill)
        self.nan = _bits(torch.full((1,), float("nan"), dtype=dtype, device="cuda"))[0]

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_ok(self):
        b = _bits(self.raw)
        return bool((b[:GUARD] == self.nan).all()) and bool((b[-GUARD:] == self.nan).all())


def _in(t, dt=None):
    """An input tensor (any device) inside a larger NaN-filled allocation on the GPU."""
    t = t if dt is None else t.to(dt)
    return Buf(tuple(t.shape), t.dtype, fill=t.cuda())


def _ptr(b):
    return None if b is None else b.ptr


def _code(capi, dt):
    return capi.UR_DT_F16 if dt == torch.float16 else capi.UR_DT_BF16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _twice(shapes, launch, what):
    """Run `launch(*buffers)` twice into fresh NaN buffers of `shapes` = [(shape, dtype) | None]; guards intact, bit-identical results.
    Returns the tensors of the first run."""
    runs = []
    for _ in range(2):
        bufs = [None if s is None else Buf(*s) for s in shapes]
        launch(*bufs)
        torch.cuda.synchronize()
        for i, b in enumerate(bufs):
            assert b is None or b.guards_ok(), f"{what}: write outside buffer {i}"
        runs.append(bufs)
    for i, (a, b) in enumerate(zip(*runs)):
        assert a is None or torch.equal(_bits(a.t), _bits(b.t)), f"{what}: buffer {i} not bit-identical between two runs"
    return [None if b is None else b.t for b in runs[0]]


def _judge(kernel, dtype, y, ref, bnd, what, rel_tol=None):
    assert bool(torch.isfinite(y).all()), what + ": output not finite"
    rel = R.rel_l2(y, ref)
    try:
        r = R.compare(y.double(), ref, bnd, what)
    finally:
        print(f"{what}: worst |y - ref| / bound {R.worst(y, ref, bnd):.3f}, rel-L2 {rel:.3e}")
    _note(kernel, dtype, r)
    if rel_tol is not None:
        assert rel < rel_tol, what


# ---- GroupNorm: statistics -> finalize -> apply, each through its own entry point ----------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.GN_CASES, ids=[c["id"] for c in T.GN_CASES])
def test_groupnorm_parity(capi, c, dtype):
    dt, lib, code = DTYPES[dtype], capi.lib, _code(capi, DTYPES[dtype])
    N, HW, C1, C2, G = c["N"], c["HW"], c["C1"], c["C2"], c["G"]
    C = C1 + C2
    x1, x2, gamma, beta = R.gn_inputs(c, dt)
    bx1, bx2 = _in(x1), (_in(x2) if C2 else None)
    bg, bb = (_in(gamma), _in(beta)) if c["affine"] else (None, None)
    stats = lib.ur_instnorm_stats if G == C else lib.ur_groupnorm_stats
    assert lib.ur_groupnorm_stats_parts(N, HW, C1) == c["P"] and (not C2 or lib.ur_groupnorm_stats_parts(N, HW, C2) == c["P2"])

    def launch(pl1, pl2, ab, mean, y):
        capi.check(stats(bx1.ptr, pl1.ptr, N, HW, C1, code, _stream()))
        if C2:
            capi.check(stats(bx2.ptr, pl2.ptr, N, HW, C2, code, _stream()))
        capi.check(lib.ur_groupnorm_finalize(pl1.ptr, c["P"], C1, _ptr(pl2), c["P2"], C2, _ptr(bg), _ptr(bb), N, HW, G, R.EPS, ab.ptr, mean.ptr, _stream()))
        capi.check(lib.ur_groupnorm_apply_act(bx1.ptr, _ptr(bx2), y.ptr, ab.ptr, N, HW, C1, C2, c["silu"], code, _stream()))

    what = f"{c['id']} [{dtype}]"
    pl1, pl2, ab, mean, y = _twice([((N, c["P"], C1, 2), torch.float32), ((N, c["P2"], C2, 2), torch.float32) if C2 else None,
                                    ((N, 2, C), torch.float32), ((N, G), torch.float32), ((N, HW, C), dt)], launch, what)
    ref = R.gn_reference(bx1.t, bx2.t if C2 else None, gamma, beta, G, c["silu"], dt)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(ab).all()) and bool(torch.isfinite(mean).all()), what + ": NaN left in an output"
    rel = R.rel_l2(y, ref["y"])
    try:
        ratios = R.gn_check(ref, y, [p for p in (pl1, pl2) if p is not None], ab, mean, what)
    finally:
        print(f"{what}: y worst ratio {R.worst(y, ref['y'], ref['y_bnd']):.3f}, ab {R.worst(ab, ref['ab'], ref['ab_bnd']):.3f}, rel-L2 {rel:.3e}")
    for name, r in ratios.items():
        _note("groupnorm " + name, dtype, r)
    assert rel < R.REL_TOL[dt], what
    if c["avgpool"]:
        nws = lib.ur_groupnorm_ws_bytes(N, HW, C1) // 4

        def pool(out, ws):
            capi.check(lib.ur_avgpool_hw(bx1.ptr, out.ptr, N, HW, C1, ws.ptr, code, _stream()))
        out, ws = _twice([((N, C1), torch.float32), ((nws,), torch.float32)], pool, what + " avgpool")
        assert bool(torch.isfinite(ws).all()), what + ": avgpool left part of its planes unwritten"
        _judge("avgpool_hw", dtype, out, ref["chan_mean"][:, :C1], ref["chan_mean_bnd"][:, :C1], what + " avgpool")


@pytest.mark.parametrize("c", T.FINALIZE_CASES, ids=[c["id"] for c in T.FINALIZE_CASES])
def test_groupnorm_finalize_on_synthetic_planes(capi, c):
    lib = capi.lib
    N, C, G = c["N"], c["C1"] + c["C2"], c["G"]
    p1, p2, gamma, beta = R.finalize_inputs(c)
    b1, b2 = _in(p1), (_in(p2) if p2 is not None else None)
    bg, bb = (_in(gamma), _in(beta)) if c["affine"] else (None, None)
    want_ab, want_mean = c["outs"] in ("ab", "both"), c["outs"] in ("mean", "both")

    def launch(ab, mean):
        capi.check(lib.ur_groupnorm_finalize(b1.ptr, c["P1"], c["C1"], _ptr(b2), c["P2"], c["C2"], _ptr(bg), _ptr(bb), N, c["HW"], G, R.EPS, _ptr(ab),
                                             _ptr(mean), _stream()))
    ab, mean = _twice([((N, 2, C), torch.float32) if want_ab else None, ((N, G), torch.float32) if want_mean else None], launch, c["id"])
    ref = R.finalize_reference(b1.t, b2.t if b2 is not None else None, gamma, beta, G, c["HW"])
    for t in (ab, mean):
        assert t is None or bool(torch.isfinite(t).all()), c["id"] + ": NaN left in an output"
    for name, r in R.gn_check(ref, None, None, ab, mean, c["id"]).items():
        print(f"{c['id']}: {name} worst ratio {r:.3f}")
        _note("groupnorm_finalize " + name, "fp32", r)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.NHWC_CASES, ids=[c["id"] for c in T.NHWC_CASES])
def test_groupnorm_nhwc_chained(capi, c, dtype):
    """ur_groupnorm_nhwc with producer-side planes of the producer's own P for x, for both sources or for neither: the ws scratch holds
    exactly the planes of the sources that came without (the guard behind it proves the size)."""
    dt, lib, code = DTYPES[dtype], capi.lib, _code(capi, DTYPES[dtype])
    N, HW, C1, C2, G = c["N"], c["HW"], c["C1"], c["C2"], c["G"]
    C = C1 + C2
    x1, x2, gamma, beta = R.gn_inputs(dict(c, affine=True), dt)
    bx1, bx2, bg, bb = _in(x1), (_in(x2) if C2 else None), _in(gamma), _in(beta)
    P1, P2 = c["pre"]
    pre1 = _in(R.producer_planes(bx1.t, P1)) if P1 else None
    pre2 = _in(R.producer_planes(bx2.t, P2)) if P2 else None
    nws = (0 if P1 else lib.ur_groupnorm_ws_bytes(N, HW, C1) // 4) + (0 if (P2 or not C2) else lib.ur_groupnorm_ws_bytes(N, HW, C2) // 4)

    def launch(y, ab, ws):
        capi.check(lib.ur_groupnorm_nhwc(bx1.ptr, _ptr(bx2), y.ptr, bg.ptr, bb.ptr, N, HW, C1, C2, G, R.EPS, c["silu"], _ptr(ws), ab.ptr, _ptr(pre1), P1,
                                         _ptr(pre2), P2, code, _stream()))
    what = f"{c['id']} [{dtype}]"
    y, ab, ws = _twice([((N, HW, C), dt), ((N, 2, C), torch.float32), ((nws,), torch.float32) if nws else None], launch, what)
    assert ws is None or bool(torch.isfinite(ws).all()), what + ": part of the scratch planes left unwritten"
    ref = R.gn_reference(bx1.t, bx2.t if C2 else None, gamma, beta, G, c["silu"], dt)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(ab).all()), what + ": NaN left in an output"
    for name, r in R.gn_check(ref, y, None, ab, None, what).items():
        print(f"{what}: {name} worst ratio {r:.3f}")
        _note("groupnorm_nhwc " + name, dtype, r)
    assert R.rel_l2(y, ref["y"]) < R.REL_TOL[dt], what


# ---- LayerNorm, row softmax ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.LN_CASES, ids=[c["id"] for c in T.LN_CASES])
def test_layernorm_parity(capi, c, dtype):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    x, gamma, beta = R.ln_inputs(c, dt)
    bx, bg, bb = _in(x), (_in(gamma) if c["gamma"] else None), (_in(beta) if c["beta"] else None)
    what = f"{c['id']} [{dtype}]"
    y, = _twice([((c["rows"], c["C"]), dt)],
                lambda y: capi.check(capi.lib.ur_layernorm_rows(bx.ptr, y.ptr, _ptr(bg), _ptr(bb), c["rows"], c["C"], R.EPS, code, _stream())), what)
    ref, bnd = R.ln_reference(bx.t, gamma, beta, dt)
    _judge("layernorm_rows", dtype, y, ref, bnd, what, R.REL_TOL[dt])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.SOFTMAX_CASES, ids=[c["id"] for c in T.SOFTMAX_CASES])
def test_softmax_rows_parity(capi, c, dtype):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    bs = _in(R.softmax_inputs(c))
    rows, cols, ldp = c["rows"], c["cols"], c["ldp"]
    what = f"{c['id']} [{dtype}]"
    p, = _twice([((rows, ldp), dt)], lambda p: capi.check(capi.lib.ur_softmax_rows_f32(bs.ptr, p.ptr, rows, cols, ldp, code, _stream())), what)
    assert bool((_bits(p[:, cols:]) == 0).all()), what + ": columns [cols, ldp) must be zero bits"
    ref, bnd = R.softmax_reference(bs.t, dt)
    _judge("softmax_rows_f32", dtype, p[:, :cols], ref, bnd, what, R.REL_TOL[dt])
    if c["kind"] == "subnormal" and dt == torch.float16:
        assert bool(((p[0, :cols] > 0) & (p[0, :cols] < 2.0 ** -14)).any()), what + ": no subnormal probability was stored"


# ---- depthwise 3x3 and the per-channel elementwise kernels ---------------------------------------------------------------------------------
def _dwconv(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    N, H, W, C, gate = c["N"], c["H"], c["W"], c["C"], c.get("gate", 0)
    x, w, b = R.dwconv_inputs(c, dt, device)
    bx, bw, bb = _in(x), _in(w), _in(b)
    what = f"{c['id']} [{dtype}]"
    y, = _twice([((N, H, W, C // 2 if gate else C), dt)],
                lambda y: capi.check(capi.lib.ur_dwconv3x3_nhwc(bx.ptr, bw.ptr, bb.ptr, y.ptr, N, H, W, C, gate, code, _stream())), what)
    ref, bnd = R.dwconv_reference(bx.t, bw.t, bb.t, gate, dt)
    _judge("dwconv3x3 strip" if W % 4 == 0 else "dwconv3x3 pixel", dtype, y, ref, bnd, what, R.REL_TOL[dt])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.DWCONV_CASES, ids=[c["id"] for c in T.DWCONV_CASES])
def test_dwconv_parity(capi, c, dtype):
    _dwconv(capi, c, dtype, "cpu")


def _scale_inputs(c, dt, n_scales, device="cpu"):
    g = torch.Generator(device=device).manual_seed(R.zlib.crc32(c["id"].encode()))
    B = c.get("N", c.get("B"))
    x = torch.randn(B, c["HW"], c["C"], generator=g, device=device).to(dt)
    s = torch.randn(n_scales, c["C"], generator=g, device=device)
    r = torch.randn(B, c["HW"], c["C"], generator=g, device=device).to(dt) if c.get("res") else None
    return x, s, r


def _scale(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    x, s, r = _scale_inputs(c, dt, c["N"], device)
    bx, bs, br = _in(x), _in(s), (_in(r) if r is not None else None)
    what = f"{c['id']} [{dtype}]"
    y, = _twice([(tuple(x.shape), dt)],
                lambda y: capi.check(capi.lib.ur_scale_channels(bx.ptr, bs.ptr, _ptr(br), y.ptr, c["N"], c["HW"], c["C"], code, _stream())), what)
    ref, bnd = R.scale_reference(bx.t, bs.t, None if br is None else br.t, dt)
    _judge("scale_channels", dtype, y, ref, bnd, what, R.REL_TOL[dt])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.SCALE_CASES, ids=[c["id"] for c in T.SCALE_CASES])
def test_scale_channels_parity(capi, c, dtype):
    _scale(capi, c, dtype, "cpu")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.FANOUT_CASES, ids=[c["id"] for c in T.FANOUT_CASES])
def test_scale_channels_fanout_gives_the_bits_of_the_single_task_kernel(capi, c, dtype):
    dt, code, lib = DTYPES[dtype], _code(capi, DTYPES[dtype]), capi.lib
    B, K, HW, C = c["B"], c["K"], c["HW"], c["C"]
    x, s, _ = _scale_inputs(c, dt, K * B)
    bx, bs = _in(x), (_in(s) if c["s"] else None)
    what = f"{c['id']} [{dtype}]"
    y, = _twice([((K * B, HW, C), dt)], lambda y: capi.check(lib.ur_scale_channels_fanout(bx.ptr, _ptr(bs), y.ptr, B, K, HW, C, code, _stream())), what)
    for k in range(K):
        if not c["s"]:
            assert torch.equal(_bits(y[k * B:(k + 1) * B]), _bits(bx.t)), what + f": slice {k} is not a bit copy of x"
            continue
        one = Buf((B, HW, C), dt)
        sk = _in(bs.t[k * B:(k + 1) * B])
        capi.check(lib.ur_scale_channels(bx.ptr, sk.ptr, None, one.ptr, B, HW, C, code, _stream()))
        torch.cuda.synchronize()
        assert torch.equal(_bits(y[k * B:(k + 1) * B]), _bits(one.t)), what + f": slice {k} differs from ur_scale_channels"
    if c["s"]:
        ref, bnd = R.scale_reference(bx.t.repeat(K, 1, 1), bs.t, None, dt)
        _judge("scale_channels_fanout", dtype, y, ref, bnd, what, R.REL_TOL[dt])


def _axpy(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    g = torch.Generator(device=device).manual_seed(R.zlib.crc32(c["id"].encode()))
    a, b = (torch.randn(c["rows"], c["C"], generator=g, device=device).to(dt) for _ in range(2))
    s = torch.randn(c["C"], generator=g, device=device)
    ba, bb, bs = _in(a), _in(b), _in(s)
    what = f"{c['id']} [{dtype}]"
    y, = _twice([((c["rows"], c["C"]), dt)],
                lambda y: capi.check(capi.lib.ur_axpy_channels(ba.ptr, bb.ptr, bs.ptr, y.ptr, c["rows"], c["C"], code, _stream())), what)
    ref, bnd = R.axpy_reference(ba.t, bb.t, bs.t, dt)
    _judge("axpy_channels", dtype, y, ref, bnd, what, R.REL_TOL[dt])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.AXPY_CASES, ids=[c["id"] for c in T.AXPY_CASES])
def test_axpy_channels_parity(capi, c, dtype):
    _axpy(capi, c, dtype, "cpu")


def _spade(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    g = torch.Generator(device=device).manual_seed(R.zlib.crc32(c["id"].encode()))
    rows, C, ldgb = c["rows"], c["C"], 2 * c["C"] + c.get("pad", 0)
    n = torch.randn(rows, C, generator=g, device=device).to(dt)
    gb = torch.randn(rows, ldgb, generator=g, device=device).to(dt)
    gb[:, 2 * C:] = float("nan")                                # the padding columns of the fused conv output are never read
    r = torch.randn(rows, C, generator=g, device=device).to(dt) if c.get("res") else None
    bn, bgb, br = _in(n), _in(gb), (_in(r) if r is not None else None)
    what = f"{c['id']} [{dtype}]"
    y, = _twice([((rows, C), dt)],
                lambda y: capi.check(capi.lib.ur_spade_modulate(bn.ptr, bgb.ptr, ldgb, _ptr(br), y.ptr, rows, C, code, _stream())), what)
    ref, bnd = R.spade_reference(bn.t, bgb.t, C, None if br is None else br.t, dt)
    _judge("spade_modulate", dtype, y, ref, bnd, what, R.REL_TOL[dt])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.SPADE_CASES, ids=[c["id"] for c in T.SPADE_CASES])
def test_spade_modulate_parity(capi, c, dtype):
    _spade(capi, c, dtype, "cpu")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.BIG_CASES, ids=[c["id"] for c in T.BIG_CASES])
def test_second_trip_through_the_grid_stride_loop(capi, c, dtype):
    """Just over 8192 x 256 threads' worth of work: the elements of the second trip are judged like every other (inputs and the fp64
    reference are made on the device - plain elementwise torch, shifted multiply-adds for the dwconv)."""
    assert T.big_threads(c) > T.GRID_THREADS
    {"scale": _scale, "axpy": _axpy, "spade": _spade, "dwconv": _dwconv}[c["op"]](capi, c, dtype, "cuda")


# ---- fp32 vector kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.LINEAR_CASES, ids=[c["id"] for c in T.LINEAR_CASES])
def test_linear_f32_parity(capi, c):
    x, w, b = R.linear_inputs(c)
    bx, bw, bb = _in(x), _in(w), (_in(b) if b is not None else None)
    M, N, K = c["M"], c["N"], c["K"]
    y, = _twice([((M, N), torch.float32)],
                lambda y: capi.check(capi.lib.ur_linear_f32(bx.ptr, bw.ptr, _ptr(bb), y.ptr, M, N, K, c["groups"], c["act"], _stream())), c["id"])
    ref, bnd = R.linear_reference(bx.t, bw.t, None if bb is None else bb.t, c["groups"], c["act"])
    # whole tensor: the 1e-5 tests/test_ops_gpu.py asks of this kernel; with GELU its stated fp32 tolerance, 2e-4 (the fitted GELU of
    # csrc/common.h is 2.5e-5 absolute off the erf form, on outputs of order 0.5)
    _judge("linear_f32", "fp32", y, ref, bnd, c["id"], 2e-4 if c["act"] == T.ACT_GELU else 1e-5)


@pytest.mark.parametrize("c", T.TFA_CASES, ids=[c["id"] for c in T.TFA_CASES])
def test_tfa_prompt_update_parity(capi, c):
    pooled, cond = R.tfa_inputs(c)
    bp, bc = _in(pooled), _in(cond)
    B, T_, D = c["B"], c["T"], c["D"]
    upd, = _twice([((B, T_, D), torch.float32)], lambda u: capi.check(capi.lib.ur_tfa_prompt_update(bp.ptr, bc.ptr, u.ptr, B, T_, D, _stream())), c["id"])
    ref, bnd = R.tfa_reference(bp.t, bc.t, T_, D)
    _judge("tfa_prompt_update", "fp32", upd, ref, bnd, c["id"], 1e-5)


@pytest.mark.parametrize("c", T.TFA_FANOUT_CASES, ids=[c["id"] for c in T.TFA_FANOUT_CASES])
def test_tfa_fanout_gives_the_bits_of_the_single_task_kernel(capi, c):
    lib = capi.lib
    B, K, T_, D, cpr = c["B"], c["K"], c["T"], c["D"], c["cpr"]
    pooled, cond = R.tfa_inputs(c, rows_cond=K * B if cpr else K)
    bp, bc = _in(pooled), _in(cond)
    upd, = _twice([((K * B, T_, D), torch.float32)],
                  lambda u: capi.check(lib.ur_tfa_prompt_update_fanout(bp.ptr, bc.ptr, u.ptr, B, K, T_, D, cpr, _stream())), c["id"])
    rows_cond = bc.t if cpr else bc.t.repeat_interleave(B, dim=0)                    # row n = k * B + b reads cond row n or k
    for k in range(K):
        one, ck = Buf((B, T_, D), torch.float32), _in(rows_cond[k * B:(k + 1) * B])
        capi.check(lib.ur_tfa_prompt_update(bp.ptr, ck.ptr, one.ptr, B, T_, D, _stream()))
        torch.cuda.synchronize()
        assert torch.equal(_bits(upd[k * B:(k + 1) * B]), _bits(one.t)), c["id"] + f": task {k} differs from ur_tfa_prompt_update"
    ref, bnd = R.tfa_reference(bp.t.repeat(K, 1, 1), rows_cond, T_, D)
    _judge("tfa_prompt_update_fanout", "fp32", upd, ref, bnd, c["id"], 1e-5)


@pytest.mark.parametrize("c", T.VMG_CASES, ids=[c["id"] for c in T.VMG_CASES])
def test_vec_mul_group_parity(capi, c):
    g = R.gen_of(c["id"])
    a, b = torch.randn(c["N"], c["C"], generator=g), torch.randn(c["N"], c["G"], generator=g)
    ba, bb = _in(a), _in(b)
    y, = _twice([((c["N"], c["C"]), torch.float32)],
                lambda y: capi.check(capi.lib.ur_vec_mul_group(ba.ptr, bb.ptr, y.ptr, c["N"], c["C"], c["G"], _stream())), c["id"])
    ref, bnd = R.vmg_reference(ba.t, bb.t, c["G"])
    _judge("vec_mul_group", "fp32", y, ref, bnd, c["id"])
