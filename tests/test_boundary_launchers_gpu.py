"""The "latent / image boundary" block of include/unirestore_hip.h (everything below "layout / boundary kernels" in csrc/elementwise.hip)
against fp64, element by element (-m gpu, bf16 and fp16): the layout passes, the scaled cast, the two bicubic resize kernels and their
ragged 8-bit forms, vae_sample, add_noise, ddim_step and the two tile kernels.

The cases are tests/boundary_cases.py; the fp64 references and the per-element bounds, with their derivations, are
tests/boundary_reference.py (the one statement of the bounds: this module only applies them).  tests/test_boundary_reference_cpu.py
holds the host-side half: property coverage, the tie-zone condition, the CPU emulation, the mutations and the refusals.

Every call goes through the raw C ABI (capi.lib) and, for every case and dtype:
  * every output lives inside a NaN-filled (8-bit and int32: pattern-filled) allocation with guard elements before and after it, which
    must come back bit-unchanged; every input sits inside a larger filled allocation too, and carries NaN wherever the kernel has no
    business reading (padding columns, outside the crop window, the eps of a tile that must be skipped);
  * the case runs twice into fresh buffers: the results must be bit-identical;
  * every output element is checked against its bound, the whole tensor against the rel-L2 tolerance; no NaN may be left anywhere that
    should have been written; the exact-bit assertions of boundary_reference apply (padding zeros, rounding ties, 16-bit copy ==
    rounding of the stored fp32 state, ragged == tensor entry point, untouched slots of a skipped tile, untouched bytes behind H W C).
The module sets no environment variables and starts no processes.  It prints the worst |y - ref| / bound per (kernel, dtype) at its end.
"""
import pytest
import torch

import boundary_cases as T
import boundary_reference as R

pytestmark = pytest.mark.gpu
DTYPES = R.DTYPES
GUARD = 64                      # guard elements before and after every buffer
WORST = {}                      # (kernel, dtype) -> largest |y - ref| / bound seen
TIES = {}                       # (kernel, dtype) -> [codes that differ from the reference inside the tie zone, codes judged]
SA, SB, CX, CE = 0.8, 0.6, 1.0532, -0.2871
PATTERN = {torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A}
F32 = torch.float32


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    yield c
    if WORST:
        print("\nlargest |y - ref| / bound per kernel:")
        for (name, dt), r in sorted(WORST.items()):
            print(f"  {name:32s} {dt}: {r:.3f}")
        for (name, dt), (d, n) in sorted(TIES.items()):
            print(f"  {name:32s} {dt}: {d} of {n} codes differ from round_half_even(255 ref), all inside the tie zone")


def _note(kernel, dtype, r):
    WORST[(kernel, dtype)] = max(WORST.get((kernel, dtype), 0.0), r)


def _bits(t):
    return t if not t.is_floating_point() else t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class Buf:
    """`shape` elements of `dtype` inside a NaN-filled (integer types: pattern-filled) allocation with GUARD elements on either side."""

    def __init__(self, shape, dtype, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.pat = PATTERN.get(dtype, float("nan"))
        self.raw = torch.full((n + 2 * GUARD,), self.pat, dtype=dtype, device="cuda")
        self.t = self.raw[GUARD:GUARD + n].view(*shape)
        if fill is not None:
            self.t.copy_(fill)
        self.fill_bits = _bits(torch.full((1,), self.pat, dtype=dtype, device="cuda"))[0]

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_ok(self):
        b = _bits(self.raw)
        return bool((b[:GUARD] == self.fill_bits).all()) and bool((b[-GUARD:] == self.fill_bits).all())


def _in(t, dt=None):
    """An input tensor (any device) inside a larger filled allocation on the GPU."""
    t = t if dt is None else t.to(dt)
    return Buf(tuple(t.shape), t.dtype, fill=t.cuda())


def _code(capi, dt):
    return capi.UR_DT_F16 if dt == torch.float16 else capi.UR_DT_BF16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _twice(shapes, launch, what, init=None):
    """Run `launch(*buffers)` twice into fresh filled buffers of `shapes` = [(shape, dtype)]; `init[i]` (optional) is copied into buffer i
    first (a kernel that works in place).  Guards intact, bit-identical results.  Returns the tensors of the first run."""
    runs = []
    for _ in range(2):
        bufs = [Buf(*s, fill=None if init is None else init[i]) for i, s in enumerate(shapes)]
        launch(*bufs)
        torch.cuda.synchronize()
        for i, b in enumerate(bufs):
            assert b.guards_ok(), f"{what}: write outside buffer {i}"
        runs.append(bufs)
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(_bits(a.t), _bits(b.t)), f"{what}: buffer {i} not bit-identical between two runs"
    return [b.t for b in runs[0]]


def _judge(kernel, dtype, y, ref, bnd, what, rel_tol=None):
    assert bool(torch.isfinite(y).all()), what + ": output not finite (a NaN was read, or an element was never written)"
    rel = R.rel_l2(y, ref)
    try:
        r = R.compare(y.double(), ref, bnd, what)
    finally:
        print(f"{what}: worst |y - ref| / bound {R.worst(y, ref, bnd):.3f}, rel-L2 {rel:.3e}")
    _note(kernel, dtype, r)
    if rel_tol is not None:
        assert rel < rel_tol, what


def _zero_bits(t, what):
    assert bool((_bits(t) == 0).all()), what + ": padding channels must be zero bits"


def _subset(c, total):
    """None for a small case (every element is judged); for a grid-stride case of a bicubic kernel the work items of the second trip
    plus an equal-sized strided sample of the first."""
    if "op" not in c:
        return None
    second = torch.arange(T.GRID_THREADS, total, device="cuda")
    return torch.cat([torch.arange(0, T.GRID_THREADS, T.GRID_THREADS // second.numel(), device="cuda")[:second.numel()], second])


# ---- layout passes and the scaled cast ---------------------------------------------------------------------------------------------------
def _layout_in(capi, c, dtype, device):
    dt, lib, code = DTYPES[dtype], capi.lib, _code(capi, DTYPES[dtype])
    N, C, H, W, Cp = c["N"], c["C"], c["H"], c["W"], c["Cpad"]
    bx = _in(R.layout_in_inputs(c, device))
    for fn, name, mul, add in ((lib.ur_nchw_f32_to_nhwc, "nchw_f32_to_nhwc", 1.0, 0.0), (lib.ur_image_to_nhwc, "image_to_nhwc", 2.0, -1.0)):
        what = f"{c['id']} {name} [{dtype}]"
        y, = _twice([((N, H, W, Cp), dt)], lambda y: capi.check(fn(bx.ptr, y.ptr, N, C, H, W, Cp, code, _stream())), what)
        _zero_bits(y[..., C:], what)
        ref, bnd = R.layout_in_reference(bx.t, mul, add, dt)
        _judge(name, dtype, y[..., :C], ref, bnd, what, R.REL_TOL[dt])
        if (mul, add) == (1.0, 0.0):
            assert torch.equal(_bits(y[..., :C]), _bits(bx.t.permute(0, 2, 3, 1).to(dt))), what + ": not the 16-bit rounding of x"


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.LAYOUT_IN_CASES, ids=[c["id"] for c in T.LAYOUT_IN_CASES])
def test_layout_in_parity(capi, c, dtype):
    _layout_in(capi, c, dtype, "cpu")


def _layout_out(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    N, C, H, W, ld = c["N"], c["C"], c["H"], c["W"], c["ld"]
    bx = _in(R.layout_out_inputs(c, dt, device))
    what = f"{c['id']} [{dtype}]"
    out, = _twice([((N, C, H, W), F32)], lambda o: capi.check(capi.lib.ur_nhwc_to_nchw_f32(bx.ptr, c["f32"], o.ptr, N, C, H, W, ld, c["mul"], c["add"], code,
                                                                                          _stream())), what)
    ref, bnd = R.layout_out_reference(bx.t, C, c["mul"], c["add"])
    _judge("nhwc_to_nchw_f32", dtype, out, ref, bnd, what, R.REL_TOL_F32)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.LAYOUT_OUT_CASES, ids=[c["id"] for c in T.LAYOUT_OUT_CASES])
def test_layout_out_parity(capi, c, dtype):
    _layout_out(capi, c, dtype, "cpu")


def _cast(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    M, C, Cp, ld = c["M"], c["C"], c["Cpad"], c["ld"]
    bx = _in(R.cast_inputs(c, dt, device))
    what = f"{c['id']} [{dtype}]"
    y, = _twice([((M, Cp), dt)], lambda y: capi.check(capi.lib.ur_f32_to_bf16_scaled(bx.ptr, ld, y.ptr, M, C, Cp, c["mul"], code, _stream())), what)
    _zero_bits(y[:, C:], what)
    ref, bnd = R.cast_reference(bx.t, C, c["mul"], dt)
    if c["kind"] == "ties":                                   # mul = 1: the bits of torch's cast - round to nearest even, +-inf beyond +-65504 in fp16
        want = bx.t[:, :C].to(dt)
        assert torch.equal(_bits(y[:, :C]), _bits(want)), what + ": differs from x.to(dtype) at a tie, an overflow or a subnormal"
        fin = torch.isfinite(want)
        _judge("f32_to_bf16_scaled", dtype, y[:, :C][fin], ref[fin], bnd[fin], what)
    else:
        _judge("f32_to_bf16_scaled", dtype, y[:, :C], ref, bnd, what, R.REL_TOL[dt])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.CAST_CASES, ids=[c["id"] for c in T.CAST_CASES])
def test_f32_to_16_scaled_parity(capi, c, dtype):
    _cast(capi, c, dtype, "cpu")


# ---- bicubic: fp32-tensor entry points ------------------------------------------------------------------------------------------------------
def _resize_in(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    N, C, Cp, OH, OW = c["N"], c["C"], c["Cpad"], c["RH"] + c["PH"], c["RW"] + c["PW"]
    bi = _in(R.resize_in_inputs(c, device))
    what = f"{c['id']} [{dtype}]"
    y, = _twice([((N, OH, OW, Cp), dt)], lambda y: capi.check(capi.lib.ur_image_resize_pad_nhwc(
        bi.ptr, y.ptr, N, C, c["H"], c["W"], c["RH"], c["RW"], c["PH"], c["PW"], Cp, c["mul"], c["add"], code, _stream())), what)
    _zero_bits(y[..., C:], what)
    sub = _subset(c, N * OH * OW)
    ref, bnd = R.resize_in_reference(bi.t, c, dt, sub)
    yy = y.view(-1, Cp)[:, :C] if sub is None else y.view(-1, Cp)[sub, :C]
    _judge("image_resize_pad_nhwc", dtype, yy, ref, bnd, what, R.REL_TOL[dt])
    assert sub is not None or bool(torch.isfinite(y).all())


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.RESIZE_IN_CASES, ids=[c["id"] for c in T.RESIZE_IN_CASES])
def test_image_resize_pad_parity(capi, c, dtype):
    _resize_in(capi, c, dtype, "cpu")


def _judge_codes(kernel, dtype, code, Rf, what, per_case=True):
    """code fp64 [P,C] as stored (NaN where the kernel stored NaN).  per_case = False: one image of a ragged canvas - the 3 % condition is
    on the canvas (asserted by the CPU module); in a 27-element image a single element is 3.7 %."""
    nf = Rf["nonfinite"]
    nf = torch.zeros_like(code, dtype=torch.bool) if nf is None else nf
    share = R.check_codes(code, Rf["ref"], Rf["E"], what, nf)
    want, _ = R.quant_reference(Rf["ref"], Rf["E"])
    d = int(((code != want) & ~nf).sum())
    print(f"{what}: {d} of {code.numel()} codes differ inside the tie zone ({100 * share:.2f} % of the elements)")
    t = TIES.setdefault((kernel, dtype), [0, 0])
    t[0], t[1] = t[0] + d, t[1] + code.numel()
    assert not per_case or share <= R.TIE_SHARE_MAX, what


def _resize_out(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    N, C, OH, OW = c["N"], c["C"], c["OH"], c["OW"]
    bx = _in(R.resize_out_inputs(c, dt, device))
    what = f"{c['id']} [{dtype}]"
    out, = _twice([((N, C, OH, OW), F32)], lambda o: capi.check(capi.lib.ur_image_unpad_resize_nchw(
        bx.ptr, c["f32"], o.ptr, N, C, c["XH"], c["XW"], c["ld"], c["CH"], c["CW"], OH, OW, c["mul"], c["add"], c["quantize"], code, _stream())), what)
    sub = _subset(c, N * OH * OW)
    Rf = R.resize_out_reference(bx.t, c, sub)
    oc = out.permute(0, 2, 3, 1).reshape(-1, C)
    oc = oc if sub is None else oc[sub]
    nf = Rf["nonfinite"]
    live = torch.ones_like(oc, dtype=torch.bool) if nf is None else ~nf
    assert c["special"] == bool((~live).any())
    if c["quantize"]:
        codes = torch.round(oc.double() * 255)
        _judge_codes("image_unpad_resize_nchw q", dtype, codes, Rf, what)
        back = (codes.cpu().float() / 255).cuda()                       # the stored value is the correctly rounded code / 255
        assert torch.equal(_bits(oc[live]), _bits(back[live])), what + ": an output is not code / 255"
        for i, (k, _) in enumerate(R.planted_ties(c)):
            assert float(codes[i * 1, 0]) == (k if k % 2 == 0 else k + 1), what + f": the exact tie {k}.5 did not round to even"
    else:
        assert torch.equal(torch.isfinite(oc), live), what + ": non-finite outputs exactly where the taps touch a non-finite sample"
        _judge("image_unpad_resize_nchw", dtype, oc[live], Rf["ref"][live], Rf["E"][live], what)
        assert c["special"] or float((oc.double() - Rf["ref"]).abs().max()) < R.BICUBIC_F32_ABS, what


_RO = T.RESIZE_OUT_CASES + T.RESIZE_OUT_SPECIAL


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", _RO, ids=[c["id"] for c in _RO])
def test_image_unpad_resize_parity(capi, c, dtype):
    _resize_out(capi, c, dtype, "cpu")


# ---- bicubic: ragged 8-bit entry points ------------------------------------------------------------------------------------------------------
def _local(sub, n, per_image):
    """The work items of image n out of a global subset (None: all of them)."""
    if sub is None:
        return None
    s = sub[(sub >= n * per_image) & (sub < (n + 1) * per_image)] - n * per_image
    return s


def _ingest(capi, cv, dtype, device):
    dt, lib, code = DTYPES[dtype], capi.lib, _code(capi, DTYPES[dtype])
    N, CH, CW = len(cv["geom"]), cv["CH"], cv["CW"]
    src, slot = R.ragged_inputs(cv, device)
    bs, bg = _in(src), _in(torch.tensor(cv["geom"], dtype=torch.int32))
    what = f"{cv['id']} ingest [{dtype}]"
    launch = lambda y, g=bg: capi.check(lib.ur_image_u8_ingest(bs.ptr, slot, g.ptr, y.ptr, N, CH, CW, 8, 2.0, -1.0, code, _stream()))
    y, = _twice([((N, CH, CW, 8), dt)], launch, what)
    _zero_bits(y[..., 3:], what)
    sub = _subset(cv, N * CH * CW)
    for n, (H, W, _, _) in enumerate(cv["geom"]):
        ci = R.ingest_case(cv, n)
        img = R.ragged_image(bs.t, n, H, W)
        s = _local(sub, n, CH * CW)
        if s is not None and s.numel() == 0:
            continue
        ref, bnd = R.resize_in_reference(img / 255.0, ci, dt, s, pre_u=1)
        yn = y[n].reshape(-1, 8)[:, :3] if s is None else y[n].reshape(-1, 8)[s, :3]
        _judge("image_u8_ingest", dtype, yn, ref, bnd, f"{what} image {n}", R.REL_TOL[dt])
        one, f = Buf((1, CH, CW, 8), dt), _in((img.cpu().float() / 255).contiguous())                  # a true fp32 division, made on the host
        capi.check(lib.ur_image_resize_pad_nhwc(f.ptr, one.ptr, 1, 3, H, W, ci["RH"], ci["RW"], ci["PH"], ci["PW"], 8, 2.0, -1.0, code, _stream()))
        torch.cuda.synchronize()
        assert torch.equal(_bits(one.t[0]), _bits(y[n])), f"{what} image {n}: not the bits of ur_image_resize_pad_nhwc"
    return y, bs, slot


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("cv", T.RAGGED_CANVASES, ids=[c["id"] for c in T.RAGGED_CANVASES])
def test_u8_ingest_parity_and_bad_rows(capi, cv, dtype):
    dt, lib, code = DTYPES[dtype], capi.lib, _code(capi, DTYPES[dtype])
    good, bs, slot = _ingest(capi, cv, dtype, "cpu")
    N, CH, CW = len(cv["geom"]), cv["CH"], cv["CW"]
    for i, clause in enumerate(T.BAD_CLAUSES):
        r = i % N
        geom = list(cv["geom"])
        geom[r] = T.bad_row(clause, geom[r], CH, CW)
        bg = _in(torch.tensor(geom, dtype=torch.int32))
        what = f"{cv['id']} ingest, row {r} with {clause} [{dtype}]"
        y, = _twice([((N, CH, CW, 8), dt)], lambda y: capi.check(lib.ur_image_u8_ingest(bs.ptr, slot, bg.ptr, y.ptr, N, CH, CW, 8, 2.0, -1.0, code, _stream())), what)
        assert bool((_bits(y[r]) == 0).all()), what + ": a bad table row must give an all-zero image"
        keep = [n for n in range(N) if n != r]
        assert torch.equal(_bits(y[keep]), _bits(good[keep])), what + ": the neighbours of a bad row changed"


def _egress(capi, cv, dtype, f32in, device, nan_image):
    dt, lib, code = DTYPES[dtype], capi.lib, _code(capi, DTYPES[dtype])
    N, CH, CW = len(cv["geom"]), cv["CH"], cv["CW"]
    slot = 3 * CH * CW + cv["slack"]
    bx, bg = _in(R.egress_inputs(cv, dt, f32in, device, nan_image)), _in(torch.tensor(cv["geom"], dtype=torch.int32))
    what = f"{cv['id']} egress f32={f32in} [{dtype}]"
    zero = torch.zeros(N, dtype=torch.int32)
    launch = lambda d, fl, g=bg: capi.check(lib.ur_image_u8_egress(bx.ptr, f32in, d.ptr, slot, g.ptr, fl.ptr, N, 3, CH, CW, 8, 0.5, 0.5, code, _stream()))
    dst, flags = _twice([((N, slot), torch.uint8), ((N,), torch.int32)], launch, what, init=[None, zero])
    assert flags.tolist() == [1 if n == nan_image else 0 for n in range(N)], what + f": nonfinite flags {flags.tolist()}"
    sub = _subset(cv, N * CH * CW)
    for n, (H, W, _, _) in enumerate(cv["geom"]):
        ce = R.egress_case(cv, n)
        assert bool((dst[n, H * W * 3:] == PATTERN[torch.uint8]).all()), f"{what} image {n}: bytes behind H W C were written"
        got = dst[n, :H * W * 3].view(H * W, 3).double()
        s = _local(sub, n, CH * CW)
        if s is not None:                                                  # canvas work items -> output pixels of this image
            oy, ox = s // CW, s % CW
            s = (oy * W + ox)[(oy < H) & (ox < W)]
            if s.numel() == 0:
                continue
        Rf = R.resize_out_reference(bx.t[n:n + 1], ce, s)
        g = got if s is None else got[s]
        if Rf["nonfinite"] is not None and bool(Rf["nonfinite"].any()):
            assert n == nan_image and bool((g[Rf["nonfinite"]] == 0).all()), f"{what} image {n}: a non-finite sample must store code 0"
            g = torch.where(Rf["nonfinite"], torch.full_like(g, float("nan")), g)
        else:
            assert n != nan_image or s is not None
        _judge_codes("image_u8_egress", dtype, g, Rf, f"{what} image {n}", per_case="op" in cv)
        one = Buf((1, 3, H, W), F32)
        capi.check(lib.ur_image_unpad_resize_nchw(bx.t[n:n + 1].data_ptr(), f32in, one.ptr, 1, 3, CH, CW, 8, ce["CH"], ce["CW"], H, W, 0.5, 0.5, 1, code,
                                                  _stream()))
        torch.cuda.synchronize()
        want = torch.round(one.t[0].permute(1, 2, 0).reshape(-1, 3).double() * 255).nan_to_num(nan=0.0)
        assert torch.equal(got, want), f"{what} image {n}: not the codes of ur_image_unpad_resize_nchw(quantize=1)"
    return dst, bx, slot


@pytest.mark.parametrize("f32in", [0, 1])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("cv", T.RAGGED_CANVASES, ids=[c["id"] for c in T.RAGGED_CANVASES])
def test_u8_egress_parity_and_bad_rows(capi, cv, dtype, f32in):
    dt, lib, code = DTYPES[dtype], capi.lib, _code(capi, DTYPES[dtype])
    good, bx, slot = _egress(capi, cv, dtype, f32in, "cpu", nan_image=2)
    N, CH, CW = len(cv["geom"]), cv["CH"], cv["CW"]
    zero = torch.zeros(N, dtype=torch.int32)
    for i, clause in enumerate(T.BAD_CLAUSES):
        r = (i + 1) % N
        geom = list(cv["geom"])
        geom[r] = T.bad_row(clause, geom[r], CH, CW)
        bg = _in(torch.tensor(geom, dtype=torch.int32))
        what = f"{cv['id']} egress f32={f32in}, row {r} with {clause} [{dtype}]"
        launch = lambda d, fl: capi.check(lib.ur_image_u8_egress(bx.ptr, f32in, d.ptr, slot, bg.ptr, fl.ptr, N, 3, CH, CW, 8, 0.5, 0.5, code, _stream()))
        dst, flags = _twice([((N, slot), torch.uint8), ((N,), torch.int32)], launch, what, init=[None, zero])
        assert flags.tolist() == [2 if n == r else (1 if n == 2 else 0) for n in range(N)], what + f": nonfinite flags {flags.tolist()}"
        assert bool((dst[r] == PATTERN[torch.uint8]).all()), what + ": a bad table row must write no byte of its slot"
        keep = [n for n in range(N) if n != r]
        assert torch.equal(dst[keep], good[keep]), what + ": the neighbours of a bad row changed"


# ---- vae_sample, add_noise, ddim_step ----------------------------------------------------------------------------------------------------------
def _state_checks(kernel, dtype, z, z16, ref, E, Cl, what):
    dt = DTYPES[dtype]
    _zero_bits(z[:, Cl:], what + " fp32 state")
    _zero_bits(z16[:, Cl:], what + " 16-bit copy")
    _judge(kernel + " fp32", dtype, z[:, :Cl], ref, E, what + " fp32 state", R.REL_TOL_F32)
    _judge(kernel + " 16-bit", dtype, z16[:, :Cl], ref, R.out_bound(ref, E, dt), what + " 16-bit copy", R.REL_TOL[dt])
    assert torch.equal(_bits(z16), _bits(z.to(dt))), what + ": the 16-bit copy is not the rounding of the stored fp32 state"


def _vae(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    N, HW, Cl, Cp = c["N"], c["HW"], c["Clat"], c["Cpad"]
    mom, noise = R.vae_inputs(c, device)
    bm, bn = _in(mom), _in(noise)
    what = f"{c['id']} [{dtype}]"
    z, z16 = _twice([((N * HW, Cp), F32), ((N * HW, Cp), dt)], lambda z, z16: capi.check(capi.lib.ur_vae_sample(
        bm.ptr, c["ld"], bn.ptr, z.ptr, z16.ptr, N, HW, Cl, Cp, T.SCALING, code, _stream())), what)
    ref, E = R.vae_reference(bm.t, bn.t, c, T.SCALING)
    _state_checks("vae_sample", dtype, z, z16, ref, E, Cl, what)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.VAE_CASES, ids=[c["id"] for c in T.VAE_CASES])
def test_vae_sample_parity(capi, c, dtype):
    _vae(capi, c, dtype, "cpu")


def _noise(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    N, HW, Cl, Cp = c["N"], c["HW"], c["Clat"], c["Cpad"]
    z0, noise = R.state_inputs(c, None, True, device)
    b0, bn = _in(z0), _in(noise)
    what = f"{c['id']} [{dtype}]"
    z, z16 = _twice([((N * HW, Cp), F32), ((N * HW, Cp), dt)], lambda z, z16: capi.check(capi.lib.ur_add_noise(
        b0.ptr, bn.ptr, z.ptr, z16.ptr, N, HW, Cl, Cp, SA, SB, code, _stream())), what)
    ref, E = R.axpby_reference(b0.t[:, :Cl], bn.t.permute(0, 2, 1).reshape(-1, Cl), SA, SB)
    _state_checks("add_noise", dtype, z, z16, ref, E, Cl, what)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.NOISE_CASES, ids=[c["id"] for c in T.NOISE_CASES])
def test_add_noise_parity(capi, c, dtype):
    _noise(capi, c, dtype, "cpu")


def _ddim(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    M, Cl, Cp, le = c["N"] * c["HW"], c["Clat"], c["Cpad"], c["ld_eps"]
    zt, eps = R.state_inputs(c, le, False, device)                      # the padding channels of the incoming state are NaN
    be = _in(eps)
    what = f"{c['id']} [{dtype}]"
    z, z16 = _twice([((M, Cp), F32), ((M, Cp), dt)], lambda z, z16: capi.check(capi.lib.ur_ddim_step(
        z.ptr, be.ptr, le, z16.ptr, M, Cl, Cp, CX, CE, code, _stream())), what, init=[zt, None])
    ref, E = R.axpby_reference(zt[:, :Cl].cuda(), be.t[:, :Cl], CX, CE)
    _state_checks("ddim_step", dtype, z, z16, ref, E, Cl, what)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.DDIM_CASES, ids=[c["id"] for c in T.DDIM_CASES])
def test_ddim_step_parity(capi, c, dtype):
    _ddim(capi, c, dtype, "cpu")


# ---- tiles ---------------------------------------------------------------------------------------------------------------------------------
def _gather(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    N, LH, LW, th, tw, Cp, nt = c["N"], c["LH"], c["LW"], c["th"], c["tw"], c["Cpad"], len(c["origins"])
    z, _, _, org = R.tile_inputs(c, device)
    bz, bo = _in(z), _in(org)
    what = f"{c['id']} gather [{dtype}]"
    tiles, = _twice([((N * nt, th, tw, Cp), dt)], lambda t: capi.check(capi.lib.ur_latent_tiles_gather(
        bz.ptr, t.ptr, N, LH, LW, Cp, nt, th, tw, bo.ptr, code, _stream())), what)
    assert torch.equal(_bits(tiles), _bits(R.gather_reference(bz.t, c, dt))), what + ": gather is exact, and a skipped tile is all-zero"
    _note("latent_tiles_gather", dtype, 0.0)


def _blend(capi, c, dtype, device):
    dt, code = DTYPES[dtype], _code(capi, DTYPES[dtype])
    N, LH, LW, th, tw, Cl, Cp, le, nt = c["N"], c["LH"], c["LW"], c["th"], c["tw"], c["Clat"], c["Cpad"], c["ld_eps"], len(c["origins"])
    z, eps, wn, org = R.tile_inputs(c, device)
    zin = z.clone()
    zin[..., Cl:] = float("nan")                                            # whatever the padding channels hold, they leave as zero
    be, bw, bo = _in(eps), _in(wn), _in(org)
    what = f"{c['id']} blend [{dtype}]"
    zt, tiles = _twice([((N, LH, LW, Cp), F32), ((N * nt, th, tw, Cp), dt)], lambda zt, t: capi.check(capi.lib.ur_latent_tiles_blend_ddim(
        zt.ptr, be.ptr, le, t.ptr, bw.ptr, N, LH, LW, Cl, Cp, nt, th, tw, bo.ptr, CX, CE, code, _stream())), what, init=[zin, None])
    ref, E, _ = R.blend_reference(z.cuda(), be.t, bw.t, c, CX, CE)
    _zero_bits(zt[..., Cl:], what)
    _judge("latent_tiles_blend_ddim", dtype, zt[..., :Cl], ref, E, what)
    probe, whole = R.tile_probe(c), zt[..., :Cl].clone()
    if probe is not None:                     # the probe is inside its bound, but 2^24 u of one term off by design: not part of the rel-L2
        whole[0, probe[0], probe[1], 0] = ref[0, probe[0], probe[1], 0]
    assert R.rel_l2(whole, ref) < R.REL_TOL_F32, what
    slots = tiles.view(N, nt, th, tw, Cp)
    nan16 = _bits(torch.full((1,), float("nan"), dtype=dt, device="cuda"))[0]
    for k, (y0, x0) in enumerate(c["origins"]):
        if T.tile_valid(c, k):
            assert torch.equal(_bits(slots[:, k]), _bits(zt[:, y0:y0 + th, x0:x0 + tw].to(dt))), what + f": slot {k} is not the rounding of the new state"
        else:
            assert bool((_bits(slots[:, k]) == nan16).all()), what + f": the slots of the skipped tile {k} were written"
    if probe is not None:
        assert float(zt[0, probe[0], probe[1], 0]) == 0.0, what + ": the covering tiles were not summed in ascending k"


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.TILE_CASES, ids=[c["id"] for c in T.TILE_CASES])
def test_latent_tiles_parity(capi, c, dtype):
    _gather(capi, c, dtype, "cpu")
    _blend(capi, c, dtype, "cpu")


# ---- the second trip through the grid-stride loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.BIG_CASES, ids=[c["id"] for c in T.BIG_CASES])
def test_second_trip_through_the_grid_stride_loop(capi, c, dtype):
    """Just over 8192 x 256 work items: the elements of the second trip are judged like every other (inputs and the fp64 reference are
    made on the device; the bicubic kernels on the second trip plus an equal-sized strided sample of the first)."""
    assert T.big_threads(c) > T.GRID_THREADS
    op = c["op"]
    if op == "u8_ingest":
        _ingest(capi, c, dtype, "cuda")
    elif op == "u8_egress":
        _egress(capi, c, dtype, 0, "cuda", None)
    else:
        {"layout_in": _layout_in, "layout_out": _layout_out, "cast": _cast, "resize_in": _resize_in, "resize_out": _resize_out, "vae": _vae,
         "noise": _noise, "ddim": _ddim, "gather": _gather, "blend": _blend}[op](capi, c, dtype, "cuda")
