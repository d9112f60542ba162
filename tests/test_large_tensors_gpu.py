"""The kernels on 2 - 4 GiB tensors: far-end offsets and the stated size limits (-m gpu, bf16; cases in tests/large_cases.py).

Every launch goes through the raw C ABI on PERIODIC inputs (tests/large_harness.py): unit i (an image, a row, or - for the
weight-dominated Linear - a weight row) is a copy of unit i mod P, built from the P distinct units the existing seeded generators
make (tests/test_conv_launchers_gpu.py, tests/norm_reference.py), and tiled on the device by chunked copies.  The fp64 reference
and the per-element bound are the existing ones (tests/conv_reference.py, tests/norm_reference.py), computed for the P units only.
No tolerance is introduced here.  For every case:
  * the planned launcher is asserted before the launch (conv cases);
  * every input sits in a NaN-guarded allocation, every output in a NaN-filled one with guard rows before and after it (and padding
    columns past the output width): the guards must come back bit-unchanged;
  * EVERY output element is checked on the device, in chunks, against reference unit i mod P within its bound;
  * the first unit, the last unit and the units straddling byte 2^31 of the large tensors are also copied to the host and
    compared there; no whole tensor is ever copied to the host;
  * a second launch into a fresh buffer must give the same bits (compared on the device, in chunks).
A test skips only when the device has less free memory than the case needs, and prints both numbers.
"""
import ctypes
import time

import pytest
import torch

import conv_launcher_cases as LC
import conv_reference as CR
import boundary_reference as BR
import large_cases as T
import large_harness as H
import norm_reference as NR
import test_conv_launchers_gpu as CL

pytestmark = pytest.mark.gpu
DT = torch.bfloat16
GUARD_ROWS = 3                  # rows of y before and after the output that must stay untouched
GUARD = 64                      # guard elements around 1-D buffers (a multiple of 16 bytes in every type)
GiB = 1 << 30
NAN_BITS = {torch.bfloat16: 0x7FC0, torch.float16: 0x7E00, torch.float32: 0x7FC00000}
INT_OF = {2: torch.int16, 4: torch.int32}


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    return c


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    import gc
    try:                                  # a device fault is sticky: nothing more is launched on the card, the module ends here
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"device error after a large-tensor case, stopping: {err}", returncode=3)
    gc.collect()
    torch.cuda.empty_cache()


def _need(nbytes, what):
    """Skip (printing the numbers) only when the device cannot hold the case."""
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    need = int(nbytes * 1.05) + GiB                      # + the comparison chunks
    print(f"{what}: needs {need / GiB:.1f} GiB of device memory, {free / GiB:.1f} GiB free of {total / GiB:.1f}")
    if free < need:
        pytest.skip(f"{what}: {free / GiB:.1f} GiB free, {need / GiB:.1f} GiB needed")


def _bits(t):
    return t.view(INT_OF[t.element_size()])


def _signed(v, nbytes):
    return v - (1 << (8 * nbytes)) if v >= 1 << (8 * nbytes - 1) else v


def _nan_value(dtype):
    return _signed(NAN_BITS[dtype], torch.empty(0, dtype=dtype).element_size())


def _fill_nan(t):
    """NaN into a flat tensor, in pieces of at most 2^28 elements."""
    for i in range(0, t.numel(), H.COPY_ELEMS):
        t[i:i + H.COPY_ELEMS].fill_(float("nan"))
    return t


class Big:
    """`rows` x `ld` elements of `dtype` inside a flat allocation with `grows` guard rows (NaN) before and after; fill: 'nan' (an
    output: everything NaN) or None (an input: only the guards are NaN, the body is written by the caller)."""

    def __init__(self, rows, ld, dtype, fill=None, grows=None):
        g = (grows if grows is not None else -(-GUARD // ld)) * ld
        self.raw = torch.empty(rows * ld + 2 * g, dtype=dtype, device="cuda")
        self.g, self.rows, self.ld, self.dtype = g, rows, ld, dtype
        if fill == "nan":
            _fill_nan(self.raw)
        else:
            self.raw[:g].fill_(float("nan"))
            self.raw[g + rows * ld:].fill_(float("nan"))
        self.t = self.raw[g:g + rows * ld].view(rows, ld)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_ok(self, what, width=None):
        b, nan = _bits(self.raw), _nan_value(self.dtype)
        H.check_fill(b[:self.g], nan, what + " guard before")
        H.check_fill(b[self.g + self.rows * self.ld:], nan, what + " guard after")
        if width is not None and width < self.ld:
            H.check_fill(_bits(self.t)[:, width:], nan, what + " padding columns")


def _periodic(src, U):
    """A guarded device tensor [U, unit] holding src [P, unit] repeated."""
    src = src.cuda()
    b = Big(U, src.shape[1], src.dtype)
    H.tile_periodic(b.t, src)
    return b


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(cid, what, worst, host, nbytes, t0):
    print(f"{cid}: {what}; largest |err| / bound {worst:.3f} (device, every element), {host:.3f} (host, spot units); "
          f"tensors {', '.join(f'{k} {v / GiB:.2f} GiB' for k, v in nbytes.items())}; {time.time() - t0:.1f} s")


# ---- conv / GEMM ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ws_full():
    return torch.empty(LC.WS_FULL // 4, dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("c", T.CONV_CASES, ids=[c["id"] for c in T.CONV_CASES])
def test_conv_large(capi, ws_full, c):
    t0 = time.time()
    U, P = T.units(c)
    pc = T.period_case(c)
    ydt = torch.float32 if c["out_f32"] else DT
    esz = 4 if c["out_f32"] else 2
    e = T.elems(c)
    M, co, names = e["M"], LC.cout_out(c), capi.launcher_names()
    OHW = c["OH"] * c["OW"]

    # the plan: launcher, split, GroupNorm pass (decides ldy), partial planes
    d = capi.ConvDesc()
    LC.fill(d, c, dict(LC.placeholders(c), workspace=LC.P), LC.WS_FULL)
    d.dtype = capi.UR_DT_BF16
    info = capi.plan_launch(d)
    assert names[info.launcher] == c["launcher"], (c["id"], names[info.launcher])
    gn_pass = bool(info.gn_pass)
    geo = LC.geometry(c, gn_pass)
    ldy = geo["ldy"]
    LC.fill(d, c, dict(LC.placeholders(c), workspace=LC.P), LC.WS_FULL, gn_pass)
    plan = capi.ConvPlan()
    capi.check(capi.lib.ur_conv2d_plan(d, plan))
    if c["id"] in T.SPLITK_CASES:
        assert info.splitk > 1 and info.reduce >= 0, (c["id"], info.splitk)
    gn_elems = c["N"] * plan.gn_parts * co * 2 if c["gn"] else 0
    _need((e["x"] + e["x2"] + e["r"] + e["w"]) * 2 + 2 * (M + 2 * GUARD_ROWS) * ldy * esz + 2 * gn_elems * 4, c["id"])

    # one period of inputs and its fp64 reference, by the generators and the bound of the small-shape matrix
    t, xs, wl = CL._inputs(pc, DT)
    ref, bnd, K = CL._reference(pc, t, xs, wl, ydt)                 # [1][rows of P units][co], fp64, on the device
    if c["unit"] == "wrow":                                          # units are output columns: [P][1][M]
        ref, bnd = (v[0].t().contiguous().unsqueeze(1) for v in (ref, bnd))
    else:
        ref, bnd = (v[0].reshape(P, -1, co) for v in (ref, bnd))
    del xs, wl

    # the launch's tensors, tiled on the device
    ptrs, keep = {}, []
    if c["unit"] == "wrow":
        ptrs["x"] = _periodic(t["x"].reshape(1, -1), 1)
        ptrs["w"] = _periodic(t["w"], U)
        ptrs["bias"] = _periodic(t["bias"].reshape(P, 1), U)
    else:
        ptrs["x"] = _periodic(t["x"].reshape(P, -1), U)
        ptrs["w"] = _periodic(t["w"].reshape(1, -1), 1)
        if c["C2"]:
            ptrs["x2"] = _periodic(t["x2"].reshape(P, -1), U)
        if c["bias"]:
            ptrs["bias"] = _periodic(t["bias"], U) if c["bias_img"] else _periodic(t["bias"].reshape(1, -1), 1)
        if c["res"]:
            ptrs["residual"] = _periodic(t["residual"].reshape(P, -1), U)
        if c["gn_ab"]:
            ptrs["gn_ab"] = _periodic(t["gn_ab"].reshape(P, -1), U)
    ptrs["workspace"] = ws_full
    del t

    def launch():
        y = Big(M, ldy, ydt, fill="nan", grows=GUARD_ROWS)
        gp = Big(c["N"] * plan.gn_parts, co * 2, torch.float32, fill="nan") if c["gn"] else None
        dd = capi.ConvDesc()
        p = {k: (v.ptr if isinstance(v, Big) else v.data_ptr()) for k, v in ptrs.items()}
        p["y"] = y.ptr
        if gp is not None:
            p["gn_part"] = gp.ptr
        LC.fill(dd, c, p, LC.WS_FULL, gn_pass)
        dd.dtype = capi.UR_DT_BF16
        capi.check(capi.lib.ur_conv2d_nhwc(ctypes.byref(dd), _stream()))
        torch.cuda.synchronize()
        return y, gp

    y, gp = launch()
    what = f"{c['id']} [{c['launcher']}, {c['cls']}]"
    y.guards_ok(what + " y", co)
    for k, v in ptrs.items():
        if isinstance(v, Big):
            v.guards_ok(what + " " + k)
    if c["unit"] == "wrow":
        yv = y.t[:, :co].t().unsqueeze(1)                            # [Cout][1][M], a strided view
    else:
        yv = y.t.view(U, -1, ldy)
    worst = H.check_periodic(yv, ref, bnd, what)
    unit_bytes = [(e[c["big"]] // U) * 2] + ([OHW * ldy * esz] if c["unit"] == "image" else [ldy * esz] if c["unit"] == "row" else [])
    host = H.host_check(yv, ref.cpu(), bnd.cpu(), H.spot_units(U, *unit_bytes), what)
    if c["gn"]:                                                      # partial planes against fp64 sums of the kernel's own 16-bit output
        gp.guards_ok(what + " gn_part")
        parts = gp.t.view(c["N"], plan.gn_parts, co, 2)
        per = max(1, H.CHUNK_ELEMS // (OHW * co))
        for i in range(0, c["N"], per):
            s = parts[i:i + per].double().sum(1)
            terms = yv[i:i + per, :, :co].double().permute(0, 2, 1)
            worst = max(worst, CR.compare_sums(s[..., 0], s[..., 1], terms, OHW, what + f" GroupNorm plane (P = {plan.gn_parts})"))
    y2, gp2 = launch()
    H.equal_chunked(_bits(y.raw), _bits(y2.raw), what + " y")
    if gp is not None:
        H.equal_chunked(_bits(gp.raw), _bits(gp2.raw), what + " gn_part")
    nbytes = {k: e[k] * 2 for k in ("x", "x2", "w", "r") if e[k] >= 1 << 24}
    nbytes["y"] = M * ldy * esz
    _report(c["id"], f"{names[info.launcher]}, splitk {info.splitk}" + (", GroupNorm pass" if gn_pass else ""), worst, host, nbytes, t0)


# ---- norms and per-channel kernels ---------------------------------------------------------------------------------------------------
def _run_rows(c, what, inputs, launch, reference, out_ld, out_dtype=DT, out_width=None, t0=None, out_rows=None):
    """Shared driver of the row- / image-periodic elementwise cases.  inputs: {name: host tensor [P, R, ld]} tiled to U units;
    launch(bufs, y) runs the export; reference(period inputs on the device) -> (ref, bnd) [P, R, width] fp64."""
    t0 = t0 or time.time()
    U, P, R = c["U"], c["P"], out_rows or c["R"]                     # R: output rows per unit
    esz = torch.empty(0, dtype=out_dtype).element_size()
    total = sum(U * v[0].numel() * v.element_size() for v in inputs.values()) + 2 * U * R * out_ld * esz
    _need(total, what)
    dev = {k: v.cuda() for k, v in inputs.items()}
    ref, bnd = reference(dev)
    bufs = {k: _periodic(v.reshape(P, -1), U) for k, v in dev.items()}

    def once():
        y = Big(U * R, out_ld, out_dtype, fill="nan", grows=GUARD_ROWS)
        launch(bufs, y)
        torch.cuda.synchronize()
        return y
    y = once()
    width = out_width or out_ld
    y.guards_ok(what + " y", width)
    for k, b in bufs.items():
        b.guards_ok(what + " " + k)
    yv = y.t.view(U, R, out_ld)
    worst = H.check_periodic(yv, ref.reshape(P, R, width), bnd.reshape(P, R, width), what)
    ub = [v[0].numel() * v.element_size() for v in inputs.values()] + [R * out_ld * esz]
    host = H.host_check(yv, ref.reshape(P, R, width).cpu(), bnd.reshape(P, R, width).cpu(), H.spot_units(U, *ub), what)
    y2 = once()
    H.equal_chunked(_bits(y.raw), _bits(y2.raw), what)
    nbytes = {k: U * v[0].numel() * v.element_size() for k, v in inputs.items() if U * v[0].numel() >= 1 << 24}
    nbytes["y"] = U * R * out_ld * esz
    _report(c["id"], c["op"], worst, host, nbytes, t0)


def _gen(c):
    return NR.gen_of(c["id"])


@pytest.mark.parametrize("c", T.ROW_CASES, ids=[c["id"] for c in T.ROW_CASES])
def test_rows_large(capi, c):
    """Row-wise exports on [rows, C]: ur_axpy_channels, ur_spade_modulate, ur_layernorm_rows, ur_softmax_rows_f32 (rows periodic)."""
    lib, code, g = capi.lib, capi.UR_DT_BF16, _gen(c)
    U, P, C, op = c["U"], c["P"], c["C"], c["op"]
    what = f"{c['id']} [{op}, {c['cls']}]"
    if op == "axpy":
        a, b = (torch.randn(P, 1, C, generator=g).to(DT) for _ in range(2))
        s = torch.randn(C, generator=g)
        sd = s.cuda()
        _run_rows(c, what, dict(a=a, b=b),
                  lambda B, y: capi.check(lib.ur_axpy_channels(B["a"].ptr, B["b"].ptr, sd.data_ptr(), y.ptr, U, C, code, _stream())),
                  lambda D: NR.axpy_reference(D["a"].view(P, C), D["b"].view(P, C), sd, DT), C)
    elif op == "spade":
        n = torch.randn(P, 1, C, generator=g).to(DT)
        gb = torch.randn(P, 1, 2 * C, generator=g).to(DT)
        r = torch.randn(P, 1, C, generator=g).to(DT)
        _run_rows(c, what, dict(n=n, gb=gb, r=r),
                  lambda B, y: capi.check(lib.ur_spade_modulate(B["n"].ptr, B["gb"].ptr, 2 * C, B["r"].ptr, y.ptr, U, C, code, _stream())),
                  lambda D: NR.spade_reference(D["n"].view(P, C), D["gb"].view(P, 2 * C), C, D["r"].view(P, C), DT), C)
    elif op == "layernorm":
        x = torch.randn(P, 1, C, generator=g).to(DT)
        gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
        gd, bd = gamma.cuda(), beta.cuda()
        _run_rows(c, what, dict(x=x),
                  lambda B, y: capi.check(lib.ur_layernorm_rows(B["x"].ptr, y.ptr, gd.data_ptr(), bd.data_ptr(), U, C, NR.EPS, code, _stream())),
                  lambda D: NR.ln_reference(D["x"].view(P, C), gamma, beta, DT), C)
    else:
        assert op == "softmax"
        s = torch.randn(P, 1, C, generator=g) * 3.0
        ldp = C + 8

        def launch(B, y):
            capi.check(lib.ur_softmax_rows_f32(B["s"].ptr, y.ptr, U, C, ldp, code, _stream()))
        # (columns [C, ldp) are written as zeros by contract: the reference and the bound there are 0)
        def reference(D):
            ref, bnd = NR.softmax_reference(D["s"].view(P, C), DT)
            z = torch.zeros(P, ldp - C, dtype=torch.float64, device=ref.device)
            return torch.cat([ref, z], 1), torch.cat([bnd, z], 1)
        _run_rows(c, what, dict(s=s), launch, reference, ldp)


@pytest.mark.parametrize("c", T.IMG_CASES, ids=[c["id"] for c in T.IMG_CASES])
def test_images_large(capi, c):
    """Per-image exports on [N, HW, C] (images periodic): ur_scale_channels, ur_scale_channels_fanout, ur_dwconv3x3_nhwc, ur_avgpool_hw
    and the GroupNorm chain with and without x2 (ur_groupnorm_nhwc runs ur_groupnorm_stats, ur_groupnorm_finalize and
    ur_groupnorm_apply_act, one after the other, through their own entry points)."""
    lib, code, g = capi.lib, capi.UR_DT_BF16, _gen(c)
    U, P, R, C, op = c["U"], c["P"], c["R"], c["C"], c["op"]
    what = f"{c['id']} [{op}, {c['cls']}]"
    if op == "scale":
        x = torch.randn(P, R, C, generator=g).to(DT)
        s = torch.randn(P, 1, C, generator=g)
        r = torch.randn(P, R, C, generator=g).to(DT)
        _run_rows(c, what, dict(x=x, s=s, r=r),
                  lambda B, y: capi.check(lib.ur_scale_channels(B["x"].ptr, B["s"].ptr, B["r"].ptr, y.ptr, U, R, C, code, _stream())),
                  lambda D: NR.scale_reference(D["x"], D["s"].view(P, C), D["r"], DT), C)
    elif op == "fanout":                                      # K tasks x B images: output image k * B + b = x[b] * s[k * B + b]
        K, Bn = c["K"], U // c["K"]
        assert Bn % P == 0                                     # so that output image i reads x image i mod P
        x = torch.randn(P, R, C, generator=g).to(DT)
        s = torch.randn(P, 1, C, generator=g)
        t0 = time.time()
        xb = _periodic(x.reshape(P, -1), Bn)
        _run_rows(c, what, dict(s=s),
                  lambda B, y: capi.check(lib.ur_scale_channels_fanout(xb.ptr, B["s"].ptr, y.ptr, Bn, K, R, C, code, _stream())),
                  lambda D: NR.scale_reference(x.cuda(), D["s"].view(P, C), None, DT), C, t0=t0)
        xb.guards_ok(what + " x")
    elif op == "dwconv":
        hh, ww = c["H"], c["W"]
        cc = dict(id=c["id"], N=P, H=hh, W=ww, C=C, gate=0)
        x, w, b = NR.dwconv_inputs(cc, DT, "cpu")
        wd, bd = w.cuda(), b.cuda()
        _run_rows(c, what, dict(x=x.reshape(P, R, C)),
                  lambda B, y: capi.check(lib.ur_dwconv3x3_nhwc(B["x"].ptr, wd.data_ptr(), bd.data_ptr(), y.ptr, U, hh, ww, C, 0, code, _stream())),
                  lambda D: NR.dwconv_reference(D["x"].view(P, hh, ww, C), wd, bd, 0, DT), C)
    elif op == "avgpool":                                      # statistics pass + finalize -> fp32 [N][C] channel means
        cc = dict(id=c["id"], N=P, HW=R, C1=C, C2=0, G=8, affine=False)
        x1, _, _, _ = NR.gn_inputs(cc, DT)
        ws = torch.empty(lib.ur_groupnorm_ws_bytes(U, R, C) // 4, dtype=torch.float32, device="cuda")

        def reference(D):
            ref = NR.gn_reference(D["x"].view(P, R, C), None, None, None, 8, 0, DT)
            return ref["chan_mean"], ref["chan_mean_bnd"]
        _run_rows(c, what, dict(x=x1.reshape(P, R, C)),
                  lambda B, y: capi.check(lib.ur_avgpool_hw(B["x"].ptr, y.ptr, U, R, C, ws.data_ptr(), code, _stream())),
                  reference, C, out_dtype=torch.float32, out_rows=1)
    else:
        assert op == "groupnorm"                               # C2 > 0: the virtual concat of two sources
        G, C2 = c["G"], c.get("C2", 0)
        C1 = C - C2
        cc = dict(id=c["id"], N=P, HW=R, C1=C1, C2=C2, G=G, affine=True)
        x1, x2, gamma, beta = NR.gn_inputs(cc, DT)
        gd, bd = gamma.cuda(), beta.cuda()
        nws = (lib.ur_groupnorm_ws_bytes(U, R, C1) + (lib.ur_groupnorm_ws_bytes(U, R, C2) if C2 else 0)) // 4
        ws = torch.empty(nws, dtype=torch.float32, device="cuda")
        ab = torch.empty(U, 2, C, dtype=torch.float32, device="cuda")
        inputs = dict(x=x1.reshape(P, R, C1))
        if C2:
            inputs["x2"] = x2.reshape(P, R, C2)

        def launch(B, y):
            capi.check(lib.ur_groupnorm_nhwc(B["x"].ptr, B["x2"].ptr if C2 else None, y.ptr, gd.data_ptr(), bd.data_ptr(), U, R, C1, C2, G, NR.EPS, 1,
                                             ws.data_ptr(), ab.data_ptr(), None, 0, None, 0, code, _stream()))

        def reference(D):
            ref = NR.gn_reference(D["x"].view(P, R, C1), D["x2"].view(P, R, C2) if C2 else None, gamma, beta, G, 1, DT)
            return ref["y"], ref["y_bnd"]
        _run_rows(c, what, inputs, launch, reference, C)


# ---- boundary kernels: the fp32 side of the launch crosses 2^32 bytes ----------------------------------------------------------------------
@pytest.mark.parametrize("c", T.BOUNDARY_CASES, ids=[c["id"] for c in T.BOUNDARY_CASES])
def test_boundary_large(capi, c):
    """ur_nhwc_to_nchw_f32, ur_image_unpad_resize_nchw, ur_image_u8_egress (decode tail) and ur_nchw_f32_to_nhwc (ingest) on periodic
    images, ur_f32_to_bf16_scaled on periodic rows."""
    lib, code = capi.lib, capi.UR_DT_BF16
    U, P, C, op = c["U"], c["P"], c["C"], c["op"]
    what = f"{c['id']} [{op}, fp32 side {T.f32_elems(c) * 4 / GiB:.2f} GiB]"
    assert T.f32_elems(c) > T.G30
    if op == "layout_out":
        hh, ww, ld = c["H"], c["W"], c["ld"]
        x = BR.layout_out_inputs(dict(c, N=P), DT)                                  # [P,H,W,ld], NaN in the columns [C, ld)
        _run_rows(c, what, dict(x=x.reshape(P, hh * ww, ld)),
                  lambda B, y: capi.check(lib.ur_nhwc_to_nchw_f32(B["x"].ptr, 0, y.ptr, U, C, hh, ww, ld, c["mul"], c["add"], code, _stream())),
                  lambda D: BR.layout_out_reference(D["x"].view(P, hh, ww, ld), C, c["mul"], c["add"]), C * hh * ww, out_dtype=torch.float32)
    elif op == "layout_in":
        hh, ww, Cp = c["H"], c["W"], c["Cpad"]
        x = BR.layout_in_inputs(dict(c, N=P))                                       # [P,C,H,W] fp32

        def reference(D):                                                            # the padding channels are written as zeros
            ref, bnd = BR.layout_in_reference(D["x"].view(P, C, hh, ww), 1.0, 0.0, DT)
            z = torch.zeros(P, hh, ww, Cp - C, dtype=torch.float64, device=ref.device)
            return torch.cat([ref, z], -1), torch.cat([bnd, z], -1)
        _run_rows(c, what, dict(x=x.reshape(P, 1, C * hh * ww)),
                  lambda B, y: capi.check(lib.ur_nchw_f32_to_nhwc(B["x"].ptr, y.ptr, U, C, hh, ww, Cp, code, _stream())), reference, Cp)
    elif op == "unpad_resize":
        XH, XW, ld, OH, OW = c["XH"], c["XW"], c["ld"], c["OH"], c["OW"]
        x = BR.resize_out_inputs(dict(c, N=P), DT)                                  # [P,XH,XW,ld], NaN outside the crop window and in [C, ld)

        def reference(D):                                                            # [P*OH*OW, C] -> NCHW units [P, C, OH*OW]
            Rf = BR.resize_out_reference(D["x"].view(P, XH, XW, ld), dict(c, N=P))
            assert not bool(Rf["nonfinite"].any())
            return tuple(v.view(P, OH * OW, C).permute(0, 2, 1).contiguous() for v in (Rf["ref"], Rf["E"]))
        _run_rows(c, what, dict(x=x.reshape(P, 1, XH * XW * ld)),
                  lambda B, y: capi.check(lib.ur_image_unpad_resize_nchw(B["x"].ptr, 0, y.ptr, U, C, XH, XW, ld, c["CH"], c["CW"], OH, OW, c["mul"],
                                                                         c["add"], 0, code, _stream())),
                  reference, OH * OW, out_dtype=torch.float32)
    elif op == "u8_egress":
        _u8_egress_large(capi, c, what)
    else:
        assert op == "cast"
        ld, Cp = c["ld"], c["Cpad"]
        x = BR.cast_inputs(dict(c, M=P), DT)                                         # [P, ld] fp32, NaN in the columns [C, ld)

        def reference(D):
            ref, bnd = BR.cast_reference(D["x"].view(P, ld), C, c["mul"], DT)
            z = torch.zeros(P, Cp - C, dtype=torch.float64, device=ref.device)
            return torch.cat([ref, z], -1), torch.cat([bnd, z], -1)
        _run_rows(c, what, dict(x=x.reshape(P, 1, ld)),
                  lambda B, y: capi.check(lib.ur_f32_to_bf16_scaled(B["x"].ptr, ld, y.ptr, U, C, Cp, c["mul"], code, _stream())), reference, Cp)


U8_PATTERN = 0xA5               # fill of the 8-bit slots: bytes the kernel must not write keep it


def _u8_egress_large(capi, c, what):
    """ur_image_u8_egress on an fp32 canvas batch past 2^32 bytes.  The geometry table is periodic too (image i has geometry i mod P).
    The P images of the first period are judged code by code by boundary_reference (resize_out_reference + check_codes, per image,
    with the bytes behind H * W * C still the fill pattern); every later slot must hold the bytes of slot i mod P (compared on the
    device, in chunks: the kernel is per image, so this checks every byte of every slot), the nonfinite flags must stay 0, the
    guards around dst and the flags untouched, and a second launch must give the same bytes."""
    t0 = time.time()
    lib, code = capi.lib, capi.UR_DT_BF16
    U, P, CH, CW, geom = c["U"], c["P"], c["CH"], c["CW"], c["geom"]
    slot = 3 * CH * CW + c["slack"]
    _need(U * CH * CW * 8 * 4 + 2 * U * slot, what)
    x = BR.egress_inputs(c, DT, 1)                                                   # fp32 [P,CH,CW,8], NaN outside each window
    bx = _periodic(x.reshape(P, -1), U)
    bg = H.tile_periodic(torch.empty(U, 4, dtype=torch.int32, device="cuda"), torch.tensor(geom, dtype=torch.int32, device="cuda"))
    G = 256

    def once():
        dst = torch.full((U * slot + 2 * G,), U8_PATTERN, dtype=torch.uint8, device="cuda")
        flags = torch.full((U + 2 * GUARD,), 7, dtype=torch.int32, device="cuda")
        flags[GUARD:GUARD + U] = 0
        capi.check(lib.ur_image_u8_egress(bx.ptr, 1, dst[G:].data_ptr(), slot, bg.data_ptr(), flags[GUARD:].data_ptr(), U, 3, CH, CW, 8, 0.5, 0.5, code, _stream()))
        torch.cuda.synchronize()
        return dst, flags
    dst, flags = once()
    H.check_fill(dst[:G], U8_PATTERN, what + " dst guard before")
    H.check_fill(dst[G + U * slot:], U8_PATTERN, what + " dst guard after")
    H.check_fill(flags[:GUARD], 7, what + " flag guard before")
    H.check_fill(flags[GUARD + U:], 7, what + " flag guard after")
    H.check_fill(flags[GUARD:GUARD + U], 0, what + " nonfinite flags")
    bx.guards_ok(what + " x")
    slots = dst[G:G + U * slot].view(U, slot)
    share = 0.0
    for n, (hh, ww, _, _) in enumerate(geom):                                        # the first period against fp64
        assert bool((slots[n, hh * ww * 3:] == U8_PATTERN).all()), f"{what} image {n}: bytes behind H W C were written"
        Rf = BR.resize_out_reference(bx.t[n].view(1, CH, CW, 8), BR.egress_case(c, n))
        assert not bool(Rf["nonfinite"].any())
        share = max(share, BR.check_codes(slots[n, :hh * ww * 3].view(hh * ww, 3).double(), Rf["ref"], Rf["E"], f"{what} image {n}"))
    per = max(1, H.CHUNK_ELEMS // (slot * P)) * P                                     # every slot against the slot of its period image
    for i in range(P, U, per):
        blk = slots[i:i + per]
        q, r = divmod(blk.shape[0], P)
        ok = bool((blk[:q * P].view(q, P, slot) == slots[:P]).all()) and bool((blk[q * P:] == slots[:r]).all())
        assert ok, f"{what}: slots [{i}, {i + blk.shape[0]}) differ from the slots of their period images"
    for i in H.spot_units(U, CH * CW * 8 * 4, slot):                                 # a few slots on the host, code by code
        hh, ww, _, _ = geom[i % P]
        Rf = BR.resize_out_reference(x[i % P].view(1, CH, CW, 8), BR.egress_case(c, i % P))
        host = slots[i].cpu()
        assert bool((host[hh * ww * 3:] == U8_PATTERN).all())
        BR.check_codes(host[:hh * ww * 3].view(hh * ww, 3).double(), Rf["ref"], Rf["E"], f"{what} image {i} (host)")
    dst2, flags2 = once()
    H.equal_chunked(dst, dst2, what + " dst")
    H.equal_chunked(flags, flags2, what + " flags")
    print(f"{c['id']}: u8_egress; every code of the first period inside the tie rule (tie-zone share {share:.4f}), every other slot equal to its "
          f"period image; tensors x {U * CH * CW * 32 / GiB:.2f} GiB, dst {U * slot / GiB:.2f} GiB; {time.time() - t0:.1f} s")
