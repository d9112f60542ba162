"""The scoring kernels at their stated size limits (-m gpu; cases in tests/scoring_large_cases.py, host gate in
tests/test_scoring_large_cpu.py): LPIPS, the classifier, the segmenter and PSNR / SSIM launched through the raw C ABI just below each
limit, on tensors whose bytes cross 2^31 or 2^32, and on the paths no small case reaches.

The inputs are periodic (tests/large_harness.py): unit i is unit i mod P of the P distinct units scoring_large_cases.build makes,
tiled on the device.  For every case:
  * every input sits between NaN (or sentinel) guards, every output in a NaN / sentinel-filled allocation with guards before and
    after it: an element the kernel did not write fails its bound, a guard it wrote fails the fill check;
  * EVERY output element is compared on the device, in chunks, with reference unit i mod P within the bound of the small-shape
    test of the same op (bit-equal for the exact ops); the first unit, the last and the one straddling byte 2^31 are also compared on
    the host;
  * a second launch into a fresh buffer must give the same bits.
No tolerance is introduced here.  A case skips only when the device has less free memory than it needs, and prints both numbers.
"""
import time

import numpy as np
import pytest
import torch

import large_harness as H
import scoring_large_cases as T

pytestmark = pytest.mark.gpu
GUARD = 64                      # guard elements before and after every buffer (a multiple of 16 bytes in every type)
GiB = 1 << 30
F32, F64, U8, I32, I64 = torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64
# dtype -> (integer view, fill pattern): NaNs for the float types, a value no result takes for the integer ones
FILL = {F32: (I32, 0x7FC00000), F64: (I64, 0x7FF8000000000000), U8: (U8, 0xA5), I32: (I32, 0x5A5A5A5A), I64: (I64, 0x5A5A5A5A5A5A5A5A)}


@pytest.fixture(scope="module")
def lib():
    from unirestore_amd import capi
    return capi.lib


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    import gc
    try:                                  # a device fault is sticky: nothing more is launched on the card, the module ends here
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"device error after a scoring limit case, stopping: {err}", returncode=3)
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


class Buf:
    """n elements of `dtype` between GUARD guard elements; out=True: everything holds the fill pattern (an output), else only the
    guards do (an input: the caller writes the body)."""

    def __init__(self, n, dtype, out=False):
        self.n, self.dtype = n, dtype
        self.raw = torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
        view, self.pattern = FILL[dtype]
        self.bits_raw = self.raw.view(view)
        if out:
            for i in range(0, self.raw.numel(), H.COPY_ELEMS):
                self.bits_raw[i:i + H.COPY_ELEMS].fill_(self.pattern)
        else:
            self.bits_raw[:GUARD].fill_(self.pattern)
            self.bits_raw[GUARD + n:].fill_(self.pattern)
        self.t = self.raw[GUARD:GUARD + n]
        self.bits = self.bits_raw[GUARD:GUARD + n]

    @property
    def ptr(self):
        return self.t.data_ptr()

    @property
    def nbytes(self):
        return self.n * self.t.element_size()

    def guards_ok(self, what):
        H.check_fill(self.bits_raw[:GUARD], self.pattern, what + " guard before")
        H.check_fill(self.bits_raw[GUARD + self.n:], self.pattern, what + " guard after")


def _tile(src, U):
    """src [P, ...] on the CPU -> a guarded device buffer of U units, unit i = src[i % P]."""
    P, unit = src.shape[0], src[0].numel()
    b = Buf(U * unit, src.dtype)
    H.tile_periodic(b.t.view(U, unit), src.reshape(P, unit).contiguous().cuda())
    return b


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _twice(lib, what, make_out, launch):
    """Launch into fresh outputs twice; the bits must agree.  Returns the first launch's outputs (a tuple of Buf)."""
    outs = []
    for _ in range(2):
        o = make_out()
        rc = launch(*o)
        assert rc == 0, (what, rc, lib.ur_last_error().decode())
        torch.cuda.synchronize()
        outs.append(o)
    for a, b in zip(*outs):
        H.equal_chunked(a.bits, b.bits, what)
    return outs[0]


def _check(y, U, ref, bnd, what, *other_unit_bytes):
    """Every element of y (U units of ref's unit shape) on the device, spot units on the host, the guards."""
    R, width = ref.shape[1:]
    yv = y.t.view(U, R, width)
    worst = H.check_periodic(yv, ref.cuda(), bnd.cuda(), what)
    host = H.host_check(yv, ref, bnd, H.spot_units(U, R * width * y.t.element_size(), *other_unit_bytes), what)
    y.guards_ok(what)
    return max(worst, host)


def _report(c, worst, t0, bound, **tensors):
    sizes = ", ".join(f"{k} {v.nbytes / GiB:.2f} GiB" for k, v in tensors.items())
    print(f"{c['id']} [{c['export']}: {', '.join(c['props'])}]: worst |err| / bound {worst:.3f} (bound: {bound}); {sizes}; {time.time() - t0:.1f} s")


def _inputs_ok(what, *bufs):
    for b in bufs:
        b.guards_ok(what + " input")


# ---- per op ------------------------------------------------------------------------------------------------------------------------

def _run_add(c, lib, u):
    n = c["n"]
    _need(4 * 4 * n, c["id"])
    a, b = _tile(u["ins"]["a"], n), _tile(u["ins"]["b"], n)
    (y,) = _twice(lib, c["id"], lambda: (Buf(n, F32, True),), lambda y: lib.ur_add_f32(a.ptr, b.ptr, y.ptr, n, _stream()))
    worst = _check(y, n, u["ref"], u["bnd"], c["id"])
    _inputs_ok(c["id"], a, b)
    return worst, "bit-equal", dict(a=a, y=y)


def _image_op(c, lib, u, out_elems_per_image, launch, key="x", extra=0):
    """One fp32 input of N periodic images, one fp32 output."""
    N = c["N"]
    x_unit = u["ins"][key][0].numel()
    _need(4 * (N * x_unit + 2 * N * out_elems_per_image) + extra, c["id"])
    x = _tile(u["ins"][key], N)
    (y,) = _twice(lib, c["id"], lambda: (Buf(N * out_elems_per_image, F32, True),), lambda y: launch(x, y))
    worst = _check(y, N, u["ref"], u["bnd"], c["id"], 4 * x_unit)
    _inputs_ok(c["id"], x)
    return worst, dict(x=x, y=y)


def _run_upsample(c, lib, u):
    from unirestore_amd import f32net
    iy, wy = f32net._device_tables((c["h"],), c["H"], 0)
    ix, wx = f32net._device_tables((c["w"],), c["W"], 0)
    worst, t = _image_op(c, lib, u, c["H"] * c["W"] * c["C"], lambda x, y: lib.ur_upsample_bilinear_ac_f32(
        x.ptr, y.ptr, c["N"], c["h"], c["w"], c["C"], c["H"], c["W"], iy.data_ptr(), wy.data_ptr(), ix.data_ptr(), wx.data_ptr(), _stream()))
    return worst, "UPSAMPLE_TOL x max |x|", t


def _run_maxpool5(c, lib, u):
    worst, t = _image_op(c, lib, u, c["H"] * c["W"] * c["C"],
                         lambda x, y: lib.ur_maxpool5_f32(x.ptr, y.ptr, c["N"], c["H"], c["W"], c["C"], _stream()))
    return worst, "bit-equal", t


def _run_maxpool2d(c, lib, u):
    oh, ow = (c["H"] - 3) // 2 + 1, (c["W"] - 3) // 2 + 1
    worst, t = _image_op(c, lib, u, oh * ow * c["C"], lambda x, y: lib.ur_maxpool2d_f32(x.ptr, y.ptr, c["N"], c["H"], c["W"], c["C"], _stream()))
    return worst, "bit-equal", t


def _run_maxpool_pad(c, lib, u):
    oh, ow = (c["H"] - 1) // 2 + 1, (c["W"] - 1) // 2 + 1
    worst, t = _image_op(c, lib, u, oh * ow * c["C"],
                         lambda x, y: lib.ur_maxpool2d_pad_f32(x.ptr, y.ptr, c["N"], c["H"], c["W"], c["C"], _stream()))
    return worst, "bit-equal", t


def _run_avgpool(c, lib, u):
    worst, t = _image_op(c, lib, u, c["C"], lambda x, y: lib.ur_avgpool_f32(x.ptr, y.ptr, c["N"], c["P"], c["C"], _stream()))
    return worst, "AVGPOOL_TOL x mean |x|", t


def _run_seg_prep(c, lib, u):
    from unirestore_amd import f32net
    iy, wy = f32net._device_tables((c["H"],), c["OH"], 0)
    ix, wx = f32net._device_tables((c["W"],), c["OW"], 0)
    worst, t = _image_op(c, lib, u, c["OH"] * c["OW"] * 3, lambda x, y: lib.ur_seg_prep(
        x.ptr, y.ptr, c["N"], 3, c["H"], c["W"], c["OH"], c["OW"], iy.data_ptr(), wy.data_ptr(), ix.data_ptr(), wx.data_ptr(), _stream()))
    return worst, "PREP_TOL (segment)", t


def _run_lpips_prep(c, lib, u):
    worst, t = _image_op(c, lib, u, c["H"] * c["W"] * 3, lambda x, y: lib.ur_lpips_prep(x.ptr, y.ptr, c["N"], 3, c["H"], c["W"], _stream()))
    return worst, "PREP_TOL (lpips)", t


def _run_classify_prep(c, lib, u):
    from unirestore_amd import classify
    N, h, w = c["N"], c["H"], c["W"]
    fw, cw, ww, tw = classify._device_table(w, 0)
    fh, ch, wh, th = classify._device_table(h, 0)
    tmp = Buf(N * 3 * h * 224, F32, True)                   # the scratch of the horizontal pass: written in full, guards untouched
    worst, t = _image_op(c, lib, u, 224 * 224 * 3, lambda x, y: lib.ur_classify_preprocess(
        x.ptr, tmp.ptr, y.ptr, N, 3, h, w, fw.data_ptr(), cw.data_ptr(), ww.data_ptr(), tw, fh.data_ptr(), ch.data_ptr(), wh.data_ptr(), th,
        _stream()), extra=tmp.nbytes)
    tmp.guards_ok(c["id"] + " tmp")
    for i in range(0, tmp.n, H.CHUNK_ELEMS):                # every element of tmp was written (no NaN left)
        assert not bool(torch.isnan(tmp.t[i:i + H.CHUNK_ELEMS]).any()), f"{c['id']}: tmp not written in full"
    return worst, "PREP_TOL (classify)", dict(t, tmp=tmp)


def _run_tta(c, lib, u):
    from unirestore_amd import f32net
    N, C, Ho, Wo = c["N"], c["C"], c["H"], c["W"]
    px = Ho * Wo
    map_elems = sum(h * w for h, w in c["maps"]) * C * N
    _need(4 * map_elems + 2 * N * px * (1 + (4 * C if c["avg"] else 0)), c["id"])
    maps = [_tile(u["ins"][f"m{k}"], N) for k in range(3)]
    iy, wy = f32net._device_tables(tuple(h for h, _ in c["maps"]), Ho, 0)
    ix, wx = f32net._device_tables(tuple(w for _, w in c["maps"]), Wo, 0)
    hw = [v for m in c["maps"] for v in m]

    def make():
        return (Buf(N * px, U8, True),) + ((Buf(N * px * C, F32, True),) if c["avg"] else ())

    def launch(pred, avg=None):
        return lib.ur_seg_tta_argmax(maps[0].ptr, maps[1].ptr, maps[2].ptr, 3, N, C, *hw, Ho, Wo, iy.data_ptr(), wy.data_ptr(), ix.data_ptr(),
                                     wx.data_ptr(), pred.ptr, avg.ptr if avg is not None else None, _stream())
    outs = _twice(lib, c["id"], make, launch)
    pred = outs[0]
    assert u["undecidable"] <= 0.005, u["undecidable"]
    worst = _check(pred, N, u["pred"], u["pred_bnd"], c["id"] + " pred")        # equal to the fp64 argmax on every decidable pixel
    tensors = dict(maps=maps[0], pred=pred)
    if c["avg"]:
        avg = outs[1]
        worst = max(worst, _check(avg, N, u["ref"], u["bnd"], c["id"] + " avg"))
        rows = avg.t.view(N * px, C)
        for i in range(0, N * px, 1 << 20):                                     # the prediction is an argmax of the kernel's own averaged logits
            v = rows[i:i + (1 << 20)]
            got = v.gather(1, pred.t[i:i + (1 << 20)].long().view(-1, 1))[:, 0]
            assert bool((got == v.max(dim=1).values).all()), f"{c['id']}: pred is not the argmax of avg in pixels [{i}, {i + (1 << 20)})"
        tensors["avg"] = avg
    _inputs_ok(c["id"], *maps)
    return worst, "TTA_TOL x max |logit|; pred bit-equal where decidable", tensors


def _run_confusion(c, lib, u):
    P, C = c["P"], c["C"]
    pred_p, target_p = T.confusion_period(c)
    want = T.confusion_expected(c, pred_p, target_p)
    tdt = I64 if c["i64"] else U8
    _need(P * (1 + (8 if c["i64"] else 1)), c["id"])
    pred = _tile(torch.from_numpy(pred_p), P)
    target = _tile(torch.from_numpy(target_p).to(tdt), P)
    ws_bytes = int(lib.ur_seg_confusion_ws_bytes(P, C))
    assert ws_bytes == min(-(-P // T.SC_CHUNK), T.SC_MAX_BLOCKS) * C * C * 4
    conf, ws = _twice(lib, c["id"], lambda: (Buf(C * C, I64, True), Buf(ws_bytes // 4, I32, True)),
                      lambda conf, ws: lib.ur_seg_confusion(pred.ptr, target.ptr, int(c["i64"]), P, C, 255, ws.ptr, ws_bytes, conf.ptr, _stream()))
    got = conf.t.cpu().numpy().reshape(C, C)
    wrong = int((got != want).sum())
    print(f"{c['id']}: {T.confusion_trips(P)} trip(s), {T.bin_passes(C)} bin pass(es), {int(want.sum())} pixels counted, {wrong} bins differ")
    assert np.array_equal(got, want), (c["id"], wrong, np.argwhere(got != want)[:6].tolist())
    assert int(got.sum()) == int(want.sum()) > 0
    conf.guards_ok(c["id"] + " conf")
    ws.guards_ok(c["id"] + " ws")
    _inputs_ok(c["id"], pred, target)
    return 0.0, "equal to numpy.bincount", dict(pred=pred, target=target)


def _run_top1(c, lib, u):
    N, C = c["N"], c["C"]
    _need(4 * N * C, c["id"])
    x = _tile(u["ins"]["x"], N)
    labels = _tile(u["labels"], N)
    pred, counts = _twice(lib, c["id"], lambda: (Buf(N, I64, True), Buf(3 * C, I64, True)),
                          lambda pred, counts: lib.ur_top1_counts(x.ptr, labels.ptr, N, C, pred.ptr, counts.ptr, _stream()))
    P = len(u["pred"])
    want = u["pred"].repeat(-(-N // P))[:N]
    lab = u["labels"].repeat(-(-N // P))[:N]
    assert torch.equal(pred.t.cpu(), want)
    wp, wl = want.numpy(), lab.numpy()
    expect = np.stack([np.bincount(wp[wp == wl], minlength=C), np.bincount(wl, minlength=C), np.bincount(wp, minlength=C)])
    assert np.array_equal(counts.t.cpu().numpy().reshape(3, C), expect) and int(expect[0].sum()) > 0
    pred.guards_ok(c["id"] + " pred")
    counts.guards_ok(c["id"] + " counts")
    _inputs_ok(c["id"], x, labels)
    return 0.0, "bit-equal", dict(logits=x)


def _run_conv(c, lib, u):
    from unirestore_amd import f32net
    oh, ow = T.conv_out(c)
    rows = c["unit"] == "row"
    U = c["W"] if rows else c["N"]
    M, cout = c["N"] * oh * ow, c["Cout"]
    x_unit = u["ins"]["x"][0].numel()
    _need(4 * (U * x_unit + M * cout * (3 if c["res"] else 2)), c["id"])
    pc = f32net.PackedConvF32(u["weight"], u["bias"], c["stride"], c["pad"], torch.device("cuda", 0))
    x = _tile(u["ins"]["x"], U)
    res = _tile(u["ins"]["res"], U) if c["res"] else None
    (y,) = _twice(lib, c["id"], lambda: (Buf(M * cout, F32, True),), lambda y: lib.ur_conv2d_f32_res(
        x.ptr, pc.w.data_ptr(), pc.bias.data_ptr(), res.ptr if res is not None else None, y.ptr, c["N"], c["H"], c["W"], c["Cin"], cout, c["k"],
        c["k"], c["stride"], c["pad"], int(c["relu"]), _stream()))
    worst = _check(y, U, u["ref"], u["bnd"], c["id"], 4 * x_unit)
    _inputs_ok(c["id"], x, *([res] if res is not None else []))
    return worst, f"CONV_TOL[{c['tol']}] x (sum |a b| + |bias| + |res|)", dict(x=x, y=y)


def _run_lpips_layer(c, lib, u):
    N, P, C = c["N"], c["P"], c["C"]
    chunks = int(lib.ur_lpips_layer_parts(P))
    assert chunks == -(-P // 64)
    _need(4 * 2 * N * P * C, c["id"])
    feat = Buf(2 * N * P * C, F32)
    halves = feat.t.view(2 * N, P * C)
    H.tile_periodic(halves[:N], u["ins"]["fp"].reshape(T.P_IMG, P * C).cuda())          # the predictions, then the targets
    H.tile_periodic(halves[N:], u["ins"]["ft"].reshape(T.P_IMG, P * C).cuda())
    lin = u["lin"].cuda()
    (part,) = _twice(lib, c["id"], lambda: (Buf(N * chunks, F64, True),),
                     lambda part: lib.ur_lpips_layer(feat.ptr, lin.data_ptr(), N, P, C, part.ptr, N * chunks * 8, _stream()))
    assert bool(torch.isfinite(part.t).all())
    total = (part.t.view(N, chunks).sum(dim=1) / P).view(N, 1, 1)                         # as test_lpips_gpu._layer_gpu
    worst = H.check_periodic(total, u["ref"].cuda(), u["bnd"].cuda(), c["id"])
    part.guards_ok(c["id"] + " part")
    _inputs_ok(c["id"], feat)
    return worst, "LAYER_TOL x layer_abs", dict(feat=feat)


def _run_lpips_finish(c, lib, u):
    N = c["N"]
    assert int(lib.ur_lpips_ws_size(N, c["H"], c["W"])) == 5 * N * 8
    ws = Buf(5 * N, F64)
    for t in range(5):
        H.tile_periodic(ws.t.view(5, N)[t].view(N, 1), u["ins"]["parts"][:, t].reshape(T.P_IMG, 1).contiguous().cuda())
    (out,) = _twice(lib, c["id"], lambda: (Buf(N, F64, True),), lambda out: lib.ur_lpips_finish(ws.ptr, 5 * N * 8, N, c["H"], c["W"], out.ptr, _stream()))
    worst = _check(out, N, u["ref"], u["bnd"], c["id"])
    _inputs_ok(c["id"], ws)
    return worst, "bit-equal (the same fp64 operations in the same order)", dict(ws=ws)


def _run_metrics(c, lib, u):
    N, C, h, w, win = c["N"], c["C"], c["H"], c["W"], c["win"]
    _need(2 * 4 * N * C * h * w, c["id"])
    pred, target = _tile(u["ins"]["pred"], N), _tile(u["ins"]["target"], N)
    ws_bytes = int(lib.ur_image_metrics_ws_size(N, C, h, w, win))
    tiles = -(-(w - win + 1) // 64) * -(-(h - win + 1) // 16)
    assert ws_bytes == 2 * N * C * tiles * 8 and C * tiles > 256
    psnr, ssim, ws = _twice(lib, c["id"], lambda: (Buf(N, F64, True), Buf(N, F64, True), Buf(ws_bytes // 8, F64, True)),
                            lambda psnr, ssim, ws: lib.ur_image_metrics(pred.ptr, target.ptr, N, C, h, w, win, 1.0, psnr.ptr, ssim.ptr, ws.ptr,
                                                                        ws_bytes, _stream()))
    dp = _check(psnr, N, u["psnr"], u["psnr_bnd"], c["id"] + " psnr")
    ds = _check(ssim, N, u["ssim"], u["ssim_bnd"], c["id"] + " ssim")
    print(f"{c['id']}: |dPSNR| / PSNR_TOL {dp:.3f}, |dSSIM| / SSIM_TOL {ds:.3f}")
    ws.guards_ok(c["id"] + " ws")
    _inputs_ok(c["id"], pred, target)
    return max(dp, ds), "PSNR_TOL / SSIM_TOL", dict(pred=pred, target=target)


RUN = {"add": _run_add, "upsample": _run_upsample, "maxpool5": _run_maxpool5, "maxpool2d": _run_maxpool2d, "maxpool_pad": _run_maxpool_pad,
       "avgpool": _run_avgpool, "seg_prep": _run_seg_prep, "lpips_prep": _run_lpips_prep, "classify_prep": _run_classify_prep, "tta": _run_tta,
       "confusion": _run_confusion, "top1": _run_top1, "conv": _run_conv, "lpips_layer": _run_lpips_layer, "lpips_finish": _run_lpips_finish,
       "metrics": _run_metrics}


@pytest.mark.parametrize("cid", [c["id"] for c in T.CASES])
def test_scoring_kernel_at_its_limit(cid, lib):
    c = T.by_id(cid)
    t0 = time.time()
    u = {} if c["op"] == "confusion" else T.build(c)
    worst, bound, tensors = RUN[c["op"]](c, lib, u)
    _report(c, worst, t0, bound, **tensors)
    assert worst <= 1.0


@pytest.mark.parametrize("op", sorted(T.LONG_AXIS))
def test_long_axis_tables_are_indexed_in_64_bits(op, lib):
    """One image of one column and 2^29 or 2^30 rows (scoring_large_cases.LONG_AXIS): `2 * oy`, `2 * (k * H + oy)` or `k * H + oy`
    pass 2^31.  Periodic caller tables make the output periodic; every row is compared with the fp64 period."""
    import segment_reference as SR
    t0 = time.time()
    d = T.LONG_AXIS[op]
    Hh, C = d["H"], d["C"]
    srcs, idx, wt, ref, bnd = T.long_axis_units(op)
    k = len(srcs)
    _need(Hh * (k * 12 + 2 * (4 * C + 1)), f"long axis {op}")
    iy, wy = Buf(k * Hh, I32), Buf(k * Hh * 2, F32)
    for j in range(k):                                          # table row j of the launch: [H] / [H][2], period 771
        H.tile_periodic(iy.t.view(k, Hh)[j].view(Hh, 1), idx[j].view(-1, 1).cuda())
        H.tile_periodic(wy.t.view(k, Hh, 2)[j], wt[j].cuda())
    ix = torch.zeros(k, dtype=torch.int32, device="cuda")
    wx = torch.tensor([[1.0, 0.0]] * k, dtype=torch.float32, device="cuda")
    maps = [s.contiguous().cuda() for s in srcs]                # [h][1][C]
    if op == "upsample":
        (y,) = _twice(lib, "long axis upsample", lambda: (Buf(Hh * C, F32, True),), lambda y: lib.ur_upsample_bilinear_ac_f32(
            maps[0].data_ptr(), y.ptr, 1, d["maps"][0], 1, C, Hh, 1, iy.ptr, wy.ptr, ix.data_ptr(), wx.data_ptr(), _stream()))
        worst = _check(y, Hh, ref, bnd, "long axis upsample")
    else:
        ok = SR.decidable(ref.permute(0, 2, 1), float(bnd.max()))                  # [P, 1]
        assert float(ok.float().mean()) >= 0.995
        pred_ref = ref.argmax(dim=2, keepdim=True).double()
        pred_bnd = torch.where(ok.view(-1, 1, 1), 0.0, 255.0).double()
        ptr = [m.data_ptr() for m in maps] + [None] * (3 - k)
        hw = [v for h in d["maps"] for v in (h, 1)] + [0] * (2 * (3 - k))
        outs = _twice(lib, f"long axis {op}", lambda: (Buf(Hh, U8, True),) + ((Buf(Hh * C, F32, True),) if d["avg"] else ()),
                      lambda pred, avg=None: lib.ur_seg_tta_argmax(*ptr, k, 1, C, *hw, Hh, 1, iy.ptr, wy.ptr, ix.data_ptr(), wx.data_ptr(), pred.ptr,
                                                                   avg.ptr if avg is not None else None, _stream()))
        worst = _check(outs[0], Hh, pred_ref, pred_bnd, f"long axis {op} pred")
        if d["avg"]:
            worst = max(worst, _check(outs[1], Hh, ref, bnd, f"long axis {op} avg"))
    _inputs_ok(f"long axis {op}", iy, wy)
    print(f"long axis {op}: H = {Hh}, worst |err| / bound {worst:.3f}; tables {(iy.nbytes + wy.nbytes) / GiB:.1f} GiB; {time.time() - t0:.1f} s")
    assert worst <= 1.0
