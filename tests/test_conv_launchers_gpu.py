"""Every conv / GEMM launcher (csrc/igemm_impl.h UR_CONV_LAUNCHERS) against fp64, element by element (-m gpu, bf16 and fp16).

The cases are tests/conv_launcher_cases.py; the bound is stated in tests/conv_reference.py:

    |y - ref| <= u_out * |ref| + 4 * sqrt(K) * 2^-24 * A + eps_act + abs_out

Each case calls ur_conv2d_nhwc with a raw descriptor and, per workspace size (the 192 MiB ops.workspace passes, one that forces
fewer splits, none, and any edge sizes of the case):
  * asserts the planned launcher (ur_conv2d_plan_launch) and the split counts before launching - a case dispatch moves fails;
  * prefills y, yt and every statistics plane with NaN (sized from ur_conv2d_plan), gives y guard rows past M and, where allowed,
    ldy > output columns: guard rows and padding columns must come back bit-unchanged;
  * runs twice into fresh NaN buffers and requires bit-identical outputs and planes;
  * checks every output element against the bound, the whole output against the rel-L2 tolerance of tests/test_ops_gpu.py, and the
    GroupNorm / row-sum planes per (image, channel) / per row against fp64 sums of the kernel's own 16-bit output.

The table also runs every (launch path, feature) and (launch path, feature pair) that planning accepts around its base cases
(tests/conv_launcher_space.py; the CPU gate in tests/test_conv_plan_cpu.py holds the table against that space).
"""
import ctypes
import math
import zlib

import pytest
import torch

import conv_launcher_cases as T
import conv_reference as R
from golden_util import rel_l2

pytestmark = pytest.mark.gpu
GUARD = 3                       # rows of y past M that must stay untouched
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
REL_TOL = {torch.bfloat16: 3e-3, torch.float16: 4e-4, torch.float32: 2e-4}
WORST = {}                      # (launcher, dtype) -> largest |y - ref| / bound seen (printed at the end of the module)


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    yield c
    if WORST:
        print("\nlargest |y - ref| / bound per launcher:")
        for (name, dt), r in sorted(WORST.items()):
            print(f"  {name:20s} {dt}: {r:.3f}")


def _nan(shape, dtype):
    return torch.full((shape,) if isinstance(shape, int) else shape, float("nan"), dtype=dtype, device="cuda")


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _inputs(c, dt):
    """Device inputs of case c (kernel layouts) and their fp64 values in logical layouts."""
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    G = T.nbatch(c)
    geo = T.geometry(c)
    N, H, W, C1, C2, Cout, KH = c["N"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"], c["KH"]
    cin = C1 + C2
    K = KH * KH * cin
    t = {}
    # x: [N,H,W,ldx] (grouped: G slices of C1 channels; bmm: B row blocks of bs_x elements)
    if c["bmm"]:
        xb = torch.randn(G * geo["bs_x"], generator=g).to(dt)
        t["x"] = xb
        xs = [xb[b * geo["bs_x"]: b * geo["bs_x"] + T.m_rows(c) * geo["ldx"]].view(T.m_rows(c), geo["ldx"])[:, :C1] for b in range(G)]
        xs = [v.double().view(1, 1, T.m_rows(c), C1) for v in xs]
    else:
        xb = torch.randn(N, H, W, geo["ldx"], generator=g).to(dt)
        t["x"] = xb
        xs = [xb[..., b * C1:(b + 1) * C1].double() for b in range(G)]
    if C2:
        x2 = torch.randn(N, H, W, C2, generator=g).to(dt)
        t["x2"] = x2
        xs = [torch.cat([xs[0], x2.double()], -1)]
    # logical weights [G*Cout, KH, KW, cin]; zero_rows trailing output channels are zero (weights and bias)
    wl = (torch.randn(G * Cout, KH, KH, cin, generator=g) / math.sqrt(K)).to(dt)
    if c["zero_rows"]:
        wl[Cout - c["zero_rows"]:] = 0
    if c["kcm"]:
        wk = wl.reshape(G * Cout, KH * KH, cin // 64, 64).permute(0, 2, 1, 3).reshape(G * Cout, K)
    else:
        wk = wl.reshape(G * Cout, K)
    if c["bmm"]:
        wb = torch.zeros(G, Cout, geo["ldw"], dtype=dt)
        wb[:, :, :K] = wk.view(G, Cout, K)
        t["w"] = wb
    else:
        t["w"] = wk.contiguous()
    if c["wfrag"]:
        nt, nc = Cout // 128, cin // 64
        t["w_frag"] = wk.view(nt, 4, 32, nc, 9, 4, 2, 8).permute(0, 3, 4, 5, 1, 6, 2, 7).contiguous()
    if c["bias"]:
        rows = N if c["bias_img"] else 1
        bias = torch.randn(rows, G * Cout, generator=g) * 0.5
        if c["zero_rows"]:
            bias[:, Cout - c["zero_rows"]:] = 0
        t["bias"] = bias.contiguous()
    if c["res"]:
        t["residual"] = torch.randn(T.m_rows(c), geo["ldr"], generator=g).to(dt)
    if c["gn_ab"]:
        ab = torch.empty(N, 2, cin)
        ab[:, 0] = torch.rand(N, cin, generator=g) + 0.5
        ab[:, 1] = torch.randn(N, cin, generator=g) * 0.5
        t["gn_ab"] = ab
    if c["ln"]:
        xv = xs[0].reshape(-1, cin)
        h = cin // 2
        st = torch.stack([torch.stack([xv[:, :h].sum(1), (xv[:, :h] ** 2).sum(1)], -1),
                          torch.stack([xv[:, h:].sum(1), (xv[:, h:] ** 2).sum(1)], -1)]).float()
        t["ln_stats"] = st.contiguous()
        t["ln_colsum"] = wk.double().sum(1).float()
    return t, xs, wl.double()


def _reference(c, t, xs, wl, dt_out):
    """(ref, bound, K) in output layout [G][M][Cout_out] (fp64, on the GPU)."""
    G, Cout, KH = T.nbatch(c), c["Cout"], c["KH"]
    M = T.m_rows(c)
    outs, bnds = [], []
    K = KH * KH * (c["C1"] + c["C2"])
    for b in range(G):
        x = xs[b if len(xs) > 1 else 0].cuda()
        amb = None
        if c["gn_ab"]:              # the loader reads act(a x + b) rounded to the 16-bit type; padding stays zero
            ab = t["gn_ab"].cuda()
            xn = x.float() * ab[:, None, None, 0] + ab[:, None, None, 1]
            xn = xn * torch.sigmoid(xn)
            x, amb = R.round_ambiguous(xn, t["x"].dtype)
        if c["ups"]:
            x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
            amb = None if amb is None else amb.repeat_interleave(2, 1).repeat_interleave(2, 2)
        w = wl[b * Cout:(b + 1) * Cout].cuda()
        acc = R.conv_nhwc(x, w, c["stride"], c["pad"], c["OH"], c["OW"])
        A = R.conv_nhwc(x.abs(), w.abs(), c["stride"], c["pad"], c["OH"], c["OW"])
        bias = None
        if c["bias"]:
            bt = t["bias"].double().cuda()[:, b * Cout:(b + 1) * Cout]
            bias = bt.repeat_interleave(c["OH"] * c["OW"], 0) if c["bias_img"] else bt.expand(M, Cout)
        ln = None
        if c["ln"]:
            st = t["ln_stats"].double().cuda().sum(0)
            dim = K
            mean = st[:, 0] / dim
            var = (st[:, 1] / dim - mean * mean).clamp_min(0)
            ln = (mean, 1.0 / torch.sqrt(var + 1e-5), t["ln_colsum"].double().cuda())
        rc0 = b * T.cout_out(c) if c["groups"] else 0             # (bmm_nt descriptors have no residual stride: one tile for every batch)
        res = t["residual"].double().cuda()[:, rc0:rc0 + T.cout_out(c)] if c["res"] else None
        ref, Ao, eps = R.epilogue(acc, A, c["act"], bias, c["out_scale"], res, ln)
        bnd = R.bound(ref, Ao, eps, K, dt_out)
        if amb is not None:
            bnd = bnd + R.ACT_D[c["act"]] * abs(c["out_scale"]) * R.conv_nhwc(amb, w.abs(), c["stride"], c["pad"], c["OH"], c["OW"])
        outs.append(ref)
        bnds.append(bnd)
    return torch.stack(outs), torch.stack(bnds), K


def _run(capi, c, t, dt, label, nbytes, ws_full):
    """One workspace variant: plan checks, two launches into NaN buffers, guard checks.  Returns (outputs, planes, info)."""
    names = capi.launcher_names()
    geo = T.geometry(c)
    dev = {k: v.cuda() for k, v in t.items()}
    ptrs = {k: dev[k].data_ptr() for k in ("x", "x2", "w", "w_frag", "bias", "residual", "gn_ab", "ln_stats", "ln_colsum") if k in dev}
    ws = None
    if nbytes is not None:
        ws = ws_full if nbytes == T.WS_FULL else torch.empty((nbytes + 3) // 4, dtype=torch.float32, device="cuda")
        ptrs["workspace"] = ws.data_ptr()
    ph = T.placeholders(c)

    def desc(gn_pass, bufs):
        d = capi.ConvDesc()
        d.dtype = capi.UR_DT_F16 if dt == torch.float16 else capi.UR_DT_BF16
        p = dict(ptrs)
        for k in ("y", "yt", "gn_part", "row_stats"):
            p[k] = bufs[k].data_ptr() if k in bufs else ph[k]
        return T.fill(d, c, p, nbytes, gn_pass)

    info = capi.plan_launch(desc(False, {}))
    assert names[info.launcher] == T.expected_launcher(c, label), (c["id"], label, names[info.launcher])
    gn_pass = bool(info.gn_pass)
    d0 = desc(gn_pass, {})
    info = capi.plan_launch(d0)
    assert names[info.launcher] == T.expected_launcher(c, label)
    plan = capi.ConvPlan()
    capi.check(capi.lib.ur_conv2d_plan(d0, plan))
    M, G, co = T.m_rows(c), T.nbatch(c), T.cout_out(c)
    ydt = torch.float32 if c["out_f32"] else dt
    ldy = geo["ldy"] if not gn_pass else T.ldy(c, True)

    def buffers():
        b = {}
        b["y"] = _nan((G - 1) * geo["bs_y"] + (M + GUARD) * ldy if c["bmm"] else (M + GUARD) * ldy, ydt)
        if c["yt"] is not None:
            ns, tr = c["yt"]
            b["yt"] = _nan((M // tr, c["Cout"] - ns, tr + 8), dt)
        if c["gn"]:
            b["gn_part"] = _nan((c["N"], plan.gn_parts, co * G, 2), torch.float32)
        if c["rows"]:
            b["row_stats"] = _nan((plan.row_stat_parts, M, 2), torch.float32)
        return b

    runs = []
    for _ in range(2):
        b = buffers()
        d = desc(gn_pass, b)
        capi.check(capi.lib.ur_conv2d_nhwc(ctypes.byref(d), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        runs.append(b)
    for k in runs[0]:
        assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), (c["id"], label, k, "not bit-identical between two runs")
    b = runs[0]
    # y -> [G][M][width]; everything else in the buffer must still be the NaN fill
    y = b["y"]
    width = co if c["yt"] is None else c["yt"][0]
    keep = torch.ones_like(y, dtype=torch.bool)
    if c["bmm"]:
        outs = []
        for g_ in range(G):
            v = y[g_ * geo["bs_y"]: g_ * geo["bs_y"] + M * ldy].view(M, ldy)
            outs.append(v[:, :width])
            keep[g_ * geo["bs_y"]: g_ * geo["bs_y"] + M * ldy].view(M, ldy)[:, :width] = False
        yo = torch.stack(outs)
    else:
        y2 = y.view(M + GUARD, ldy)
        kv = keep.view(M + GUARD, ldy)
        if c["groups"]:
            yo = y2[:M, :co * G].view(M, G, co).permute(1, 0, 2)
            kv[:M, :co * G] = False
        else:
            yo = y2[:M, :width][None]
            kv[:M, :width] = False
    untouched = _bits(y)[keep]
    assert bool((untouched == _bits(_nan(1, ydt))[0]).all()), (c["id"], label, "write outside the output (guard rows / padding columns)")
    return yo, b, info, gn_pass


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.CASES, ids=[c["id"] for c in T.CASES])
def test_launcher_parity(capi, c, dtype):
    dt = DTYPES[dtype]
    t, xs, wl = _inputs(c, dt)
    ydt = torch.float32 if c["out_f32"] else dt
    ref, bnd, K = _reference(c, t, xs, wl, ydt)
    # the transposed columns are 16-bit whatever y is: the same bound with the 16-bit output terms (u_out |ref| + abs_out)
    bnd_t = bnd + (R.U_OUT[dt] - R.U_OUT[ydt]) * ref.abs() + (R.ABS_OUT[dt] - R.ABS_OUT[ydt])
    ws_full = torch.empty(T.WS_FULL // 4, dtype=torch.float32, device="cuda")
    d = capi.ConvDesc()
    ph = dict(T.placeholders(c), workspace=T.P)
    T.fill(d, c, ph, T.WS_FULL)
    d.dtype = capi.UR_DT_F16 if dt == torch.float16 else capi.UR_DT_BF16
    split_full = capi.plan_launch(d).splitk
    M = T.m_rows(c)
    co, G = T.cout_out(c), T.nbatch(c)
    for label, nbytes in T.ws_variants(c, split_full):
        yo, b, info, gn_pass = _run(capi, c, t, dt, label, nbytes, ws_full)
        if label == "full":
            assert info.splitk == split_full
        elif label == "less":
            assert info.splitk < split_full, (c["id"], info.splitk, split_full)
        elif label == "none":
            assert info.splitk == 1
        what = f"{c['id']} [{dtype}, workspace {label}, {capi.launcher_names()[info.launcher]}]"
        got = yo.double()
        width = got.shape[-1]
        worst = R.compare(got, ref[..., :width], bnd[..., :width], what + " y")
        assert rel_l2(got.float().cpu(), ref[..., :width].float().cpu()) < REL_TOL[ydt], what
        if c["zero_rows"] and not c["res"]:
            assert bool((got[..., co - c["zero_rows"]:] == 0).all()), what + ": padded channels must be exactly 0"
        if c["yt"] is not None:
            ns, tr = c["yt"]
            yt = b["yt"]
            vt = yt[..., :tr].permute(0, 2, 1).reshape(M, c["Cout"] - ns).double()
            worst = max(worst, R.compare(vt[None], ref[..., ns:], bnd_t[..., ns:], what + " yt"))
            assert bool(torch.isnan(yt[..., tr:].float()).all()), what + ": yt padding written"
        y16 = got if not c["out_f32"] else None
        if c["gn"]:
            P = b["gn_part"].shape[1]
            s = b["gn_part"].double().sum(1)                               # [N][C][2]
            yy = y16.permute(1, 0, 2).reshape(c["N"], M // c["N"], G * co).permute(0, 2, 1)
            worst = max(worst, R.compare_sums(s[..., 0], s[..., 1], yy, M // c["N"], what + f" GroupNorm plane (P = {P})"))
        if c["rows"]:
            s = b["row_stats"].double().sum(0)                             # [M][2]
            worst = max(worst, R.compare_sums(s[:, 0], s[:, 1], y16[0], width, what + " row sums"))     # (with yt: the columns below n_split)
        key = (capi.launcher_names()[info.launcher], dtype)
        WORST[key] = max(WORST.get(key, 0.0), worst)
    # ur_groupconv3x3_nhwc builds the same descriptor (its weights are tap-major: the chunk-major group loop is reachable only raw)
    wrapper = not (c["res"] or c["bias_img"] or c["out_f32"] or c["out_scale"] != 1.0)       # (the wrapper takes none of these)
    if c["groups"] and not c["kcm"] and wrapper:
        dev = {k: v.cuda() for k, v in t.items()}
        y = torch.empty(M, co * G, dtype=dt, device="cuda")
        capi.check(capi.lib.ur_groupconv3x3_nhwc(dev["x"].data_ptr(), dev["w"].data_ptr(), dev["bias"].data_ptr(), y.data_ptr(), c["N"], c["H"],
                                                 c["W"], c["C1"], c["Cout"], G, c["act"], ws_full.data_ptr(), T.WS_FULL,
                                                 capi.UR_DT_F16 if dt == torch.float16 else capi.UR_DT_BF16,
                                                 torch.cuda.current_stream().cuda_stream))
        want, _, _, _ = _run(capi, c, t, dt, "full", T.WS_FULL, ws_full)
        assert torch.equal(y.view(M, G, co).permute(1, 0, 2), want)
