"""Every attention kernel behind ur_attention_fwd_ws (csrc/attention.hip d = 64 / 128, attention512.hip, the ping-pong kernel of
attention_pp.hip and its key-split combine kernel) against fp64, element by element (-m gpu, bf16 and fp16), and modules/nn.py
attention_gemm, the GEMM fallback for other head dims.

The cases are tests/attention_cases.py; the fp64 reference and the per-element bound, with its derivation, are
tests/attention_reference.py (the one statement of the bound: this module only applies it).

Each case calls the C ABI with raw pointers and, per workspace variant (exact, 16 bytes short, none):
  * asserts the plan (ur_attention_plan_launch on the very pointers of the launch) against the case's expected kernel, n_full and
    n_split before launching - a case dispatch moves fails;
  * gives q, k and V^T NaN guard rows behind Tq / Tk / H*D inside their batch strides (V^T columns [Tk, ldvt) are zero, the header's
    contract), o NaN-prefilled with 3 guard rows per batch and, where the case says so, ldo > H*D: the output must be finite, guard
    rows and padding columns must come back bit-unchanged;
  * prefills the split workspace with NaN and puts a NaN guard behind ur_attention_workspace_bytes: the guard must come back
    unchanged, a launch planned unsplit must not touch the workspace at all, a split one must leave finite (m, l) in every row;
  * runs twice into fresh buffers and requires bit-identical outputs;
  * checks every element against the bound and the whole tensor against the rel-L2 tolerance of tests/test_ops_gpu.py.
Where a case has a split and an unsplit ping-pong variant, both must be inside the bound, agree bit for bit on every query tile
before n_full and differ somewhere behind it (the split really ran).  Where the dispatcher runs the 128-query kernel when the split
is refused (320, 380, 516 tiles) there is no unsplit ping-pong launch to compare with; plan and workspace contents prove the split.
"""
import math
import zlib

import pytest
import torch

import attention_cases as T
import attention_reference as R

pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
WS_GUARD = 64                   # floats behind the workspace that must stay untouched
WORST = {}                      # (kernel, dtype) -> largest |o - ref| / bound seen (printed at the end of the module)


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    yield c
    if WORST:
        print("\nlargest |o - ref| / bound per attention kernel:")
        for (name, dt), r in sorted(WORST.items()):
            print(f"  {name:24s} {dt}: {r:.3f}")


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _untouched(t):
    return bool((_bits(t) == _bits(_nan((1,), t.dtype))[0]).all())


def _device_inputs(c, dt, q, k, v):
    """Kernel-layout operands of case c on the GPU: (tensors to keep alive, q pointer, k pointer, vt pointer)."""
    g = T.geometry(c)
    C, Tq, Tk = g["C"], c["Tq"], c["Tk"]
    qb = _nan(g["q_shape"], dt)
    qb[:, :Tq, :C] = q.to(dt).cuda()
    if c["layout"] == "packed":
        qb[:, :Tk, C:2 * C] = k.to(dt).cuda()                   # the V third stays NaN: no kernel reads it
        kb, kptr = qb, qb.data_ptr() + 2 * C
    else:
        kb = _nan(g["k_shape"], dt)
        kb[:, :Tk, :C] = k.to(dt).cuda()                        # "kv": the V half of the K | V tensor stays NaN
        kptr = kb.data_ptr()
    vt = _nan(g["vt_shape"], dt)
    vt[:, :C, :Tk] = v.transpose(1, 2).to(dt).cuda()
    vt[:, :C, Tk:] = 0                                          # the header's contract for columns [Tk, ldvt)
    return (qb, kb, vt), qb.data_ptr(), kptr, vt.data_ptr()


def _launch(capi, c, dt, variant, ptrs):
    """One launch of a workspace variant into fresh NaN buffers after its plan check.  Returns (o buffer, plan, kernel name)."""
    g = T.geometry(c)
    qp, kp, vp = ptrs
    o = _nan(g["o_shape"], dt)
    has, nbytes = T.ws_arg(c, variant)
    ws = _nan((T.ws_bytes(c) // 4 + WS_GUARD,), torch.float32) if has else None
    args = T.plan_args(c, variant, q=qp, k=kp, vt=vp, o=o.data_ptr(), ws=ws.data_ptr() if has else None)
    plan = capi.attention_plan(*args)
    name = capi.attention_kernel_names()[plan.kernel]
    assert (name, plan.n_full, plan.n_split) == c["plans"][variant], (c["id"], variant)
    capi.check(capi.lib.ur_attention_fwd_ws(*args[:17], R.scale_of(c["scale"], c["D"]), args[17], args[18],
                                            capi.UR_DT_F16 if dt == torch.float16 else capi.UR_DT_BF16,
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    what = f"{c['id']} [{variant}]"
    if has:
        n = T.ws_bytes(c) // 4
        assert _untouched(ws[n:]), what + ": write behind ur_attention_workspace_bytes"
        if plan.n_split == 0:
            assert _untouched(ws), what + ": an unsplit launch wrote to the workspace"
        else:
            rows = ws[:n].view(plan.n_split * 2 * 256, 68)
            assert bool(torch.isfinite(rows[:, :66]).all()), what + ": split workspace rows not fully written"
            assert bool((rows[:, 65] > 0).all()), what + ": a key half left a row sum <= 0"
    return o, plan, name


def _output(c, o, what):
    """The [B][Tq][H*D] output inside buffer o; everything else in the buffer must still be the NaN fill."""
    C, Tq = T.channels(c), c["Tq"]
    keep = torch.ones_like(o, dtype=torch.bool)
    keep[:, :Tq, :C] = False
    assert bool((_bits(o)[keep] == _bits(_nan((1,), o.dtype))[0]).all()), what + ": write outside the output (guard rows / padding columns)"
    return o[:, :Tq, :C]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.LAUNCHED, ids=[c["id"] for c in T.LAUNCHED])
def test_attention_parity(capi, c, dtype):
    dt = DTYPES[dtype]
    B, H, Tq, Tk, D = c["B"], c["H"], c["Tq"], c["Tk"], c["D"]
    gen = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    q, k, v = R.inputs(c["kind"], c["scale"], B, H, Tq, Tk, D, dt, gen, nb=1 if c["shared"] else B)
    keep, *ptrs = _device_inputs(c, dt, q, k, v)
    scale = R.scale_of(c["scale"], D)
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    refs = {}
    outs = {}
    for variant in c["plans"]:
        o1, plan, name = _launch(capi, c, dt, variant, ptrs)
        o2, _, _ = _launch(capi, c, dt, variant, ptrs)
        what = f"{c['id']} [{dtype}, workspace {variant}, {name}]"
        assert torch.equal(_bits(o1), _bits(o2)), what + ": not bit-identical between two runs"
        out = _output(c, o1, what)
        assert bool(torch.isfinite(out).all()), what + ": output not finite"
        pingpong = name == T.PP
        if pingpong not in refs:
            refs[pingpong] = R.reference(qd, kd, vd, H, D, scale, dt, pingpong)
        ref, bnd = refs[pingpong]
        got = out.double()
        rel = R.rel_l2(got, ref)
        try:
            worst = R.compare(got, ref, bnd, H, D, what)
        finally:
            err = (got - ref).abs()
            ratio = float((err / bnd.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
            print(f"{what}: worst |o - ref| / bound {ratio:.3f}, rel-L2 {rel:.3e}")
        assert rel < R.REL_TOL[dt], what
        key = (name + (" + key split" if plan.n_split else ""), dtype)
        WORST[key] = max(WORST.get(key, 0.0), worst)
        outs[variant] = (out, plan, name)
    # split against unsplit ping-pong
    if "exact" in outs and outs["exact"][1].n_split:
        o_split, plan, _ = outs["exact"]
        other = next((outs[v] for v in ("short", "none") if v in outs and outs[v][2] == T.PP), None)
        if other is not None:
            o_plain = other[0]
            assert other[1].n_split == 0 and other[1].n_full == plan.n_full + plan.n_split
            nq = Tq // 256
            dev = o_split.device
            tile = ((torch.arange(B, device=dev)[:, None, None] * H + torch.arange(H, device=dev)[None, None, :]) * nq +
                    (torch.arange(Tq, device=dev) // 256)[None, :, None])                      # [B][Tq][H]
            before = (tile < plan.n_full)[..., None].expand(B, Tq, H, D)
            a, b = _bits(o_split.reshape(B, Tq, H, D)), _bits(o_plain.reshape(B, Tq, H, D))
            assert torch.equal(a[before], b[before]), c["id"] + ": split and unsplit launches differ on a tile before n_full"
            assert not torch.equal(a[~before], b[~before]), c["id"] + ": split and unsplit launches agree bit for bit - did the split run?"
    del keep


# one plain-layout shape per kernel: ops.attention (the front end every module calls) must give the bits of the raw call
OPS_SHAPES = [(T.PP, 2, 5, 512, 512, 64, "packed"), (T.PP, 32, 5, 1024, 1024, 64, "packed"), (T.K64, 2, 5, 256, 77, 64, "kv"),
              (T.K128, 2, 4, 256, 77, 128, "separate"), (T.K512, 1, 2, 64, 77, 512, "separate")]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kernel,B,H,Tq,Tk,D,layout", OPS_SHAPES, ids=[f"{s[0]}_b{s[1]}" for s in OPS_SHAPES])
def test_ops_attention_gives_the_bits_of_the_raw_call(capi, kernel, B, H, Tq, Tk, D, layout, dtype):
    from unirestore_amd import ops
    dt = DTYPES[dtype]
    C = H * D
    gen = torch.Generator().manual_seed(Tq + Tk + D)
    shared = layout == "kv"
    nb = 1 if shared else B
    ldvt = (Tk + 7) // 8 * 8
    vt = torch.zeros(nb, C, ldvt, dtype=dt)
    vt[:, :, :Tk] = torch.randn(nb, C, Tk, generator=gen).to(dt)
    vt = vt.cuda()
    if layout == "packed":
        qkv = torch.randn(B, Tq, 3 * C, generator=gen).to(dt).cuda()
        q, k, ldq, ldk = qkv, qkv[:, :, C:], 3 * C, 3 * C
    else:
        q = torch.randn(B, Tq, C, generator=gen).to(dt).cuda()
        ldk = 2 * C if shared else C
        k = torch.randn(nb, Tk, ldk, generator=gen).to(dt).cuda()
        ldq = C
    bs_q, bs_k, bs_vt = Tq * ldq, 0 if shared else Tk * ldk, 0 if shared else C * ldvt
    scale = 1.0 / math.sqrt(D)
    o_ops = ops.attention(q, k, vt, H, D, Tq, Tk, scale, ldq=ldq, ldk=ldk, bs_q=bs_q, bs_k=bs_k, bs_vt=bs_vt, batch=B)
    nws = capi.lib.ur_attention_workspace_bytes(B, H, Tq, Tk, D)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device="cuda")
    o_raw = _nan((B, Tq, C), dt)
    args = (q.data_ptr(), k.data_ptr(), vt.data_ptr(), o_raw.data_ptr(), B, H, Tq, Tk, D, ldq, ldk, ldvt, C, bs_q, bs_k, bs_vt, Tq * C,
            ws.data_ptr() if nws else None, nws)
    plan = capi.attention_plan(*args)
    assert capi.attention_kernel_names()[plan.kernel] == kernel and (plan.n_split > 0) == (nws > 0)
    capi.check(capi.lib.ur_attention_fwd_ws(*args[:17], scale, args[17], args[18], capi.UR_DT_F16 if dt == torch.float16 else capi.UR_DT_BF16,
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(_bits(o_ops), _bits(o_raw))


@pytest.fixture(params=list(DTYPES))
def ops_dt(request):
    """The op front end with the compute dtype under test selected (ops.softmax_rows writes the current compute dtype)."""
    from unirestore_amd import ops as o
    dt = o.set_dtype(request.param)
    yield o, dt
    o.set_dtype("bf16")


@pytest.mark.parametrize("heads,d", [(8, 40), (2, 96)])
@pytest.mark.parametrize("t", [256, 100])
def test_attention_gemm_matches_fp64(ops_dt, heads, d, t):
    """modules/nn.py attention_gemm (head dims other than 64 / 128 / 512): bmm_nt on strided views of the fused QKV output +
    softmax_rows with ldp = ldvt + bmm_nt against V^T.  P is rounded to 16 bits between two GEMMs: the 2 x GEMM tolerance of
    tests/test_ops_gpu.py test_attention for the whole tensor, 10 x that for every (row, head) separately."""
    ops, dt = ops_dt
    from unirestore_amd.modules import nn as unn
    b, c = 2, heads * d
    gen = torch.Generator().manual_seed(heads * 1000 + d + t)
    q, k, v = R.inputs("randn", "passed", b, heads, t, t, d, dt, gen)
    ldvt = ops.round_up(t, 8)
    qk = torch.cat([q, k, torch.full_like(q, float("nan"))], -1).to(dt).cuda()      # [B][T][3C]: the V third is never read
    vt = torch.zeros(b, c, ldvt, dtype=dt)
    vt[:, :, :t] = v.transpose(1, 2).to(dt)
    o = unn.attention_gemm(qk[:, :, :c], qk[:, :, c:2 * c], vt.cuda(), heads, d, t)
    torch.cuda.synchronize()
    assert o.shape == (b, t, c) and o.dtype == dt and bool(torch.isfinite(o).all())
    ref, _ = R.reference(q.cuda(), k.cuda(), v.cuda(), heads, d, 1.0 / math.sqrt(d), dt, False)
    tol = 2 * (3e-3 if dt == torch.bfloat16 else 4e-4)
    rel = R.rel_l2(o, ref)
    err = (o.double() - ref).view(b, t, heads, d).norm(dim=-1) / ref.view(b, t, heads, d).norm(dim=-1).clamp_min(1e-3)
    print(f"attention_gemm heads {heads} d {d} t {t} {dt}: rel-L2 {rel:.3e}, worst row {float(err.max()):.3e}")
    assert rel < tol
    assert float(err.max()) < 10 * tol
