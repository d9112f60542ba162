"""Every fused chain kernel (csrc/tchain.hip: ur_ff_geglu_fused, ur_transformer_head_fused, ur_transformer_tail_fused, ur_csce_fused)
against a staged fp64 reference, element by element (-m gpu, bf16 and fp16).

The cases are tests/chain_cases.py; the stream decoder, the reference and the per-element bound, with its derivation, are
tests/chain_reference.py (the one statement of the bound: this module only applies it).

Each case calls the C ABI with raw pointers and
  * gives every input NaN guard rows behind T (and NaN row gaps where ldx > C);
  * NaN-prefills every output (y, h0, q, k, vt, gn_part) with guard rows / planes behind it and padding columns where ldy > C: outputs
    must be finite, guards and padding must come back bit-unchanged;
  * puts a NaN guard tile behind the weight stream and passes stream_bytes exactly (past its end the ring re-fetches the LAST tile:
    a fetch of the tile behind it would bring NaN into the ring);
  * runs twice into fresh buffers and requires bit-identical outputs; where the case says gn = "both", also with gn_part = NULL, and
    y must not change by a bit;
  * checks every element against the bound, the whole tensor against the rel-L2 tolerances of tests/test_chain_gpu.py (on the
    branch y - residual, as there; on y itself where the residual is the offset input of MLP), V^T in its own
    [N][320][tokens per image] layout, HEAD's q / k / v also against the fp64 fold of the kernel's own h0, and the GroupNorm
    partial planes with compare_sums per (image, part, channel).
"""
import pytest
import torch

import chain_cases as T
import chain_reference as R
from conv_reference import compare, compare_sums

pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
GUARD = 3                       # guard rows behind every input and output, guard planes behind gn_part
RESIDUAL = {T.MLP: "x", T.CSCE: "x", T.TAIL: "xres"}
OUTPUTS = {T.MLP: ("y",), T.HEAD: ("h0", "q", "k", "vt"), T.TAIL: ("y",), T.CSCE: ("y",)}
WORST = {}                      # (kernel, dtype) -> largest |y - ref| / bound seen (printed at the end of the module)


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    yield c
    if WORST:
        print("\nlargest |y - ref| / bound per chain kernel:")
        for (name, dt), r in sorted(WORST.items()):
            print(f"  {T.SYMBOL[name]:28s} {dt}: {r:.3f}")


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _rows(v, dt, ld=None):
    """[T][w] values -> NaN buffer [T + GUARD][ld] holding them"""
    ld = v.shape[1] if ld is None else ld
    b = _nan((v.shape[0] + GUARD, ld), dt)
    b[:v.shape[0], :v.shape[1]] = v.to(dt).cuda()
    return b


def _launch(capi, c, dt, inp, stream, gn):
    """one launch into fresh NaN buffers -> {output name: its region of the buffer} after the guard checks"""
    k, N, hw, tt = c["kernel"], c["N"], c["hw"], c["T"]
    what = f"{c['id']} [{dt}]"
    bufs = {n: _rows(v, dt, c["ldx"] if k == T.MLP else None) for n, v in inp.items() if n != "ab"}
    if "ab" in inp:
        bufs["ab"] = torch.cat([inp["ab"].cuda().reshape(-1), _nan((2 * T.C,), torch.float32)])
    outs = {n: _nan((tt + GUARD, c["ldy"] if k == T.MLP else T.C), dt) for n in OUTPUTS[k] if n != "vt"}
    if k == T.HEAD:
        outs["vt"] = _nan((N * T.C + GUARD, hw), dt)
    parts = hw // T.TOK
    if gn:
        outs["gn_part"] = _nan((N * parts + GUARD, T.C, 2), torch.float32)
    ptr = {n: t.data_ptr() for n, t in {**bufs, **outs}.items()}
    ptr["stream"] = stream.data_ptr()
    args = T.call_args(k, T.launch_ints(c), ptr, capi.UR_DT_F16 if dt == torch.float16 else capi.UR_DT_BF16, T.ntiles(c) * R.TILE,
                       torch.cuda.current_stream().cuda_stream, R.LN_EPS, c["scale"])
    capi.check(getattr(capi.lib, T.SYMBOL[k])(*args))
    torch.cuda.synchronize()
    nanbits = {t.dtype: _bits(_nan((1,), t.dtype))[0] for t in outs.values()}
    res = {}
    for n, t in outs.items():
        rows = {"vt": N * T.C, "gn_part": N * parts}.get(n, tt)
        cols = T.C if t.dim() == 2 and n != "vt" else t.shape[1]
        keep = torch.ones_like(t, dtype=torch.bool)
        keep[:rows, :cols] = False
        assert bool((_bits(t)[keep] == nanbits[t.dtype]).all()), f"{what} {n}: write outside the output (guard rows / padding columns)"
        res[n] = t[:rows, :cols]
        assert bool(torch.isfinite(res[n]).all()), f"{what} {n}: output not finite"
    return res


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.CASES, ids=[c["id"] for c in T.CASES])
def test_chain_parity(capi, c, dtype):
    dt = DTYPES[dtype]
    k, N, hw = c["kernel"], c["N"], c["hw"]
    m = R.make(c, dt)
    st = R.pack(c, m, dt, "cpu")
    dec, _ = R.decode(k, st, dt, c["hidden"])
    inp = R.inputs_of(c, m)
    stream = torch.cat([st, torch.full((R.TILE // 4,), float("nan")).view(torch.uint8)]).cuda()        # + a NaN guard tile
    gn = k in (T.TAIL, T.CSCE) and c["gn"] != "no"
    what = f"{c['id']} [{dtype}]"
    o1 = _launch(capi, c, dt, inp, stream, gn)
    o2 = _launch(capi, c, dt, inp, stream, gn)
    for n in o1:
        assert torch.equal(_bits(o1[n]), _bits(o2[n])), f"{what} {n}: not bit-identical between two runs"
    if c["gn"] == "both" and k in (T.TAIL, T.CSCE):
        o3 = _launch(capi, c, dt, inp, stream, False)
        assert torch.equal(_bits(o1["y"]), _bits(o3["y"])), what + ": y differs between gn_part given and NULL"
    ref, _ = R.reference(c, {n: v.cuda() for n, v in dec.items()}, {n: v.cuda() for n, v in inp.items()}, dt)
    worst = 0.0
    try:
        for n, (r, b) in ref.items():
            if n == "v":                                                  # V^T in its own layout [N][320][tokens per image]
                got = o1["vt"].double().view(N, T.C, hw)
                r, b = (z.view(N, hw, T.C).transpose(1, 2) for z in (r, b))
            else:
                got = o1[n].double()
            # rel-L2 on the branch y - residual as tests/test_chain_gpu.py takes it; not where the residual carries the offset (MLP,
            # "offset": |x| = 8 x the branch, the one rounding of y alone is 2e-2 of the branch in bf16) - there on y itself
            res = inp[RESIDUAL[k]].cuda().double() if n == "y" and not (k == T.MLP and c["kind"] == "offset") else 0.0
            rel = R.rel_l2(got - res, r - res)
            ratio = float(((got - r).abs() / b.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
            print(f"{what} {n}: worst |y - ref| / bound {ratio:.3f}, rel-L2 {rel:.3e}")
            worst = max(worst, compare(got, r, b, f"{what} {n}"))
            assert rel < R.REL_TOL[dt] / (2 if n == "h0" else 1), f"{what} {n}"
        if k == T.HEAD:                                                   # q / k / v from the kernel's own h0: no ambiguity term
            own = R.reference_from_h0({n: v.cuda() for n, v in dec.items()}, o1["h0"].double(), dt)
            for n, (r, b) in own.items():
                got = o1["vt"].double().view(N, T.C, hw).transpose(1, 2).reshape(-1, T.C) if n == "v" else o1[n].double()
                worst = max(worst, compare(got, r, b, f"{what} {n} from the kernel's h0"))
        if gn:
            g = o1["gn_part"].double().view(N, hw // T.TOK, T.C, 2)
            worst = max(worst, compare_sums(g[..., 0], g[..., 1], R.gn_terms(o1["y"], c), T.TOK, what + " gn_part"))
    finally:
        WORST[(k, dtype)] = max(WORST.get((k, dtype), 0.0), worst)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("row", T.REFUSALS, ids=[r[0] for r in T.REFUSALS])
def test_refusals_on_device_buffers(capi, row, dt):
    """The argument checks with real device buffers behind the pointers (sized so that a wrongly accepted call stays inside them; a
    NULL row is refused by the next check if the pointer check lets it through: chain_cases.py)."""
    names = sorted({p for k in T.KERNELS for p in T.POINTERS[k]} | {"gn_part"})
    keep = {n: torch.zeros(max(T.REFUSAL_T * T.REFUSAL_LD * 2, T.REFUSAL_TILES * R.TILE), dtype=torch.uint8, device="cuda") for n in names}
    symbol, args, code = T.refusal_call(row, {n: t.data_ptr() for n, t in keep.items()}, capi.UR_DT_F16 if dt == "fp16" else capi.UR_DT_BF16, R.TILE)
    assert getattr(capi.lib, symbol)(*args) == code, (row[0], capi.lib.ur_last_error())
    torch.cuda.synchronize()
