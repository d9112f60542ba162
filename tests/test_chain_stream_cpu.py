"""CPU-side checks of the fused chains (csrc/tchain.hip): the packers of unirestore_amd/chain.py against the read-side decoder of
tests/chain_reference.py, the launchers' argument checks (tests/chain_cases.py REFUSALS), and the per-element bound of
chain_reference re-established on a CPU emulation of the kernels' arithmetic: valid (the emulation of every launched case stays
inside it, in both types) and sharp (six mutations of the emulation leave it; a k tile scaled by 1.05 does so under the whole-tensor
rel-L2 tolerance of tests/test_chain_gpu.py)."""
import functools

import pytest
import torch

import chain_cases as T
import chain_reference as R
from conv_reference import U_OUT, compare, compare_sums
from unirestore_amd import capi, chain

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
RESIDUAL = {T.MLP: "x", T.CSCE: "x", T.TAIL: "xres"}      # rel-L2 is taken on the branch y - residual, as tests/test_chain_gpu.py does
RESOLVED = {}                   # (input kind, dtype) -> [median over elements of bound / (u_out * max(|ref|, rms(ref)))] per case


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RESOLVED:
        print("\nmedian over elements of bound / (u_out * max(|ref|, rms ref)), per input kind (range over its cases):")
        for (kind, dt), v in sorted(RESOLVED.items()):
            print(f"  {kind:10s} {dt}: {min(v):.2f} .. {max(v):.2f}")


@functools.lru_cache(maxsize=None)
def _case(cid, dtype):
    """(case, master weights + inputs, stream, decoded stream, used-word mask) of a case, built once"""
    c, dt = T.BY_ID[cid], DTYPES[dtype]
    m = R.make(c, dt)
    st = R.pack(c, m, dt, "cpu")
    dec, used = R.decode(c["kernel"], st, dt, c["hidden"])
    return c, m, st, dec, used


@functools.lru_cache(maxsize=None)
def _reference(cid, dtype):
    c, m, _, dec, _ = _case(cid, dtype)
    return R.reference(c, dec, R.inputs_of(c, m), DTYPES[dtype])


def _same(a, b):
    return a.shape == b.shape and bool((a.double() == b.double()).all())


def _folded(w, b, g, be, dt):
    """what a LayerNorm-folded stage must hold: dt(W gamma), W beta + b, the column sums of the ROUNDED weights"""
    wf = w * g[None, :]
    return wf.to(dt), w @ be + (b if b is not None else 0.0), wf.to(dt).float().sum(1)


# ---- packers vs the read-side decoder --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("cid", ["mlp_h64", "mlp_h192", "head_1x128", "tail_tk77", "tail_tk1", "tail_tk80", "csce_1x128"])
def test_packed_stream_decodes_to_the_weights(cid, dtype):
    c, m, st, dec, used = _case(cid, dtype)
    dt, k, hid = DTYPES[dtype], c["kernel"], c["hidden"]
    assert st.dtype == torch.uint8 and st.numel() == T.ntiles(c) * chain.TILE and chain.TILE == R.TILE == capi.lib.ur_chain_tile_bytes()
    assert T.ntiles(c) == {T.MLP: 3 * hid // 64, T.HEAD: 20, T.TAIL: 25 + 3 * hid // 64, T.CSCE: 14}[k]
    assert bool((st.view(torch.int16)[~used] == 0).all()), "bytes the layout leaves unused are not zero"
    if k in (T.MLP, T.TAIL):
        w, b, cs = _folded(m["ff1_w"], m["ff1_b"], m["ln3_g"], m["ln3_b"], dt)
        assert _same(dec["ff1_w"], w) and _same(dec["ff1_b"], b) and _same(dec["ff1_cs"], cs)
        assert _same(dec["ff2_w"], m["ff2_w"].to(dt)) and _same(dec["ff2_b"], m["ff2_b"])
    if k == T.HEAD:
        assert _same(dec["in_w"], m["in_w"].to(dt)) and _same(dec["in_b"], m["in_b"])
        for n in ("q", "k", "v"):
            w, b, cs = _folded(m[n + "_w"], None, m["ln1_g"], m["ln1_b"], dt)
            assert _same(dec[n + "_w"], w) and _same(dec[n + "_b"], b) and _same(dec[n + "_cs"], cs), n
    if k == T.CSCE:
        for n in ("proj", "t0", "t2"):
            assert _same(dec[n + "_w"], m[n + "_w"].to(dt)) and _same(dec[n + "_b"], m[n + "_b"]), n
        assert dec["proj_w"].shape == (T.C, T.CCOND)
    if k == T.TAIL:
        for n in ("o1", "o2", "out"):
            assert _same(dec[n + "_w"], m[n + "_w"].to(dt)) and _same(dec[n + "_b"], m[n + "_b"]), n
        w, b, cs = _folded(m["q2_w"], None, m["ln2_g"], m["ln2_b"], dt)
        assert _same(dec["q2_w"], w) and _same(dec["q2_b"], b) and _same(dec["q2_cs"], cs)
        tk = c["tk"]
        ctx16 = m["ctx"].to(dt).float()
        kc = (ctx16 @ m["k2_w"].to(dt).float().t()).to(dt)                       # [tk][320]
        vc = (ctx16 @ m["v2_w"].to(dt).float().t()).to(dt)
        assert dec["K"].shape == (T.HEADS, 96, 64) and dec["VT"].shape == (T.HEADS, 64, 128)
        for hd in range(T.HEADS):
            sl = slice(64 * hd, 64 * hd + 64)
            assert _same(dec["K"][hd, :tk], kc[:, sl]) and bool((dec["K"][hd, tk:] == 0).all()), hd
            assert _same(dec["VT"][hd, :, :tk], vc[:, sl].t()) and bool((dec["VT"][hd, :, tk:] == 0).all()), hd


# ---- argument checks (host side: nothing is launched) --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refusal_ptrs():
    """Buffers of a refusal call.  Without a GPU the addresses are placeholders (a refused call never touches them, and a wrongly
    accepted one cannot launch); with one they are real allocations of the size chain_cases documents, and a NULL row whose
    pointer check is broken is refused by the next check (chain_cases.py), never launched."""
    names = sorted({p for k in T.KERNELS for p in T.POINTERS[k]} | {"gn_part"})
    if torch.cuda.is_available():
        keep = {n: torch.zeros(max(T.REFUSAL_T * T.REFUSAL_LD * 2, T.REFUSAL_TILES * R.TILE), dtype=torch.uint8, device="cuda") for n in names}
        yield {n: t.data_ptr() for n, t in keep.items()}
    else:
        yield {n: (i + 1) << 24 for i, n in enumerate(names)}


@pytest.mark.parametrize("dt", [capi.UR_DT_BF16, capi.UR_DT_F16], ids=list(DTYPES))
@pytest.mark.parametrize("row", T.REFUSALS, ids=[r[0] for r in T.REFUSALS])
def test_refusals(row, dt, refusal_ptrs):
    assert (T.INVALID, T.UNSUPPORTED) == (capi.UR_E_INVALID, capi.UR_E_UNSUPPORTED)
    symbol, args, code = T.refusal_call(row, refusal_ptrs, dt, R.TILE)
    assert getattr(capi.lib, symbol)(*args) == code, (row[0], capi.lib.ur_last_error())


def test_refusal_table_covers_the_argument_checks():
    ids = {r[0] for r in T.REFUSALS}
    for k in T.KERNELS:
        assert {f"{k}_c256", f"{k}_t0", f"{k}_t100", f"{k}_stream_short"} <= ids
        assert {f"{k}_null_{p}" for p in T.POINTERS[k]} <= ids
    assert {"tail_heads4", "tail_tk0", "tail_tk81", "csce_ccond128", "mlp_ldx324", "mlp_ldx312", "mlp_hidden0", "mlp_hidden96"} <= ids


# ---- the bound is valid: the emulation of every launched case stays inside it ---------------------------------------------------------
def _check(c, outs, ref, dtype, what):
    """every output of an emulated / mutated run against the staged reference; returns the worst ratio"""
    worst = 0.0
    for name, (r, b) in ref.items():
        worst = max(worst, compare(outs[name].double(), r, b, f"{what} {name}"))
    return worst


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("cid", [c["id"] for c in T.CASES])
def test_emulation_inside_the_bound(cid, dtype):
    c, m, _, dec, _ = _case(cid, dtype)
    dt = DTYPES[dtype]
    ref, info = _reference(cid, dtype)
    outs = R.emulate(c, dec, R.inputs_of(c, m), dt)
    worst = _check(c, outs, ref, dtype, f"{cid} [{dtype}]")
    if "gn_part" in outs:
        g = outs["gn_part"].double()
        worst = max(worst, compare_sums(g[..., 0], g[..., 1], R.gn_terms(outs["y"], c), T.TOK, f"{cid} [{dtype}] gn_part"))
    r, b = ref["y"] if "y" in ref else ref["q"]
    res = float((b / (U_OUT[dt] * torch.maximum(r.abs(), r.pow(2).mean().sqrt()))).median())
    RESOLVED.setdefault((c["kind"], dtype), []).append(res)
    print(f"{cid} [{dtype}]: worst |emulation - ref| / bound {worst:.3f}, median bound {res:.2f} output ulps")
    # the properties the input kinds promise, on the staged reference
    if c["kind"] == "offset":
        assert info["ln_ratio"] and all(float(x.min()) >= 6.0 for x in info["ln_ratio"]), [float(x.min()) for x in info["ln_ratio"]]
    if c["kind"] == "peaked":
        rows = (info["w_max"] >= 0.9) & info["p_subnormal"]
        assert float(rows.double().mean()) >= 0.25, float(rows.double().mean())
    if c["kind"] == "gelu_tail":
        g = info["gate"]
        assert float(g.min()) < -6 and float(g.max()) > 6 and float(((g > -6) & (g < -3)).double().mean()) > 0.1


# ---- the bound is sharp ----------------------------------------------------------------------------------------------------------------
def _mutation(name, cid, dtype):
    c, m, _, dec, _ = _case(cid, dtype)
    if name == "colsum_unrounded":                       # column sums of the unrounded w * gamma
        return ("colsum_unrounded", "ff1", (m["ff1_w"] * m["ln3_g"][None, :]).sum(1))
    return {"no_swap23": ("no_swap23", "t0", 3), "key_mask": ("key_mask",), "no_bias": ("no_bias", "in"),
            "neighbour_image": ("neighbour_image",), "ktile_scale": ("ktile_scale", "ff2", 7, 1.05)}[name]


# (mutation, case, dtypes in which the whole-tensor rel-L2 of tests/test_chain_gpu.py must still pass).  The unrounded column sums do
# NOT hide under that tolerance at |mean| >= 6 std: the column sum is off by the summed rounding errors of 320 weights, ~1.1e-3 of
# the row's norm in bf16, times |mean| / std - 1.1e-2 .. 1.4e-2 on HEAD's q / k / v, 2.7e-2 on the MLP branch (6e-3 allowed), and
# 1.5e-3 / 3.4e-3 in fp16 (8e-4).
# GAP, not closed here: behind TAIL's residuals the same mutation (q2 / FF1 column sums) does hide under the tolerance (5.6e-3) and
# the staged bound, 3-4 output ulps wide there, does not see it either (0 elements outside).  TAIL stores none of its intermediates,
# so no check from the kernel's own values (as reference_from_h0 does for HEAD) is possible; what pins TAIL's column sums is the
# packer test above (they must be the sums of the ROUNDED weights, bit for bit) and the MLP / HEAD offset cases, which run the same
# fold_ln and the same epilogue code.
MUTATIONS = [("colsum_unrounded", "mlp_t256_offset", ()), ("no_swap23", "csce_1x128", ()), ("key_mask", "tail_tk9", ()),
             ("no_bias", "head_1x128", ()), ("neighbour_image", "head_3x128_per_image", ()), ("ktile_scale", "tail_h1280_tk77", ("bf16",))]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name,cid,l2_passes", MUTATIONS, ids=[x[0] for x in MUTATIONS])
def test_mutation_leaves_the_bound(name, cid, l2_passes, dtype):
    c, m, _, dec, _ = _case(cid, dtype)
    dt = DTYPES[dtype]
    ref, _ = _reference(cid, dtype)
    outs = R.emulate(c, dec, R.inputs_of(c, m), dt, fault=_mutation(name, cid, dtype))
    outside = sum(int((~((outs[n].double() - r).abs() <= b)).sum()) for n, (r, b) in ref.items())
    total = sum(r.numel() for r, _ in ref.values())
    rels = []
    for n, (r, _) in ref.items():
        res = m[RESIDUAL[c["kernel"]]].double() if n == "y" else 0.0
        rels.append(R.rel_l2(outs[n].double() - res, r - res))
    print(f"{name} on {cid} [{dtype}]: {outside} of {total} elements outside the bound, rel-L2 {max(rels):.2e} (tolerance {R.REL_TOL[dt]:.0e})")
    assert outside > 0
    with pytest.raises(AssertionError):
        _check(c, outs, ref, dtype, name)
    if dtype in l2_passes:
        assert max(rels) < R.REL_TOL[dt], "the mutation was meant to hide under the whole-tensor tolerance"
