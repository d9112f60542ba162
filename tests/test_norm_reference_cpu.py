"""CPU gate of the norm / per-channel kernel parity matrix (tests/norm_cases.py, tests/norm_reference.py): nothing here needs a GPU.

  * the pure-Python mirror of gn_geom against ur_groupnorm_stats_parts / ur_groupnorm_ws_bytes, over a sweep of shapes and at the
    literal P of every GroupNorm case;
  * every property listed in norm_cases.PROPERTIES is held by at least one launched case;
  * the refusal table: every row returns UR_E_INVALID on the host (placeholder pointers, nothing is launched);
  * the numpy fp32 emulation of every family satisfies the per-element bound on every case, in both 16-bit types;
  * every mutation of norm_reference.MUTATIONS fails the element bound on at least one case; whether the whole-tensor rel-L2
    tolerance of tests/test_ops_gpu.py would have caught it is recorded (printed: the table of DESIGN.md 6m).
The five grid-stride cases (BIG_CASES) are launched on the GPU only; their reference runs on the device.
"""
import pytest
import torch

import norm_cases as T
import norm_reference as R

DTYPES = R.DTYPES


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    return c


def test_geometry_mirror_matches_the_library(capi):
    lib = capi.lib
    for N in (1, 2, 3, 8, 64):
        for HW in (1, 16, 63, 64, 65, 256, 300, 361, 1021, 1024, 4096, 10000, 16384):
            for C in (8, 64, 96, 128, 192, 296, 320, 640, 1280, 1920, 2560):
                assert lib.ur_groupnorm_stats_parts(N, HW, C) == T.stats_parts(N, HW, C), (N, HW, C)
                assert lib.ur_groupnorm_ws_bytes(N, HW, C) == T.ws_bytes(N, HW, C), (N, HW, C)
                cvs, slabs, Rr, chunks, ppb, last = T.gn_geom(N, HW, C, 2)
                assert (C // 8) % cvs == 0 and cvs * Rr <= 256 and (chunks - 1) * ppb < HW <= chunks * ppb and 0 < last <= ppb
    for c in T.GN_CASES:
        for C, P in ((c["C1"], c["P"]), (c["C2"], c["P2"])):
            if C:
                assert lib.ur_groupnorm_stats_parts(c["N"], c["HW"], C) == P == T.stats_parts(c["N"], c["HW"], C), c["id"]
                assert lib.ur_groupnorm_ws_bytes(c["N"], c["HW"], C) == c["N"] * P * C * 8, c["id"]
        assert lib.ur_groupnorm_ab_bytes(c["N"], c["C1"] + c["C2"]) == c["N"] * (c["C1"] + c["C2"]) * 8
    for fn, args, want in T.QUERY_REFUSALS:
        assert getattr(lib, fn)(*args) == want, (fn, args)


def test_every_property_is_held_by_a_launched_case():
    for cases, props in T.PROPERTIES:
        for name, holds in props.items():
            assert any(holds(c) for c in cases), f"no case with: {name}"
    ids = [c["id"] for cases in (T.GN_CASES, T.FINALIZE_CASES, T.NHWC_CASES, T.LN_CASES, T.SOFTMAX_CASES, T.DWCONV_CASES, T.SCALE_CASES,
                                 T.FANOUT_CASES, T.AXPY_CASES, T.SPADE_CASES, T.LINEAR_CASES, T.TFA_CASES, T.TFA_FANOUT_CASES, T.VMG_CASES,
                                 T.BIG_CASES) for c in cases]
    assert len(ids) == len(set(ids))
    assert sum(c["avgpool"] for c in T.GN_CASES) >= 3
    # the shape lists, literally
    assert {(c["rows"], c["C"]) for c in T.LN_CASES} >= {(1, 8), (15, 64), (16, 320), (17, 512), (33, 520), (5, 1280), (4, 1536), (3, 1544), (2, 2048)}
    assert {(c["rows"], c["cols"], c["ldp"]) for c in T.SOFTMAX_CASES} >= {(3, 1, 8), (2, 77, 77), (2, 77, 80), (5, 255, 256), (4, 256, 256),
                                                                            (3, 257, 264), (2, 333, 336), (2, 1029, 1032)}
    assert {(c["N"], c["H"], c["W"], c["C"], c["gate"]) for c in T.DWCONV_CASES} >= {(2, 1, 1, 8, 0), (1, 3, 4, 16, 1), (2, 5, 8, 64, 1), (2, 9, 11, 64, 0),
                                                                                    (2, 9, 11, 64, 1), (1, 1, 12, 8, 0), (1, 6, 1, 8, 0), (3, 4, 5, 24, 0)}
    assert {(c["M"], c["N"], c["K"], c["groups"], c["act"]) for c in T.LINEAR_CASES} >= {
        (1, 1, 1, 1, T.ACT_NONE), (9, 5, 257, 1, T.ACT_GELU), (50, 1280, 320, 1, T.ACT_SILU), (17, 8, 1280, 1, T.ACT_TANH), (5, 96, 96, 4, T.ACT_NONE),
        (8, 6, 520, 2, T.ACT_RELU)}
    assert {(c["B"], c["T"], c["D"]) for c in T.TFA_CASES} >= {(2, 2, 48), (1, 1, 256), (2, 3, 300), (1, 4, 768)}
    assert {(c["N"], c["C"], c["G"]) for c in T.VMG_CASES} >= {(2, 64, 4), (1, 8, 8), (3, 96, 1)}
    assert {c["K"] for c in T.FANOUT_CASES} >= {1, 3, 8} and any(not c["s"] for c in T.FANOUT_CASES)
    assert {(c["K"], c["cpr"]) for c in T.TFA_FANOUT_CASES} >= {(1, 0), (3, 0), (3, 1), (1, 1)}
    for c in T.BIG_CASES:                       # just over one grid of 8192 x 256 threads: the second trip is short
        assert T.GRID_THREADS < T.big_threads(c) < 1.02 * T.GRID_THREADS, c["id"]


REFUSALS = T.refusals()


@pytest.mark.parametrize("fn,args", [(r[1], r[2]) for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusal(capi, fn, args):
    """One wrong argument in an otherwise valid call: UR_E_INVALID from the host-side check, with the entry point's name in the message."""
    assert getattr(capi.lib, fn)(*args) == capi.UR_E_INVALID, (fn, args)
    msg = capi.lib.ur_last_error().decode()
    assert msg.startswith("ur_"), msg


def test_refusal_table_names_the_parent_crashes():
    rows = {r[0] for r in REFUSALS}
    assert {"vec_mul_group:G=0", "groupnorm_apply_act:C1=0", "groupnorm_nhwc:C1=0", "layernorm_rows:C=2056", "layernorm_rows:C=0",
            "softmax_rows_f32:dtype=7", "scale_channels:N=0", "axpy_channels:rows=0", "dwconv3x3_nhwc:N=0", "vec_mul_group:N=0"} <= rows


# ---- the emulation satisfies the bound -------------------------------------------------------------------------------------------------
WORST = {}


def _note(family, dtype, r):
    WORST[(family, dtype)] = max(WORST.get((family, dtype), 0.0), r)
    assert r <= 1.0, (family, dtype, r)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.GN_CASES, ids=[c["id"] for c in T.GN_CASES])
def test_emulated_groupnorm_within_bound(c, dtype):
    dt = DTYPES[dtype]
    x1, x2, gamma, beta = R.gn_inputs(c, dt)
    ref = R.gn_reference(x1, x2, gamma, beta, c["G"], c["silu"], dt)
    y, pl1, pl2, ab, mean = R.emu_groupnorm(x1, x2, gamma, beta, c["G"], c["silu"], dt)
    assert pl1.shape[1] == c["P"] and (pl2 is None or pl2.shape[1] == c["P2"])
    planes = [torch.from_numpy(p) for p in (pl1, pl2) if p is not None]
    for name, r in R.gn_check(ref, y, planes, torch.from_numpy(ab), torch.from_numpy(mean), c["id"]).items():
        _note("groupnorm " + name, dtype, r)
    assert R.rel_l2(y, ref["y"]) < R.REL_TOL[dt]


@pytest.mark.parametrize("c", T.FINALIZE_CASES, ids=[c["id"] for c in T.FINALIZE_CASES])
def test_emulated_finalize_within_bound(c):
    p1, p2, gamma, beta = R.finalize_inputs(c)
    ref = R.finalize_reference(p1, p2, gamma, beta, c["G"], c["HW"])
    ab, mean = R.emu_gn_finalize(p1.numpy(), None if p2 is None else p2.numpy(), gamma, beta, c["G"], c["HW"])
    for name, r in R.gn_check(ref, None, None, torch.from_numpy(ab), torch.from_numpy(mean), c["id"]).items():
        _note("finalize " + name, "fp32", r)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.LN_CASES, ids=[c["id"] for c in T.LN_CASES])
def test_emulated_layernorm_within_bound(c, dtype):
    dt = DTYPES[dtype]
    x, gamma, beta = R.ln_inputs(c, dt)
    ref, bnd = R.ln_reference(x, gamma, beta, dt)
    _note("layernorm", dtype, R.compare(R.emu_layernorm(x, gamma, beta, dt).double(), ref, bnd, c["id"]))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", T.SOFTMAX_CASES, ids=[c["id"] for c in T.SOFTMAX_CASES])
def test_emulated_softmax_within_bound(c, dtype):
    dt = DTYPES[dtype]
    s = R.softmax_inputs(c)
    ref, bnd = R.softmax_reference(s, dt)
    p = R.emu_softmax(s, dt)
    _note("softmax", dtype, R.compare(p.double(), ref, bnd, c["id"]))
    if c["kind"] == "subnormal" and dt == torch.float16:
        small = ref[0] < 2.0 ** -14
        assert int(small.sum()) >= c["cols"] - 1 and bool((p[0][small] > 0).any()), "the case must reach fp16 subnormal probabilities"
    if c["std"] == 30:
        assert bool((p == 0).any()) and float(ref.max()) > 0.9, "the case must have peaked rows and exact zeros"


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_emulated_elementwise_within_bound(dtype):
    dt = DTYPES[dtype]
    for c in T.DWCONV_CASES:
        x, w, b = R.dwconv_inputs(c, dt)
        ref, bnd = R.dwconv_reference(x, w, b, c["gate"], dt)
        _note("dwconv", dtype, R.compare(R.emu_dwconv(x, w, b, c["gate"], dt).double(), ref, bnd, c["id"]))
    for c in T.SCALE_CASES:
        g = R.gen_of(c["id"])
        x = torch.randn(c["N"], c["HW"], c["C"], generator=g).to(dt)
        s = torch.randn(c["N"], c["C"], generator=g)
        r = torch.randn(c["N"], c["HW"], c["C"], generator=g).to(dt) if c["res"] else None
        ref, bnd = R.scale_reference(x, s, r, dt)
        _note("scale_channels", dtype, R.compare(R.emu_scale(x, s, r, dt).double(), ref, bnd, c["id"]))
    for c in T.AXPY_CASES:
        g = R.gen_of(c["id"])
        a, b = (torch.randn(c["rows"], c["C"], generator=g).to(dt) for _ in range(2))
        s = torch.randn(c["C"], generator=g)
        ref, bnd = R.axpy_reference(a, b, s, dt)
        _note("axpy_channels", dtype, R.compare(R.emu_axpy(a, b, s, dt).double(), ref, bnd, c["id"]))
    for c in T.SPADE_CASES:
        g = R.gen_of(c["id"])
        n = torch.randn(c["rows"], c["C"], generator=g).to(dt)
        gb = torch.randn(c["rows"], 2 * c["C"] + c["pad"], generator=g).to(dt)
        r = torch.randn(c["rows"], c["C"], generator=g).to(dt) if c["res"] else None
        ref, bnd = R.spade_reference(n, gb, c["C"], r, dt)
        _note("spade_modulate", dtype, R.compare(R.emu_spade(n, gb, c["C"], r, dt).double(), ref, bnd, c["id"]))


def test_emulated_fp32_kernels_within_bound():
    for c in T.LINEAR_CASES:
        x, w, b = R.linear_inputs(c)
        ref, bnd = R.linear_reference(x, w, b, c["groups"], c["act"])
        _note("linear_f32", "fp32", R.compare(R.emu_linear(x, w, b, c["groups"], c["act"]).double(), ref, bnd, c["id"]))
    for c in T.TFA_CASES:
        pooled, cond = R.tfa_inputs(c)
        ref, bnd = R.tfa_reference(pooled, cond, c["T"], c["D"])
        _note("tfa_prompt_update", "fp32", R.compare(R.emu_tfa(pooled, cond, c["T"], c["D"]).double(), ref, bnd, c["id"]))
    for c in T.VMG_CASES:
        g = R.gen_of(c["id"])
        a, b = torch.randn(c["N"], c["C"], generator=g), torch.randn(c["N"], c["G"], generator=g)
        ref, bnd = R.vmg_reference(a, b, c["G"])
        _note("vec_mul_group", "fp32", R.compare(R.emu_vmg(a, b, c["G"]).double(), ref, bnd, c["id"]))


# ---- every mutation fails the element bound -----------------------------------------------------------------------------------------------
def _mutated_runs(name, dt):
    """(case id, {quantity: worst ratio}, rel-L2 of the output) of every case the mutation applies to."""
    fam = R.MUTATIONS[name][0]
    if fam == "groupnorm":
        for c in T.GN_CASES:
            if name == "source2_stride_c1" and not c["C2"]:
                continue
            x1, x2, gamma, beta = R.gn_inputs(c, dt)
            ref = R.gn_reference(x1, x2, gamma, beta, c["G"], c["silu"], dt)
            y, pl1, pl2, ab, mean = R.emu_groupnorm(x1, x2, gamma, beta, c["G"], c["silu"], dt, mutation=name)
            S = torch.cat([torch.from_numpy(p).double().sum(1) for p in (pl1, pl2) if p is not None], 1)
            yield c["id"], {"y": R.worst(y, ref["y"], ref["y_bnd"]), "ab": R.worst(torch.from_numpy(ab), ref["ab"], ref["ab_bnd"]),
                            "planes": max(R.worst(S[..., 0], ref["S"], ref["S_bnd"]), R.worst(S[..., 1], ref["Q"], ref["Q_bnd"]))}, R.rel_l2(y, ref["y"])
    elif fam == "layernorm":
        for c in T.LN_CASES:
            x, gamma, beta = R.ln_inputs(c, dt)
            ref, bnd = R.ln_reference(x, gamma, beta, dt)
            y = R.emu_layernorm(x, gamma, beta, dt, masked_lanes_add_mean2=True)
            yield c["id"], {"y": R.worst(y, ref, bnd)}, R.rel_l2(y, ref)
    else:
        for c in T.SOFTMAX_CASES:
            s = R.softmax_inputs(c)
            ref, bnd = R.softmax_reference(s, dt)
            y = R.emu_softmax(s, dt, three_waves=True)
            yield c["id"], {"y": R.worst(y, ref, bnd)}, R.rel_l2(y, ref)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(R.MUTATIONS))
def test_mutation_fails_the_element_bound(name, dtype):
    """Every mutation must leave the bound of some quantity (the output, or the ab table / the planes in their own units) on at least
    one case.  Printed next to it: on which cases the whole-tensor rel-L2 of tests/test_ops_gpu.py would have failed."""
    dt = DTYPES[dtype]
    caught, l2_caught, rows = [], [], []
    for cid, ratios, rel in _mutated_runs(name, dt):
        rows.append((cid, ratios, rel))
        if max(ratios.values()) > 1:
            caught.append(cid)
        if not rel < R.REL_TOL[dt]:
            l2_caught.append(cid)
    missed = [cid for cid in caught if cid not in l2_caught]
    print(f"\nmutation {name} [{dtype}]: a bound fails on {len(caught)} of {len(rows)} cases, rel-L2 < {R.REL_TOL[dt]:g} fails on {len(l2_caught)}; "
          f"caught by the bounds only: {missed}")
    for cid, ratios, rel in rows:
        print(f"    {cid:28s} " + "  ".join(f"{k} {v:9.3g}" for k, v in ratios.items()) + f"   rel-L2 {rel:.3e}")
    assert caught, f"{name}: no case fails a bound"
    assert not [cid for cid in l2_caught if cid not in caught], "rel-L2 fails where every element is inside its bound: the bound is too wide"


def test_print_worst_ratios():
    """Not a check of its own: prints what the tests above collected (run the module with -s)."""
    print("\nlargest |y - ref| / bound of the CPU emulation:")
    for (fam, dt), r in sorted(WORST.items()):
        print(f"  {fam:24s} {dt}: {r:.3f}")
