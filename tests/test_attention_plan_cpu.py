"""CPU-side checks of the attention family: the dispatch of ur_attention_fwd_ws seen through the host-only ur_attention_plan_launch over
the whole case table (tests/attention_cases.py), its argument checks, and the per-element bound of tests/attention_reference.py
re-established on a CPU emulation of the kernels' arithmetic."""
import os
import subprocess
import sys
import zlib

import pytest
import torch

import attention_cases as T
import attention_reference as R
from unirestore_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _plan(c, variant):
    p = capi.attention_plan(*T.plan_args(c, variant))
    return capi.attention_kernel_names()[p.kernel], p


def test_kernel_names():
    names = capi.attention_kernel_names()
    assert tuple(names) == T.KERNELS and capi.lib.ur_attention_kernel_count() == 4
    assert capi.lib.ur_attention_kernel_name(-1) is None and capi.lib.ur_attention_kernel_name(4) is None


@pytest.mark.parametrize("c", T.CASES, ids=[c["id"] for c in T.CASES])
def test_case_plans_as_the_table_says(c):
    assert len({x["id"] for x in T.CASES}) == len(T.CASES)
    assert capi.lib.ur_attention_workspace_bytes(c["B"], c["H"], c["Tq"], c["Tk"], c["D"]) == c["ws_tiles"] * 2 * 256 * 68 * 4
    assert ("exact" in c["plans"]) == (c["ws_tiles"] > 0) and "none" in c["plans"]
    for variant, (kernel, n_full, n_split) in c["plans"].items():
        name, p = _plan(c, variant)
        assert (name, p.n_full, p.n_split) == (kernel, n_full, n_split), (c["id"], variant)
        if name == T.PP:
            assert p.n_full + p.n_split == c["Tq"] // 256 * c["B"] * c["H"] and p.workgroups == p.n_full + 2 * p.n_split
            assert p.n_split in (0, c["ws_tiles"]) and (variant == "exact" or p.n_split == 0)
        else:
            per_wg = 32 if name == T.K512 else 128
            assert p.workgroups == (c["Tq"] + per_wg - 1) // per_wg * c["B"] * c["H"]


def test_table_reaches_every_kernel_and_three_splits():
    """Every kernel is the expected plan of at least three LAUNCHED cases, and the key split runs with three different n_split."""
    hits = {k: set() for k in T.KERNELS}
    splits = set()
    for c in T.LAUNCHED:
        for kernel, _, n_split in c["plans"].values():
            hits[kernel].add(c["id"])
            if n_split:
                splits.add(n_split)
    assert all(len(v) >= 3 for v in hits.values()), {k: len(v) for k, v in hits.items()}
    assert len(splits) >= 3, splits
    kinds = {c["kind"] for c in T.LAUNCHED}
    assert kinds == set(R.KINDS)
    assert {c["scale"] for c in T.LAUNCHED if T.PP in [p[0] for p in c["plans"].values()]} >= {"folded", "passed"}
    # the threshold pair of the fill rule and the workspace-less production shapes
    by_id = {c["id"]: c for c in T.CASES}
    assert by_id["q64_b76h5_t256_380"]["plans"]["none"][0] == T.K64 and by_id["pp_b77h5_t256_385"]["plans"]["none"] == T.pp(385)
    assert by_id["pp_b8h10_t1024"]["plans"]["none"][0] == T.K64 and by_id["pp_b19h5_t1024_380"]["plans"]["none"][0] == T.K64


def test_alignment_rule_reads_the_pointer_values():
    c = next(x for x in T.CASES if x["id"] == "pp_tq512_tk256")
    assert _plan(c, "none")[0] == T.PP
    a = list(T.plan_args(c, "none"))
    for i, off, want in ((0, 8, T.K64), (1, 8, T.K64), (2, 8, T.K64), (3, 4, T.K64), (3, 8, T.PP)):
        b = list(a)
        b[i] += off
        assert capi.attention_kernel_names()[capi.attention_plan(*b).kernel] == want, (i, off)


def test_invalid_arguments():
    c = next(x for x in T.CASES if x["id"] == "pp_chain_b8h5_t4096")
    a = list(T.plan_args(c, "exact"))
    D, LDQ, LDVT, WS = 8, 9, 11, 17

    def rc(**kw):
        b = list(a)
        for k, v in kw.items():
            b[{"D": D, "ldq": LDQ, "ldvt": LDVT, "ws": WS, "q": 0, "B": 4}[k]] = v
        return capi.lib.ur_attention_plan_launch(*b, capi.AttentionPlan()), capi.lib.ur_last_error().decode()

    assert rc()[0] == 0
    for kw, msg in ((dict(D=96), "head dim must be 64, 128 or 512"), (dict(ldvt=4088), "leading dims"), (dict(ldq=324), "leading dims"),
                    (dict(ws=T.P + 8), "workspace must be 16-byte aligned"), (dict(q=None), "null pointer"), (dict(B=0), "empty problem")):
        code, err = rc(**kw)
        assert code == capi.UR_E_INVALID and msg in err and err.startswith("ur_attention_plan_launch: "), (kw, err)
        # the launch runs the same checks before any HIP call (no stream, no device needed) and returns the same code
        b = list(a)
        for k, v in kw.items():
            b[{"D": D, "ldq": LDQ, "ldvt": LDVT, "ws": WS, "q": 0, "B": 4}[k]] = v
        assert capi.lib.ur_attention_fwd_ws(*b[:17], 0.125, *b[17:], capi.UR_DT_BF16, None) == capi.UR_E_INVALID
        assert msg in capi.lib.ur_last_error().decode()


def test_plan_honours_ur_attn_nopp():
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport attention_cases as T\nfrom unirestore_amd import capi\n"
            "n = capi.attention_kernel_names()\n"
            "print(' '.join(n[capi.attention_plan(*T.plan_args(c, v)).kernel] for c in T.CASES for v in c['plans']))\n") % (
                ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UR_ATTN_NOPP="1"), capture_output=True, text=True, check=True)
    got = out.stdout.split()
    want = [T.K64 if p[0] == T.PP else p[0] for c in T.CASES for p in c["plans"].values()]
    assert got == want and T.K64 in got


# ---------------------------------------------------------------------------------------------------------------- the bound
# scaled-down shapes (B, H, Tq, Tk, D) for the emulation: several 64-key tiles, a ragged one, every head dim
EMU_SHAPES = [(2, 2, 96, 320, 64), (1, 2, 64, 77, 128), (1, 1, 48, 256, 512), (4, 1, 64, 1024, 64)]
EMU_WORST = {}


@pytest.fixture(scope="module")
def emu_report():
    yield
    if EMU_WORST:
        print("\nCPU emulation, largest |o - ref| / bound per (input kind, dtype):")
        for (kind, dt), r in sorted(EMU_WORST.items()):
            print(f"  {kind:12s} {dt}: {r:.3f}")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kind", R.KINDS)
def test_bound_holds_for_the_emulated_kernel_arithmetic(emu_report, kind, dtype):
    """The emulation of tests/attention_reference.py (64-key tiles, fp32 scores and accumulators, 16-bit P against a stale maximum
    with 2^8 or 2^14 head-room, row sum from the rounded P) stays inside the bound for every input kind, both types, both scale
    conventions, with and without the ping-pong kernel's second rounding of q."""
    dt = DTYPES[dtype]
    worst = 0.0
    for B, H, Tq, Tk, D in EMU_SHAPES:
        for scale in (("one",) if kind == "negative" else ("folded", "passed")):
            gen = torch.Generator().manual_seed(zlib.crc32(f"{kind}{Tk}{D}{scale}".encode()))
            q, k, v = R.inputs(kind, scale, B, H, Tq, Tk, D, dt, gen)
            for headroom, pingpong in ((8.0, False), (14.0, D == 64)):
                ref, bnd = R.reference(q, k, v, H, D, R.scale_of(scale, D), dt, pingpong)
                o = R.emulate(q, k, v, H, D, R.scale_of(scale, D), dt, headroom, pingpong)
                what = f"{kind} {dtype} B{B} H{H} Tq{Tq} Tk{Tk} D{D} {scale} head-room 2^{headroom:.0f}"
                worst = max(worst, R.compare(o.double(), ref, bnd, H, D, what))
    EMU_WORST[(kind, dtype)] = worst
    assert worst < 1.0


def test_bound_needs_the_subnormal_term_in_fp16():
    """E_sub of the bound (tests/attention_reference.py) is not slack: without it the emulated fp16 arithmetic leaves the bound on
    the "dominant" inputs, where one key has nearly all the weight, a tiny v, and every other P is an fp16 subnormal."""
    dt = torch.float16
    B, H, Tq, Tk, D = 4, 1, 64, 1024, 64
    gen = torch.Generator().manual_seed(zlib.crc32(f"dominant{Tk}{D}passed".encode()))
    q, k, v = R.inputs("dominant", "passed", B, H, Tq, Tk, D, dt, gen)
    o = R.emulate(q, k, v, H, D, R.scale_of("passed", D), dt, 8.0, False).double()
    ref, bnd = R.reference(q, k, v, H, D, R.scale_of("passed", D), dt, False)
    assert R.compare(o, ref, bnd, H, D) < 1.0
    ref, bnd = R.reference(q, k, v, H, D, R.scale_of("passed", D), dt, False, e_sub=False)
    with pytest.raises(AssertionError, match=r"\(batch 0, query \d+, head 0, channel \d+\)"):
        R.compare(o, ref, bnd, H, D)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_element_check_sees_what_the_whole_tensor_norm_cannot(dtype):
    """One 256-query tile of one head scaled by 1.05 (bf16; 1.01 in fp16, whose tolerance is 8 x tighter) in a B = 8, H = 5,
    T = 4096 output: the whole-tensor rel-L2 stays inside its tolerance, the element check fails and names the tile.
    Synthetic tensors: ref ~ softmax-averaged values, a bound of a few
    output roundings as the real one gives for plain inputs."""
    dt = DTYPES[dtype]
    B, H, T, D = 8, 5, 4096, 64
    g = torch.Generator().manual_seed(1)
    ref = (torch.randn(B, T, H * D, generator=g) * 0.05).double()
    u = R.U_OUT[dt]
    bnd = u * ref.abs() + R.ABS_OUT[dt] + R.C_BOUND * u * 0.02 * (1 + ref.abs())
    o = ref.float().to(dt).double()
    assert R.compare(o, ref, bnd, H, D) < 1.0
    bad = o.clone()
    factor = 1.05 if dt == torch.bfloat16 else 1.01
    bad[5, 768:1024, 2 * D:3 * D] = (ref[5, 768:1024, 2 * D:3 * D] * factor).float().to(dt).double()
    assert R.rel_l2(bad, ref) < 0.6 * R.REL_TOL[dt]                     # the old check passes with room to spare
    with pytest.raises(AssertionError, match=r"\(batch 5, query 7\d\d, head 2, channel \d+\)"):
        R.compare(bad, ref, bnd, H, D)
    nan = o.clone()
    nan[7, 4095, 319] = float("nan")
    with pytest.raises(AssertionError, match=r"\(batch 7, query 4095, head 4, channel 63\)"):
        R.compare(nan, ref, bnd, H, D)
