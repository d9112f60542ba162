"""Host gate of the scoring limit cases (tests/scoring_large_cases.py, run on the GPU by tests/test_scoring_large_gpu.py), and the
stand-alone host program that checks the 1-D launch helper (csrc/launch_size.h) under UBSan / ASan.  Nothing here needs a GPU:
  * the case table reaches every launching export of f32_layers.hip, lpips.hip, classify.hip, segment.hip and metrics.hip, both
    kernels of the ops that have a float4 and a scalar one, and every named property (confusion trips, bin passes, tensors past 2^31 / 2^32);
  * every "limit" case sits at the stated limit from below, and one more unit is refused before any HIP call;
  * the fp64 reference of one period of each case, against the reference's own fp32 restatement, stays inside the bound the GPU test
    uses, and the decidability cap of the argmax cases holds - so the GPU test hides nothing under a cap.
"""
import os
import shutil
import subprocess

import pytest

import scoring_large_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["id"]: c for c in T.CASES}


def test_launch_helper_host_program_under_ubsan_and_asan(tmp_path):
    """tests/launch_size_main.cpp: ur::grid_1d at 1, 255, 256, 257, 2^31 - 257, 2^31 - 256, 2^31 - 1 and 2^32 against literals."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++, clang++ or c++): the build of the library needs one as well"
    exe = tmp_path / "launch_size_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "launch_size_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("PASSED") and "FAIL" not in r.stdout and not r.stderr, (r.stdout, r.stderr)


def test_the_scoring_files_launch_through_the_helper():
    """No `(total + 255) / 256`-style block count is left in the scoring files (nor in elementwise.hip, whose two such launches were
    converted with them)."""
    import re
    pat = re.compile(r"dim3\(\s*\(+[^;]*\+\s*(255|63)\)\s*/")
    for name in ("f32_layers.hip", "lpips.hip", "classify.hip", "segment.hip", "metrics.hip", "elementwise.hip"):
        src = open(os.path.join(ROOT, "unirestore_amd", "csrc", name)).read()
        assert not pat.search(src), name
    for name in ("f32_layers.hip", "lpips.hip", "classify.hip", "segment.hip"):
        assert "UR_GRID_1D(" in open(os.path.join(ROOT, "unirestore_amd", "csrc", name)).read(), name


def test_case_table_reaches_every_export_kernel_and_property():
    from unirestore_amd import capi
    assert len(CASES) == len(T.CASES)
    ran = {c["export"] for c in T.CASES}
    for name in T.LAUNCHING_EXPORTS:
        assert hasattr(capi.lib, name), name
        assert name in ran or name in T.NOT_RUN, name
    assert ran <= set(T.LAUNCHING_EXPORTS) and not (ran & set(T.NOT_RUN))
    # every launching export of the four sections of the header is in the list (the others are host-side size helpers)
    header = open(os.path.join(ROOT, "include", "unirestore_hip.h")).read()
    import re
    declared = set(re.findall(r"\b(ur_(?:image_metrics|lpips_\w+|conv2d_f32\w*|maxpool\w+|classify_\w+|avgpool_f32|top1_counts|seg_\w+|upsample_bilinear_ac_f32|add_f32))\(", header))
    helpers = {"ur_image_metrics_ws_size", "ur_lpips_tap_hw", "ur_lpips_layer_parts", "ur_lpips_ws_size", "ur_conv2d_f32_wpack_dims", "ur_seg_confusion_ws_bytes"}
    assert declared - helpers == set(T.LAUNCHING_EXPORTS), declared ^ (set(T.LAUNCHING_EXPORTS) | helpers)
    for name in T.TWO_KERNELS:
        paths = {p for c in T.CASES if c["export"] == name for p in c["props"] if p in ("vector", "scalar")}
        assert paths == {"vector", "scalar"}, (name, paths)
    claimed = {p for c in T.CASES for p in c["props"]}
    assert set(T.PROPERTIES) <= claimed, set(T.PROPERTIES) - claimed


def test_claimed_properties_are_true():
    """Each property a case claims, recomputed from its shape."""
    for c in T.CASES:
        props, op = c["props"], c["op"]
        if op == "confusion":
            trips, passes = T.confusion_trips(c["P"]), T.bin_passes(c["C"])
            for k in (1, 2, 3):
                assert (f"trip {k}" in props) == (trips == k and c["P"] <= 3 * T.TRIP and c["P"] > 5000), (c["id"], trips)
            assert ("2 bin passes" in props) <= (passes == 2) and ("255 bin passes" in props) == (passes == 255), (c["id"], passes)
            assert ("C = 1" in props) == (c["C"] == 1) and ("int64 targets" in props) == c["i64"]
        if op == "add":
            assert ("vector" in props) == (c["n"] % 4 == 0) and ("scalar" in props) == (c["n"] % 4 == 1)
        if op in ("upsample", "maxpool5"):
            assert ("vector" in props) == (c["C"] % 4 == 0)
        if op == "tta":
            assert ("avg null" in props) == (not c["avg"]) and ("avg given" in props) == c["avg"]
        if op == "avgpool":
            assert 4 * (c["N"] - 1) * c["P"] * c["C"] > 1 << 31
        if op == "conv":
            oh, ow = T.conv_out(c)
            m, k = c["N"] * oh * ow, c["Cin"] * c["k"] * c["k"]
            xbytes = 4 * c["N"] * c["H"] * c["W"] * c["Cin"]
            assert ("vector" in props) == (c["Cin"] % 4 == 0)
            assert ("x past 2^32 bytes" in props) == (xbytes > 1 << 32) and ("x past 2^31 bytes" in props) == (1 << 31 < xbytes <= 1 << 32)
            assert ("y past 2^31 elements" in props) == (m * c["Cout"] > 1 << 31) and ("residual" in props) == c["res"]
            assert ("K tail" in props) <= (k % 16 != 0) and ("Cout tail" in props) <= (c["Cout"] % 64 != 0)
            assert ("M tail of 1 row" in props) == (m % 128 == 1)
            assert m <= (1 << 31) - 1 - 128 and c["N"] * c["H"] * c["W"] < 1 << 31          # accepted
        if op == "lpips_layer":
            assert 2 * c["N"] * c["P"] * c["C"] > 1 << 31 and c["P"] % 64 != 0 and c["N"] <= 65535
        if op == "metrics":
            tiles = -(-(c["W"] - c["win"] + 1) // 64) * -(-(c["H"] - c["win"] + 1) // 16)
            assert 4 * c["N"] * c["C"] * c["H"] * c["W"] > 1 << 32 and c["C"] * tiles > 256 and c["N"] * c["C"] * tiles <= ((1 << 31) - 1) // 256


def test_limit_cases_sit_at_the_stated_limit_and_the_next_unit_is_refused():
    from unirestore_amd import capi
    header = open(os.path.join(ROOT, "include", "unirestore_hip.h")).read()
    assert T.GRID == (1 << 31) - 256
    for words in ("below 2^31 - 256", "n in [1, 2^31 - 256)", "P in [1, 2^31)", "N*H*W must be below 2^28", "below 2^31 - 128"):
        assert words in header, words
    limits = [c for c in T.CASES if "limit" in c["props"]]
    assert len(limits) >= 17
    for c in limits:
        assert c["limit"] in (T.GRID, T.INT31, T.P28), c["id"]
        assert c["count"] < c["limit"], c["id"]
        slack = c["limit"] - 1 - c["count"]
        if c["id"] in T.EXACT:
            assert slack == 0, (c["id"], slack)                      # the header's limit minus one, exactly
        elif c["op"] == "add":
            assert slack < 4 and c["n"] % 4 == ("scalar" in c["props"])      # the largest n of its residue class mod 4
        else:
            assert c["count"] % c["N"] == 0 and c["count"] + c["count"] // c["N"] >= c["limit"], c["id"]      # one more image is past it
        if c["limit"] == T.GRID:
            assert slack < 256, (c["id"], slack)                     # inside the last block below the launch limit
        rc = T.refusal(c, capi.lib)
        assert rc == capi.UR_E_INVALID, (c["id"], rc)
        msg = capi.lib.ur_last_error().decode()
        assert c["export"] in msg, (c["id"], msg)
        assert "2^31" in msg or "2^28" in msg, (c["id"], msg)
    # limit + 0 itself, where the count can be set directly
    P = 256
    assert capi.lib.ur_add_f32(P, P + 256, P + 512, T.GRID, None) == capi.UR_E_INVALID
    assert capi.lib.ur_seg_confusion(P, P, 0, T.INT31, 19, 255, P, 1 << 40, P, None) == capi.UR_E_INVALID
    assert capi.lib.ur_maxpool2d_pad_f32(P, P + 256, T.GRID // 4, 1, 1, 4, None) == capi.UR_E_INVALID       # N*C = 2^31 - 256
    assert capi.lib.ur_avgpool_f32(P, P + 256, T.GRID // 4, 1, 4, None) == capi.UR_E_INVALID
    assert capi.lib.ur_top1_counts(P, P, 1, T.GRID, P, P, None) == capi.UR_E_INVALID
    assert capi.lib.ur_lpips_prep(P, P + 256, 1 << 18, 3, 32, 32, None) == capi.UR_E_INVALID                # N*H*W = 2^28


@pytest.mark.parametrize("cid", [c["id"] for c in T.CASES if c["op"] != "confusion"])
def test_reference_of_one_period_stays_inside_the_bound(cid):
    """fp32's own restatement against the fp64 reference on the P units of the case: inside the bound the GPU test applies (the bound
    is 8 x the fp32 error measured on the small cases, so this says the large shapes are no harder), finite, and - for the argmax
    cases - at most 0.5 % of the pixels undecidable."""
    import torch
    c = CASES[cid]
    u = T.build(c)
    if c["op"] == "metrics":                                   # fp64 on both sides: the yardstick itself, on one period
        for k in ("psnr", "ssim"):
            assert u[k].shape == (T.P_IMG, 1, 1) and u[k].dtype == torch.float64 and bool(torch.isfinite(u[k]).all()) and bool((u[k + "_bnd"] > 0).all())
        assert 10 < float(u["psnr"].min()) < 40 and 0 < float(u["ssim"].min()) <= float(u["ssim"].max()) < 1
        assert all(t.shape == (T.P_IMG, c["C"], c["H"], c["W"]) for t in u["ins"].values())
        return
    if c["op"] == "top1":
        x = u["ins"]["x"]
        assert u["pred"].tolist() == [int(torch.where(torch.isnan(r), torch.tensor(float("inf")), r).argmax()) for r in x]
        assert bool((u["labels"] >= 0).all()) and bool((u["labels"] < c["C"]).all())
        return
    ref, bnd = u["ref"], u["bnd"]
    assert ref.dtype == torch.float64 and bnd.shape == ref.shape and bool(torch.isfinite(ref).all()) and bool((bnd >= 0).all())
    for t in u["ins"].values():
        assert t.shape[0] in (T.P_IMG, T.P_FLAT) and t.shape[0] % 2 == 1
    if "ref32" in u:
        ratio = float(((u["ref32"].double() - ref).abs() / bnd.clamp_min(1e-300)).max())
        print(f"{cid}: fp32 restatement against fp64: {ratio:.3f} of the bound")
        assert bool((bnd > 0).all()) and ratio <= 1.0, (cid, ratio)
    else:
        assert float(bnd.abs().max()) == 0.0, cid                     # an exact op: bit-equal
    if c["op"] == "tta":
        print(f"{cid}: {u['undecidable']:.4%} of the pixels undecidable")
        assert u["undecidable"] <= 0.005 and len(set(u["pred"].flatten().tolist())) >= 5


def test_confusion_periods_and_expected_counts():
    """The periodic confusion inputs: numpy.bincount on the period and its tail equals numpy.bincount on the whole sequence (checked
    where the whole sequence is small), every class but the absent row occurs, and the counts add up to the labelled pixels."""
    import numpy as np
    for c in T.CASES:
        if c["op"] != "confusion":
            continue
        pred, target = T.confusion_period(c)
        assert len(pred) % 2 == 1 and len(pred) % T.SC_CHUNK != 0
        want = T.confusion_expected(c, pred, target)
        C = c["C"]
        assert want.shape == (C, C) and int(want.sum()) > 0.7 * c["P"]
        if c["P"] <= 3 * T.TRIP:
            reps = -(-c["P"] // len(pred))
            p, t = np.tile(pred, reps)[:c["P"]], np.tile(target, reps)[:c["P"]]
            keep = (t < C) & (t != 255)
            assert np.array_equal(want, np.bincount(t[keep] * C + p[keep], minlength=C * C).reshape(C, C)), c["id"]
        if C == 19:
            assert int(want[C - 1].sum()) == 0 and bool((want[:C - 1] > 0).all())
