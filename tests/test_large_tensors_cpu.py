"""Host side of the large-tensor tests (no GPU): the case table of tests/large_cases.py against the host planner, the stated size
limits from both sides (placeholder pointers: nothing is launched), and the periodic harness of tests/large_harness.py on small
tensors."""
import ast
import os

import pytest

import conv_launcher_cases as LC
import large_cases as T
from unirestore_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = LC.P


def _desc(c, ws=LC.WS_FULL):
    d = capi.ConvDesc()
    LC.fill(d, c, dict(LC.placeholders(c), workspace=P), ws)
    d.dtype = capi.UR_DT_BF16
    return d


def _plan(c):
    """(launcher name, info) or (None, error message)."""
    info = capi.ConvLaunchInfo()
    rc = capi.lib.ur_conv2d_plan_launch(_desc(c), info)
    if rc != 0:
        assert rc == capi.UR_E_INVALID, (c["id"], rc)
        return None, capi.lib.ur_last_error().decode()
    return capi.launcher_names()[info.launcher], info


def test_case_table_needs_no_torch():
    for mod in ("large_cases.py", "conv_launcher_cases.py"):
        tree = ast.parse(open(os.path.join(ROOT, "tests", mod)).read())
        names = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names} | \
                {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
        assert names <= {"conv_launcher_cases"}, (mod, names)


def test_every_launcher_is_reached_at_both_sizes_or_listed_unreachable():
    names = capi.launcher_names()
    hit, moved = {}, []
    for c in T.CONV_CASES:
        name, _ = _plan(c)
        if name != c["launcher"]:
            moved.append(f"{c['id']}: plans to {name}, expected {c['launcher']}")
        hit.setdefault(name, set()).add(c["cls"])
    assert not moved, "\n".join(moved)
    assert set(T.UNREACHABLE) <= set(names)
    for n in names:
        if n in T.UNREACHABLE:
            why, near, lands = T.UNREACHABLE[n]
            assert n not in hit, f"{n} is listed as unreachable ({why}) but a case reaches it"
            assert T.elems(near)["x"] > T.G30 and _plan(near)[0] == lands != n, (n, _plan(near)[0])
        else:
            assert {"past2g", "limit"} <= hit.get(n, set()), f"{n}: needs a past2g and a limit case, has {hit.get(n)}"


def test_size_classes_are_what_they_claim():
    for c in T.CONV_CASES:
        e = T.elems(c)
        E = e[c["big"]]
        if c["cls"] == "past2g":              # E is the launch's largest 16-bit tensor
            assert E == max(e[k] for k in ("x", "x2", "w", "r") + (() if c["out_f32"] else ("y",))), (c["id"], e)
            assert T.G30 < E < T.G30 * 1.02, (c["id"], E)
        elif c["cls"] == "past2^31":
            assert c["big"] == "y" and T.G31 < E < T.G31 * 1.02, (c["id"], E)      # only y: x, x2 and w have a stated limit
        elif c["cls"] == "limit":
            # E is the limited source (y and the residual, which have no limit, may be larger); one more unit is refused by the
            # stated limit, or leaves the launcher (its own dispatch rule ends there)
            assert c["big"] in ("x", "w") and T.SRC_LIMIT * 0.999 < E < (T.SRC_LIMIT if c["big"] == "x" else T.W_LIMIT), (c["id"], E)
            if c["id"] == "l_linear_v1_side":          # the far side of the g1 rule (its own test below); l_v1_128x128 is the last M
                continue
            name, info = _plan(T.next_unit(c))
            assert name != c["launcher"], c["id"]
            assert name is not None or ("ur_conv2d_nhwc" in info and "must be below 2^31" in info), (c["id"], info)
    for c in T.ROW_CASES + T.IMG_CASES:
        E = T.big_elems(c)
        lo = T.G31 if c["cls"] == "past2^31" else T.G30
        assert lo < E < lo * 1.02 and c["P"] % 2 == 1, (c["id"], E)
        if c["cls"] == "limit":                                            # the GroupNorm family's N limit, from the accepted side
            assert c["U"] == T.GN_MAX_N and c["op"] in ("groupnorm", "avgpool")
            continue
        assert c["U"] % c["P"] != 0 or c["op"] == "fanout", c["id"]        # a partial last period (fan-out: B a multiple of P)
    for c in T.BOUNDARY_CASES:
        assert T.f32_elems(c) > T.G30 and c["U"] % c["P"] != 0, c["id"]
    assert {c["op"] for c in T.BOUNDARY_CASES} == {"layout_out", "layout_in", "cast", "unpad_resize", "u8_egress"}


def test_the_two_linear_cases_plan_on_opposite_sides_of_the_g1_rule():
    by = {c["id"]: c for c in T.CONV_CASES}
    a, b = by["l_linear_g1_side"], by["l_linear_v1_side"]
    for c in (a, b):
        assert (c["C1"], LC.geometry(c)["ldx"], c["KH"]) == (64, 64, 1)
    assert (a["W"], b["W"]) == ((1 << 25) - 6, (1 << 25) - 5)
    assert _plan(a)[0].startswith("g1_") and not _plan(b)[0].startswith("g1_")
    # the rule itself: M * ldx + K < 2^31 - 256
    assert a["W"] * 64 + 64 < T.G31 - 256 <= b["W"] * 64 + 64


def test_features_and_split_k_are_covered():
    for name, has in T.FEATURES.items():
        assert any(has(c) for c in T.CONV_CASES), f"no large case runs: {name}"
    by = {c["id"]: c for c in T.CONV_CASES}
    for cid in T.SPLITK_CASES:
        _, info = _plan(by[cid])
        assert info.splitk > 1 and info.reduce >= 0, cid
    assert any(c["cls"] == "prod" and (c["N"], c["H"], c["W"], c["C1"], c["Cout"]) == (24, 512, 512, 256, 256) for c in T.CONV_CASES)
    ops = {c["op"] for c in T.ROW_CASES + T.IMG_CASES}
    assert ops == {"axpy", "spade", "layernorm", "softmax", "scale", "fanout", "dwconv", "groupnorm", "avgpool"}


# ---- the stated limits (include/unirestore_hip.h "size limits"), from both sides ---------------------------------------------------
@pytest.mark.parametrize("rid,c,frag", T.REFUSED, ids=[r[0] for r in T.REFUSED])
def test_conv_refuses_the_first_shape_past_each_limit(rid, c, frag):
    name, msg = _plan(c)
    assert name is None and "ur_conv2d_nhwc" in msg and frag in msg, (rid, name, msg)
    # the launch refuses it too, before any HIP call (placeholder pointers, no stream, no device)
    assert capi.lib.ur_conv2d_nhwc(_desc(c), None) == capi.UR_E_INVALID
    assert frag in capi.lib.ur_last_error().decode()


def test_conv_limits_are_exact():
    # x: N*H*W*ldx = 2^31 is refused, 8 elements fewer are planned (a Linear with rows of 8)
    m = T.SRC_LIMIT // 8
    assert _plan(T.lin("x_at", "", "", "x", m, 8, 8))[0] is None
    assert _plan(T.lin("x_in", "", "", "x", m - 1, 8, 8))[0] is not None
    # x2 alone
    assert _plan(T.lin("x2_at", "", "", "x2", T.SRC_LIMIT // 16, 8, 8, C2=16))[0] is None
    assert _plan(T.lin("x2_in", "", "", "x2", T.SRC_LIMIT // 16 - 1, 8, 8, C2=16))[0] is not None
    # w: Cout * ldw
    assert 24 * 89478472 == T.W_LIMIT - 64 and 8 * 268435424 == T.W_LIMIT
    assert _plan(T.lin("w_at", "", "", "w", 8, 8, 268435424))[0] is None and "2^31 - 256" in _plan(T.lin("w_at", "", "", "w", 8, 8, 268435424))[1]
    assert _plan(T.lin("w_in", "", "", "w", 8, 8, 268435420))[0] is not None
    # the tile grid of the planned launcher: 2^20 row tiles of 128 x 8 column tiles of 128 = 2^23 is refused, 7 column tiles are planned
    assert _plan(T.lin("grid_at", "", "", "y", 1 << 27, 8, 1024))[0] is None
    name, _ = _plan(T.lin("grid_in", "", "", "y", 1 << 27, 8, 896))
    assert name in ("g1_128x128", "v1_128x128") and ((1 << 27) // 128) * (1024 // 128) == T.GRID_LIMIT
    assert _plan(T.lin("grid_ok", "", "", "y", (1 << 25) - 1, 64, 512))[0] is not None      # 2^18 x 4 workgroups: far below the wrap
    # the grouped wrapper builds the same descriptor (ldx = Cg * groups): 14352 images of 29 x 43 x 120 are refused through it too
    assert capi.lib.ur_groupconv3x3_nhwc(P, P, None, P, 14352, 29, 43, 8, 4, 15, 0, None, 0, capi.UR_DT_BF16, None) == capi.UR_E_INVALID
    assert "must be below 2^31" in capi.lib.ur_last_error().decode()
    # ur_gemm_bias_act: its own row bound, then the same checks
    args = (P, P, None, None, P)
    tail = (64, 64, 64, 0, 0, None, 0, capi.UR_DT_BF16, None)
    assert capi.lib.ur_gemm_bias_act(*args, 1 << 31, 64, 64, *tail) == capi.UR_E_INVALID
    assert "ur_gemm_bias_act" in capi.lib.ur_last_error().decode()
    assert capi.lib.ur_gemm_bias_act(*args, 1 << 25, 64, 64, *tail) == capi.UR_E_INVALID
    assert "must be below 2^31" in capi.lib.ur_last_error().decode()


def test_no_descriptor_launcher_sees_a_source_that_ends_past_0xffffff00():
    """The LDS-DMA kernels read x, x2 and w through buffer descriptors that return zeros from byte offset 0xffffff00 on; a source
    whose bytes reach past it must plan to a launcher that reads through 64-bit pointers.  Shapes with 2^31 - 8 ... 2^31 - 120
    elements, 1x1 and 3x3, with and without the features that steer dispatch."""
    seen = set()
    shapes = [T.conv("d", "", "", "x", 14351, Cout=co, KH=kh, **T.G2943) for co in (8, 64, 128, 160, 256) for kh in (1, 3)]
    shapes += [T.lin("d", "", "", "x", (T.G31 - 8 * j) // ld, k, co, ldx_pad=ld - k, act=act)
               for j in (1, 5, 15) for ld, k in ((8, 8), (24, 8), (56, 32), (72, 64), (328, 320)) if (T.G31 - 8 * j) % ld == 0
               for co, act in ((64, T.NONE), (128, T.NONE), (160, T.NONE), (256, T.GATE), (1280, T.GEGLU))]
    assert len(shapes) > 20
    for c in shapes:
        e = T.elems(c)
        if e["M"] >= T.ROWS_LIMIT:
            continue
        assert e["x"] * 2 > T.IG_OOB_BYTES, e
        name, info = _plan(c)
        if name is None and "tile grid" in info:
            continue
        assert name is not None, info
        assert name not in T.DESCRIPTOR_LAUNCHERS, (name, e)
        seen.add(name)
    assert len(seen) >= 4, seen
    # the halo / whole-image kernels take images of a multiple of 64 pixels: with ldx % 8 == 0 their x is a multiple of 512 elements,
    # so no batch of such images ends inside (2^32 - 1024, 2^32) bytes.  Swept on the planner: the largest accepted batch of every
    # eligible geometry, and the batches around it, either end at or below 2^32 - 1024 bytes or are refused.
    halo = [n for n in T.DESCRIPTOR_LAUNCHERS if n.startswith(("halo", "himg", "wstream"))]
    reached = set()
    for hh, ww in ((8, 32), (16, 32), (8, 64), (24, 96), (40, 160), (8, 8), (16, 16), (4, 16), (8, 16)):
        for ups in (False, True):
            for c1, pad, c2 in ((64, 0, 0), (64, 8, 0), (64, 56, 0), (128, 0, 0), (256, 24, 0), (64, 0, 64), (128, 0, 128)):
                for cout in (8, 128, 160):
                    per = hh * ww * (c1 + pad)
                    for n in range(max(1, (T.G31 - 1) // per - 4), (T.G31 - 1) // per + 2):
                        c = T.conv("s", "", "", "x", n, hh, ww, c1, cout, C2=c2, ldx_pad=pad, ups=ups)
                        name, _ = _plan(c)
                        if name in halo:
                            reached.add(name)
                            assert T.elems(c)["x"] % 512 == 0 and T.elems(c)["x"] * 2 <= T.G31 * 2 - 1024 < T.IG_OOB_BYTES, (name, c["N"], hh, ww)
    assert {"halo_8x32_128", "halo_8x32_160", "halo_thin_32", "himg_16x16", "himg_8x8x4"} <= reached, reached
    for c in T.CONV_CASES:
        if c["launcher"].startswith(("halo", "himg")):
            assert T.elems(c)["x"] % 512 == 0 and T.elems(c)["x"] * 2 <= T.IG_OOB_BYTES, c["id"]


def test_task_chunks_follow_the_conv_limit():
    from unirestore_amd import tiling
    assert tiling.TASK_CHUNK_MAX_ELEMS == T.SRC_LIMIT                      # the limit stands as it was: nothing was found past it
    assert tiling.task_chunks(8, 3, 512, 512, 256) == [(0, 3)]            # the production configuration still decodes in one chunk
    assert _plan(T.conv("prod", "", "", "x", 24, 512, 512, 256, 256))[0] is not None


def test_norm_exports_refuse_what_their_grids_cannot_hold():
    lib, bf = capi.lib, capi.UR_DT_BF16
    for name, call in (
            ("ur_groupnorm_stats", lambda n: lib.ur_groupnorm_stats(P, P, n, 64, 64, bf, None)),
            ("ur_groupnorm_finalize", lambda n: lib.ur_groupnorm_finalize(P, 1, 64, None, 0, 0, None, None, n, 64, 8, 1e-5, P, None, None)),
            ("ur_groupnorm_apply_act", lambda n: lib.ur_groupnorm_apply_act(P, None, P, P, n, 64, 64, 0, 0, bf, None)),
            ("ur_groupnorm_nhwc", lambda n: lib.ur_groupnorm_nhwc(P, None, P, None, None, n, 64, 64, 0, 8, 1e-5, 0, P, P, None, 0, None, 0, bf, None)),
            ("ur_avgpool_hw", lambda n: lib.ur_avgpool_hw(P, P, n, 64, 64, P, bf, None))):
        assert call(65536) == capi.UR_E_INVALID, name
        msg = lib.ur_last_error().decode()
        assert name in msg and "65535" in msg, msg


# ---- the harness on small tensors ---------------------------------------------------------------------------------------------------
def test_harness_tiles_and_rejects_one_corrupt_element_in_the_last_period(monkeypatch):
    import torch
    import large_harness as H
    g = torch.Generator().manual_seed(5)
    Pn, U, R, width, ld = 3, 32, 7, 5, 8                                  # 10 whole periods and a partial one
    src = torch.randn(Pn, R, ld, generator=g).to(torch.bfloat16)
    monkeypatch.setattr(H, "COPY_ELEMS", 4 * Pn * R * ld + 1)            # several capped copies
    y = H.tile_periodic(torch.empty(U, R, ld, dtype=torch.bfloat16), src)
    for i in range(U):
        assert torch.equal(y[i], src[i % Pn]), i
    ref = src[..., :width].double() * (1 + 2.0 ** -10)                    # a reference the bf16 values meet within 2^-8 relative
    bnd = 2.0 ** -8 * ref.abs()
    for chunk in (1 << 25, Pn * R * width, R * width, 11):                # whole tensor, one period, less than a period (row blocks)
        r = H.check_periodic(y, ref, bnd, "ok", chunk_elems=chunk)
        assert 0 < r < 1.0
    assert abs(H.host_check(y, ref, bnd, H.spot_units(U, 1 << 29), "host") - r) < 1e-12
    # one element of the partial last period, moved by 3 % - far inside any rel-L2 tolerance of the whole tensor
    for unit, row, col in ((U - 1, R - 1, width - 1), (U - 2, 0, 0), (17, 3, 2)):
        bad = y.clone()
        bad[unit, row, col] = (bad[unit, row, col].double() * 1.03 + 1e-3).to(torch.bfloat16)
        for chunk in (1 << 25, Pn * R * width, 11):
            with pytest.raises(AssertionError, match=f"unit {unit} .* row {row} col {col}"):
                H.check_periodic(bad, ref, bnd, "bad", chunk_elems=chunk)
        with pytest.raises(AssertionError):
            H.host_check(bad, ref, bnd, [unit], "bad")
    nan = y.clone()
    nan[U - 1, 2, 1] = float("nan")
    with pytest.raises(AssertionError):
        H.check_periodic(nan, ref, bnd, "nan")
    # padding columns are not looked at by the bound check; the fill check sees them
    pad = y.clone()
    pad[5, 1, width] = 1.0
    assert H.check_periodic(pad, ref, bnd, "pad") == r
    bits = y.view(torch.int16)
    H.equal_chunked(bits.reshape(-1), bits.clone().reshape(-1), "same", chunk_elems=13)
    other = bits.clone().reshape(-1)
    other[-1] ^= 1
    with pytest.raises(AssertionError):
        H.equal_chunked(bits.reshape(-1), other, "diff", chunk_elems=13)
    fill = torch.full((9, 4), 0x7FC0, dtype=torch.int16)
    H.check_fill(fill, 0x7FC0, "fill", chunk_elems=8)
    fill[8, 3] = 0
    with pytest.raises(AssertionError):
        H.check_fill(fill, 0x7FC0, "fill", chunk_elems=8)
    assert H.spot_units(10, 1 << 29, 1 << 28) == [0, 4, 8, 9] and H.spot_units(3, 1 << 20) == [0, 2]
