"""The space of (launch path, epilogue feature) combinations that conv / GEMM dispatch accepts, enumerated on the host, and what the
case table of tests/conv_launcher_cases.py covers of it.  Torch-free: planning (ur_conv2d_plan, ur_conv2d_plan_launch) reads no data.

What a launch executes is the launcher times the epilogue / reduce path the features select (csrc/igemm_impl.h: staged or direct
epilogue, the epi_frag_pass instances, three reduce kinds, three sources of the GroupNorm sums).  So every base case is planned with
one and with two features switched on, at the full and at a NULL workspace, and each (path, feature) and (path, feature pair) of a
variant the plan accepts on the base's launcher is "reachable".  The gate in tests/test_conv_plan_cpu.py holds the table against it.
"""
import itertools

import conv_launcher_cases as LC

# The cases of the table when the space was defined: a fixed list, so that the space does not grow with the table.
BASES = [
    "h128_res_silu_gn", "h128_ups_cat_rowbias_gelu_gnab", "h128_chunksplit_gnab_res_gn", "h160_res_gelu_gn",
    "h160_ups_cat_rowbias_silu_gn", "h160_chunksplit_res_gn", "thin_c3_f32", "thin_c4_res", "thin_c8_silu", "thin_c32_f32_res",
    "himg16_n1_res_gn", "himg16_n3_cat_rowbias_silu_gn", "himg16_n4_gelu", "himg16_n5_ups_gnab_gn", "himg16_n16_res_gn",
    "himg8_n4_res_gn", "himg8_n16_cat_rowbias_silu_gn", "wstream_n1_res_gn", "wstream_n3_cat_rowbias_silu", "wstream_n4_gn_ws_edge",
    "wstream_n5_res_gn", "wstream_n16_gelu_gn", "gemm256_geglu_res_rows", "gemm256_gate_gnpass", "gemm320_geglu_res",
    "gemm320_gate_rows", "v1_128x128_3x3_split", "v1_128x128_3x3_s2_asym", "v1_128x128_3x3_split_gn", "v1_128x128_geglu_ktail",
    "v1_128x128_ln_rows_split", "v1_128x128_yt_split", "v1_128x128_f32_scale_split", "v1_128x160_3x3_split_gn", "v1_128x160_cat",
    "v1_128x64_ktail", "v1_128x64_gn", "v1_256x32_ragged_n_f32", "v1_256x32_rows_gn", "v1_64x64_cat_split", "v1_64x64_rows_split",
    "v1_64x64_ln_split", "v2_256x32_s2_asym_f32", "v2_256x32_split_gn", "v2_128x64_split_gn", "v2_128x64_rows_gelu",
    "v2_256x160_s2_gnpass", "v2_256x128_asym_f32_scale", "v2_256x128_rowbias_gn", "g1_128x128_ragged_res_gelu", "g1_128x128_rows",
    "g1_128x160_ragged", "g1_128x64_ragged", "g1_64x64_ragged_yt", "g1_64x64_gn", "g1_64x64_deep_ragged_ln", "g1_128x64_deep_ragged",
    "group_generic", "group_halo_loop", "bmm_f32_scale", "bmm_split",
]
assert len(BASES) == len(set(BASES)) == 61


def _yt_spec(c):
    """(n_split, t_rows) of the yt toggle: the upper half of the columns (from a multiple of 4) goes out transposed, in blocks of
    the largest of 100 / 64 / 50 / 32 rows that divides M."""
    M = LC.m_rows(c)
    tr = next((t for t in (100, 64, 50, 32) if M % t == 0), None)
    ns = c["Cout"] // 2 // 4 * 4
    return (ns, tr) if tr and 0 < ns < c["Cout"] else None


def _on(key, value=True, when=lambda c: True):
    """A toggle: case dict -> the case with `key` switched on, or None where the case already has it or it does not apply."""
    def f(c):
        off = c[key] in (False, None, LC.NONE) if key != "out_scale" else c[key] == 1.0
        if not off or not when(c):
            return None
        v = value(c) if callable(value) else value
        return None if v is None else dict(c, **{key: v})
    return f


# feature -> change to a case dict.  Each switches one epilogue feature on and leaves the geometry alone.
TOGGLES = {
    "res": _on("res"),
    "act": _on("act", LC.SILU),                                                        # (pair activations belong to their launchers)
    "bias_img": _on("bias_img", when=lambda c: c["bias"]),
    "gn": _on("gn", when=lambda c: LC.cout_out(c) % 8 == 0),
    "gn_ab": _on("gn_ab"),
    "rows": _on("rows"),
    "ln": _on("ln", when=lambda c: c["KH"] == 1 and c["C2"] == 0),
    "yt": _on("yt", _yt_spec, when=lambda c: c["KH"] == 1 and not LC.is_pair(c)),
    "out_f32": _on("out_f32"),
    "out_scale": _on("out_scale", 0.5),
}
GEOMETRIC = ("cat", "ups", "s2", "asym", "nobias")       # carried by a case, counted in pairs, never toggled


def features(c):
    """The features case c runs: the toggled ones it has on, plus the geometric ones."""
    f = {"res": c["res"], "act": c["act"] in (LC.SILU, LC.GELU), "bias_img": c["bias_img"], "gn": c["gn"], "gn_ab": c["gn_ab"],
         "rows": c["rows"], "ln": c["ln"], "yt": c["yt"] is not None, "out_f32": c["out_f32"], "out_scale": c["out_scale"] != 1.0,
         "cat": c["C2"] > 0, "ups": c["ups"], "s2": c["stride"] == 2, "asym": tuple(c["pad"]) != (c["KH"] // 2, c["KH"] // 2),
         "nobias": not c["bias"]}
    return frozenset(k for k, v in f.items() if v)


def path(info, names):
    """What runs, from ur_conv_launch_info alone: (launcher, "unsplit" or (reduce kind, reduce_ri), gn_pass, group_loop)."""
    split = "unsplit" if info.splitk <= 1 else (info.reduce, info.reduce_ri)
    return (names[info.launcher], split, int(info.gn_pass), int(info.group_loop))


def plan(capi, c, nbytes, dtype):
    """(ur_conv_launch_info, prologue_ok) of case c at a workspace of nbytes (None: NULL), as the GPU test launches it (a dense
    output where the GroupNorm sums come from the extra pass); None where ur_conv2d_plan or the launch plan refuses it."""
    def planned(gn_pass):
        d = capi.ConvDesc()
        LC.fill(d, c, dict(LC.placeholders(c), workspace=LC.P if nbytes is not None else None), nbytes, gn_pass)
        d.dtype = dtype
        p, info = capi.ConvPlan(), capi.ConvLaunchInfo()
        if capi.lib.ur_conv2d_plan(d, p) != 0 or capi.lib.ur_conv2d_plan_launch(d, info) != 0:
            return None
        return info, p.prologue_ok
    r = planned(False)
    if r is not None and r[0].gn_pass:
        r = planned(True)
    return r


def combos(feats):
    """The single features and the feature pairs (sorted tuples) of a feature set."""
    fs = sorted(feats)
    return [(f,) for f in fs] + list(itertools.combinations(fs, 2))


def combo_id(p, combo):
    launcher, split, gn_pass, loop = p
    s = "unsplit" if split == "unsplit" else f"reduce{split[0]}.{split[1]}"
    return f"{launcher}/{s}{'/gn_pass' if gn_pass else ''}{'/group_loop' if loop else ''}:{'+'.join(combo)}"


def reachable(capi, dtype):
    """Ids (combo_id) of every (path, feature) and (path, feature pair) a base reaches with at most two toggles, at the full or a NULL
    workspace, where ur_conv2d_plan accepts the variant, honours gn_ab where it is set, and keeps the base's launcher."""
    names = capi.launcher_names()
    by_id = {c["id"]: c for c in LC.CASES}
    out = set()
    for cid in BASES:
        base = by_id[cid]
        for nbytes in (LC.WS_FULL, None):
            b = plan(capi, base, nbytes, dtype)
            assert b is not None, f"base case {cid} is refused"
            for k in (0, 1, 2):
                for tog in itertools.combinations(TOGGLES, k):
                    v = base
                    for t in tog:
                        v = v and TOGGLES[t](v)
                    if not v:
                        continue
                    r = plan(capi, v, nbytes, dtype)
                    if r is None or (v["gn_ab"] and not r[1]) or r[0].launcher != b[0].launcher:
                        continue
                    p = path(r[0], names)
                    out.update(combo_id(p, cb) for cb in combos(features(v)))
    return out


def covered(capi, dtype, cases=None):
    """Ids of every (path, feature) and (path, feature pair) the table runs: each case at each of its workspace sizes."""
    names = capi.launcher_names()
    out = set()
    for c in LC.CASES if cases is None else cases:
        full = plan(capi, c, LC.WS_FULL, dtype)
        assert full is not None, f"case {c['id']} is refused: {capi.lib.ur_last_error().decode()}"
        for _, nbytes in LC.ws_variants(c, full[0].splitk):
            r = plan(capi, c, nbytes, dtype)
            assert r is not None, f"case {c['id']} is refused at {nbytes} workspace bytes: {capi.lib.ur_last_error().decode()}"
            p = path(r[0], names)
            out.update(combo_id(p, cb) for cb in combos(features(c)))
    return out


def is_pair_id(i):
    return "+" in i.rsplit(":", 1)[1]
