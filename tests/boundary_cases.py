"""The cases of the image / latent boundary parity matrix, literal (tests/test_boundary_launchers_gpu.py launches them,
tests/test_boundary_reference_cpu.py asserts that every property of PROPERTIES is held by at least one launched case and runs the
refusal table).  The block under test is "latent / image boundary" of include/unirestore_hip.h: everything below
"layout / boundary kernels" in csrc/elementwise.hip.  Shapes are the smallest at which each kernel can still go wrong; only BIG_CASES
comes near workload size (the second trip through the grid-stride loop).
"""
P = 1 << 20                      # placeholder pointer of the host-only refusal table (16-byte aligned, never dereferenced)
UR_E_INVALID = -1
BF16, F16 = 0, 1
SCALING = 0.18215                # the latent scaling factor of the VAE


def _ids(prefix, keys, rows, **extra):
    return [dict(zip(keys, r), id=prefix + "_" + "_".join(str(v) for v in r), **extra) for r in rows]


# ---- layout in: ur_nchw_f32_to_nhwc, ur_image_to_nhwc (N, C, H, W, Cpad) --------------------------------------------------------
LAYOUT_IN_SHAPES = [(1, 3, 1, 1, 8), (2, 3, 5, 7, 8), (3, 1, 3, 5, 8), (2, 4, 9, 11, 8), (1, 8, 4, 4, 8), (2, 3, 16, 24, 16)]
LAYOUT_IN_CASES = _ids("lin", ("N", "C", "H", "W", "Cpad"), LAYOUT_IN_SHAPES)

# ---- layout out: ur_nhwc_to_nchw_f32 (N, C, H, W, ld) x x_is_f32 x (mul, add) -------------------------------------------------------
LAYOUT_OUT_SHAPES = [(2, 3, 5, 7, 8), (1, 4, 9, 11, 4), (2, 3, 1, 1, 16)]
MUL_ADD = [(0.5, 0.5), (1.0, 0.0), (1.0 / SCALING, 0.0)]
LAYOUT_OUT_CASES = [dict(id=f"lout_{n}_{c}_{h}_{w}_{ld}_f{f}_m{i}", N=n, C=c, H=h, W=w, ld=ld, f32=f, mul=m, add=a)
                    for (n, c, h, w, ld) in LAYOUT_OUT_SHAPES for f in (0, 1) for i, (m, a) in enumerate(MUL_ADD)]

# ---- ur_f32_to_bf16_scaled (M, C, Cpad, ld) ------------------------------------------------------------------------------------------
CAST_SHAPES = [(1, 4, 8, 4), (35, 4, 8, 8), (64, 4, 8, 16), (7, 8, 8, 8)]
CAST_CASES = _ids("cast", ("M", "C", "Cpad", "ld"), CAST_SHAPES, kind="randn", mul=1.0 / SCALING) + \
    [dict(id="cast_ties", M=24, C=4, Cpad=8, ld=8, kind="ties", mul=1.0)]

# ---- ur_image_resize_pad_nhwc (N, C, H, W, RH, RW, PH, PW, Cpad) ---------------------------------------------------------------------
RESIZE_IN_SHAPES = [(2, 3, 5, 7, 13, 9, 3, 7, 8), (1, 3, 37, 29, 8, 8, 0, 0, 8), (1, 3, 1, 1, 8, 8, 0, 0, 8), (1, 3, 2, 3, 16, 16, 5, 0, 8),
                    (2, 3, 8, 8, 8, 8, 7, 7, 8), (1, 3, 5, 9, 5, 9, 0, 0, 8), (1, 3, 8, 12, 8, 24, 4, 0, 8), (1, 1, 6, 10, 40, 64, 0, 0, 16)]
RESIZE_IN_CASES = _ids("rin", ("N", "C", "H", "W", "RH", "RW", "PH", "PW", "Cpad"), RESIZE_IN_SHAPES, mul=2.0, add=-1.0)

# ---- ur_image_unpad_resize_nchw (N, C, XH, XW, ld, CH, CW, OH, OW) x x_is_f32 x quantize -------------------------------------------------
RESIZE_OUT_SHAPES = [(2, 3, 16, 16, 8, 13, 9, 5, 7), (1, 3, 8, 8, 8, 8, 8, 37, 29), (1, 3, 8, 8, 4, 1, 1, 8, 8), (2, 3, 12, 20, 8, 12, 20, 12, 20),
                     (1, 3, 12, 20, 8, 9, 20, 9, 20), (1, 1, 40, 64, 16, 40, 64, 6, 10)]
_RO_KEYS = ("N", "C", "XH", "XW", "ld", "CH", "CW", "OH", "OW")
RESIZE_OUT_CASES = [dict(zip(_RO_KEYS, r), id="rout_" + "_".join(str(v) for v in r) + f"_f{f}_q{q}", f32=f, quantize=q, mul=0.5, add=0.5, special=False)
                    for r in RESIZE_OUT_SHAPES for f in (0, 1) for q in (0, 1)]
# NaN, +inf, -inf, +1e30, -1e30 and a finite 3e38 whose SAMPLE (v * mul + add, an fp32 value) overflows, inside the window; 12 -> 9 puts
# every output at a fractional position of 1/6, 1/2 or 5/6: no cubic weight is near zero, so the sign of w * 1e30 is not in doubt
SPECIAL_POS = {"nan": (0, 0, 1, 1), "+inf": (0, 1, 9, 2), "-inf": (0, 2, 2, 10), "+1e30": (0, 0, 9, 9), "-1e30": (0, 1, 2, 5), "3e38": (0, 2, 6, 5)}
RESIZE_OUT_SPECIAL = [dict(zip(_RO_KEYS, (1, 3, 14, 14, 8, 12, 12, 9, 9)), id=f"rout_special_q{q}", f32=1, quantize=q, mul=2.0, add=0.5, special=True)
                      for q in (0, 1)]

# ---- ragged 8-bit: canvas (CH, CW), images (H, W) -> (RH, RW); slot_bytes > 3 CH CW; bad rows once per clause of ragged_geom_ok ---------------
RAGGED_CANVASES = [
    dict(id="rag_24x20", CH=24, CW=20, geom=[(24, 20, 24, 20), (12, 10, 24, 20), (13, 11, 20, 16), (17, 20, 17, 20)], slack=37),
    dict(id="rag_16x16", CH=16, CW=16, geom=[(16, 16, 16, 16), (8, 8, 16, 16), (9, 9, 9, 9), (3, 3, 9, 10)], slack=5),
]
BAD_CLAUSES = ["H=0", "H<0", "H>RH", "RH>CH", "CH-RH>=RH", "W=0", "W>RW", "RW>CW", "CW-RW>=RW"]


def ragged_geom_ok(H, W, RH, RW, CH, CW):
    return H > 0 and W > 0 and H <= RH and W <= RW and RH <= CH and RW <= CW and CH - RH < RH and CW - RW < RW


def bad_row(clause, row, CH, CW):
    """`row` = (H, W, RH, RW) with exactly the one clause of ragged_geom_ok broken."""
    H, W, RH, RW = row
    out = {"H=0": (0, W, RH, RW), "H<0": (-H, W, RH, RW), "H>RH": (RH + 1, W, RH, RW), "RH>CH": (H, W, CH + 1, RW),
           "CH-RH>=RH": (min(H, CH // 2), W, CH // 2, RW), "W=0": (H, 0, RH, RW), "W>RW": (H, RW + 1, RH, RW), "RW>CW": (H, W, RH, CW + 1),
           "CW-RW>=RW": (H, min(W, CW // 2), RH, CW // 2)}[clause]
    assert not ragged_geom_ok(*out, CH, CW)
    return out


# ---- ur_vae_sample (N, HW, Clat, Cpad, ld); ur_add_noise / ur_ddim_step on the same (N, HW, Clat, Cpad) x ld_eps ------------------------------
VAE_SHAPES = [(1, 1, 4, 8, 8), (2, 35, 4, 8, 8), (2, 64, 4, 8, 16), (1, 7, 8, 8, 16), (3, 5, 4, 4, 8)]
VAE_CASES = _ids("vae", ("N", "HW", "Clat", "Cpad", "ld"), VAE_SHAPES)
NOISE_CASES = _ids("noise", ("N", "HW", "Clat", "Cpad", "ld"), VAE_SHAPES)
DDIM_CASES = [dict(id=f"ddim_{n}_{hw}_{cl}_{cp}_e{le}", N=n, HW=hw, Clat=cl, Cpad=cp, ld_eps=le)
              for (n, hw, cl, cp, _) in VAE_SHAPES for le in sorted({cl, 8, 16}) if le >= cl]

# ---- tiles (N, LH, LW, th, tw, origins) x (Clat, Cpad, ld_eps) -------------------------------------------------------------------------
TILE_SHAPES = [(1, 8, 8, 8, 8, [(0, 0)]),
               (2, 12, 10, 8, 8, [(0, 0), (0, 2), (4, 0), (4, 2)]),
               (1, 6, 22, 6, 10, [(0, 0), (0, 4), (0, 8), (0, 12)]),
               (2, 12, 12, 8, 8, [(0, 0), (4, 4), (5, 4), (-2, 0), (0, -1), (4, 5)]),
               (1, 8, 16, 8, 8, [(0, 0), (0, 3), (0, 5), (0, 8)])]        # synthetic weights, three tiles deep: carries the summation-order probe
TILE_CHANNELS = [(4, 8, 8), (4, 8, 4), (8, 8, 8), (4, 16, 8)]
TILE_CASES = [dict(id=f"tile{i}_c{cl}_{cp}_{le}", N=n, LH=lh, LW=lw, th=th, tw=tw, origins=org, Clat=cl, Cpad=cp, ld_eps=le, plan=(i in (1, 2)))
              for i, (n, lh, lw, th, tw, org) in enumerate(TILE_SHAPES) for (cl, cp, le) in TILE_CHANNELS]


def tile_valid(c, k):
    y0, x0 = c["origins"][k]
    return y0 >= 0 and x0 >= 0 and y0 + c["th"] <= c["LH"] and x0 + c["tw"] <= c["LW"]


def tile_cover(c):
    """[LH][LW] number of valid tiles that cover each latent pixel."""
    cov = [[0] * c["LW"] for _ in range(c["LH"])]
    for k, (y0, x0) in enumerate(c["origins"]):
        if tile_valid(c, k):
            for y in range(y0, y0 + c["th"]):
                for x in range(x0, x0 + c["tw"]):
                    cov[y][x] += 1
    return cov


# ---- second trip through the grid-stride loop: nblocks() caps the grid at 8192 blocks of 256 threads; one case per kernel ----------------------
GRID_THREADS = 8192 * 256
BIG_CASES = [
    dict(id="big_layout_in", op="layout_in", N=1, C=3, H=1450, W=1450, Cpad=8),                            # 2,102,500 pixels
    dict(id="big_layout_out", op="layout_out", N=1, C=3, H=1450, W=1450, ld=8, f32=0, mul=0.5, add=0.5),
    dict(id="big_cast", op="cast", M=2100000, C=4, Cpad=8, ld=8, kind="randn", mul=1.0 / SCALING),
    dict(id="big_resize_in", op="resize_in", N=1, C=3, H=725, W=731, RH=1440, RW=1440, PH=10, PW=10, Cpad=8, mul=2.0, add=-1.0),
    # 32 small images, not one large one: the bound's position term grows with the source coordinate, and with it the tie zone (3 % cap)
    dict(id="big_resize_out", op="resize_out", N=32, C=3, XH=132, XW=136, ld=8, CH=129, CW=131, OH=257, OW=257, f32=0, quantize=1, mul=0.5,
         add=0.5, special=False),
    dict(id="big_u8_ingest", op="u8_ingest", CH=1025, CW=1025, geom=[(1025, 1025, 1025, 1025), (600, 700, 1000, 1010)], slack=64),
    dict(id="big_u8_egress", op="u8_egress", CH=182, CW=182, geom=[(182, 182, 182, 182)] * 63 + [(181, 179, 182, 182)], slack=64),   # small images: as above
    dict(id="big_vae", op="vae", N=2, HW=1050000, Clat=4, Cpad=8, ld=8),
    dict(id="big_noise", op="noise", N=2, HW=1050000, Clat=4, Cpad=8, ld=8),
    dict(id="big_ddim", op="ddim", N=2, HW=1050000, Clat=4, Cpad=8, ld_eps=8),
    dict(id="big_gather", op="gather", N=2, LH=600, LW=600, th=513, tw=512, origins=[(0, 0), (0, 88), (87, 0), (87, 88)], Clat=4, Cpad=8, ld_eps=8,
         plan=False),
    dict(id="big_blend", op="blend", N=2, LH=1025, LW=1025, th=600, tw=600, origins=[(0, 0), (0, 425), (425, 0), (425, 425)], Clat=4, Cpad=8,
         ld_eps=8, plan=False),
]


def big_threads(c):
    """Work items (= threads wanted) of the launch."""
    op = c["op"]
    if op in ("layout_in", "layout_out"):
        return c["N"] * c["H"] * c["W"]
    if op == "cast":
        return c["M"]
    if op == "resize_in":
        return c["N"] * (c["RH"] + c["PH"]) * (c["RW"] + c["PW"])
    if op == "resize_out":
        return c["N"] * c["OH"] * c["OW"]
    if op in ("u8_ingest", "u8_egress"):
        return len(c["geom"]) * c["CH"] * c["CW"]
    if op in ("vae", "noise", "ddim"):
        return c["N"] * c["HW"]
    if op == "gather":
        return c["N"] * len(c["origins"]) * c["th"] * c["tw"]
    return c["N"] * c["LH"] * c["LW"]


# ---- properties the table must hold (each by at least one launched case) -----------------------------------------------------------------
def _frac(i, o):
    return o % i != 0 and i % o != 0


LAYOUT_IN_PROPERTIES = {
    "one pixel": lambda c: c["H"] * c["W"] == 1,
    "C == Cpad": lambda c: c["C"] == c["Cpad"],
    "C = 1": lambda c: c["C"] == 1,
    "Cpad = 16": lambda c: c["Cpad"] == 16,
    "odd H and W, N > 1": lambda c: c["H"] % 2 and c["W"] % 2 and c["N"] > 1,
    "more than one block": lambda c: c["N"] * c["H"] * c["W"] > 256,
}
LAYOUT_OUT_PROPERTIES = {
    "ld == C": lambda c: c["ld"] == c["C"],
    "ld > C (NaN columns)": lambda c: c["ld"] > c["C"],
    "fp32 input": lambda c: c["f32"] == 1,
    "16-bit input": lambda c: c["f32"] == 0,
    "mul, add = 0.5, 0.5": lambda c: (c["mul"], c["add"]) == (0.5, 0.5),
    "mul, add = 1, 0": lambda c: (c["mul"], c["add"]) == (1.0, 0.0),
    "mul = 1 / 0.18215": lambda c: c["mul"] == 1.0 / SCALING,
}
CAST_PROPERTIES = {
    "ld == C": lambda c: c["ld"] == c["C"],
    "ld > Cpad": lambda c: c["ld"] > c["Cpad"],
    "C == Cpad": lambda c: c["C"] == c["Cpad"],
    "one row": lambda c: c["M"] == 1,
    "ties, overflow and subnormals with mul = 1": lambda c: c["kind"] == "ties" and c["mul"] == 1.0,
}
RESIZE_IN_PROPERTIES = {
    "non-integer upscale with pad": lambda c: _frac(c["H"], c["RH"]) and c["RH"] > c["H"] and c["PH"] > 0 and c["PW"] > 0,
    "more than 4x down": lambda c: c["H"] > 4 * c["RH"],
    "one source pixel": lambda c: c["H"] == 1 and c["W"] == 1,
    "source narrower than the four taps": lambda c: c["H"] < 4 and c["W"] < 4 and c["H"] * c["W"] > 1,
    "no resize, PH = RH - 1": lambda c: (c["H"], c["W"]) == (c["RH"], c["RW"]) and c["PH"] == c["RH"] - 1 and c["PW"] == c["RW"] - 1,
    "plain copy": lambda c: (c["H"], c["W"], c["PH"], c["PW"]) == (c["RH"], c["RW"], 0, 0),
    "one axis resized": lambda c: c["H"] == c["RH"] and c["W"] != c["RW"],
    "an output whose source position is an exact integer": lambda c: c["H"] == c["RH"] and c["W"] != c["RW"],
    "C = 1, Cpad = 16": lambda c: c["C"] == 1 and c["Cpad"] == 16,
    "N > 1": lambda c: c["N"] > 1,
}
RESIZE_OUT_PROPERTIES = {
    "crop and non-integer downscale": lambda c: c["CH"] < c["XH"] and c["CW"] < c["XW"] and _frac(c["OH"], c["CH"]) and c["OH"] < c["CH"],
    "more than 4x up": lambda c: c["OH"] > 4 * c["CH"],
    "one-pixel window, ld == C + 1": lambda c: c["CH"] * c["CW"] == 1 and c["ld"] == c["C"] + 1,
    "no crop, no resize": lambda c: (c["XH"], c["XW"], c["CH"], c["CW"]) == (c["CH"], c["CW"], c["OH"], c["OW"]),
    "crop only": lambda c: c["CH"] < c["XH"] and (c["CH"], c["CW"]) == (c["OH"], c["OW"]),
    "C = 1, ld = 16": lambda c: c["C"] == 1 and c["ld"] == 16,
    "fp32 input, quantised": lambda c: c["f32"] == 1 and c["quantize"] == 1,
    "16-bit input, quantised": lambda c: c["f32"] == 0 and c["quantize"] == 1,
    "fp32 input, not quantised": lambda c: c["f32"] == 1 and c["quantize"] == 0,
    "16-bit input, not quantised": lambda c: c["f32"] == 0 and c["quantize"] == 0,
}
RAGGED_PROPERTIES = {
    "an image that fills its canvas": lambda c: any((h, w) == (c["CH"], c["CW"]) for h, w, _, _ in c["geom"]),
    "an image that is only padded (RH == H, RW == W, RH < CH)": lambda c: any((h, w) == (rh, rw) and rh < c["CH"] for h, w, rh, rw in c["geom"]),
    "an image resized and padded on both axes": lambda c: any(h < rh < c["CH"] and w < rw < c["CW"] for h, w, rh, rw in c["geom"]),
    "an image resized to the whole canvas": lambda c: any(h < rh == c["CH"] and w < rw == c["CW"] for h, w, rh, rw in c["geom"]),
    "every row obeys ragged_geom_ok": lambda c: all(ragged_geom_ok(*g, c["CH"], c["CW"]) for g in c["geom"]),
    "slot_bytes larger than the canvas": lambda c: c["slack"] > 0,
    "odd sizes": lambda c: any(h % 2 and w % 2 for h, w, _, _ in c["geom"]),
}
VAE_PROPERTIES = {
    "one pixel": lambda c: c["N"] * c["HW"] == 1,
    "Cpad == Clat": lambda c: c["Cpad"] == c["Clat"],
    "Clat = 8": lambda c: c["Clat"] == 8,
    "ld > 2 Clat (NaN columns)": lambda c: c["ld"] > 2 * c["Clat"],
    "ld == 2 Clat": lambda c: c["ld"] == 2 * c["Clat"],
    "N = 3, odd HW": lambda c: c["N"] == 3 and c["HW"] % 2,
}
DDIM_PROPERTIES = {
    "ld_eps == Clat < Cpad": lambda c: c["ld_eps"] == c["Clat"] < c["Cpad"],
    "ld_eps = 8": lambda c: c["ld_eps"] == 8,
    "ld_eps = 16": lambda c: c["ld_eps"] == 16,
    "ld_eps > Cpad": lambda c: c["ld_eps"] > c["Cpad"],
    "Cpad == Clat": lambda c: c["Cpad"] == c["Clat"],
}
TILE_PROPERTIES = {
    "one tile that is the latent": lambda c: len(c["origins"]) == 1 and (c["th"], c["tw"]) == (c["LH"], c["LW"]),
    "pixels covered by one, two and three tiles": lambda c: {1, 2, 3} <= {v for r in tile_cover(c) for v in r},
    "pixels covered by four tiles": lambda c: 4 in {v for r in tile_cover(c) for v in r},
    "a tile that sticks out at the bottom": lambda c: any(y + c["th"] > c["LH"] and y >= 0 and x >= 0 for y, x in c["origins"]),
    "a tile that sticks out at the right": lambda c: any(x + c["tw"] > c["LW"] and y >= 0 and x >= 0 for y, x in c["origins"]),
    "a tile with a negative y origin": lambda c: any(y < 0 for y, _ in c["origins"]),
    "a tile with a negative x origin": lambda c: any(x < 0 for _, x in c["origins"]),
    "pixels no valid tile covers": lambda c: 0 in {v for r in tile_cover(c) for v in r},
    "ld_eps == Clat < Cpad": lambda c: c["ld_eps"] == c["Clat"] < c["Cpad"],
    "Clat = 8": lambda c: c["Clat"] == 8,
    "Cpad = 16 (channels past the eight the kernel keeps)": lambda c: c["Cpad"] == 16,
    "weights of the host plan": lambda c: c["plan"],
    "N > 1": lambda c: c["N"] > 1,
}
BIG_PROPERTIES = {f"second trip: {op}": (lambda c, op=op: c["op"] == op and GRID_THREADS < big_threads(c) < 1.02 * GRID_THREADS)
                  for op in ("layout_in", "layout_out", "cast", "resize_in", "resize_out", "u8_ingest", "u8_egress", "vae", "noise", "ddim", "gather",
                             "blend")}
PROPERTIES = [(LAYOUT_IN_CASES, LAYOUT_IN_PROPERTIES), (LAYOUT_OUT_CASES, LAYOUT_OUT_PROPERTIES), (CAST_CASES, CAST_PROPERTIES),
              (RESIZE_IN_CASES, RESIZE_IN_PROPERTIES), (RESIZE_OUT_CASES, RESIZE_OUT_PROPERTIES), (RAGGED_CANVASES, RAGGED_PROPERTIES),
              (VAE_CASES, VAE_PROPERTIES), (DDIM_CASES, DDIM_PROPERTIES), (TILE_CASES, TILE_PROPERTIES), (BIG_CASES, BIG_PROPERTIES)]
ALL_CASE_LISTS = [LAYOUT_IN_CASES, LAYOUT_OUT_CASES, CAST_CASES, RESIZE_IN_CASES, RESIZE_OUT_CASES, RESIZE_OUT_SPECIAL, RAGGED_CANVASES, VAE_CASES,
                  NOISE_CASES, DDIM_CASES, TILE_CASES, BIG_CASES]


# ---- refusal table: a valid call with ONE thing wrong must return UR_E_INVALID before anything is launched (placeholder pointers) -------------------
_GOOD = {
    "ur_nchw_f32_to_nhwc": dict(x=P, y=P, N=1, C=3, H=4, W=4, Cpad=8, dtype=BF16, stream=None),
    "ur_image_to_nhwc": dict(img=P, y=P, N=1, C=3, H=4, W=4, Cpad=8, dtype=BF16, stream=None),
    "ur_nhwc_to_nchw_f32": dict(x=P, f32=0, out=P, N=1, C=3, H=4, W=4, ld=8, mul=1.0, add=0.0, dtype=BF16, stream=None),
    "ur_f32_to_bf16_scaled": dict(x=P, ld=8, y=P, M=4, C=4, Cpad=8, mul=1.0, dtype=BF16, stream=None),
    "ur_image_resize_pad_nhwc": dict(img=P, y=P, N=1, C=3, H=5, W=7, RH=13, RW=9, PH=3, PW=7, Cpad=8, mul=2.0, add=-1.0, dtype=BF16, stream=None),
    "ur_image_unpad_resize_nchw": dict(x=P, f32=0, out=P, N=1, C=3, XH=16, XW=16, ld=8, CH=13, CW=9, OH=5, OW=7, mul=0.5, add=0.5, quantize=1, dtype=BF16,
                                       stream=None),
    "ur_image_u8_ingest": dict(src=P, slot_bytes=3 * 24 * 20, geom=P, y=P, N=2, CH=24, CW=20, Cpad=8, mul=2.0, add=-1.0, dtype=BF16, stream=None),
    "ur_image_u8_egress": dict(x=P, f32=0, dst=P, slot_bytes=3 * 24 * 20, geom=P, nonfinite=P, N=2, C=3, XH=24, XW=20, ld=8, mul=0.5, add=0.5, dtype=BF16,
                               stream=None),
    "ur_vae_sample": dict(moments=P, ld=8, noise=P, z=P, z16=P, N=1, HW=4, Clat=4, Cpad=8, scale=SCALING, dtype=BF16, stream=None),
    "ur_add_noise": dict(z0=P, noise=P, zt=P, zt16=P, N=1, HW=4, Clat=4, Cpad=8, sa=0.8, sb=0.6, dtype=BF16, stream=None),
    "ur_ddim_step": dict(zt=P, eps=P, ld_eps=8, zt16=P, M=4, Clat=4, Cpad=8, c_x=1.1, c_e=-0.3, dtype=BF16, stream=None),
    "ur_latent_tiles_gather": dict(z=P, tiles=P, N=1, LH=12, LW=10, Cpad=8, T=4, th=8, tw=8, origins=P, dtype=BF16, stream=None),
    "ur_latent_tiles_blend_ddim": dict(zt=P, eps=P, ld_eps=8, tiles=P, wn=P, N=1, LH=12, LW=10, Clat=4, Cpad=8, T=4, th=8, tw=8, origins=P, c_x=1.1,
                                       c_e=-0.3, dtype=BF16, stream=None),
}
_BAD = {
    "ur_nchw_f32_to_nhwc": [dict(x=None), dict(y=None), dict(N=0), dict(C=0), dict(H=0), dict(W=0), dict(W=-4), dict(Cpad=2), dict(dtype=7)],
    "ur_image_to_nhwc": [dict(img=None), dict(y=None), dict(N=0), dict(N=-1), dict(C=0), dict(H=0), dict(W=0), dict(Cpad=2), dict(dtype=7)],
    "ur_nhwc_to_nchw_f32": [dict(x=None), dict(out=None), dict(N=0), dict(C=0), dict(H=0), dict(H=-4), dict(W=0), dict(ld=2), dict(dtype=7)],
    "ur_f32_to_bf16_scaled": [dict(x=None), dict(y=None), dict(M=0), dict(M=-4), dict(C=0), dict(Cpad=2), dict(ld=2), dict(dtype=7)],
    "ur_image_resize_pad_nhwc": [dict(img=None), dict(y=None), dict(N=0), dict(C=0), dict(C=-3), dict(H=0), dict(W=0), dict(RH=0), dict(RW=0), dict(Cpad=2),
                                 dict(PH=13), dict(PW=9), dict(PH=-1), dict(dtype=7)],
    "ur_image_unpad_resize_nchw": [dict(x=None), dict(out=None), dict(N=0), dict(C=0), dict(OH=0), dict(OW=0), dict(ld=2), dict(CH=0), dict(CW=0),
                                   dict(CH=17), dict(CW=17), dict(dtype=7)],
    "ur_image_u8_ingest": [dict(src=None), dict(geom=None), dict(y=None), dict(N=0), dict(CH=0), dict(CW=0), dict(Cpad=2), dict(slot_bytes=3 * 24 * 20 - 1),
                           dict(dtype=7)],
    "ur_image_u8_egress": [dict(x=None), dict(dst=None), dict(geom=None), dict(nonfinite=None), dict(N=0), dict(C=0), dict(XH=0), dict(XW=0), dict(ld=2),
                           dict(slot_bytes=3 * 24 * 20 - 1), dict(dtype=7)],
    "ur_vae_sample": [dict(moments=None), dict(noise=None), dict(z=None), dict(z16=None), dict(N=0), dict(HW=0), dict(HW=-4), dict(Clat=0), dict(Cpad=2),
                      dict(ld=7), dict(dtype=7)],
    "ur_add_noise": [dict(z0=None), dict(noise=None), dict(zt=None), dict(zt16=None), dict(N=0), dict(HW=0), dict(Clat=0), dict(Clat=-4), dict(Cpad=2),
                     dict(dtype=7)],
    "ur_ddim_step": [dict(zt=None), dict(eps=None), dict(zt16=None), dict(M=0), dict(M=-4), dict(Clat=0), dict(Cpad=2), dict(ld_eps=2), dict(dtype=7)],
    "ur_latent_tiles_gather": [dict(z=None), dict(tiles=None), dict(origins=None), dict(N=0), dict(LH=0), dict(LW=0), dict(Cpad=0), dict(T=0), dict(th=0),
                               dict(tw=0), dict(th=13), dict(tw=11), dict(dtype=7)],
    "ur_latent_tiles_blend_ddim": [dict(zt=None), dict(eps=None), dict(tiles=None), dict(wn=None), dict(origins=None), dict(N=0), dict(LH=0), dict(LW=0),
                                   dict(T=0), dict(th=0), dict(tw=0), dict(th=13), dict(Clat=0), dict(Clat=9, Cpad=16, ld_eps=16), dict(Cpad=2),
                                   dict(ld_eps=2), dict(dtype=7)],
}
# the rows the parent commit did not refuse: a launch with a zero or negative element count, or channels silently dropped
PARENT_ACCEPTED = [
    "nchw_f32_to_nhwc:N=0", "nchw_f32_to_nhwc:C=0", "nchw_f32_to_nhwc:H=0", "nchw_f32_to_nhwc:W=0", "nchw_f32_to_nhwc:W=-4",
    "image_to_nhwc:N=0", "image_to_nhwc:N=-1", "image_to_nhwc:C=0", "image_to_nhwc:H=0", "image_to_nhwc:W=0",
    "nhwc_to_nchw_f32:N=0", "nhwc_to_nchw_f32:C=0", "nhwc_to_nchw_f32:H=0", "nhwc_to_nchw_f32:H=-4", "nhwc_to_nchw_f32:W=0",
    "f32_to_bf16_scaled:M=0", "f32_to_bf16_scaled:M=-4", "f32_to_bf16_scaled:C=0",
    "image_resize_pad_nhwc:C=0", "image_resize_pad_nhwc:C=-3", "image_unpad_resize_nchw:C=0",
    "vae_sample:N=0", "vae_sample:HW=0", "vae_sample:HW=-4", "vae_sample:Clat=0",
    "add_noise:N=0", "add_noise:HW=0", "add_noise:Clat=0", "add_noise:Clat=-4", "add_noise:Cpad=2",
    "ddim_step:M=0", "ddim_step:M=-4", "ddim_step:Clat=0", "ddim_step:Cpad=2",
]


def refusals():
    """[(id, function name, argument tuple)]"""
    rows = []
    for fn, bads in _BAD.items():
        for bad in bads:
            assert set(bad) <= set(_GOOD[fn]), (fn, bad)
            args = dict(_GOOD[fn], **bad)
            rows.append((fn[3:] + ":" + ",".join(f"{k}={'NULL' if v is None else v}" for k, v in bad.items()), fn, tuple(args.values())))
    return rows
