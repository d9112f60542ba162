"""The JPEG round trip of ur_jpeg_roundtrip (the specification is the comment above its declaration in include/unirestore_hip.h)
restated in numpy int64: colour conversion, chroma reduction, the forward "islow" DCT, quantisation, dequantisation, the inverse
"islow" DCT, fancy upsampling and colour conversion back.  test_jpeg_cpu.py holds it against Pillow's save + open byte for byte;
test_jpeg_gpu.py holds the kernels against it.  Nothing here is imported from the package under test."""
import numpy as np

# Annex K of the JPEG standard, in natural (row-major) order
LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
                   99] + [99] * 32, dtype=np.int64).reshape(8, 8)
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def D(v, n):
    return (v + (1 << (n - 1))) >> n


def quant_tables(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (LUMA, CHROMA))


def pad_to(p, rows, cols):
    """Edge replication of the last two axes up to rows x cols."""
    return np.pad(p, [(0, 0)] * (p.ndim - 2) + [(0, rows - p.shape[-2]), (0, cols - p.shape[-1])], mode="edge")


def up8(v):
    return (v + 7) // 8 * 8


def fdct_1d(d, first):
    """jfdctint.c along the last axis (8 entries); first: pass 1 (rows), else pass 2 (columns)."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else D(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else D(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    o[2] = D(z1 + t13 * F_0_765, n)
    o[6] = D(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    o[7], o[5], o[3], o[1] = D(t4 + z1 + z3, n), D(t5 + z2 + z4, n), D(t6 + z2 + z3, n), D(t7 + z1 + z4, n)
    return np.stack(o, -1)


def idct_1d(c, first):
    """jidctint.c along the last axis; first: pass 1 (columns, D(., 11)), else pass 2 (rows, D(., 18))."""
    c = [c[..., i] for i in range(8)]
    z1 = (c[2] + c[6]) * F_0_541
    t2, t3 = z1 - c[6] * F_1_847, z1 + c[2] * F_0_765
    t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    n = 11 if first else 18
    return np.stack([D(t10 + t3, n), D(t11 + t2, n), D(t12 + t1, n), D(t13 + t0, n), D(t13 - t0, n), D(t12 - t1, n), D(t11 - t2, n),
                     D(t10 - t3, n)], -1)


def code_plane(p, q):
    """One padded plane [rows, cols] (multiples of 8) of 0..255 through DCT, quantiser and back -> 0..255."""
    r, c = p.shape
    b = p.reshape(r // 8, 8, c // 8, 8).transpose(0, 2, 1, 3) - 128               # [by, bx, y, x]
    b = fdct_1d(b, True)                                                          # rows
    b = fdct_1d(b.swapaxes(-1, -2), False).swapaxes(-1, -2)                        # columns
    d = q << 3
    b = np.sign(b) * ((np.abs(b) + (d >> 1)) // d) * q
    b = idct_1d(b.swapaxes(-1, -2), True).swapaxes(-1, -2)                         # columns
    b = idct_1d(b, False)                                                         # rows
    return np.clip(b + 128, 0, 255).transpose(0, 2, 1, 3).reshape(r, c)


def roundtrip(x, quality, subsampling=2):
    """x uint8 [H, W, 3] or [N, H, W, 3] -> the bytes a baseline JPEG of that quality decodes to (subsampling 0 = 4:4:4, 2 = 4:2:0)."""
    if x.ndim == 4:
        return np.stack([roundtrip(i, quality, subsampling) for i in x])
    assert subsampling in (0, 2) and 1 <= quality <= 100
    h, w, _ = x.shape
    ql, qc = quant_tables(quality)
    r, g, b = (x[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    y = code_plane(pad_to(y, up8(h), up8(w)), ql)[:h, :w]
    if subsampling == 0:
        cb, cr = (code_plane(pad_to(p, up8(h), up8(w)), qc)[:h, :w] for p in (cb, cr))
    else:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        chb, cwb = up8(ch), up8(cw)
        bias = np.where(np.arange(cwb) % 2 == 0, 1, 2)

        def reduce_(p):
            p = pad_to(p, 2 * ch, 2 * cwb)
            s = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
            return pad_to(s, chb, cwb)                 # rows beyond ch copy the last REDUCED row

        def enlarge(p):
            p = p[:ch, :cw]
            above, below = np.vstack([p[:1], p[:-1]]), np.vstack([p[1:], p[-1:]])
            v = np.empty((2 * ch, cw), dtype=np.int64)
            v[0::2], v[1::2] = 3 * p + above, 3 * p + below
            left, right = np.hstack([v[:, :1], v[:, :-1]]), np.hstack([v[:, 1:], v[:, -1:]])
            o = np.empty((2 * ch, 2 * cw), dtype=np.int64)
            o[:, 0::2], o[:, 1::2] = (3 * v + left + 8) >> 4, (3 * v + right + 7) >> 4
            return o[:h, :w]
        cb, cr = (enlarge(code_plane(reduce_(p), qc)) for p in (cb, cr))
    cb, cr = cb - 128, cr - 128
    out = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(out, 0, 255).astype(np.uint8)


def pillow_roundtrip(x, quality, subsampling=2):
    """What the reference's jpeg_compression does to one uint8 [H, W, 3] image, through Pillow."""
    import io

    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    buf.seek(0)
    return np.asarray(Image.open(buf).convert("RGB"))
