"""JPEG compression as a degradation of clean 8-bit images on the GPU (csrc/jpeg.hip; the kernels' specification is the
ur_jpeg_roundtrip comment of include/unirestore_hip.h, the derivation notes are DESIGN.md 6r).

`roundtrip` returns the bytes Pillow reads back from `save(buf, "JPEG", quality=q)`, which is the reference's `jpeg_compression`
(src/data/corruption), without writing a JPEG: only the lossy steps change pixels.  A quality is an integer 1..100 or one of the
reference's five severities by name ("s1".."s5").  There is no randomness: the result depends on (image, quality, subsampling).
`degrade` is `roundtrip` inside the reference's resize-down / resize-back wrapper (unirestore_amd.resize), whose short edge is drawn
from (seed, stem).
`unirestore_amd.corrupt` still lists jpeg_compression as unbuilt; this module is its sibling, not a member of corrupt.NAMES.
"""
import numpy as np

SEVERITY_QUALITY = (25, 18, 15, 10, 7)             # the reference's jpeg_compression constants, severity 1..5
SUBSAMPLINGS = {"4:2:0": 2, "4:4:4": 0}            # -> Pillow's codes, which ur_jpeg_roundtrip takes
MIN_SIDE = 16                                      # the comparison with Pillow holds from one 16 x 16 MCU upwards

# Annex K of the JPEG standard, natural (row-major) order
LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                 100, 103, 99], dtype=np.int32).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
                   99] + [99] * 32, dtype=np.int32).reshape(8, 8)


def check_quality(quality) -> int:
    if isinstance(quality, bool) or not hasattr(quality, "__index__") or not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be an integer in [1, 100], got {quality!r}")
    return int(quality)


def quality_of(spec) -> int:
    """An integer 1..100 (or its decimal string), or "s1".."s5": the quality of the reference's severity 1..5."""
    if isinstance(spec, str):
        text = spec.strip()
        if len(text) == 2 and text[0] == "s" and text[1] in "12345":
            return SEVERITY_QUALITY[int(text[1]) - 1]
        if not text.isdigit():
            raise ValueError(f"quality {spec!r}: give an integer 1..100 or a severity s1..s5")
        spec = int(text)
    return check_quality(spec)


def subsampling_code(subsampling) -> int:
    """"4:2:0" / "4:4:4" (or Pillow's codes 2 / 0) -> the code ur_jpeg_roundtrip takes."""
    if subsampling in SUBSAMPLINGS:
        return SUBSAMPLINGS[subsampling]
    if not isinstance(subsampling, (str, bool)) and subsampling in SUBSAMPLINGS.values():
        return int(subsampling)
    raise ValueError(f"subsampling {subsampling!r}: choose from {', '.join(SUBSAMPLINGS)}")


def quant_tables(quality):
    """(luminance, chrominance) int32 [8, 8] of a quality, as libjpeg's jpeg_set_quality builds them for a baseline file: the
    Annex-K entry scaled by s = 5000 // quality below 50, else 200 - 2 quality, as (base s + 50) // 100 clamped to [1, 255].
    ur_jpeg_roundtrip builds the same two tables on the host, once per call."""
    q = check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * s + 50) // 100, 1, 255).astype(np.int32) for t in (LUMA, CHROMA))


def roundtrip(images_u8, quality, subsampling="4:2:0"):
    """images_u8: device uint8 [N, H, W, 3] (H, W >= 16) -> the bytes their JPEGs of `quality` (see `quality_of`) decode to, uint8 of
    the same shape.  Every image is compressed on its own: the result does not depend on the batch around it."""
    from . import ops
    q, code = quality_of(quality), subsampling_code(subsampling)
    shape = tuple(getattr(images_u8, "shape", ()))
    if len(shape) == 4 and (shape[1] < MIN_SIDE or shape[2] < MIN_SIDE):
        raise ValueError(f"jpeg.roundtrip: H and W must be >= {MIN_SIDE} (one 4:2:0 MCU), got {shape[1]} x {shape[2]}")
    return ops.jpeg_roundtrip(images_u8, q, code)


def degrade(images_u8, quality, seeds, stems, resize, subsampling="4:2:0"):
    """`roundtrip` inside the reference's resize-down / resize-back wrapper (unirestore_amd.resize.inside), as corrupt.degrade is
    for the corruptions.  resize None: `roundtrip` itself (seeds and stems are not looked at).  resize = (lo, hi), lo >= MIN_SIDE:
    image n's short edge is resize.draw_short_edge(seeds[n], stems[n], lo, hi).  -> uint8 of the input's shape."""
    if resize is None:
        return roundtrip(images_u8, quality, subsampling)
    from . import resize as rz
    q, code = quality_of(quality), subsampling_code(subsampling)
    return rz.inside(images_u8, seeds, stems, resize, lambda batch, s, t: roundtrip(batch, q, code), MIN_SIDE, "jpeg.degrade", rz.MIN_SIDE)


def plan_files(sizes, qualities, batch_size: int):
    """[(quality, [indices])]: every file at every quality, grouped by (shape, quality) in input order, groups cut into batches,
    batches ordered by (first member, the quality's place in the list)."""
    groups = {}
    for k, q in enumerate(qualities):
        for i, hw in enumerate(sizes):
            groups.setdefault((tuple(hw), k, q), []).append(i)
    cuts = [(key[1], key[2], idx[s:s + batch_size]) for key, idx in groups.items() for s in range(0, len(idx), batch_size)]
    cuts.sort(key=lambda c: (c[2][0], c[0]))
    return [(q, idx) for _, q, idx in cuts]
