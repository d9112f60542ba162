"""Seeded inputs of the NIQE tests and the tolerances of the GPU checks: the smallest shapes at which each kernel of
csrc/niqe.hip can still go wrong.  No case holds a flat block: inside one, y - mu is rounding noise whose signs decide the
features, and two correct implementations disagree.

  two_blocks    2 x 3 x  96 x 192  uniform noise on the 8-bit grid: the minimum size; every MSCN tile touches the replicate border
  ragged        2 x 3 x 200 x 301  a smooth sinusoid plus Gaussian noise of std 0.02 (image 0) and 0.1 (image 1), 8 bit: cropped to
                                   192 x 288, so the border sits at the crop's edge and not the image's; the small sigma of image 0
                                   is the E[x^2] - mu^2 cancellation
  unquantised   3 x 3 x 192 x 192  fp32 uniform: luma values off the grid get rounded; N = 3
  ycbcr         two_blocks under the other luma formula
"""
import functools
import math

import torch

CASES = ("two_blocks", "ragged", "unquantised", "ycbcr")
SEEDS = {"two_blocks": 11, "ragged": 12, "unquantised": 13, "ycbcr": 11}


def color_space(case: str) -> str:
    return "ycbcr" if case == "ycbcr" else "yiq"


def _q8(x: torch.Tensor) -> torch.Tensor:
    return (torch.round(x.clamp(0, 1) * 255) / 255).float()


def images(case: str) -> torch.Tensor:
    """The fp32 NCHW batch of a case, on the host."""
    g = torch.Generator().manual_seed(SEEDS[case])
    if case in ("two_blocks", "ycbcr"):
        return _q8(torch.rand(2, 3, 96, 192, generator=g, dtype=torch.float64))
    if case == "ragged":
        yy, xx = torch.meshgrid(torch.arange(200, dtype=torch.float64), torch.arange(301, dtype=torch.float64), indexing="ij")
        chans = [0.5 + 0.3 * torch.sin(2 * math.pi * (yy / (61.0 + 7 * c) + xx / (83.0 - 5 * c))) for c in range(3)]
        base = torch.stack(chans)[None].repeat(2, 1, 1, 1)
        std = torch.tensor([0.02, 0.1], dtype=torch.float64).reshape(2, 1, 1, 1)
        return _q8(base + std * torch.randn(2, 3, 200, 301, generator=g, dtype=torch.float64))
    if case == "unquantised":
        return torch.rand(3, 3, 192, 192, generator=g, dtype=torch.float32)
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def reference(case: str) -> dict:
    """The yardstick's intermediates of a case (niqe_reference.pipeline, order 0): computed once, shared, not to be changed."""
    import niqe_reference as ref
    return ref.pipeline(images(case), color_space(case), 0)


PARAMS_SEED = 5


def params_host(seed: int = PARAMS_SEED):
    """(mu [36], cov [36, 36]) of a seeded symmetric positive definite stand-in, built here and not by the product."""
    g = torch.Generator().manual_seed(1000 + seed)
    mu = torch.randn(36, generator=g, dtype=torch.float64)
    a = torch.randn(36, 36, generator=g, dtype=torch.float64)
    return mu, a @ a.T / 36 + 0.1 * torch.eye(36, dtype=torch.float64)


# What the tolerances apply to: a quantity's difference is taken relative to the largest magnitude of its column in the case (the
# "mean" features pass through zero).  Columns: the whole field for luma, halve and mscn; each of the 30 (field, moment) pairs;
# each of the 36 features; the scores of the case.
QUANTITIES = ("halve", "mscn", "moments", "features", "score")
FACTOR = 16.0                                            # the kernels' tree sums follow neither host order
FLOOR = 1e-12

# MEASURED[case][quantity]: the largest column-relative difference between the two summation orders of tests/niqe_reference.py
# (tools/niqe_tolerances.py measures it and writes profiles/niqe_tolerances.txt; tests/test_niqe_cpu.py re-measures it), rounded up
# to two digits.  The smallest margin of an R from a midpoint of the rho grid was 8.1e-8 (unquantised) against an order-to-order
# difference of R of at most 6.2e-14 (ragged): the alpha indices are comparable exactly.
MEASURED = {
    "two_blocks": dict(halve=4.2e-16, mscn=5.3e-14, moments=1.1e-14, features=3.2e-14, score=2.3e-16),
    "ragged": dict(halve=5.2e-16, mscn=1.5e-12, moments=9.7e-14, features=2.2e-13, score=4.4e-16),
    "unquantised": dict(halve=5.6e-16, mscn=5.0e-14, moments=1.1e-14, features=3.6e-14, score=4.6e-16),
    "ycbcr": dict(halve=4.5e-16, mscn=5.6e-14, moments=1.3e-14, features=2.6e-14, score=5.7e-16),
}
# TOLERANCE[case][quantity] = max(16 x MEASURED, 1e-12): what a GPU result may differ from the yardstick by
#   ragged: mscn 2.4e-11, moments 1.552e-12, features 3.52e-12; everything else sits on the floor, 1e-12
TOLERANCE = {case: {q: max(FACTOR * v, FLOOR) for q, v in row.items()} for case, row in MEASURED.items()}
MIN_MARGIN = 1e-9                                        # of an R from the nearest midpoint of the rho grid, relative


def tolerance(case: str, quantity: str) -> float:
    """The GPU tolerance of a quantity (luma is integral and must be equal)."""
    return TOLERANCE[case][quantity]


def measure(case: str) -> dict:
    """Run the yardstick in both summation orders on a case: {quantity: the largest column-relative difference} plus `margin` (the
    smallest relative distance of an R from a rho midpoint), `r_diff` (the largest order-to-order difference of an R) and
    `same_index` / `same_nan` (the alpha indices and NaN masks of the two orders agree)."""
    import niqe_reference as ref
    a, b = reference(case), ref.pipeline(images(case), color_space(case), 1)
    mu, cov = params_host()
    return dict(
        halve=column_rel(b["halve"], a["halve"], 0),
        mscn=max(column_rel(b[k], a[k], 0) for k in ("mscn1", "mscn2")),
        moments=max(column_rel(b[k], a[k], 2) for k in ("moments1", "moments2")),
        features=column_rel(b["features"], a["features"], 1),
        score=column_rel(ref.score(b["features"], mu, cov), ref.score(a["features"], mu, cov), 0),
        margin=min(ref.midpoint_margin(a[k]) for k in ("R1", "R2")),
        r_diff=max(column_rel(b[k], a[k], 0) for k in ("R1", "R2")),
        same_index=all(torch.equal(a[k], b[k]) for k in ("index1", "index2")),
        same_nan=torch.equal(torch.isnan(a["features"]), torch.isnan(b["features"])),
        luma_equal=torch.equal(a["luma"], b["luma"]))


def column_rel(a: torch.Tensor, b: torch.Tensor, column_dims: int) -> float:
    """max over columns of max|a - b| / max|b|: the last `column_dims` axes index the columns, everything in front is reduced.
    NaNs must sit in the same places and are left out."""
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.equal(torch.isnan(a), torch.isnan(b)), "the NaN masks differ"
    lead = a.ndim - column_dims
    fa = a.reshape(-1, *a.shape[lead:]) if lead else a[None]
    fb = b.reshape(-1, *b.shape[lead:]) if lead else b[None]
    d = torch.nan_to_num((fa - fb).abs(), nan=0.0).amax(dim=0)
    ref = torch.nan_to_num(fb.abs(), nan=0.0).amax(dim=0)
    ok = ref > 0
    if not bool(ok.any()):
        return 0.0 if float(d.max()) == 0.0 else float("inf")
    assert float(d[~ok].max() if bool((~ok).any()) else 0.0) == 0.0, "a difference in an all-zero column"
    return float((d[ok] / ref[ok]).max())
