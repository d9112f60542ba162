"""Measure how far the two summation orders of tests/niqe_reference.py lie apart on the cases of tests/niqe_cases.py and write
profiles/niqe_tolerances.txt: per case and quantity the measured column-relative difference, the value stored in
niqe_cases.MEASURED (the measurement rounded up) and the GPU tolerance max(16 x stored, 1e-12).  Host only.

    python tools/niqe_tolerances.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import niqe_cases as C  # noqa: E402


def main():
    lines = ["NIQE: order-to-order differences of the fp64 host yardstick (tests/niqe_reference.py, order 0 vs order 1) and the GPU",
             "tolerances they give.  A difference is relative to the largest magnitude of the quantity's column in the case.",
             f"tolerance = max({C.FACTOR:g} x stored, {C.FLOOR:g}); stored = tests/niqe_cases.MEASURED, the measurement rounded up.",
             "", f"{'case':<12} {'quantity':<9} {'stored':<9} {'tolerance':<10} measured here"]
    ok = True
    for case in C.CASES:
        m = C.measure(case)
        for q in C.QUANTITIES:
            lines.append(f"{case:<12} {q:<9} {C.MEASURED[case][q]:.2e}  {C.TOLERANCE[case][q]:.3e}  {m[q]:.3e}")
            ok = ok and C.MEASURED[case][q] >= m[q]
        lines.append(f"{case:<12} smallest margin of an R from a rho midpoint {m['margin']:.3e}; largest order-to-order difference of an R "
                     f"{m['r_diff']:.3e}; same alpha indices: {m['same_index']}; same NaN masks: {m['same_nan']}")
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "niqe_tolerances.txt"), "w") as f:
        f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
