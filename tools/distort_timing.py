"""Measured, not gated (profiles/distort_timing.txt): glass_blur, snow and elastic_transform (distort.distort) per 512 x 512 image
on an MI355X at B = 8, severity 3, next to gaussian_blur and zoom_blur (corrupt.corrupt), the nearest older kernels in kind, in the
same run.  HIP events around every one of `reps` warm calls after a warm-up; the median and the smallest call are printed, divided
by B.  A call includes the host-side table building and uploads of the planner.  `python tools/distort_timing.py [--reps 50]` prints
the report; redirect it into profiles/distort_timing.txt."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch
from unirestore_amd import corrupt, distort

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
B, RES, SEV = 8, 512, 3
g = torch.Generator().manual_seed(0)
xd = torch.randint(0, 256, (B, RES, RES, 3), generator=g, dtype=torch.uint8).to(dev)
stems = [f"img_{i:03d}" for i in range(B)]
print(f"{torch.cuda.get_device_name(0)}; B = {B}, {RES} x {RES}, severity {SEV}; HIP events around each of {a.reps} warm calls (tables built "
      "and uploaded per call), ms per image: median and smallest call")
runs = [(n, distort.distort) for n in distort.NAMES] + [("gaussian_blur", corrupt.corrupt), ("zoom_blur", corrupt.corrupt)]
for rep in range(2):                                   # the five alternate twice: the spread between the passes is the noise
    for name, fn in runs:
        for _ in range(5):
            fn(xd, name, SEV, 42, stems)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(xd, name, SEV, 42, stems)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / B)
        print(json.dumps(dict(corruption=name, severity=SEV, pass_=rep, gpu_ms_per_image_median=round(statistics.median(ms), 4),
                              gpu_ms_per_image_min=round(min(ms), 4))))
