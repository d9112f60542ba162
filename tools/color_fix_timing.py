"""Timing of the colour fix (ops.color_fix, DiffUIE.set_color_fix) on one MI355X.

  python tools/color_fix_timing.py --ops [--reps 30]
      ops.color_fix alone, both modes, at B = 8, 512 x 512 and at 1 x 1024 x 1024 (ld 8, bf16 source): device events around each call
      after warm-up, next to the bytes a pass has to move (c read + s read + out written) over 8 TB/s.  Under
      `rocprofv3 --kernel-trace --stats -- python tools/color_fix_timing.py --ops --shape 8,512,512` the trace splits a call into
      its kernels (cf_wavelet_cols_kernel, cf_wavelet_rows_kernel, cf_adain_stats_kernel, cf_adain_finalize_kernel,
      cf_adain_apply_kernel).
  python tools/color_fix_timing.py --forward [--reps 9] [--steps 20] [--only-off]
      Full-size model with bench.py's seeded random weights, B = 8 at 512 x 512, graph replay: the fix off, "wavelet" and "adain"
      alternated rep by rep.  --only-off never touches set_color_fix: it also runs on a tree that has none (the parent commit, for
      "off costs nothing" on the same box).
Prints one JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes / s (spec)


def pass_bytes(n, h, w, ld_c=8, ld_s=8):
    """What one pass over the canvas has to move when every padded pixel is touched once: c read + s read + out written."""
    return n * h * w * (4 * ld_c + 2 * ld_s + 4 * ld_c)


def run_ops(a):
    from unirestore_amd import ops
    dev = torch.device("cuda", 0)
    shapes = [tuple(int(v) for v in a.shape.split(","))] if a.shape else [(8, 512, 512), (1, 1024, 1024)]
    g = torch.Generator().manual_seed(5)
    for n, h, w in shapes:
        s = (torch.rand(n, h, w, 8, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
        c = (s.float() * 0.9 + 0.05 + 0.05 * torch.randn(n, h, w, 8, generator=g).to(dev)).contiguous()
        for mode in ("wavelet", "adain"):
            for _ in range(3):
                ops.color_fix(c, s, mode)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for e0, e1 in ev:
                e0.record()
                ops.color_fix(c, s, mode)
                e1.record()
            torch.cuda.synchronize()
            us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
            floor = pass_bytes(n, h, w) / HBM_PEAK * 1e6
            print(json.dumps(dict(op="color_fix", mode=mode, shape=[n, h, w], reps=a.reps, call_us_median=round(statistics.median(us), 1),
                                  call_us_min=round(min(us), 1), pass_bytes=pass_bytes(n, h, w), pass_floor_us=round(floor, 1),
                                  gpu=torch.cuda.get_device_name(0))), flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run_forward(a):
    import bench
    dev = torch.device("cuda", 0)
    m = bench.build_model(a.steps, dev, 0, 1, dtype=a.dtype)
    g = torch.Generator().manual_seed(11)
    b, res = 8, 512
    img = torch.rand(b, 3, res, res, generator=g).to(dev)
    noise = tuple(torch.randn(b, 4, res // 8, res // 8, generator=g).to(dev) for _ in range(2))
    modes = [None] if a.only_off else [None, "wavelet", "adain"]
    times = {mode: [] for mode in modes}

    def call(mode):
        if not a.only_off:
            m.color_fix = mode                       # (not set_color_fix: the graphs of all three modes stay captured)
        return m(img, "ir", noise=noise)
    for mode in modes:
        call(mode), call(mode)                       # capture, then one warm replay
    for _ in range(a.reps):
        for mode in modes:
            times[mode].append(timed(lambda: call(mode)))
    for mode in modes:
        t = times[mode]
        print(json.dumps(dict(case=f"forward B={b} {res}x{res}", fix=mode or "off", steps=a.steps, dtype=a.dtype, reps=a.reps,
                              ms_median=round(statistics.median(t), 2), ms_minmax=[round(min(t), 2), round(max(t), 2)],
                              tree="only-off" if a.only_off else "this")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", action="store_true")
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--shape", default=None, metavar="N,H,W")
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--only-off", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("color_fix_timing.py needs a GPU: it measures, it does not estimate")
    if a.ops:
        a.reps = a.reps or 30
        run_ops(a)
    if a.forward:
        a.reps = a.reps or 9
        with torch.no_grad():
            run_forward(a)


if __name__ == "__main__":
    main()
