"""Time the evaluator's PSNR / SSIM step for one batch on both metric paths: `ops.image_metrics` (HIP, fp64) and the host fp64
path (`runner.psnr_per_image` + `runner.ssim`, the default `metrics_device="cpu"`), on the same seeded 8-bit-quantised pair on
cuda:0.  The host path is timed from device tensors, as the runner calls it (device-to-host copy included).

  python tools/metrics_timing.py [--batch 8 --res 512 --reps 20 --cpu-reps 3] [--out result.json]

Prints one JSON line: median / min ms per call of each path (GPU: host clock around each call + device synchronise, after
warm-up), the host thread count torch uses, and the largest PSNR / SSIM difference between the paths.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _times(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from unirestore_amd import ops, runner
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    tgt = torch.rand(a.batch, 3, a.res, a.res, generator=g, device=dev)
    pred = (tgt + 0.08 * torch.randn(tgt.shape, generator=g, device=dev)).clamp(0, 1)
    tgt, pred = (torch.round(x * 255) / 255 for x in (tgt, pred))

    def cpu_path():
        return runner.psnr_per_image(pred, tgt).sum(), runner.ssim(pred, tgt) * a.batch

    for _ in range(3):
        ops.image_metrics(pred, tgt)
    gpu_ms = _times(lambda: ops.image_metrics(pred, tgt), a.reps)
    cpu_path()
    cpu_ms = _times(cpu_path, a.cpu_reps)
    ps, ss = ops.image_metrics(pred, tgt)
    cps = runner.psnr_per_image(pred, tgt)
    css = torch.tensor([runner.ssim(pred[i:i + 1], tgt[i:i + 1]) for i in range(a.batch)], dtype=torch.float64)
    res = dict(batch=a.batch, res=a.res, gpu_ms_median=round(statistics.median(gpu_ms), 4), gpu_ms_min=round(min(gpu_ms), 4),
               gpu_reps=a.reps, cpu_ms_median=round(statistics.median(cpu_ms), 1), cpu_ms_min=round(min(cpu_ms), 1),
               cpu_reps=a.cpu_reps, cpu_threads=torch.get_num_threads(), host_cpus=os.cpu_count(),
               max_abs_dpsnr_db=float((ps.cpu() - cps).abs().max()), max_abs_dssim=float((ss.cpu() - css).abs().max()),
               gpu=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
