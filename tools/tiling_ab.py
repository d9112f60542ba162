"""Same-box A/B of tiled latent sampling vs whole-latent sampling: one DiffUIE.forward of the full-size model (seeded random
weights, as bench.py) at B=1, 20 DDIM steps, bf16, task 'ir', timed as hipGraph replays.  One (size, mode) per process, so every
run can sit under its own time limit:

  python tools/tiling_ab.py --res 2048x2048 --mode tiled [--tile 64 --stride 48] [--reps 3] [--out result.json]

Prints one JSON line: ms per forward (mean of `reps` replays after one capture + one warm replay), tile count, peak memory.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", required=True, help="HxW of the input image")
    ap.add_argument("--mode", choices=["whole", "tiled"], required=True)
    ap.add_argument("--tile", type=int, default=64)
    ap.add_argument("--stride", type=int, default=48)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h, w = (int(v) for v in a.res.lower().split("x"))
    from bench import build_model
    from unirestore_amd.modules.model import resize_pad_plan
    dev = torch.device("cuda", 0)
    model = build_model(a.steps, dev, 0, 1, a.dtype)
    if a.mode == "tiled":
        model.set_latent_tiling(a.tile, a.stride)
    rh, rw, ph, pw = resize_pad_plan(h, w)
    lh, lw = (rh + ph) // 8, (rw + pw) // 8
    plan = model._tile_plan(lh, lw)
    g = torch.Generator(device=dev).manual_seed(7)
    img = torch.rand(1, 3, h, w, generator=g, device=dev)
    nz = (torch.randn(1, 4, lh, lw, generator=g, device=dev), torch.randn(1, 4, lh, lw, generator=g, device=dev))
    t0 = time.perf_counter()
    y = model(img, "ir", noise=nz)                 # warm-up + capture + first replay
    torch.cuda.synchronize()
    t_capture = time.perf_counter() - t0
    y = model(img, "ir", noise=nz)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        y = model(img, "ir", noise=nz)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.reps * 1e3
    res = dict(res=f"{h}x{w}", latent=f"{lh}x{lw}", mode=a.mode, tile=a.tile if a.mode == "tiled" else None,
               stride=a.stride if a.mode == "tiled" else None, tiles=1 if plan is None else plan[0], steps=a.steps, dtype=a.dtype,
               ms_per_forward=round(ms, 1), reps=a.reps, capture_s=round(t_capture, 1),
               peak_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1), output_finite=bool(torch.isfinite(y).all()),
               gpu=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
