"""Measured, not gated (profiles/resize_timing.txt): the antialiased 8-bit resize and the resize-down / corrupt / resize-back wrapper
on an MI355X at B = 8, 512 x 512.  GPU figures: HIP events around every one of `reps` warm calls (the upload of the cached host
tables and the workspace allocation of a call are inside the figure), median, ms per batch.  Host figure: torch's CPU
interpolate(uint8, antialias=True) of the same batch on the same box at 16 threads, median wall time of `reps` calls.  The resizes:
512 -> 128 (the reference's smallest short edge), 512 -> 333, 128 -> 512 and 333 -> 512 (the way back), bilinear and bicubic; every
GPU result is compared with the host's bytes.  Then corrupt.corrupt against corrupt.degrade(resize=(128, 512)) for four corruptions.
`python tools/resize_timing.py [--reps 50]` prints the report; redirect it into profiles/resize_timing.txt."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch
import torch.nn.functional as F
from unirestore_amd import corrupt, resize

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--threads", type=int, default=16)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
torch.set_num_threads(a.threads)
torch.cuda.set_device(0)
B, RES = 8, 512
yy, xx = np.mgrid[0:RES, 0:RES]
base = np.stack([128 + 100 * np.sin(0.02 * (i + 1) * xx + i) * np.cos(0.015 * (i + 2) * yy) for i in range(3)], -1)
x = torch.stack([torch.from_numpy(np.clip(np.roll(base, 37 * n, 1) + np.random.default_rng(n).normal(0, 6, base.shape), 0, 255).astype(np.uint8))
                 for n in range(B)])


def gpu_ms(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def cpu_ms(fn):
    for _ in range(3):
        fn()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


print(f"{torch.cuda.get_device_name(0)}; B = {B}; GPU: HIP events around each of {a.reps} warm calls, median ms per batch; host: "
      f"F.interpolate(uint8 NCHW, antialias=True), {torch.get_num_threads()} threads, {torch.backends.cpu.get_cpu_capability()}, median ms per batch")
for mode in ("bilinear", "bicubic"):
    for src, dst in ((512, 128), (512, 333), (128, 512), (333, 512)):
        xs = x if src == RES else torch.from_numpy(np.ascontiguousarray(x.numpy()[:, :src, :src]))
        xd = xs.cuda()
        nchw = xs.permute(0, 3, 1, 2).contiguous()
        y = resize.resize_u8(xd, (dst, dst), mode)
        host = F.interpolate(nchw, size=(dst, dst), mode=mode, antialias=True)
        equal = bool(torch.equal(y.cpu(), host.permute(0, 2, 3, 1)))
        print(json.dumps(dict(mode=mode, resize=f"{src} -> {dst}", gpu_ms_per_batch=round(gpu_ms(lambda: resize.resize_u8(xd, (dst, dst), mode)), 4),
                              host_ms_per_batch=round(cpu_ms(lambda: F.interpolate(nchw, size=(dst, dst), mode=mode, antialias=True)), 3),
                              equal_to_host=equal)))
xd = x.cuda()
stems = [f"img_{n:03d}" for n in range(B)]
edges = [resize.draw_short_edge(42, s, 128, 512) for s in stems]
print(f"corrupt.corrupt at 512 x 512 against corrupt.degrade(resize=(128, 512)), severity 3, seed 42; the eight short edges: {edges} "
      "(eight groups of one image: sixteen resizes and eight corruptions per call)")
for name in ("contrast", "gaussian_noise", "gaussian_blur", "pixelate"):
    print(json.dumps(dict(corruption=name, corrupt_ms_per_batch=round(gpu_ms(lambda: corrupt.corrupt(xd, name, 3, 42, stems)), 4),
                          degrade_ms_per_batch=round(gpu_ms(lambda: corrupt.degrade(xd, name, 3, 42, stems, resize=(128, 512))), 4))))
