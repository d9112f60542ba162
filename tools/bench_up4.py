"""Per-shape timing of the six "nearest-2x upsample + 3x3 conv" layers of the 512 x 512 forward: the 9-tap launch against the folded
one (ur_conv_desc.w_up4, four 2x2 phase convs), in one process.  Event-timed graph replays, as tools/bench_shapes.py.  ONLY=<substring> picks layers.
Matrix-pipe busy of a launch: a counter run of its own,
  NOGRAPH=1 ONLY=640@32 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d <dir> -- python tools/bench_up4.py
and SQ_VALU_MFMA_BUSY_CYCLES / (128 x GRBM_GUI_ACTIVE) per kernel (the normalisation of profiles/r6_pmc_conv_final.json)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
from unirestore_amd import capi, ops


def gtime(f, reps=20):
    """GPU time per call: `reps` launches captured in one hipGraph (no host launch overhead), replayed 3x.
    NOGRAPH=1: plain launches between two events (for a counter-collection run, which sees no kernels inside a graph)."""
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    if os.environ.get("NOGRAPH"):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            f()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (3 * reps)


B = int(os.environ.get("B", 8))
# (name, source H, W, C, launches per forward)
SHAPES = [("unet 640@32->64", 32, 32, 640, 20), ("unet 1280@16->32", 16, 16, 1280, 20), ("unet 1280@8->16", 8, 8, 1280, 20),
          ("vae 256@256->512", 256, 256, 256, 1), ("vae 512@128->256", 128, 128, 512, 1), ("vae 512@64->128", 64, 64, 512, 1)]
names = capi.launcher_names()
print(f"{'layer':20s} {'M':>8s} {'9-tap us':>9s} {'TF/s':>6s} {'folded us':>9s} {'TF/s(4/9)':>9s} {'x':>5s} {'cnt':>4s} {'saved ms/fwd':>12s}  kernel")
tot = 0.0
for name, h, w, c, cnt in SHAPES:
    if os.environ.get("ONLY") and os.environ["ONLY"] not in name:
        continue
    x = torch.randn(B, h, w, c, device="cuda").to(torch.bfloat16)
    wt = torch.randn(c, c, 3, 3) / (9 * c) ** 0.5
    pc = ops.pack_conv(wt, torch.randn(c), "cuda")
    m = B * 4 * h * w
    t9 = gtime(lambda: ops.conv(x, pc, upsample=True, gn=True))
    fl = 2.0 * m * c * c * 9
    plan = ops.conv_plan(x, pc, upsample=True, gn=True, up4=True)
    kern = names[ops.conv_launch(x, pc, upsample=True, gn=True, up4=True).launcher]
    if plan.up4:
        w4 = pc.up4(wt)
        t4 = gtime(lambda: ops.conv(x, pc, upsample=True, gn=True, up4=w4))
        tot += (t9 - t4) * cnt / 1e3
        print(f"{name:20s} {m:8d} {t9:9.1f} {fl / t9 / 1e6:6.0f} {t4:9.1f} {fl * 4 / 9 / t4 / 1e6:9.0f} {t9 / t4:5.2f} {cnt:4d} {(t9 - t4) * cnt / 1e3:12.2f}  {kern} (folded)")
    else:
        print(f"{name:20s} {m:8d} {t9:9.1f} {fl / t9 / 1e6:6.0f} {'-':>9s} {'-':>9s} {'-':>5s} {cnt:4d} {0.0:12.2f}  {kern} (9-tap: not eligible)")
print(f"saved per forward (sum over the folded layers): {tot:.2f} ms")
