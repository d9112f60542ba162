"""Time the RetinaNet scoring (`detect.raw`: torchvision's retinanet_resnet50_fpn_v2 in exact fp32, csrc/detect.hip + the
convolution of csrc/f32_layers.hip) on cuda:0.  Seeded random weights (no trained weights are needed to time the kernels; the
stand-ins pass about 7 % of the largest level's logits through the 0.05 threshold, far more than a trained detector does, so
the select and the NMS see a heavy load).

  python tools/detect_timing.py [--batch 8 --res 512 --reps 20] [--out profiles/detect_timing.txt]

Prints JSON lines.  First `detect.raw` at --batch images of --res x --res: median / min ms per call (host clock around each call +
device synchronise, after warm-up), then per phase - preprocess, trunk, FPN, head convolutions, GroupNorm, select per level,
decode, NMS - every launch group timed by its own hipEvent pair inside the same calls, the median per group summed.  Then
`ur_groupnorm_relu_f32` beside torch's own fp32 `F.relu(F.group_norm(x, 32))` on the five head shapes of that batch (torch on
its own NCHW layout), alternating in one process, medians over --reps.  Records, not thresholds.
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
import torch.nn.functional as F  # noqa: E402

ARCH = "retinanet_resnet50_fpn_v2"


def _host_times(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def step_network(a, lines):
    from unirestore_amd import detect, f32net
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.round(torch.rand(a.batch, 3, a.res, a.res, generator=g, device=dev) * 255) / 255
    w = detect.random_weights(ARCH, 0)
    for _ in range(3):
        out = detect.raw(x, w)
    total_ms = _host_times(lambda: detect.raw(x, w), a.reps)
    lines.append(json.dumps(dict(arch=ARCH, batch=a.batch, res=a.res, classes=w.num_classes, canvas=list(detect.canvas_size(*detect.resized_size(a.res, a.res, w.min_size, w.max_size))),
                                 raw_ms_median=round(statistics.median(total_ms), 3), raw_ms_min=round(min(total_ms), 3),
                                 detections=out[3].cpu().tolist(), reps=a.reps, gpu=torch.cuda.get_device_name(0))))
    print(lines[-1], flush=True)
    groups, state = [], dict(tower=False, level=0)
    names = ("prep", "conv2d_f32", "upsample_nearest_add_f32", "groupnorm_relu_f32", "det_select", "det_decode", "det_nms", "_tower")
    real = {n: getattr(detect, n) for n in names}
    real_trunk = f32net.resnet_trunk

    def wrap(fn, family):
        def timed(*args, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            y = fn(*args, **kw)
            e.record()
            groups.append((family() if callable(family) else family, s, e))
            return y
        return timed

    def tower(*args, **kw):
        state["tower"] = True
        try:
            return real["_tower"](*args, **kw)
        finally:
            state["tower"] = False

    def select_family():
        state["level"] += 1
        return f"select level {(state['level'] - 1) % detect.LEVELS}"
    detect.prep = wrap(real["prep"], "preprocess")
    f32net.resnet_trunk = wrap(real_trunk, "trunk")
    detect.conv2d_f32 = wrap(real["conv2d_f32"], lambda: "head convolutions" if state["tower"] else "FPN convolutions")
    detect.upsample_nearest_add_f32 = wrap(real["upsample_nearest_add_f32"], "FPN nearest + add")
    detect.groupnorm_relu_f32 = wrap(real["groupnorm_relu_f32"], "GroupNorm + ReLU")
    detect.det_select = wrap(real["det_select"], select_family)
    detect.det_decode = wrap(real["det_decode"], "decode")
    detect.det_nms = wrap(real["det_nms"], "NMS")
    detect._tower = tower
    per_group, fams = None, None
    try:
        for _ in range(a.reps):
            groups.clear()
            detect.raw(x, w)
            torch.cuda.synchronize()
            ms = [s.elapsed_time(e) for _, s, e in groups]
            per_group = [[m] for m in ms] if per_group is None else [p + [m] for p, m in zip(per_group, ms)]
            fams = [f for f, _, _ in groups]
    finally:
        for n in names:
            setattr(detect, n, real[n])
        f32net.resnet_trunk = real_trunk
    families = {}
    for fam, p in zip(fams, per_group):
        f = families.setdefault(fam, dict(launch_groups=0, ms=0.0))
        f["launch_groups"] += 1
        f["ms"] += statistics.median(p)
    summed = sum(f["ms"] for f in families.values())
    for fam, f in families.items():
        lines.append(json.dumps(dict(arch=ARCH, phase=fam, launch_groups=f["launch_groups"], ms_sum=round(f["ms"], 3), share=round(f["ms"] / summed, 3))))
        print(lines[-1], flush=True)
    lines.append(json.dumps(dict(arch=ARCH, phase_ms_sum=round(summed, 3),
                                 note="the FPN's and the heads' convolutions include P6 computed twice (once with the ReLU for P7); a select "
                                      "is eleven launches: four histogram + pick passes, count, compaction, sort")))
    print(lines[-1], flush=True)


def step_groupnorm(a, lines):
    from unirestore_amd import detect
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(5)
    w = dict(min_size=800, max_size=1333)
    hp, wp = detect.canvas_size(*detect.resized_size(a.res, a.res, w["min_size"], w["max_size"]))
    gamma, beta = 0.5 + torch.rand(256, generator=g, device=dev), 0.1 * torch.randn(256, generator=g, device=dev)
    for h, wd in detect.level_sizes(hp, wp):
        x = torch.randn(a.batch, h, wd, 256, generator=g, device=dev)
        xt = x.permute(0, 3, 1, 2).contiguous()                       # torch on its own layout
        ours = lambda: detect.groupnorm_relu_f32(x, gamma, beta, 32)                               # noqa: E731
        theirs = lambda: F.relu(F.group_norm(xt, 32, gamma, beta, detect.GN_EPS))                 # noqa: E731
        diff = float((ours().permute(0, 3, 1, 2) - theirs()).abs().max())
        for fn in (ours, theirs):
            for _ in range(3):
                fn()
        ta, tb = [], []
        for _ in range(a.reps):
            for fn, out in ((ours, ta), (theirs, tb)):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                torch.cuda.synchronize()
                out.append(s.elapsed_time(e))
        nbytes = 8.0 * x.numel()
        lines.append(json.dumps(dict(compare="ur_groupnorm_relu_f32 (NHWC) vs torch F.relu(F.group_norm) fp32 (NCHW)", shape=[a.batch, h, wd, 256], groups=32,
                                     ours_ms=round(statistics.median(ta), 4), torch_ms=round(statistics.median(tb), 4),
                                     ours_min_ms=round(min(ta), 4), torch_min_ms=round(min(tb), 4),
                                     ratio_ours_over_torch=round(statistics.median(ta) / statistics.median(tb), 3),
                                     ours_gb_per_s=round(nbytes / statistics.median(ta) / 1e6, 1), max_abs_diff=float(f"{diff:.2e}"), reps=a.reps)))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    step_network(a, lines)
    step_groupnorm(a, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
