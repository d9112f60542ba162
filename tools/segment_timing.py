"""Time the segmenter scoring (`ops.segment`: three scales of preprocess + RefineNet-LW in exact fp32 + the multi-scale argmax;
csrc/segment.hip + csrc/f32_layers.hip) on cuda:0, per shape.  Seeded random weights (segment.random_weights: no trained weights
are needed to time the kernels) and seeded 8-bit-quantised images.

  python tools/segment_timing.py [--arch rflw101 --shapes 8x512x512,2x960x1664 --reps 10] [--out profiles/segment_timing.txt]

Prints one JSON line per shape: median / min ms per call of the whole `ops.segment` (host clock around each call + device
synchronise, after warm-up); the convolutions' share - every convolution launch of the three scales timed by its own hipEvent
pair in separate passes, the median per launch summed, and the FLOPs the network needs (2 M K Cout per launch, from the shapes)
over that sum as TFLOP/s; and `ur_seg_tta_argmax` alone under hipEvents on the three logit maps of that shape, beside torch's own
`interpolate` x 3, `stack`, `mean`, `argmax` on the same device tensors (NCHW copies made outside the timed region) - what the
kernel replaces; no earlier path of this project exists to compare with.
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


def _host_times(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def _event_times(fn, reps):
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="rflw101")
    ap.add_argument("--shapes", default="8x512x512,2x960x1664")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from unirestore_amd import f32net, ops, segment
    dev = torch.device("cuda", 0)
    w = segment.random_weights(a.arch, 0)
    lines = []
    for shape in a.shapes.split(","):
        n, h, wd = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(3)
        x = torch.round(torch.rand(n, 3, h, wd, generator=g, device=dev) * 255) / 255
        for _ in range(2):
            ops.segment(x, w)
        total_ms = _host_times(lambda: ops.segment(x, w), a.reps)
        launches, real = [], f32net.conv2d_f32

        def timed(xi, pc, res=None, relu=True):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            y = real(xi, pc, res, relu)
            e.record()
            launches.append((s, e, 2.0 * y.shape[0] * y.shape[1] * y.shape[2] * pc.cout * pc.cin * pc.kh * pc.kw))
            return y
        per_launch, flops = None, 0.0
        f32net.conv2d_f32 = timed
        try:
            for _ in range(max(a.reps // 2, 3)):
                launches.clear()
                segment.segment(x, w)
                torch.cuda.synchronize()
                ms = [s.elapsed_time(e) for s, e, _ in launches]
                per_launch = [[m] for m in ms] if per_launch is None else [p + [m] for p, m in zip(per_launch, ms)]
                flops = sum(f for _, _, f in launches)
        finally:
            f32net.conv2d_f32 = real
        conv_ms = sum(statistics.median(p) for p in per_launch)
        # the last kernel alone, on this shape's three logit maps, against what it replaces
        maps = [segment.logits(segment.prep(x, (segment.scaled_size(h, s), segment.scaled_size(wd, s))), w) for s in segment.SCALES]
        nchw = [m.permute(0, 3, 1, 2).contiguous() for m in maps]

        def torch_path():
            return torch.stack([F.interpolate(m, size=(h, wd), mode="bilinear", align_corners=True) for m in nchw]).mean(0).argmax(dim=1)
        for _ in range(3):
            pred = segment.tta_argmax(maps, (h, wd))
            ref = torch_path()
        agree = float((pred.long() == ref).float().mean())
        tta_ms = _event_times(lambda: segment.tta_argmax(maps, (h, wd)), a.reps)
        torch_ms = _event_times(torch_path, a.reps)
        lines.append(json.dumps(dict(
            arch=a.arch, batch=n, h=h, w=wd, classes=w.num_classes, segment_ms_median=round(statistics.median(total_ms), 3),
            segment_ms_min=round(min(total_ms), 3), reps=a.reps, conv_launches=len(per_launch), conv_gflop=round(flops / 1e9, 1),
            conv_ms_sum=round(conv_ms, 3), conv_tflops=round(flops / conv_ms / 1e9, 1), fp32_matrix_peak_tflops=155.0,
            tta_argmax_ms_median=round(statistics.median(tta_ms), 4), tta_argmax_ms_min=round(min(tta_ms), 4),
            torch_interp_mean_argmax_ms_median=round(statistics.median(torch_ms), 4), torch_interp_mean_argmax_ms_min=round(min(torch_ms), 4),
            tta_pixels_agreeing_with_torch=round(agree, 6), gpu=torch.cuda.get_device_name(0))))
        print(lines[-1], flush=True)
        del maps, nchw
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
