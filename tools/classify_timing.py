"""Time the classifier scoring (`ops.classify`: preprocess + ResNet in exact fp32, csrc/classify.hip + csrc/f32_layers.hip) for one
batch on cuda:0, per architecture.  Seeded random weights (classify.random_weights: no trained weights are needed to time the
kernels) and seeded 8-bit-quantised images.

  python tools/classify_timing.py [--batch 16 --res 512 --reps 20 --archs resnet18,resnet50,resnet101] [--out profiles/classify_timing.txt]

Prints one JSON line per architecture: median / min ms per call of preprocess + network (host clock around each call + device
synchronise, after warm-up), of the preprocess alone, and the convolutions' share - every convolution launch (the FC layer
included) timed by its own hipEvent pair in separate passes, the median per launch summed, and the FLOPs the network needs
(2 M K Cout per launch, from the shapes) over that sum as TFLOP/s, beside the 84 TF the same kernel reaches on AlexNet's
five convolutions (profiles/lpips_timing.txt) and MI355X's 155 TF fp32-matrix peak.
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


def _host_times(fn, reps):
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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--archs", default="resnet18,resnet50,resnet101")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from unirestore_amd import classify, f32net, ops
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.round(torch.rand(a.batch, 3, a.res, a.res, generator=g, device=dev) * 255) / 255
    lines = []
    for arch in a.archs.split(","):
        w = classify.random_weights(arch, 0)
        for _ in range(3):
            ops.classify(x, w)
        total_ms = _host_times(lambda: ops.classify(x, w), a.reps)
        prep_ms = _host_times(lambda: classify.preprocess(x), a.reps)
        # every convolution launch under its own event pair (separate passes: the events serialise nothing, but keep them out of
        # the end-to-end figure above)
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
            for _ in range(a.reps):
                launches.clear()
                classify.forward(x, w)
                torch.cuda.synchronize()
                ms = [s.elapsed_time(e) for s, e, _ in launches]
                per_launch = [[m] for m in ms] if per_launch is None else [p + [m] for p, m in zip(per_launch, ms)]
                flops = sum(f for _, _, f in launches)
        finally:
            f32net.conv2d_f32 = real
        conv_ms = sum(statistics.median(p) for p in per_launch)
        lines.append(json.dumps(dict(
            arch=arch, batch=a.batch, res=a.res, classes=w.num_classes, classify_ms_median=round(statistics.median(total_ms), 3),
            classify_ms_min=round(min(total_ms), 3), preprocess_ms_median=round(statistics.median(prep_ms), 3), reps=a.reps,
            conv_launches=len(per_launch), conv_gflop=round(flops / 1e9, 1), conv_ms_sum=round(conv_ms, 3),
            conv_tflops=round(flops / conv_ms / 1e9, 1), alexnet_conv_tflops=84.0, fp32_matrix_peak_tflops=155.0,
            gpu=torch.cuda.get_device_name(0))))
        print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
