"""Time the DeepLabV3+ scoring (`ops.deeplab`: three scales of Normalize + DeepLabV3+ in exact fp32 + the two-stage multi-scale
argmax; csrc/segment.hip + csrc/f32_layers.hip) on cuda:0, per shape.  Seeded random weights (deeplab.random_weights: no trained
weights are needed to time the kernels) and seeded 8-bit-quantised images.

  python tools/deeplab_timing.py [--arch dlv3pr50 --shapes 8x512x512,2x960x1664 --reps 10] [--out profiles/deeplab_timing.txt]

Prints one JSON line per shape: median / min ms per call of the whole `ops.deeplab` (host clock around each call + device
synchronise, after warm-up); the three dilated ASPP launches (3 x 3, 2048 -> 256, dilation 6 / 12 / 18, each into its slice of the
1280-channel tensor) on the scale-1 layer4 map under hipEvents, as TFLOP/s counting every tap (2 M K Cout), beside the same three
launches at dilation 1 and padding 1 - what the dilation costs the gather; and `ur_dlv3_tta_argmax` alone on the three classifier
maps of that shape, beside torch's own `interpolate` x 2 per scale, `stack`, `mean`, `argmax` on the same device tensors (NCHW
copies made outside the timed region) - what the kernel replaces.  With --out the lines are APPENDED to the file, which also
holds the parent / this-commit figures of the two older scorers that share the convolution kernel.
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
    ap.add_argument("--arch", default="dlv3pr50")
    ap.add_argument("--shapes", default="8x512x512,2x960x1664")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from unirestore_amd import deeplab, f32net, ops
    dev = torch.device("cuda", 0)
    w = deeplab.random_weights(a.arch, 0)
    lines = []
    for shape in a.shapes.split(","):
        n, h, wd = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(3)
        x = torch.round(torch.rand(n, 3, h, wd, generator=g, device=dev) * 255) / 255
        for _ in range(2):
            ops.deeplab(x, w)
        total_ms = _host_times(lambda: ops.deeplab(x, w), a.reps)
        # the three dilated ASPP launches on the scale-1 layer4 map, and the same filters at dilation 1
        out = f32net.resnet_trunk(deeplab.prep(x), w.backbone, w.stages)[3]
        branches = torch.empty(n, out.shape[1], out.shape[2], 5 * deeplab.ASPP_CH, dtype=torch.float32, device=dev)
        dilated = [w.convs[f"classifier.aspp.convs.{i}.0"] for i in (1, 2, 3)]
        dense = []
        for pc in dilated:
            d1 = f32net.PackedConvF32.__new__(f32net.PackedConvF32)
            d1.__dict__.update(pc.__dict__)
            d1.pad = d1.dilation = 1
            dense.append(d1)

        def aspp(convs):
            for i, pc in enumerate(convs, 1):
                f32net.conv2d_f32(out, pc, out=(branches, i * deeplab.ASPP_CH))
        flops = 3 * 2.0 * n * out.shape[1] * out.shape[2] * deeplab.ASPP_CH * 2048 * 9
        for _ in range(2):
            aspp(dilated)
            aspp(dense)
        aspp_ms = _event_times(lambda: aspp(dilated), a.reps)
        dense_ms = _event_times(lambda: aspp(dense), a.reps)
        # the last kernel alone, on this shape's three classifier maps, against what it replaces
        sizes = [(deeplab.scaled_size(h, s), deeplab.scaled_size(wd, s)) for s in deeplab.SCALES]
        maps = [deeplab.logits(deeplab.prep(x, sz), w) for sz in sizes]
        nchw = [m.permute(0, 3, 1, 2).contiguous() for m in maps]

        def torch_path():
            ups = [F.interpolate(F.interpolate(m, size=sz, mode="bilinear", align_corners=False), size=(h, wd), mode="bilinear", align_corners=True)
                   for m, sz in zip(nchw, sizes)]
            return torch.stack(ups).mean(0).argmax(dim=1)
        for _ in range(3):
            pred = deeplab.tta_argmax(maps, sizes, (h, wd))
            ref = torch_path()
        agree = float((pred.long() == ref).float().mean())
        tta_ms = _event_times(lambda: deeplab.tta_argmax(maps, sizes, (h, wd)), a.reps)
        torch_ms = _event_times(torch_path, a.reps)
        lines.append(json.dumps(dict(
            arch=a.arch, batch=n, h=h, w=wd, classes=w.num_classes, deeplab_ms_median=round(statistics.median(total_ms), 3),
            deeplab_ms_min=round(min(total_ms), 3), reps=a.reps, aspp_map=[out.shape[1], out.shape[2]], aspp_gflop=round(flops / 1e9, 1),
            aspp_dilated_ms_median=round(statistics.median(aspp_ms), 4), aspp_dilated_tflops=round(flops / statistics.median(aspp_ms) / 1e9, 1),
            aspp_dilation1_ms_median=round(statistics.median(dense_ms), 4), aspp_dilation1_tflops=round(flops / statistics.median(dense_ms) / 1e9, 1),
            fp32_matrix_peak_tflops=155.0, tta_argmax_ms_median=round(statistics.median(tta_ms), 4), tta_argmax_ms_min=round(min(tta_ms), 4),
            torch_interp2_mean_argmax_ms_median=round(statistics.median(torch_ms), 4),
            torch_interp2_mean_argmax_ms_min=round(min(torch_ms), 4), tta_pixels_agreeing_with_torch=round(agree, 6),
            gpu=torch.cuda.get_device_name(0))))
        print(lines[-1], flush=True)
        del maps, nchw, branches, out
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
