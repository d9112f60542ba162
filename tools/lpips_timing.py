"""Time ops.lpips (AlexNet LPIPS, exact fp32, csrc/lpips.hip + csrc/f32_layers.hip) for one evaluator batch, and each of its five convolutions alone.

  python tools/lpips_timing.py [--batch 8 --res 512 --reps 20] [--out result.txt]

Seeded random weights (lpips.random_weights: no real weights are needed to time the kernels) and a seeded 8-bit-quantised pair
on cuda:0.  Prints one JSON line for the whole metric (median / min ms per call, host clock around each call + device
synchronise, after warm-up; 2 * batch images go through AlexNet), then one line per convolution launch (hipEvent pair around
the launch, median of --reps, after warm-up): its GEMM shape, ms, and TFLOP/s beside MI355X's 155 TF fp32-matrix peak (the
fp32-input MFMA runs at the fp32 vector rate) and the 52 TF of an untuned fp32 VALU GEMM.
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

PEAK_TF, VALU_TF = 155.0, 52.0


def _wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def _events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from unirestore_amd import f32net, lpips, ops
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    tgt = torch.rand(a.batch, 3, a.res, a.res, generator=g, device=dev)
    pred = (tgt + 0.08 * torch.randn(tgt.shape, generator=g, device=dev)).clamp(0, 1)
    tgt, pred = (torch.round(x * 255) / 255 for x in (tgt, pred))
    w = lpips.random_weights(0, dev)

    for _ in range(3):
        ops.lpips(pred, tgt, w)
    ms = _wall(lambda: ops.lpips(pred, tgt, w), a.reps)
    lines = []
    f = lpips.prep(torch.cat([pred, tgt]))
    flops_all, conv_ms_all = 0.0, 0.0
    for i, (pc, pool) in enumerate(zip(w.convs, lpips.POOL_BEFORE)):
        if pool:
            f = f32net.maxpool2d_f32(f)
        x = f
        for _ in range(3):
            f = f32net.conv2d_f32(x, pc)
        t = statistics.median(_events(lambda: f32net.conv2d_f32(x, pc), a.reps))
        m, k = f.shape[0] * f.shape[1] * f.shape[2], pc.cin * pc.kh * pc.kw
        flops = 2.0 * m * k * pc.cout
        flops_all += flops
        conv_ms_all += t
        lines.append(json.dumps(dict(conv=i + 1, M=m, K=k, Cout=pc.cout, kernel=f"{pc.kh}x{pc.kw}/{pc.stride}", gflop=round(flops / 1e9, 2),
                                     ms=round(t, 4), tflops=round(flops / t / 1e9, 1), of_fp32_matrix_peak=round(flops / t / 1e9 / PEAK_TF, 3))))
    head = json.dumps(dict(batch=a.batch, res=a.res, images_through_alexnet=2 * a.batch, lpips_ms_median=round(statistics.median(ms), 3),
                           lpips_ms_min=round(min(ms), 3), reps=a.reps, conv_gflop=round(flops_all / 1e9, 1), conv_ms_sum=round(conv_ms_all, 3),
                           conv_tflops=round(flops_all / conv_ms_all / 1e9, 1), fp32_matrix_peak_tflops=PEAK_TF, fp32_valu_gemm_tflops=VALU_TF,
                           gpu=torch.cuda.get_device_name(0)))
    text = "\n".join([head] + lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
