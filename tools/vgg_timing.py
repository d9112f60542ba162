"""Time the VGG scoring (`ops.vgg`: the classifier's preprocess + torchvision's VGG16 in exact fp32, csrc/vgg.hip + the convolution
of csrc/f32_layers.hip) on cuda:0.  Seeded random weights (no trained weights are needed to time the kernels).

  python tools/vgg_timing.py --step linear|network [--batch 16 --res 512 --reps 30] [--out profiles/vgg_timing.txt --append]

Prints JSON lines.  --step linear: the three Linears of VGG16 at their real sizes (25088 -> 4096, 4096 -> 4096, 4096 -> 1000) at
M = 2, 16 and 32 rows: ur_vgg_linear_f32 (both launches) beside THE SAME LAYER through f32net.conv2d_f32 on [M,1,1,K] - the only
fp32 GEMM the project had - in one process on one device, alternating, every launch timed by its own hipEvent pair after a 512 MB
fill has evicted the caches (the 67 MB and 16 MB matrices would otherwise stay in the 256 MB Infinity Cache from one repetition to
the next, which no evaluator run gives them), medians over --reps; the weight bytes over the time as GB/s, and that against the
micro-architecture guide's 6.3 TB/s copy figure.  --step network: vgg16 at --batch images of --res x --res: median / min ms per call
of preprocess + network (host clock around each call + device synchronise, after warm-up), and per kernel family - convolutions,
max-pools, Linears - every launch timed by its own hipEvent pair, the median per launch summed, with the family's FLOPs over that
sum as TFLOP/s and its bytes over it as GB/s.
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

HBM_COPY_GBS = 6300.0                        # the micro-architecture guide's achieved copy bandwidth of the whole chip
LAYERS = (("classifier.0", 25088, 4096), ("classifier.3", 4096, 4096), ("classifier.6", 4096, 1000))
ROWS = (2, 16, 32)


def _host_times(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def _cold_pair(a_fn, b_fn, reps, flush):
    """Median ms of two launches measured alternately, each after `flush` was overwritten (the caches hold none of its operands)."""
    for fn in (a_fn, b_fn):
        for _ in range(3):
            fn()
    ta, tb = [], []
    for _ in range(reps):
        for fn, out in ((a_fn, ta), (b_fn, tb)):
            flush.add_(1.0)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            out.append(s.elapsed_time(e))
    return statistics.median(ta), statistics.median(tb), min(ta), min(tb)


def step_linear(a, lines):
    from unirestore_amd import f32net, vgg
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(3)
    flush = torch.zeros(128 << 20, dtype=torch.float32, device=dev)      # 512 MB
    for key, k, n in LAYERS:
        w = (2 * torch.rand(n, k, generator=g) - 1) / k ** 0.5
        b = 0.1 * torch.randn(n, generator=g)
        pl = vgg.PackedLinearF32(w, b, dev)
        pc = f32net.PackedConvF32(w.view(n, k, 1, 1), b, 1, 0, dev)
        del w
        for m in ROWS:
            x = torch.relu(torch.randn(m, k, generator=g)).to(dev)
            ours = lambda: vgg.linear(x, pl, relu=True)                                              # noqa: E731
            conv = lambda: f32net.conv2d_f32(x.view(m, 1, 1, k), pc, relu=True)                      # noqa: E731
            diff = float((ours() - conv().view(m, n)).abs().max())
            new_ms, conv_ms, new_min, conv_min = _cold_pair(ours, conv, a.reps, flush)
            wbytes = 4.0 * n * k
            lines.append(json.dumps(dict(
                compare="ur_vgg_linear_f32 vs f32net.conv2d_f32 on [M,1,1,K]", layer=key, K=k, N=n, M=m, splits=pl.splits,
                workgroups=-(-n // 128) * pl.splits * -(-m // 32), conv_workgroups=-(-m // 128) * -(-n // 64),
                new_ms=round(new_ms, 4), conv_ms=round(conv_ms, 4), new_min_ms=round(new_min, 4), conv_min_ms=round(conv_min, 4),
                ratio_new_over_conv=round(new_ms / conv_ms, 3), clears_0p97=bool(new_ms <= 0.97 * conv_ms),
                new_gb_per_s=round(wbytes / new_ms / 1e6, 1), conv_gb_per_s=round(wbytes / conv_ms / 1e6, 1),
                new_share_of_6p3_tb_per_s=round(wbytes / new_ms / 1e6 / HBM_COPY_GBS, 3), new_tflops=round(2.0 * m * n * k / new_ms / 1e9, 2),
                max_abs_diff=float(f"{diff:.2e}"), reps=a.reps, cold_caches=True, gpu=torch.cuda.get_device_name(0))))
            print(lines[-1], flush=True)
        del pl, pc
        torch.cuda.empty_cache()


def step_network(a, lines):
    from unirestore_amd import classify, f32net, ops, vgg
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.round(torch.rand(a.batch, 3, a.res, a.res, generator=g, device=dev) * 255) / 255
    w = vgg.random_weights("vgg16", 0)
    for _ in range(3):
        ops.vgg(x, w)
    total_ms = _host_times(lambda: ops.vgg(x, w), a.reps)
    prep_ms = _host_times(lambda: classify.preprocess(x), a.reps)
    lines.append(json.dumps(dict(arch="vgg16", batch=a.batch, res=a.res, classes=w.num_classes, hidden=w.hidden,
                                 vgg_ms_median=round(statistics.median(total_ms), 3), vgg_ms_min=round(min(total_ms), 3),
                                 preprocess_ms_median=round(statistics.median(prep_ms), 3), reps=a.reps, gpu=torch.cuda.get_device_name(0))))
    print(lines[-1], flush=True)
    launches = []
    real = dict(conv=f32net.conv2d_f32, pool=vgg.maxpool2, linear=vgg.linear)

    def wrap(fn, family, work):
        def timed(*args, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            y = fn(*args, **kw)
            e.record()
            launches.append((family, s, e) + work(y, *args, **kw))
            return y
        return timed
    f32net.conv2d_f32 = wrap(real["conv"], "convolutions", lambda y, xi, pc, *r, **k: (
        2.0 * (y.numel() // pc.cout) * pc.cout * pc.cin * pc.kh * pc.kw, 4.0 * (xi.numel() + y.numel() + pc.w.numel())))
    vgg.maxpool2 = wrap(real["pool"], "maxpools", lambda y, xi: (0.0, 4.0 * (xi.numel() + y.numel())))
    vgg.linear = wrap(real["linear"], "linears", lambda y, xi, pl, relu=False: (
        2.0 * xi.shape[0] * pl.n * pl.k, 4.0 * (pl.w.numel() + xi.numel() + y.numel() * (1 + 2 * pl.splits))))
    per_launch, meta = None, None
    try:
        for _ in range(a.reps):
            launches.clear()
            vgg.forward(x, w)
            torch.cuda.synchronize()
            ms = [s.elapsed_time(e) for _, s, e, _, _ in launches]
            per_launch = [[m] for m in ms] if per_launch is None else [p + [m] for p, m in zip(per_launch, ms)]
            meta = [(fam, fl, by) for fam, _, _, fl, by in launches]
    finally:
        f32net.conv2d_f32, vgg.maxpool2, vgg.linear = real["conv"], real["pool"], real["linear"]
    families = {}
    for (fam, fl, by), p in zip(meta, per_launch):
        f = families.setdefault(fam, dict(launches=0, ms=0.0, flop=0.0, bytes=0.0))
        f["launches"] += 1
        f["ms"] += statistics.median(p)
        f["flop"] += fl
        f["bytes"] += by
    summed = sum(f["ms"] for f in families.values())
    for fam, f in families.items():
        lines.append(json.dumps(dict(arch="vgg16", family=fam, launches=f["launches"], ms_sum=round(f["ms"], 3), share=round(f["ms"] / summed, 3),
                                     gflop=round(f["flop"] / 1e9, 2), tflops=round(f["flop"] / f["ms"] / 1e9, 2) if f["flop"] else None,
                                     gb_per_s=round(f["bytes"] / f["ms"] / 1e6, 1))))
        print(lines[-1], flush=True)
    lines.append(json.dumps(dict(arch="vgg16", launch_ms_sum=round(summed, 3),
                                 note="the 7 x 7 map skips the adaptive average pool's launch; in the network the Linears follow each "
                                      "other, so the later two may find part of their weights in the Infinity Cache")))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["linear", "network"], required=True)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    lines = []
    (step_linear if a.step == "linear" else step_network)(a, lines)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
