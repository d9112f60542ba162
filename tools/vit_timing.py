"""Time the ViT scoring (`ops.vit`: the classifier's preprocess + a VisionTransformer in exact fp32, csrc/vit.hip + the
convolution of csrc/f32_layers.hip) for one batch on cuda:0.  Seeded random weights (vit.random_weights: no trained weights are
needed to time the kernels) and seeded 8-bit-quantised images.

  python tools/vit_timing.py [--batch 16 --res 512 --reps 20 --arch vit_b_16] [--out profiles/vit_timing.txt]

Prints JSON lines: (1) median / min ms per call of preprocess + network (host clock around each call + device synchronise, after
warm-up) and of the preprocess alone; (2) per kernel family - patch conv, in_proj, out_proj, fc1, fc2, head, attention, layernorm,
gelu, embed - every launch timed by its own hipEvent pair in separate passes, the median per launch summed, with the FLOPs the
family needs over that sum as TFLOP/s (Linears: 2 M K Cout; attention: 4 N H S^2 d; none for the element-wise families) and
its bytes over it as GB/s; (3) torch's own fp32 F.scaled_dot_product_attention and F.layer_norm on the tensors one layer of the
network hands to the project's kernels, beside those kernels, and which of the two is faster.
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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--arch", default="vit_b_16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from unirestore_amd import classify, f32net, ops, vit
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.round(torch.rand(a.batch, 3, a.res, a.res, generator=g, device=dev) * 255) / 255
    w = vit.random_weights(a.arch, 0)
    cfg = w.config
    for _ in range(3):
        ops.vit(x, w)
    total_ms = _host_times(lambda: ops.vit(x, w), a.reps)
    prep_ms = _host_times(lambda: classify.preprocess(x), a.reps)
    lines = [json.dumps(dict(arch=a.arch, batch=a.batch, res=a.res, classes=w.num_classes, tokens=w.seq_len,
                             vit_ms_median=round(statistics.median(total_ms), 3), vit_ms_min=round(min(total_ms), 3),
                             preprocess_ms_median=round(statistics.median(prep_ms), 3), reps=a.reps, gpu=torch.cuda.get_device_name(0)))]
    print(lines[-1])

    # every launch under its own event pair, by family (separate passes: keep the events out of the end-to-end figure above)
    family_of = {id(pc): ("patch_conv" if k == "conv_proj" else k.rsplit(".", 1)[-1]) for k, pc in w.linears.items()}
    launches = []
    real = dict(conv=f32net.conv2d_f32, ln=f32net.layernorm_f32, gelu=f32net.gelu_f32, embed=vit.embed, attention=vit.attention)

    def wrap(fn, family, work):
        def timed(*args, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            y = fn(*args, **kw)
            e.record()
            launches.append((family(*args), s, e) + work(y, *args, **kw))
            return y
        return timed

    def conv_work(y, xi, pc, res=None, relu=True):
        m = y.numel() // pc.cout
        return 2.0 * m * pc.cout * pc.cin * pc.kh * pc.kw, 4.0 * (xi.numel() + y.numel() * (2 if res is not None else 1) + pc.w.numel())

    def attn_work(y, qkv, heads):
        n, s, _ = qkv.shape
        return 4.0 * n * heads * s * s * vit.HEAD_DIM, 4.0 * (qkv.numel() + y.numel())
    f32net.conv2d_f32 = wrap(real["conv"], lambda xi, pc, *r: family_of[id(pc)], conv_work)
    f32net.layernorm_f32 = wrap(real["ln"], lambda *r: "layernorm", lambda y, xi, *r, **k: (0.0, 4.0 * (y.numel() * 2)))
    f32net.gelu_f32 = wrap(real["gelu"], lambda *r: "gelu", lambda y, *r, **k: (0.0, 8.0 * y.numel()))
    vit.embed = wrap(real["embed"], lambda *r: "embed", lambda y, *r, **k: (0.0, 12.0 * y.numel()))
    vit.attention = wrap(real["attention"], lambda *r: "attention", attn_work)
    per_launch, meta = None, None
    try:
        for _ in range(a.reps):
            launches.clear()
            vit.forward(x, w)
            torch.cuda.synchronize()
            ms = [s.elapsed_time(e) for _, s, e, _, _ in launches]
            per_launch = [[m] for m in ms] if per_launch is None else [p + [m] for p, m in zip(per_launch, ms)]
            meta = [(fam, fl, by) for fam, _, _, fl, by in launches]
    finally:
        f32net.conv2d_f32, f32net.layernorm_f32, f32net.gelu_f32, vit.embed, vit.attention = (
            real["conv"], real["ln"], real["gelu"], real["embed"], real["attention"])
    families = {}
    for (fam, fl, by), p in zip(meta, per_launch):
        f = families.setdefault(fam, dict(launches=0, ms=0.0, flop=0.0, bytes=0.0))
        f["launches"] += 1
        f["ms"] += statistics.median(p)
        f["flop"] += fl
        f["bytes"] += by
    summed = sum(f["ms"] for f in families.values())
    for fam, f in families.items():
        lines.append(json.dumps(dict(family=fam, launches=f["launches"], ms_sum=round(f["ms"], 3), share=round(f["ms"] / summed, 3),
                                     gflop=round(f["flop"] / 1e9, 1), tflops=round(f["flop"] / f["ms"] / 1e9, 1) if f["flop"] else None,
                                     gb_per_s=round(f["bytes"] / f["ms"] / 1e6, 1))))
        print(lines[-1])
    lines.append(json.dumps(dict(launch_ms_sum=round(summed, 3), fp32_matrix_peak_tflops=155.0)))
    print(lines[-1])

    # torch's own fp32 operators on one layer's tensors
    n, s, d, h = a.batch, w.seq_len, cfg.hidden_dim, cfg.num_heads
    tokens = torch.randn(n, s, d, generator=g, device=dev)
    gamma, beta = w.norms["encoder.ln"]
    qkv = torch.randn(n, s, 3 * d, generator=g, device=dev)
    q, k, v = (t.reshape(n, s, h, vit.HEAD_DIM).transpose(1, 2).contiguous() for t in qkv.split(d, dim=2))
    pairs = (("attention", lambda: vit.attention(qkv, h), lambda: F.scaled_dot_product_attention(q, k, v)),
             ("layernorm", lambda: f32net.layernorm_f32(tokens, gamma, beta, vit.LN_EPS), lambda: F.layer_norm(tokens, (d,), gamma, beta, vit.LN_EPS)))
    for name, ours, theirs in pairs:
        for fn in (ours, theirs):
            for _ in range(3):
                fn()
        mine, torchs = statistics.median(_event_times(ours, a.reps)), statistics.median(_event_times(theirs, a.reps))
        lines.append(json.dumps(dict(compare=name, shape=[n, s, d], hip_ms=round(mine, 4), torch_fp32_ms=round(torchs, 4),
                                     faster="hip" if mine < torchs else "torch", ratio_hip_over_torch=round(mine / torchs, 2),
                                     note="torch's attention is timed on already split, head-major q, k, v; the HIP kernel reads in_proj's "
                                          "[N,S,3D] output as it is" if name == "attention" else "same tensors")))
        print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
