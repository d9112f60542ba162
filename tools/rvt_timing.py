"""Time the RVT scoring (`ops.rvt`: the classifier's preprocess + the reference's PoolingTransformer in exact fp32, csrc/rvt.hip +
csrc/vit.hip + the convolution of csrc/f32_layers.hip) for one batch on cuda:0.  Seeded random weights (rvt.random_weights: no
trained weights are needed to time the kernels) and seeded 8-bit-quantised images.

  python tools/rvt_timing.py [--batch 16 --res 512 --reps 20 --archs rvt_tiny_plus,rvt_base_plus] [--out profiles/rvt_timing.txt]

Prints JSON lines: (1) per arch, median / min ms per call of preprocess + network (host clock around each call + device synchronise,
after warm-up) and of the preprocess alone; (2) per arch and kernel family - stem convs, qkv, proj, fc1, fc2, head, attention (gated
and not), dwconv (the MLP's and the head pooling), layernorm, gelu, maxpool, avgpool - every launch timed by its own hipEvent pair
in separate passes, the median per launch summed, with the family's FLOPs over that sum as TFLOP/s and its bytes over it as GB/s;
(3) the gated and the ungated attention launch beside ur_vit_attention_f32 on the same 196-token, 12-head, d = 64 tensors, and the
d = 32 launch of rvt_tiny's stage 0; (4) ur_dwconv3x3_f32 with its GELU beside torch's own fp32 F.conv2d(groups=C) + F.gelu on the
same tensors (torch in its own NCHW layout), for the MLP shapes of rvt_tiny and rvt_small and for the head pooling.  Every pair is
taken in one process on one device, alternating, so the two figures of a pair share the box and its clocks.
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


def _pair(a_fn, b_fn, reps):
    """Median ms of two launches measured alternately."""
    for fn in (a_fn, b_fn):
        for _ in range(3):
            fn()
    ta, tb = [], []
    for _ in range(reps):
        ta += _event_times(a_fn, 1)
        tb += _event_times(b_fn, 1)
    return statistics.median(ta), statistics.median(tb)


def time_arch(arch, x, reps, lines):
    from unirestore_amd import classify, f32net, ops, rvt
    w = rvt.random_weights(arch, 0)
    for _ in range(3):
        ops.rvt(x, w)
    total_ms = _host_times(lambda: ops.rvt(x, w), reps)
    prep_ms = _host_times(lambda: classify.preprocess(x), reps)
    lines.append(json.dumps(dict(arch=arch, batch=x.shape[0], res=x.shape[2], classes=w.num_classes, maps=w.maps, dims=w.dims, gated_blocks=len(w.gates),
                                 rvt_ms_median=round(statistics.median(total_ms), 3), rvt_ms_min=round(min(total_ms), 3),
                                 preprocess_ms_median=round(statistics.median(prep_ms), 3), reps=reps, gpu=torch.cuda.get_device_name(0))))
    print(lines[-1])

    def conv_family(key):
        return "stem_convs" if key.startswith("patch_embed") else key if key == "head" else key.rsplit(".", 1)[-1]
    family_of = {id(pc): conv_family(k) for k, pc in w.linears.items()}
    launches = []
    real = dict(conv=f32net.conv2d_f32, ln=f32net.layernorm_f32, gelu=f32net.gelu_f32, pool=f32net.avgpool_f32, maxpool=f32net.maxpool2d_pad_f32,
                attention=rvt.attention, dw=rvt.dwconv3x3)

    def wrap(fn, family, work):
        def timed(*args, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            y = fn(*args, **kw)
            e.record()
            launches.append((family(*args, **kw), s, e) + work(y, *args, **kw))
            return y
        return timed

    def conv_work(y, xi, pc, res=None, relu=True):
        return 2.0 * (y.numel() // pc.cout) * pc.cout * pc.cin * pc.kh * pc.kw, 4.0 * (xi.numel() + y.numel() + pc.w.numel())

    def attn_work(y, qkv, heads, gate=None):
        n, s, d3 = qkv.shape
        return 4.0 * n * s * s * (d3 // 3), 4.0 * (qkv.numel() + y.numel() + (0 if gate is None else gate.numel()))
    f32net.conv2d_f32 = wrap(real["conv"], lambda xi, pc, *r, **k: family_of[id(pc)], conv_work)
    f32net.layernorm_f32 = wrap(real["ln"], lambda *r, **k: "layernorm", lambda y, *r, **k: (0.0, 8.0 * y.numel()))
    f32net.gelu_f32 = wrap(real["gelu"], lambda *r, **k: "gelu", lambda y, *r, **k: (0.0, 8.0 * y.numel()))
    f32net.avgpool_f32 = wrap(real["pool"], lambda *r, **k: "avgpool", lambda y, xi, *r, **k: (0.0, 4.0 * xi.numel()))
    f32net.maxpool2d_pad_f32 = wrap(real["maxpool"], lambda *r, **k: "maxpool", lambda y, xi, *r, **k: (0.0, 4.0 * (xi.numel() + y.numel())))
    rvt.attention = wrap(real["attention"], lambda qkv, heads, gate=None: "attention_gated" if gate is not None else "attention", attn_work)
    rvt.dwconv3x3 = wrap(real["dw"], lambda xi, wt, b, mult=1, stride=1, gelu=False: "dwconv_mlp" if gelu else "dwconv_pool",
                         lambda y, xi, *r, **k: (18.0 * y.numel(), 4.0 * (xi.numel() + y.numel())))
    per_launch, meta = None, None
    try:
        for _ in range(reps):
            launches.clear()
            rvt.forward(x, w)
            torch.cuda.synchronize()
            ms = [s.elapsed_time(e) for _, s, e, _, _ in launches]
            per_launch = [[m] for m in ms] if per_launch is None else [p + [m] for p, m in zip(per_launch, ms)]
            meta = [(fam, fl, by) for fam, _, _, fl, by in launches]
    finally:
        (f32net.conv2d_f32, f32net.layernorm_f32, f32net.gelu_f32, f32net.avgpool_f32, f32net.maxpool2d_pad_f32, rvt.attention, rvt.dwconv3x3) = (
            real["conv"], real["ln"], real["gelu"], real["pool"], real["maxpool"], real["attention"], real["dw"])
    families = {}
    for (fam, fl, by), p in zip(meta, per_launch):
        f = families.setdefault(fam, dict(launches=0, ms=0.0, flop=0.0, bytes=0.0))
        f["launches"] += 1
        f["ms"] += statistics.median(p)
        f["flop"] += fl
        f["bytes"] += by
    summed = sum(f["ms"] for f in families.values())
    for fam, f in families.items():
        lines.append(json.dumps(dict(arch=arch, family=fam, launches=f["launches"], ms_sum=round(f["ms"], 3), share=round(f["ms"] / summed, 3),
                                     gflop=round(f["flop"] / 1e9, 2), tflops=round(f["flop"] / f["ms"] / 1e9, 2) if f["flop"] else None,
                                     gb_per_s=round(f["bytes"] / f["ms"] / 1e6, 1))))
        print(lines[-1])
    lines.append(json.dumps(dict(arch=arch, launch_ms_sum=round(summed, 3))))
    print(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--archs", default="rvt_tiny,rvt_tiny_plus,rvt_small,rvt_small_plus,rvt_base,rvt_base_plus")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from unirestore_amd import f32net, rvt, vit
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.round(torch.rand(a.batch, 3, a.res, a.res, generator=g, device=dev) * 255) / 255
    lines = []
    for arch in a.archs.split(","):
        time_arch(arch, x, a.reps, lines)

    # the attention launches beside the ViT kernel on the same tensors (196 tokens, 12 heads, d = 64), and rvt_tiny's d = 32 launch
    n, s, heads = a.batch, 196, 12
    qkv = torch.randn(n, s, 3 * heads * 64, generator=g, device=dev)
    gate = torch.sigmoid(torch.randn(heads, s, s, generator=g, device=dev))
    assert torch.equal(rvt.attention(qkv, heads), vit.attention(qkv, heads))
    for label, fn in (("ungated", lambda: rvt.attention(qkv, heads)), ("gated", lambda: rvt.attention(qkv, heads, gate))):
        mine, vits = _pair(fn, lambda: vit.attention(qkv, heads), a.reps)
        lines.append(json.dumps(dict(compare=f"rvt attention ({label}) vs ur_vit_attention_f32", shape=[n, s, 3 * heads * 64], heads=heads, d=64,
                                     rvt_ms=round(mine, 4), vit_ms=round(vits, 4), ratio_rvt_over_vit=round(mine / vits, 3))))
        print(lines[-1])
    qkv32 = torch.randn(n, s, 3 * 6 * 32, generator=g, device=dev)
    gate32 = torch.sigmoid(torch.randn(6, s, s, generator=g, device=dev))
    plain, gated = _pair(lambda: rvt.attention(qkv32, 6), lambda: rvt.attention(qkv32, 6, gate32), a.reps)
    lines.append(json.dumps(dict(compare="rvt attention d = 32 (rvt_tiny stage 0), ungated vs gated", shape=[n, s, 3 * 6 * 32], heads=6, d=32,
                                 ungated_ms=round(plain, 4), gated_ms=round(gated, 4))))
    print(lines[-1])

    # the depthwise convolution beside torch's own fp32 operators on the same tensors (torch in NCHW, its own layout)
    for label, side, c, mult, stride, act in (("rvt_tiny stage 0 MLP", 14, 768, 1, 1, True), ("rvt_tiny stage 1 MLP", 7, 1536, 1, 1, True),
                                              ("rvt_small MLP", 14, 1536, 1, 1, True), ("rvt_tiny head pooling", 14, 192, 2, 2, False)):
        xi = torch.randn(n, side, side, c, generator=g, device=dev)
        w4 = torch.randn(c * mult, 1, 3, 3, generator=g, device=dev) / 3
        b = torch.randn(c * mult, generator=g, device=dev)
        wp = rvt.pack_dw_weight(w4.cpu()).to(dev)
        x_nchw = xi.permute(0, 3, 1, 2).contiguous()

        def theirs():
            y = F.conv2d(x_nchw, w4, b, stride=stride, padding=1, groups=c)
            return F.gelu(y) if act else y
        ours = lambda: rvt.dwconv3x3(xi, wp, b, mult, stride, gelu=act)                                   # noqa: E731
        diff = float((ours() - theirs().permute(0, 2, 3, 1)).abs().max())
        mine, torchs = _pair(ours, theirs, a.reps)
        unfused = statistics.median(_event_times(lambda: f32net.gelu_f32(rvt.dwconv3x3(xi, wp, b, mult, stride), inplace=True), a.reps)) if act else None
        lines.append(json.dumps(dict(compare="ur_dwconv3x3_f32 vs torch F.conv2d(groups=C)" + (" + F.gelu" if act else ""), case=label,
                                     shape=[n, side, side, c], mult=mult, stride=stride, hip_ms=round(mine, 4), torch_fp32_ms=round(torchs, 4),
                                     faster="hip" if mine < torchs else "torch", ratio_hip_over_torch=round(mine / torchs, 3),
                                     hip_conv_then_gelu_ms=None if unfused is None else round(unfused, 4), max_abs_diff=float(f"{diff:.2e}"))))
        print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
