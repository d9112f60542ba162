"""Time the Swin-V2 scoring (`ops.swin`: the classifier's preprocess + a SwinTransformer V2 in exact fp32, csrc/swin.hip +
csrc/vit.hip + the convolution of csrc/f32_layers.hip) for one batch on cuda:0.  Seeded random weights (swin.random_weights: no
trained weights are needed to time the kernels) and seeded 8-bit-quantised images.

  python tools/swin_timing.py [--batch 16 --res 512 --reps 20 --arch swin_v2_b] [--others] [--out profiles/swin_timing.txt]

Prints JSON lines: (1) median / min ms per call of preprocess + network (host clock around each call + device synchronise, after
warm-up) and of the preprocess alone; (2) per kernel family - patch conv, qkv, proj, mlp.0, mlp.3, reduction, head, window
attention, layernorm, layernorm_res, gelu, avgpool - every launch timed by its own hipEvent pair in separate passes, the median per
launch summed, with the FLOPs the family needs over that sum as TFLOP/s (Linears: 2 M K Cout; window attention: 4 x 64 x 64 x 32 per
(image, window, head), padded windows included; none for the element-wise families) and its bytes over it as GB/s; (3) the window
attention kernel beside torch's own fp32 operators for what it fuses - F.pad, torch.roll, the window partition, F.normalize, the
two matmuls with bias, mask and softmax, the reverse, the roll back and the crop - on the tensors one shifted block of the network
hands to it, and which of the two is faster; (4) with --others, `ops.classify` (resnet50) and `ops.vit` (vit_b_16) on the same
batch: the figures to hold against the same call on the parent commit, whose kernels this change does not edit.
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


def torch_window_attention(qkv, qkv_bias, scale, bias, shift, mask):
    """torch's own fp32 operators for what ur_swin_attention_f32 fuses, on the same inputs: the padded places take qkv_bias."""
    n, h, w, c3 = qkv.shape
    c, heads = c3 // 3, c3 // 96
    ph, pw = -(-h // 8) * 8, -(-w // 8) * 8
    x = F.pad(qkv - qkv_bias, (0, 0, 0, pw - w, 0, ph - h)) + qkv_bias
    sy, sx = (shift if ph > 8 else 0), (shift if pw > 8 else 0)
    if sy or sx:
        x = torch.roll(x, shifts=(-sy, -sx), dims=(1, 2))
    x = x.view(n, ph // 8, 8, pw // 8, 8, c3).permute(0, 1, 3, 2, 4, 5).reshape(-1, 64, c3)
    q, k, v = x.reshape(-1, 64, 3, heads, 32).permute(2, 0, 3, 1, 4)
    attn = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1) * scale.view(heads, 1, 1) + bias
    if mask is not None:
        nw = mask.shape[0]
        attn = (attn.view(-1, nw, heads, 64, 64) + mask.view(1, nw, 1, 64, 64)).view(-1, heads, 64, 64)
    y = (F.softmax(attn, dim=-1) @ v).transpose(1, 2).reshape(-1, 64, c)
    y = y.view(n, ph // 8, pw // 8, 8, 8, c).permute(0, 1, 3, 2, 4, 5).reshape(n, ph, pw, c)
    if sy or sx:
        y = torch.roll(y, shifts=(sy, sx), dims=(1, 2))
    return y[:, :h, :w].contiguous()


def region_mask(h, w, shift, dev):
    ph, pw = -(-h // 8) * 8, -(-w // 8) * 8
    sy, sx = (shift if ph > 8 else 0), (shift if pw > 8 else 0)
    if not (sy or sx):
        return None
    ids = torch.zeros(ph, pw, device=dev)
    count = 0
    for ys in ((0, -8), (-8, -sy), (-sy, None)):
        for xs in ((0, -8), (-8, -sx), (-sx, None)):
            ids[ys[0]:ys[1], xs[0]:xs[1]] = count
            count += 1
    ids = ids.view(ph // 8, 8, pw // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64)
    diff = ids.unsqueeze(1) - ids.unsqueeze(2)
    return torch.where(diff != 0, -100.0, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--arch", default="swin_v2_b")
    ap.add_argument("--others", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from unirestore_amd import classify, f32net, ops, swin
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.round(torch.rand(a.batch, 3, a.res, a.res, generator=g, device=dev) * 255) / 255
    w = swin.random_weights(a.arch, 0)
    cfg = w.config
    for _ in range(3):
        ops.swin(x, w)
    total_ms = _host_times(lambda: ops.swin(x, w), a.reps)
    prep_ms = _host_times(lambda: classify.preprocess(x), a.reps)
    lines = [json.dumps(dict(arch=a.arch, batch=a.batch, res=a.res, classes=w.num_classes, maps=swin.maps(cfg),
                             swin_ms_median=round(statistics.median(total_ms), 3), swin_ms_min=round(min(total_ms), 3),
                             preprocess_ms_median=round(statistics.median(prep_ms), 3), reps=a.reps, gpu=torch.cuda.get_device_name(0)))]
    print(lines[-1])

    # every launch under its own event pair, by family (separate passes: keep the events out of the end-to-end figure above)
    def conv_family(key):
        return "patch_conv" if key == "features.0.0" else key if key == "head" else key.split(".", 3)[-1] if ".attn." in key or ".mlp." in key else "reduction"
    family_of = {id(pc): conv_family(k) for k, pc in w.linears.items()}
    launches = []
    real = dict(conv=f32net.conv2d_f32, ln=f32net.layernorm_f32, gelu=f32net.gelu_f32, pool=f32net.avgpool_f32, attention=swin.window_attention,
                lnres=swin.layernorm_res)

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
        return 2.0 * m * pc.cout * pc.cin * pc.kh * pc.kw, 4.0 * (xi.numel() + y.numel() + pc.w.numel())

    def attn_work(y, qkv, *rest):
        n, h, wd, c3 = qkv.shape
        units = n * (-(-h // 8)) * (-(-wd // 8)) * (c3 // 96)
        return 4.0 * units * 64 * 64 * 32, 4.0 * (qkv.numel() + y.numel())
    f32net.conv2d_f32 = wrap(real["conv"], lambda xi, pc, *r: family_of[id(pc)], conv_work)
    f32net.layernorm_f32 = wrap(real["ln"], lambda *r: "layernorm", lambda y, *r, **k: (0.0, 8.0 * y.numel()))
    f32net.gelu_f32 = wrap(real["gelu"], lambda *r: "gelu", lambda y, *r, **k: (0.0, 8.0 * y.numel()))
    f32net.avgpool_f32 = wrap(real["pool"], lambda *r: "avgpool", lambda y, xi, *r, **k: (0.0, 4.0 * xi.numel()))
    swin.window_attention = wrap(real["attention"], lambda *r: "window_attention", attn_work)
    swin.layernorm_res = wrap(real["lnres"], lambda *r: "layernorm_res", lambda y, *r, **k: (0.0, 12.0 * y.numel()))
    per_launch, meta = None, None
    try:
        for _ in range(a.reps):
            launches.clear()
            swin.forward(x, w)
            torch.cuda.synchronize()
            ms = [s.elapsed_time(e) for _, s, e, _, _ in launches]
            per_launch = [[m] for m in ms] if per_launch is None else [p + [m] for p, m in zip(per_launch, ms)]
            meta = [(fam, fl, by) for fam, _, _, fl, by in launches]
    finally:
        f32net.conv2d_f32, f32net.layernorm_f32, f32net.gelu_f32, f32net.avgpool_f32, swin.window_attention, swin.layernorm_res = (
            real["conv"], real["ln"], real["gelu"], real["pool"], real["attention"], real["lnres"])
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
    linear_ms = sum(f["ms"] for fam, f in families.items() if f["flop"] and fam != "window_attention")
    linear_flop = sum(f["flop"] for fam, f in families.items() if f["flop"] and fam != "window_attention")
    lines.append(json.dumps(dict(launch_ms_sum=round(summed, 3), linears_ms_sum=round(linear_ms, 3), linears_tflops=round(linear_flop / linear_ms / 1e9, 1),
                                 fp32_matrix_peak_tflops=155.0)))
    print(lines[-1])

    # torch's own fp32 operators on the tensors of one shifted block per stage
    for stage, side in enumerate(swin.maps(cfg)):
        pre = f"features.{2 * stage + 1}.1"
        if pre not in w.attn:
            continue
        qkv_bias, scale, bias = w.attn[pre]
        n, c = a.batch, cfg.embed_dim * 2 ** stage
        qkv = torch.randn(n, side, side, 3 * c, generator=g, device=dev)
        mask = region_mask(side, side, swin.SHIFT, dev)
        ours = lambda: swin.window_attention(qkv, qkv_bias, scale, bias, swin.SHIFT)                      # noqa: E731
        theirs = lambda: torch_window_attention(qkv, qkv_bias, scale, bias, swin.SHIFT, mask)            # noqa: E731
        diff = float((ours() - theirs()).abs().max())
        for fn in (ours, theirs):
            for _ in range(3):
                fn()
        mine, torchs = statistics.median(_event_times(ours, a.reps)), statistics.median(_event_times(theirs, a.reps))
        lines.append(json.dumps(dict(compare="window_attention", block=pre, shape=[n, side, side, 3 * c], hip_ms=round(mine, 4),
                                     torch_fp32_ms=round(torchs, 4), faster="hip" if mine < torchs else "torch",
                                     ratio_hip_over_torch=round(mine / torchs, 3), max_abs_diff=float(f"{diff:.2e}"),
                                     note="torch: pad + roll + partition + normalize + two matmuls with bias, mask and softmax + reverse + roll "
                                          "back + crop as separate fp32 operators, the mask built beforehand; both read the qkv Linear's output")))
        print(lines[-1])
    if a.others:
        from unirestore_amd import vit
        for name, fn in (("classify resnet50", (lambda wr: lambda: ops.classify(x, wr))(classify.random_weights("resnet50", 0, 1000))),
                         ("vit vit_b_16", (lambda wv: lambda: ops.vit(x, wv))(vit.random_weights("vit_b_16", 0)))):
            for _ in range(3):
                fn()
            ms = _host_times(fn, a.reps)
            lines.append(json.dumps(dict(existing=name, batch=a.batch, res=a.res, ms_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3))))
            print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
