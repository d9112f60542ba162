"""Host restatements for the detector tests: the RetinaNet of unirestore_amd/detect.py in NCHW with torch's own F.conv2d,
F.batch_norm, F.group_norm, F.interpolate, F.relu and torch.sigmoid on the same state dict (fp64 for the reference, fp32 to measure
what fp32 itself loses), and plain-Python select / decode / NMS / mAP.  The tolerances of test_detect_gpu.py are stated here: each
is 4 x the largest error torch's own fp32 CPU forward of the same restatement shows against fp64 on the test's cases (the kernels'
fp64 moments should beat it; the margin covers another summation order), measured by `python tests/detect_reference.py` and
recorded in profiles/detect_tolerances.txt."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from unirestore_amd import detect as D

ARCH = "retinanet_resnet50_fpn_v2"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# ---- measured constants (python tests/detect_reference.py prints them; profiles/detect_tolerances.txt keeps the run) -------------
# GroupNorm: max |fp32 CPU F.group_norm (+ relu) - fp64| over GN_CASES, with and without ReLU
E32_GN = 8.292e-07
GN_TOL = 4 * E32_GN
# network: max over levels, networks (K = 5, 91) and images (40x56, 48x48) of max |fp32 CPU - fp64| / max |fp64| per level
E32_LOGITS, E32_REGS = 1.354e-06, 2.260e-06
LOGITS_TOL, REGS_TOL = 4 * E32_LOGITS, 4 * E32_REGS

GN_CASES = (((2, 5, 7, 64), 32), ((1, 1, 1, 256), 32), ((3, 13, 13, 256), 32), ((1, 9, 4, 96), 3))      # NHWC shape, groups
NEAREST_PAIRS = ((1, 2), (4, 7), (7, 13), (13, 25), (25, 50))
NET_SEED, NET_MIN, NET_MAX = 3, 64, 96
NET_IMAGES = ((40, 56), (48, 48))


def nchw(t):
    return t.permute(0, 3, 1, 2)


def gn_case(shape, groups, seed=0):
    g = torch.Generator().manual_seed(seed + shape[1] * 131 + shape[3])
    x = torch.randn(shape, generator=g) * 2 + 0.5
    return x, 0.5 + torch.rand(shape[3], generator=g), 0.3 * torch.randn(shape[3], generator=g)


def group_norm(x_nhwc, gamma, beta, groups, relu, dtype=torch.float64):
    y = F.group_norm(nchw(x_nhwc).to(dtype), groups, gamma.to(dtype), beta.to(dtype), D.GN_EPS)
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1)


def images(hw, n=2, seed=0):
    g = torch.Generator().manual_seed(seed + hw[0] * 1000 + hw[1])
    return torch.rand(n, 3, hw[0], hw[1], generator=g)


# ---- the network ---------------------------------------------------------------------------------------------------------------

def prep(x, min_size, max_size, dtype=torch.float64):
    """GeneralizedRCNNTransform on one batch of equal-size images: (canvas NCHW, (rh, rw))."""
    x = x.to(dtype)
    x = (x - torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    rh, rw = D.resized_size(x.shape[2], x.shape[3], min_size, max_size)
    x = F.interpolate(x, size=(rh, rw), mode="bilinear", align_corners=False)
    hp, wp = D.canvas_size(rh, rw)
    return F.pad(x, (0, wp - rw, 0, hp - rh)), (rh, rw)


def _bn(x, sd, key, dtype):
    return F.batch_norm(x, sd[f"{key}.running_mean"].to(dtype), sd[f"{key}.running_var"].to(dtype), sd[f"{key}.weight"].to(dtype),
                        sd[f"{key}.bias"].to(dtype), False, 0.0, 1e-5)


def trunk(x, sd, dtype):
    p = "backbone.body."

    def cb(x, c, b, stride, pad):
        return _bn(F.conv2d(x, sd[f"{p}{c}.weight"].to(dtype), None, stride, pad), sd, f"{p}{b}", dtype)
    x = F.max_pool2d(F.relu(cb(x, "conv1", "bn1", 2, 3)), 3, 2, 1)
    feats = []
    for li, depth in enumerate(D.ARCHS[ARCH], 1):
        for bi in range(depth):
            q = f"layer{li}.{bi}"
            stride = 2 if (li > 1 and bi == 0) else 1
            idn = cb(x, f"{q}.downsample.0", f"{q}.downsample.1", stride, 0) if f"{p}{q}.downsample.0.weight" in sd else x
            y = F.relu(cb(x, f"{q}.conv1", f"{q}.bn1", 1, 0))
            y = F.relu(cb(y, f"{q}.conv2", f"{q}.bn2", stride, 1))
            x = F.relu(cb(y, f"{q}.conv3", f"{q}.bn3", 1, 0) + idn)
        feats.append(x)
    return feats[1:]


def _conv(x, sd, key, dtype, stride=1, pad=1, bias=True):
    return F.conv2d(x, sd[f"{key}.weight"].to(dtype), sd[f"{key}.bias"].to(dtype) if bias else None, stride, pad)


def fpn(cs, sd, dtype):
    f = "backbone.fpn."
    inner = _conv(cs[2], sd, f"{f}inner_blocks.2.0", dtype, pad=0)
    out = [None, None, _conv(inner, sd, f"{f}layer_blocks.2.0", dtype)]
    for i in (1, 0):
        lat = _conv(cs[i], sd, f"{f}inner_blocks.{i}.0", dtype, pad=0)
        inner = lat + F.interpolate(inner, size=lat.shape[-2:], mode="nearest")
        out[i] = _conv(inner, sd, f"{f}layer_blocks.{i}.0", dtype)
    p6 = _conv(cs[2], sd, f"{f}extra_blocks.p6", dtype, stride=2)
    p7 = _conv(F.relu(p6), sd, f"{f}extra_blocks.p7", dtype, stride=2)
    return out + [p6, p7]


def tower(x, sd, tower_key, last, dtype):
    for i in range(4):
        x = _conv(x, sd, f"{tower_key}.{i}.0", dtype, bias=False)
        x = F.relu(F.group_norm(x, D.GN_GROUPS, sd[f"{tower_key}.{i}.1.weight"].to(dtype), sd[f"{tower_key}.{i}.1.bias"].to(dtype), D.GN_EPS))
    return _conv(x, sd, last, dtype)


def head_outputs(x, sd, min_size, max_size, dtype=torch.float64):
    """(logits [N, HWA, K] per level, regressions [N, HWA, 4] per level, geometry) as detect.head_outputs, on the host."""
    sd = {k: v for k, v in sd.items()}
    canvas, resized = prep(x, min_size, max_size, dtype)
    feats = fpn(trunk(canvas, sd, dtype), sd, dtype)
    n = x.shape[0]
    k = sd[f"{D.CLS_KEY}.weight"].shape[0] // D.NUM_ANCHORS
    logits = [tower(f, sd, D.TOWERS[0], D.CLS_KEY, dtype).permute(0, 2, 3, 1).reshape(n, -1, k) for f in feats]
    regs = [tower(f, sd, D.TOWERS[1], D.REG_KEY, dtype).permute(0, 2, 3, 1).reshape(n, -1, 4) for f in feats]
    return logits, regs, dict(resized=resized, canvas=tuple(canvas.shape[2:]), sizes=[tuple(f.shape[2:]) for f in feats])


# ---- post-processing, one image at a time, plain Python / numpy ------------------------------------------------------------------

def generate_anchors(level):
    """`AnchorGenerator.generate_anchors` restated with numpy fp32 scalars."""
    out = []
    for r in D.ASPECT_RATIOS:
        hr = np.sqrt(np.float32(r))
        wr = np.float32(1) / hr
        for s in D.ANCHOR_SIZES[level]:
            w, h = wr * np.float32(s), hr * np.float32(s)
            out.append([float(np.round(-w / np.float32(2))), float(np.round(-h / np.float32(2))), float(np.round(w / np.float32(2))),
                        float(np.round(h / np.float32(2)))])
    return out


def select(logits_l, lt, k):
    """logits_l: a [HWA, K] array of one image and level -> (flat indices, logits) of the first min(k, count) candidates > lt in
    the order (logit descending, flat index ascending); a NaN is no candidate."""
    flat = np.asarray(logits_l).reshape(-1)
    with np.errstate(invalid="ignore"):
        idx = np.flatnonzero(flat > lt)
    order = sorted(idx.tolist(), key=lambda i: (-float(flat[i]), i))[:k]
    return np.asarray(order, dtype=np.int64), flat[order] if order else flat[:0]


def sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, dtype=np.float64)))


def decode(reg, anchor_idx, level, wf, strides, img_size, ratios):
    """fp64 boxes of anchors `anchor_idx` of one image and level: (raw, clipped, scaled) [n, 4]."""
    base = np.asarray(generate_anchors(level), dtype=np.float64)
    reg = np.asarray(reg, dtype=np.float64)
    raw = np.zeros((len(anchor_idx), 4))
    for j, an in enumerate(anchor_idx):
        a, cell = an % D.NUM_ANCHORS, an // D.NUM_ANCHORS
        sx, sy = (cell % wf) * strides[1], (cell // wf) * strides[0]
        x1, y1, x2, y2 = base[a] + np.array([sx, sy, sx, sy])
        w, h = x2 - x1, y2 - y1
        cx, cy = x1 + 0.5 * w, y1 + 0.5 * h
        dx, dy, dw, dh = reg[an]
        dw, dh = min(dw, D.BBOX_XFORM_CLIP), min(dh, D.BBOX_XFORM_CLIP)
        pcx, pcy, pw, ph = dx * w + cx, dy * h + cy, math.exp(dw) * w, math.exp(dh) * h
        raw[j] = [pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph]
    clipped = raw.copy()
    clipped[:, 0::2] = np.clip(clipped[:, 0::2], 0, img_size[1])
    clipped[:, 1::2] = np.clip(clipped[:, 1::2], 0, img_size[0])
    scaled = clipped * np.array([ratios[1], ratios[0], ratios[1], ratios[0]])
    return raw, clipped, scaled


def iou(a, b):
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def nms(boxes, scores, labels, thresh, max_out, near=None, dtype=np.float64):
    """Class-aware greedy NMS: the kept positions in the order (score descending, position ascending), at most max_out.  The IoU
    is formed in `dtype` operation by operation as torchvision's nms forms it (np.float32: the kernel's own arithmetic).  near: a
    set that receives every position whose IoU with a kept box of its label lies within 1e-4 of thresh."""
    b = np.asarray(boxes, dtype=dtype).reshape(-1, 4)
    scores, labels = np.asarray(scores), np.asarray(labels)
    order = sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    kept_by_label, keep = {}, []
    zero = dtype(0)
    for i in order:
        mine = kept_by_label.setdefault(int(labels[i]), [])
        ok = True
        if mine:
            k = b[mine]
            iw = np.maximum(np.minimum(k[:, 2], b[i, 2]) - np.maximum(k[:, 0], b[i, 0]), zero)
            ih = np.maximum(np.minimum(k[:, 3], b[i, 3]) - np.maximum(k[:, 1], b[i, 1]), zero)
            inter = iw * ih
            with np.errstate(invalid="ignore", divide="ignore"):
                v = inter / (area[mine] + area[i] - inter)
            if near is not None and bool((np.abs(v.astype(np.float64) - thresh) < 1e-4).any()):
                near.add(i)
            ok = not bool((v > dtype(thresh)).any())
        if ok:
            mine.append(i)
            keep.append(i)
            if len(keep) >= max_out:
                break
    return keep


def postprocess(logits, regs, geometry, orig_size, n, score_thresh, k, nms_thresh, max_out, lt=None):
    """The whole post-processing of image n on per-level arrays (numpy or torch, any dtype): dict(index, level, anchors, labels,
    scores, raw, clipped, scaled, keep, counts) with the candidates concatenated level by level."""
    lt = D.logit_threshold(score_thresh) if lt is None else lt
    (rh, rw), (hp, wp) = geometry["resized"], geometry["canvas"]
    ratios = (float(np.float32(orig_size[0]) / np.float32(rh)), float(np.float32(orig_size[1]) / np.float32(rw)))
    out = dict(index=[], level=[], anchors=[], labels=[], scores=[], logits=[], raw=[], clipped=[], scaled=[], counts=[])
    for l, (lg, rg, (fh, fw)) in enumerate(zip(logits, regs, geometry["sizes"])):
        lg_n, rg_n = np.asarray(lg[n].double().cpu()), np.asarray(rg[n].double().cpu())
        kk = lg_n.shape[-1]
        idx, vals = select(lg_n, lt, k)
        raw, clipped, scaled = decode(rg_n, idx // kk, l, fw, (hp // fh, wp // fw), (rh, rw), ratios)
        out["index"] += idx.tolist(); out["level"] += [l] * len(idx); out["anchors"] += (idx // kk).tolist(); out["labels"] += (idx % kk).tolist()
        out["logits"] += vals.tolist(); out["scores"] += sigmoid64(vals).tolist()
        out["raw"] += raw.tolist(); out["clipped"] += clipped.tolist(); out["scaled"] += scaled.tolist(); out["counts"].append(len(idx))
    out["near"] = set()
    out["keep"] = nms(out["clipped"], out["scores"], out["labels"], nms_thresh, max_out, out["near"])
    return out


# ---- mAP, brute force ------------------------------------------------------------------------------------------------------------

def mean_ap(detections, targets, thr=0.5, max_dets=100):
    """pycocotools' AP at one IoU threshold restated with plain loops: {"map", "per_class"}."""
    classes = sorted({int(c) for t in targets for c in np.asarray(t["labels"]).tolist()} |
                     {int(c) for d in detections for c in np.asarray(d["labels"]).tolist()})
    per_class = {}
    for c in classes:
        rows, n_gt = [], 0
        for img, (d, t) in enumerate(zip(detections, targets)):
            g = [list(map(float, b)) for b, l in zip(np.asarray(t["boxes"]).reshape(-1, 4).tolist(), np.asarray(t["labels"]).tolist()) if l == c]
            n_gt += len(g)
            dd = [(float(s), list(map(float, b))) for b, s, l in zip(np.asarray(d["boxes"]).reshape(-1, 4).tolist(), np.asarray(d["scores"]).tolist(),
                                                                     np.asarray(d["labels"]).tolist()) if l == c]
            dd = sorted(dd, key=lambda e: -e[0])[:max_dets]               # (sorted is stable)
            used = [False] * len(g)
            for s, b in dd:
                best, m = min(thr, 1 - 1e-10), -1
                for j, gb in enumerate(g):
                    if used[j]:
                        continue
                    union = (b[2] - b[0]) * (b[3] - b[1]) + (gb[2] - gb[0]) * (gb[3] - gb[1])
                    iw, ih = max(min(b[2], gb[2]) - max(b[0], gb[0]), 0.0), max(min(b[3], gb[3]) - max(b[1], gb[1]), 0.0)
                    v = iw * ih / (union - iw * ih) if union - iw * ih > 0 else 0.0
                    if v < best:
                        continue
                    best, m = v, j
                if m >= 0:
                    used[m] = True
                rows.append((s, m >= 0))
        if n_gt == 0:
            continue
        rows = sorted(rows, key=lambda e: -e[0])
        tp = fp = 0
        rc, pr = [], []
        for _s, hit in rows:
            tp, fp = tp + hit, fp + (not hit)
            rc.append(tp / n_gt)
            pr.append(tp / (tp + fp + np.spacing(1)))
        for i in range(len(pr) - 1, 0, -1):
            pr[i - 1] = max(pr[i - 1], pr[i])
        total = 0.0
        q = []
        for r in np.linspace(0.0, 1.0, 101):
            i = next((i for i, v in enumerate(rc) if v >= r), None)
            q.append(pr[i] if i is not None else 0.0)
        total = float(np.mean(q))
        per_class[c] = total
    return {"map": float(np.mean(list(per_class.values()))) if per_class else -1.0, "per_class": per_class}


def random_scene(g, n_img=50, classes=4):
    """Seeded random detections and targets with many near-duplicates (ties in IoU and score)."""
    dets, tgts = [], []
    for _ in range(n_img):
        ng = int(torch.randint(0, 5, (1,), generator=g))
        gb = torch.randint(0, 40, (ng, 2), generator=g).float()
        gb = torch.cat([gb, gb + torch.randint(4, 30, (ng, 2), generator=g).float()], 1)
        gl = torch.randint(1, classes + 1, (ng,), generator=g)
        nd = int(torch.randint(0, 9, (1,), generator=g))
        src = torch.randint(0, max(ng, 1), (nd,), generator=g)
        db = (gb[src] if ng else torch.zeros(nd, 4)) + torch.randint(-3, 4, (nd, 4), generator=g).float() * (torch.rand(nd, 1, generator=g) < 0.7)
        db = torch.stack([db[:, 0], db[:, 1], torch.maximum(db[:, 2], db[:, 0] + 1), torch.maximum(db[:, 3], db[:, 1] + 1)], 1)
        dl = torch.where(torch.rand(nd, generator=g) < 0.8, gl[src] if ng else torch.ones(nd, dtype=torch.int64), torch.randint(1, classes + 1, (nd,), generator=g))
        ds = torch.randint(1, 10, (nd,), generator=g).float() / 10
        dets.append(dict(boxes=db, scores=ds, labels=dl))
        tgts.append(dict(boxes=gb, labels=gl))
    return dets, tgts


# ---- measuring the constants -------------------------------------------------------------------------------------------------------

def measure():
    lines = []
    e = 0.0
    for shape, groups in GN_CASES:
        x, gm, bt = gn_case(shape, groups)
        for relu in (False, True):
            err = float((group_norm(x, gm, bt, groups, relu, torch.float32).double() - group_norm(x, gm, bt, groups, relu)).abs().max())
            lines.append(f"groupnorm {shape}/{groups} relu={int(relu)}: max |fp32 CPU - fp64| {err:.3e}")
            e = max(e, err)
    lines.append(f"E32_GN = {e:.3e}  (GN_TOL = 4 x)")
    el = er = 0.0
    for kk in (5, 91):
        sd = D.random_state_dict(ARCH, NET_SEED, kk)
        for hw in NET_IMAGES:
            x = images(hw)
            l64, r64, _ = head_outputs(x, sd, NET_MIN, NET_MAX)
            l32, r32, _ = head_outputs(x, sd, NET_MIN, NET_MAX, torch.float32)
            for lv in range(D.LEVELS):
                a = float((l32[lv].double() - l64[lv]).abs().max() / l64[lv].abs().max())
                b = float((r32[lv].double() - r64[lv]).abs().max() / r64[lv].abs().max())
                lines.append(f"network K={kk} image {hw} level {lv}: logits {a:.3e} of max |logit| {float(l64[lv].abs().max()):.2f}, "
                             f"regressions {b:.3e} of max |reg| {float(r64[lv].abs().max()):.2f}")
                el, er = max(el, a), max(er, b)
    lines.append(f"E32_LOGITS = {el:.3e}, E32_REGS = {er:.3e}  (LOGITS_TOL, REGS_TOL = 4 x)")
    return lines


if __name__ == "__main__":
    print("\n".join(measure()))
