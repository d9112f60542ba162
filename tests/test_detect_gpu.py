"""RetinaNet scoring on the GPU (unirestore_amd/detect.py, csrc/detect.hip): every new kernel against its host restatement
(detect_reference.py) - GroupNorm + ReLU and the whole network against fp64 within 4 x torch's own measured fp32 error, the
nearest-upsample sum against torch's bits, the thresholded top-k, the decode and the NMS on cases whose decisions are exact - then
the pipeline end to end, batch-place independence, bit-reproducibility (eager and graph replay), a NaN image, and the caller path
(LitUniFIE, cli.validate).  The weights are seeded stand-ins - no trained weights exist where this runs, so nothing here says
anything about any published mAP."""
import copy
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detect_reference as R
from test_detect_cpu import write_pairs
from tiny_cfg import TINY, model_kwargs, randomise_
from unirestore_amd import detect

pytestmark = pytest.mark.gpu

_W, _REF = {}, {}


def _weights(k=5, **kw):
    """The stand-in weights of a case on the device, from the SAME state dict the fp64 restatement reads."""
    key = (k, tuple(sorted(kw.items())))
    if key not in _W:
        kw = dict(dict(min_size=R.NET_MIN, max_size=R.NET_MAX), **kw)
        _W[key] = detect.DetectorWeights(R.ARCH, detect.random_state_dict(R.ARCH, R.NET_SEED, k), **kw)
    return _W[key]


def _reference(k, hw):
    """The fp64 head outputs of the case's two images: computed once, shared, never changed."""
    if (k, hw) not in _REF:
        _REF[(k, hw)] = R.head_outputs(R.images(hw), detect.random_state_dict(R.ARCH, R.NET_SEED, k), R.NET_MIN, R.NET_MAX)
    return _REF[(k, hw)]


# ---- GroupNorm + ReLU ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,groups", R.GN_CASES, ids=["x".join(map(str, c[0])) for c in R.GN_CASES])
def test_groupnorm_relu_matches_fp64(shape, groups):
    x, gm, bt = R.gn_case(shape, groups)
    for relu in (False, True):
        want = R.group_norm(x, gm, bt, groups, relu)
        got = detect.groupnorm_relu_f32(x.cuda(), gm.cuda(), bt.cuda(), groups, relu=relu)
        err = float((got.cpu().double() - want).abs().max())
        print(f"groupnorm {shape}/{groups} relu={int(relu)}: max |err| {err:.2e} (bound {R.GN_TOL:.2e}, fp32 CPU {R.E32_GN:.2e})")
        assert tuple(got.shape) == shape and err <= R.GN_TOL
        if relu:
            assert float(got.min()) == 0.0
    # a pointer that is 4 but not 16 bytes aligned, for the input, the parameters and (through the allocator) nothing else
    buf = torch.zeros(x.numel() + 1, device="cuda")
    buf[1:] = x.cuda().view(-1)
    par = torch.zeros(2 * shape[3] + 3, device="cuda")
    par[1:1 + shape[3]], par[2 + shape[3]:2 + 2 * shape[3]] = gm.cuda(), bt.cuda()
    xs, gs, bs = buf[1:].view(shape), par[1:1 + shape[3]], par[2 + shape[3]:2 + 2 * shape[3]]
    assert xs.data_ptr() % 16 == 4 and gs.data_ptr() % 16 == 4
    assert torch.equal(detect.groupnorm_relu_f32(xs, gs, bs, groups), detect.groupnorm_relu_f32(x.cuda(), gm.cuda(), bt.cuda(), groups))


def test_groupnorm_nan_stays_in_its_image():
    shape, groups = (3, 13, 13, 256), 32
    x, gm, bt = R.gn_case(shape, groups)
    clean = detect.groupnorm_relu_f32(x.cuda(), gm.cuda(), bt.cuda(), groups)
    x[1, 4, 5, 77] = float("nan")
    got = detect.groupnorm_relu_f32(x.cuda(), gm.cuda(), bt.cuda(), groups)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    g = 77 // 8
    assert bool(torch.isnan(got[1, :, :, 8 * g:8 * g + 8]).all())                 # the NaN's own group
    rest = torch.ones(256, dtype=torch.bool)
    rest[8 * g:8 * g + 8] = False
    assert torch.equal(got[1][..., rest.cuda()], clean[1][..., rest.cuda()])     # and nothing else of that image
    with pytest.raises(ValueError):
        detect.groupnorm_relu_f32(x.cuda(), gm.cuda(), bt.cuda(), 7)


# ---- lateral + nearest(top) ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [256, 3])
def test_upsample_nearest_add_is_torchs_bits(c):
    g = torch.Generator().manual_seed(c)
    pairs = R.NEAREST_PAIRS
    for i, (h, oh) in enumerate(pairs):
        w, ow = pairs[(i + 2) % len(pairs)]                        # the axes mixed: 4 x 13 -> 7 x 25 among them
        a, b = torch.randn(2, oh, ow, c, generator=g).cuda(), torch.randn(2, h, w, c, generator=g).cuda()
        want = a + F.interpolate(b.permute(0, 3, 1, 2), size=(oh, ow), mode="nearest").permute(0, 2, 3, 1)
        got = detect.upsample_nearest_add_f32(a, b)
        assert torch.equal(got, want.contiguous()), (h, w, oh, ow)
    assert (4, 13) in [(pairs[i][0], pairs[(i + 2) % 5][0]) for i in range(5)]


# ---- the thresholded top-k -------------------------------------------------------------------------------------------------------

def _check_select(logits, reg, k, lt):
    """ur_det_select against the host restatement: counts, indices, anchors, labels exactly; scores within 2 ulp."""
    n, hwa, kk = logits.shape
    scores, anchors, labels, counts, bad, index = detect.det_select(logits.cuda(), None if reg is None else reg.cuda(), k, lt, want_index=True)
    counts = counts.cpu().tolist()
    for i in range(n):
        idx, vals = R.select(logits[i].numpy(), lt, k)
        assert counts[i] == len(idx), (i, counts[i], len(idx))
        m = counts[i]
        assert index[i, :m].cpu().tolist() == idx.tolist()
        assert anchors[i, :m].cpu().tolist() == (idx // kk).tolist() and labels[i, :m].cpu().tolist() == (idx % kk).tolist()
        want = R.sigmoid64(vals).astype(np.float32)
        got = scores[i, :m].cpu().numpy()
        assert m == 0 or bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 2 * np.spacing(want).astype(np.float64)).all())
        assert not scores[i, m:].any() and not index[i, m:].any()                # zero beyond the count
    return counts, bad.cpu().tolist()


@pytest.mark.parametrize("hwa,kk", [(9, 91), (9 * 35, 5), (9 * 13 * 17, 91)], ids=["1x1x91", "35x5", "13x17x91"])
def test_select_matches_the_restatement(hwa, kk):
    g = torch.Generator().manual_seed(hwa)
    logits = torch.randint(-40, 40, (2, hwa, kk), generator=g).float() / 8          # multiples of 1/8 in [-5, 5): ties everywhere
    reg = torch.randn(2, hwa, 4, generator=g)
    total = hwa * kk
    assert _check_select(logits, reg, 50, 100.0) == ([0, 0], [0, 0])               # nothing above the threshold
    low = logits.clamp(max=4.5)                                                   # a handful of candidates above 4.5, whatever the size
    for i in range(2):
        spots = torch.randperm(total, generator=g)[:min(70, total // 4)]
        low[i].view(-1)[spots[::2]] = 4.875
        low[i].view(-1)[spots[1::2]] = 4.625
    counts, _ = _check_select(low, reg, 1024, 4.5)                                # count < k
    assert all(0 < c < 1024 for c in counts) and counts[0] == int((low[0] > 4.5).sum())
    counts, _ = _check_select(low, reg, 1024, 4.625)                              # a logit equal to the threshold is no candidate
    assert 0 < counts[0] == int((low[0] > 4.625).sum()) < int((low[0] >= 4.625).sum())
    counts, _ = _check_select(logits, reg, 50, 0.0)                               # count > k, a tie group straddles the cut
    flat = logits[0].reshape(-1)
    ranked = sorted(flat[flat > 0.0].tolist(), reverse=True)
    assert counts == [50, 50] and len(ranked) > 51 and ranked[49] == ranked[50]
    assert _check_select(logits, reg, 50, -100.0)[0] == [50, 50]                   # every logit above the threshold
    if total <= 1024:
        assert _check_select(logits, reg, 1024, float("-inf"))[0] == [total, total]
    bad = logits.clone()
    bad[1, hwa // 2, kk // 3] = float("nan")                                      # dropped, and flagged for its image only
    bad[1, 0, 0] = 4.875
    assert _check_select(bad, reg, 50, 0.0)[1] == [0, 1]
    assert _check_select(logits, None, 50, 0.0)[1] == [0, 0]
    reg2 = reg.clone()
    reg2[0, hwa - 1, 3] = float("inf")                                            # a regression counts as well
    assert _check_select(logits, reg2, 50, 0.0)[1] == [1, 0]
    with pytest.raises(ValueError):
        detect.det_select(logits.cuda(), reg.cuda(), 1025, 0.0)


# ---- decode ----------------------------------------------------------------------------------------------------------------------

def test_decode_matches_fp64_on_every_level():
    hp, wp, rh, rw, oh, ow = 64, 96, 64, 89, 40, 56
    ratios = (float(np.float32(oh) / np.float32(rh)), float(np.float32(ow) / np.float32(rw)))
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    for level, (fh, fw) in enumerate(detect.level_sizes(hp, wp)):
        hwa = fh * fw * detect.NUM_ANCHORS
        reg = torch.randn(2, hwa, 4, generator=g) * 0.7
        reg[:, ::5, 2] = 5.0                                                      # dw above the clamp log(1000 / 16) = 4.135
        reg[:, 1::7, 3] = 4.2
        reg[:, ::3, 0] = 3.0                                                      # centres that leave the image
        reg[:, 2::11, 1] = -4.0
        anchors = torch.stack([torch.arange(hwa), torch.arange(hwa).flip(0)]).int()
        counts = torch.tensor([hwa, max(hwa // 2, 1)], dtype=torch.int32)
        clipped, scaled, raw = detect.det_decode(reg.cuda(), anchors.cuda(), counts.cuda(), detect.base_anchors(level).cuda(), fw,
                                                 (hp // fh, wp // fw), (rh, rw), ratios, want_raw=True)
        for n in range(2):
            m = int(counts[n])
            w_raw, w_clip, w_scaled = R.decode(reg[n].numpy(), anchors[n, :m].tolist(), level, fw, (hp // fh, wp // fw), (rh, rw), ratios)
            cx, cy = (w_raw[:, 0] + w_raw[:, 2]) / 2, (w_raw[:, 1] + w_raw[:, 3]) / 2
            bw, bh = w_raw[:, 2] - w_raw[:, 0], w_raw[:, 3] - w_raw[:, 1]
            bound = 16 * 2.0 ** -24 * np.stack([np.abs(cx) + bw, np.abs(cy) + bh, np.abs(cx) + bw, np.abs(cy) + bh], 1)
            e_raw = np.abs(raw[n, :m].cpu().double().numpy() - w_raw)
            e_clip = np.abs(clipped[n, :m].cpu().double().numpy() - w_clip)
            e_scaled = np.abs(scaled[n, :m].cpu().double().numpy() - w_scaled)
            worst = max(worst, float((e_raw / bound).max()))
            assert bool((e_raw <= bound).all()), (level, n, float((e_raw / bound).max()))
            assert bool((e_clip <= bound + 2.0 ** -20).all()) and bool((e_scaled <= bound + 2.0 ** -20).all())
            assert not raw[n, m:].any() and not clipped[n, m:].any() and not scaled[n, m:].any()
            aw = (detect.base_anchors(level)[:, 2] - detect.base_anchors(level)[:, 0]).double().numpy()
            assert 62.4 * aw.min() <= float(bw.max()) <= 62.5 * aw.max() * (1 + 1e-12)   # dw = 5 was clamped: exp(log(1000 / 16)) = 62.5 anchors wide
            assert bool((w_clip != w_raw).any()) and 0 <= float(clipped[n].min()) and float(clipped[n, :, 0::2].max()) <= rw
    print(f"decode: worst |err| / bound {worst:.3f}")


# ---- NMS -------------------------------------------------------------------------------------------------------------------------

def _nms_case(m, seed):
    """m integer boxes in [0, 1024) clustered around a few centres, labels in 0..2, scores from sixteen values; the first two are the
    pair at IoU exactly 0.5, the next two one box under two labels, apart from every other box."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randint(100, 900, (max(m // 12, 1), 2), generator=g)
    pick = torch.randint(0, len(centres), (m,), generator=g)
    half = torch.randint(8, 60, (m, 2), generator=g)
    c = centres[pick] + torch.randint(-12, 13, (m, 2), generator=g)
    boxes = torch.cat([(c - half).clamp(0, 1022), (c + half).clamp(1, 1023)], 1).float()
    boxes[:, 2:] = torch.maximum(boxes[:, 2:], boxes[:, :2] + 1)
    labels = torch.randint(0, 3, (m,), generator=g).int()
    scores = (torch.randint(1, 16, (m,), generator=g).float() / 16)
    if m >= 2:
        boxes[0], boxes[1] = torch.tensor([0., 0., 3., 2.]), torch.tensor([1., 0., 4., 2.])
        labels[:2], scores[:2] = 1, 1.0
    if m >= 4:
        boxes[2] = boxes[3] = torch.tensor([990., 990., 1020., 1020.])             # (every other box ends below 973)
        labels[2], labels[3], scores[2:4] = 0, 2, 15 / 16
    return boxes, scores, labels


def _dup_case(m, seed, clusters=60):
    """m near-duplicates of `clusters` well-separated integer boxes under 3 labels - what a trained detector hands to the NMS: a kept
    box suppresses candidates thousands of sorted positions behind it."""
    g = torch.Generator().manual_seed(seed)
    grid = torch.arange(clusters)
    centres = torch.stack([60 + 110 * (grid % 8), 60 + 110 * (grid // 8)], 1)
    half = torch.randint(30, 45, (clusters, 2), generator=g)
    pick = torch.randint(0, clusters, (m,), generator=g)
    lo = centres[pick] - half[pick] + torch.randint(-2, 3, (m, 2), generator=g)
    hi = centres[pick] + half[pick] + torch.randint(-2, 3, (m, 2), generator=g)
    boxes = torch.cat([lo, hi], 1).clamp(0, 1023).float()
    return boxes, torch.randint(1, 64, (m,), generator=g).float() / 64, torch.randint(0, 3, (m,), generator=g).int()


def _check_nms(cases, d):
    boxes, scores, labels = (torch.stack([c[i] for c in cases]) for i in range(3))
    m = boxes.shape[1]
    counts = torch.full((1, len(cases)), m, dtype=torch.int32)
    yb, ys, yl, keep, yc, yf = detect.det_nms(boxes.cuda(), boxes.cuda(), scores.cuda(), labels.cuda(), counts.cuda(), None, m, 0.5, d)
    wants = []
    for n in range(len(cases)):
        want = R.nms(boxes[n].numpy(), scores[n].numpy(), labels[n].numpy(), 0.5, d)
        c = int(yc[n])
        assert c == len(want) and keep[n, :c].cpu().tolist() == want, (m, d, n, c, len(want))
        assert torch.equal(yb[n, :c].cpu(), boxes[n][want].view(-1, 4)) and yl[n, :c].cpu().tolist() == labels[n][want].tolist()
        wants.append(want)
    return wants


def test_nms_suppresses_far_behind_a_kept_box():
    """More candidates than the workgroup has threads: a kept box and the duplicates it suppresses lie more than 1024 sorted
    positions apart, so a thread must compare every one of its positions behind the box, not only the first."""
    m = 5000
    # every survivor is wanted: the walk goes through all 5000 positions
    for want, (boxes, scores, labels) in zip(_check_nms([_nms_case(m, 10 + m), _nms_case(m, 20 + m)], m), [_nms_case(m, 10 + m), _nms_case(m, 20 + m)]):
        assert 1024 < len(want) < m and want[:4] == [0, 1, 2, 3]
    # duplicates: the reference keeps fewer than detections_per_img = 300
    cases = [_dup_case(m, 31), _dup_case(m, 32)]
    for want, (boxes, scores, labels) in zip(_check_nms(cases, 300), cases):
        assert 60 <= len(want) < 300
        order = sorted(range(m), key=lambda i: (-float(scores[i]), i))
        first = order[0]
        far = [i for i in order[1025:] if labels[i] == labels[first] and R.iou(boxes[first].tolist(), boxes[i].tolist()) > 0.5]
        assert far and not set(far) & set(want)            # suppressed by the first kept box from more than 1024 positions away


@pytest.mark.parametrize("m", [0, 1, 65, 300, 1000, 5000])
def test_nms_keeps_the_restatements_positions(m):
    cases = [_nms_case(m, 10 + m), _nms_case(m, 20 + m)]
    boxes, scores, labels = (torch.stack([c[i] for c in cases]) for i in range(3))
    counts = torch.full((1, 2), m, dtype=torch.int32)
    for d in (300, 7):
        yb, ys, yl, keep, yc, yf = detect.det_nms(boxes.cuda(), boxes.cuda(), scores.cuda(), labels.cuda(), counts.cuda(), None, max(m, 1), 0.5, d)
        assert yl.dtype == torch.int64 and yf.cpu().tolist() == [0, 0]
        for n in range(2):
            want = R.nms(boxes[n].numpy(), scores[n].numpy(), labels[n].numpy(), 0.5, d)
            c = int(yc[n])
            assert c == len(want) and keep[n, :c].cpu().tolist() == want, (m, d, n)
            assert keep[n, c:].cpu().tolist() == [-1] * (d - c) and not ys[n, c:].any() and not yb[n, c:].any()
            assert torch.equal(yb[n, :c].cpu(), boxes[n][want].view(-1, 4)) and torch.equal(ys[n, :c].cpu(), scores[n][want])
            assert yl[n, :c].cpu().tolist() == labels[n][want].tolist()
            if m >= 2:
                assert want[:2] == [0, 1]                                          # IoU exactly 0.5 does not suppress
            if m >= 4:
                assert want[2:4] == [2, 3] and torch.equal(boxes[n][2], boxes[n][3])  # one box, two labels: both are kept
            if m >= 65 and d == 300:
                assert len(want) < m                                               # something was suppressed ...
                assert len({float(scores[n][i]) for i in want}) < len(want)        # equal scores: the position decided
            if d == 7 and m >= 65:
                assert c == 7
    # only the first counts[n] positions are candidates, and a set flag empties the image
    if m >= 65:
        part = torch.tensor([[m // 2, m]], dtype=torch.int32)
        flags = torch.tensor([[0, 1]], dtype=torch.int32)
        _, _, _, keep, yc, yf = detect.det_nms(boxes.cuda(), boxes.cuda(), scores.cuda(), labels.cuda(), part.cuda(), flags.cuda(), m, 0.5, 300)
        want = R.nms(boxes[0][:m // 2].numpy(), scores[0][:m // 2].numpy(), labels[0][:m // 2].numpy(), 0.5, 300)
        assert keep[0, :int(yc[0])].cpu().tolist() == want and int(yc[1]) == 0 and yf.cpu().tolist() == [0, 1]


# ---- the network -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 91])
@pytest.mark.parametrize("hw", R.NET_IMAGES, ids=["40x56", "48x48"])
def test_head_outputs_match_fp64(k, hw):
    w = _weights(k)
    want_l, want_r, want_geo = _reference(k, hw)
    logits, regs, geo = detect.head_outputs(R.images(hw).cuda(), w)
    assert geo == want_geo and geo["canvas"] == ((64, 96) if hw == (40, 56) else (64, 64)) and geo["sizes"][-1] == (1, 1)
    for lv in range(detect.LEVELS):
        assert tuple(logits[lv].shape) == tuple(want_l[lv].shape) and tuple(regs[lv].shape) == tuple(want_r[lv].shape)
        el = float((logits[lv].cpu().double() - want_l[lv]).abs().max() / want_l[lv].abs().max())
        er = float((regs[lv].cpu().double() - want_r[lv]).abs().max() / want_r[lv].abs().max())
        print(f"K={k} {hw} level {lv}: logits {el:.2e} of max |logit| (bound {R.LOGITS_TOL:.2e}), regressions {er:.2e} (bound {R.REGS_TOL:.2e})")
        assert el <= R.LOGITS_TOL and er <= R.REGS_TOL


# ---- end to end ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 91])
def test_pipeline_is_the_restatement_on_the_gpus_own_head_outputs(k):
    """select / decode / NMS on the host, applied to the head outputs the GPU computed: the same candidates, the same kept
    positions (the NMS restated in the kernel's own fp32 operations on the GPU's boxes and scores, so no decision is borderline),
    the boxes within the decode bound."""
    w = _weights(k)
    hw = R.NET_IMAGES[0]
    x = R.images(hw).cuda()
    logits, regs, geo = detect.head_outputs(x, w)
    topk = 50
    boxes, scores, labels, counts, bad, cand = detect.postprocess(logits, regs, geo, hw, topk_candidates=topk, want_candidates=True)
    dets, flags = detect.forward(x, w, topk_candidates=topk)
    assert flags.tolist() == [0, 0] and bad.cpu().tolist() == [0, 0]
    for n in range(2):
        ref = R.postprocess(logits, regs, geo, hw, n, 0.05, topk, 0.5, 300)
        lv_counts = cand["counts"][:, n].cpu().tolist()
        assert lv_counts == ref["counts"] and max(lv_counts) == topk and any(0 < c < topk for c in lv_counts), lv_counts     # a cut level, an uncut one
        pos = [l * topk + j for l, c in enumerate(lv_counts) for j in range(c)]
        assert cand["anchors"][n].cpu()[pos].tolist() == ref["anchors"] and cand["labels"][n].cpu()[pos].tolist() == ref["labels"]
        got_clip, want_raw = cand["clipped"][n].cpu()[pos].double().numpy(), np.asarray(ref["raw"])
        cx, cy = (want_raw[:, 0] + want_raw[:, 2]) / 2, (want_raw[:, 1] + want_raw[:, 3]) / 2
        bw, bh = want_raw[:, 2] - want_raw[:, 0], want_raw[:, 3] - want_raw[:, 1]
        bound = 16 * 2.0 ** -24 * np.stack([np.abs(cx) + bw, np.abs(cy) + bh, np.abs(cx) + bw, np.abs(cy) + bh], 1) + 2.0 ** -20
        assert bool((np.abs(got_clip - np.asarray(ref["clipped"])) <= bound).all())
        assert bool((np.abs(cand["scaled"][n].cpu()[pos].double().numpy() - np.asarray(ref["scaled"])) <= bound).all())
        # the NMS in the kernel's arithmetic on the GPU's own candidates
        keep = R.nms(cand["clipped"][n].cpu()[pos].numpy(), cand["scores"][n].cpu()[pos].numpy(), ref["labels"], 0.5, 300, dtype=np.float32)
        c = int(counts[n])
        assert c == len(keep) and cand["keep"][n, :c].cpu().tolist() == [pos[i] for i in keep] and c >= 20
        assert labels[n, :c].cpu().tolist() == [ref["labels"][i] for i in keep]
        assert torch.equal(boxes[n, :c].cpu(), cand["scaled"][n].cpu()[[pos[i] for i in keep]])
        d = dets[n]
        assert torch.equal(d["boxes"], boxes[n, :c]) and torch.equal(d["scores"], scores[n, :c]) and torch.equal(d["labels"], labels[n, :c])
        assert d["labels"].dtype == torch.int64 and bool((d["scores"][:-1] >= d["scores"][1:]).all()) and float(d["scores"].min()) > 0.05
        slack = 1 + 2.0 ** -22                       # the clip is at the resized size; fp32(size * fp32(original / resized)) may round up
        assert float(d["boxes"].min()) >= 0 and float(d["boxes"][:, 0::2].max()) <= hw[1] * slack and float(d["boxes"][:, 1::2].max()) <= hw[0] * slack


def test_pipeline_against_the_fp64_pipeline():
    """detect.forward against the restatement run in fp64 from the images on.  A detection whose fp64 score lies within 1e-5 of the
    score threshold, or whose fp64 IoU with a kept box of its label within 1e-4 of the NMS threshold, is left out of the comparison
    (at most 2 % of them); every other one must be found, with its box within the decode bound plus what the regressions'
    tolerance d = REGS_TOL max |reg| moves a box: each coordinate is dx w + cx -+ exp(dw) w / 2, so d (w + exp(dw) w / 2) to first order;
    2 d (anchor size + decoded size) is allowed, the anchor's long side taken as twice its scale; a score may differ by a quarter
    (the sigmoid's largest slope) of the logits' tolerance LOGITS_TOL max |logit|.  topk_candidates = 1000 cuts no
    level of this network, so no candidate depends on the order of nearly equal logits."""
    k, hw = 5, R.NET_IMAGES[0]
    w = _weights(k)
    logits64, regs64, geo = _reference(k, hw)
    dets, flags = detect.forward(R.images(hw).cuda(), w)
    lt64 = float(np.log(0.05 / 0.95))
    for n in range(2):
        ref = R.postprocess(logits64, regs64, geo, hw, n, 0.05, 1000, 0.5, 300, lt=lt64)
        assert max(ref["counts"]) < 1000
        kept = ref["keep"]
        unsure = {i for i in range(len(ref["scores"])) if abs(ref["scores"][i] - 0.05) < 1e-5} | ref["near"]
        want = {(ref["level"][i], ref["anchors"][i], ref["labels"][i]): i for i in kept}
        assert len(unsure & set(kept)) <= 0.02 * len(kept) and len(kept) >= 50
        unsure_ids = {(ref["level"][i], ref["anchors"][i], ref["labels"][i]) for i in unsure}
        d = dets[n]
        # the GPU's detections, named by (level, anchor, label): the anchor is found again through the fp64 candidates
        by_box = {}
        for i in range(len(ref["scores"])):
            by_box.setdefault(ref["labels"][i], []).append(i)
        got = set()
        dmax = max(float(r.abs().max()) for r in regs64) * R.REGS_TOL
        smax = max(float(l.abs().max()) for l in logits64) * R.LOGITS_TOL / 4 + 2.0 ** -24
        for b, s, l in zip(d["boxes"].cpu().double().numpy(), d["scores"].cpu().tolist(), d["labels"].cpu().tolist()):
            idx = by_box.get(l, [])
            errs = [float(np.abs(np.asarray(ref["scaled"][i]) - b).max()) for i in idx]
            j = idx[int(np.argmin(errs))]
            raw = ref["raw"][j]
            size = max(raw[2] - raw[0], raw[3] - raw[1])
            tol = 16 * 2.0 ** -24 * (max(abs(v) for v in raw) + size) + 2.0 ** -20 + 2 * dmax * (2 * detect.ANCHOR_SIZES[ref["level"][j]][2] + size)
            assert min(errs) <= tol and abs(s - ref["scores"][j]) <= smax, (min(errs), tol, s - ref["scores"][j], smax)
            got.add((ref["level"][j], ref["anchors"][j], l))
        assert got - unsure_ids == set(want) - unsure_ids, (sorted(got ^ set(want)))
    assert flags.tolist() == [0, 0]


def test_one_512_image_at_the_real_sizes():
    w = detect.random_weights(R.ARCH, R.NET_SEED, 91)
    assert (w.min_size, w.max_size, w.num_classes) == (800, 1333, 91)
    x = R.images((512, 512), n=1)
    boxes, scores, labels, counts, bad = detect.raw(x.cuda(), w)
    assert tuple(boxes.shape) == (1, 300, 4) and tuple(scores.shape) == (1, 300) and labels.dtype == torch.int64 and tuple(counts.shape) == (1,)
    c = int(counts[0])
    assert 0 < c <= 300 and int(bad[0]) == 0 and bool(torch.isfinite(boxes).all())
    assert float(boxes.min()) >= 0 and float(boxes.max()) <= 512 * (1 + 2.0 ** -22) and float(scores[0, :c].min()) > 0.05 and int(labels.max()) < 91
    assert bool((boxes[0, :c, 2] >= boxes[0, :c, 0]).all()) and not boxes[0, c:].any()


# ---- invariance and determinism ----------------------------------------------------------------------------------------------------

def _same(a, b, i, j):
    return all(torch.equal(a[t][i], b[t][j]) for t in range(5))


def test_detections_do_not_depend_on_the_place_in_the_batch():
    w = _weights(5)
    x = torch.cat([R.images((40, 56), n=2, seed=s) for s in (0, 7)])[:3].contiguous().cuda()
    whole = detect.raw(x, w)
    assert len({bytes(whole[0][i].cpu().numpy().tobytes()) for i in range(3)}) == 3 and int(whole[3].min()) > 0
    for i in range(3):
        assert _same(detect.raw(x[i:i + 1].contiguous(), w), whole, 0, i)
        order = [j for j in range(3) if j != i]
        order.insert((i + 1) % 3, i)
        assert _same(detect.raw(x[order].contiguous(), w), whole, (i + 1) % 3, i)


def test_deterministic_eager_and_graph_replay():
    w = _weights(5)
    x = R.images((40, 56)).cuda()
    a = detect.raw(x, w)
    b = detect.raw(x, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        detect.raw(x, w)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = detect.raw(x, w)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(a, b, c)) and int(a[3].min()) > 0


def test_a_nan_pixel_flags_its_image_and_leaves_the_others_alone():
    w = _weights(5)
    x = torch.cat([R.images((40, 56), n=2, seed=s) for s in (0, 7)])[:3].contiguous()
    clean = detect.raw(x.cuda(), w)
    x[1, 0, 3, 4] = float("nan")
    got = detect.raw(x.cuda(), w)
    assert got[4].cpu().tolist() == [0, 1, 0] and int(got[3][1]) == 0 and not got[0][1].any() and not got[1][1].any()
    assert _same(got, clean, 0, 0) and _same(got, clean, 2, 2)
    dets, flags = detect.forward(x.cuda(), w)
    assert flags.tolist() == [0, 1, 0] and len(dets[1]["scores"]) == 0 and tuple(dets[1]["boxes"].shape) == (0, 4)


def test_ops_reject_bad_inputs():
    from unirestore_amd import ops
    w = _weights(5)
    x = R.images((40, 56)).cuda()
    for bad in (x.double(), x.cpu(), x[0], x[:, :1].contiguous(), x[:0].contiguous()):
        with pytest.raises(ValueError):
            ops.detect(bad, w)
    with pytest.raises(ValueError):
        ops.detect(x, {"arch": R.ARCH})
    for kw in (dict(topk_candidates=0), dict(topk_candidates=1025), dict(detections_per_img=0)):
        with pytest.raises(ValueError):
            ops.detect(x, w, **kw)
    out = ops.detect(x, w, detections_per_img=7)
    assert len(out) == 2 and all(len(d["scores"]) == 7 for d in out)


# ---- the caller ------------------------------------------------------------------------------------------------------------------

def _kwargs():
    kw = copy.deepcopy(model_kwargs(2))
    kw["tedit"]["task"] = ["ir", "cls", "seg", "det"]
    return kw


def _tiny_model():
    import unirestore_amd.modules as M
    from oracle.model import DiffUIE as ODiffUIE
    torch.manual_seed(0)
    o = randomise_(ODiffUIE(**_kwargs(), **TINY).eval(), 0)
    p = M.DiffUIE(**_kwargs(), **TINY).eval()
    p.load_state_dict(o.state_dict())
    return p


def _targets(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        m = int(torch.randint(1, 4, (1,), generator=g))
        xy = torch.stack([torch.randint(0, hw[1] - 24, (m,), generator=g), torch.randint(0, hw[0] - 24, (m,), generator=g)], 1).float()
        out.append(dict(boxes=torch.cat([xy, xy + torch.randint(8, 24, (m, 2), generator=g).float()], 1), labels=torch.randint(1, 5, (m,), generator=g)))
    return out


def test_litunifie_scores_the_det_output_and_leaves_the_rest_alone():
    from unirestore_amd import ops, runner
    model = _tiny_model()
    w = _weights(5)
    tasks = ["ir", "det"]
    batches = []
    for b in range(2):
        hq = R.images((64, 64), seed=100 + b).cuda()
        lq = (0.6 * hq + 0.3 * R.images((64, 64), seed=200 + b).cuda()).clamp(0, 1)
        batches.append((lq, hq, _targets(2, (64, 64), 300 + b)))

    def run(detectors, with_boxes, **kw):
        lit = runner.LitUniFIE(_kwargs(), model=model, detectors=detectors, **kw)
        outs = []
        for b, (lq, hq, gt) in enumerate(batches):
            torch.manual_seed(40 + b)                # the forward's noise draws: the same for every instance
            outs.append(lit.validation_step((lq, hq, gt if with_boxes else None, ["a", "b"], "ir"), tasks=tasks)[-1])
        return lit, lit.metrics(), outs
    lit0, m0, o0 = run(None, False)
    lit1, m1, o1 = run({"rn": w}, True, det_score=0.05, det_iou=0.5)
    for a, b in zip(o0, o1):
        assert all(torch.equal(a[t], b[t]) for t in tasks)                        # restoring does not depend on the scoring
    assert set(m1) == set(m0) | {"val_lq/rn", "val_input/rn", "det_nonfinite"} and all(m1[k] == m0[k] for k in m0)
    assert set(lit1.totals) == set(lit0.totals) | {"det/rn", "det_input/rn"} and m1["det_nonfinite"] == [0, 0]
    gts = [t for _, _, gt in batches for t in gt]
    for key, side in (("val_lq/rn", [o["det"] for o in o1]), ("val_input/rn", [lq for lq, _, _ in batches])):
        dets = [d for img in side for d in ops.detect(img.float().contiguous(), w)]
        want = ops.mean_ap(dets, gts, 0.5)
        print(key, m1[key], sum(len(d["scores"]) for d in dets))
        assert m1[key] == want and 0.0 <= want <= 1.0
    with pytest.raises(ValueError, match="boxes"):
        run({"rn": w}, False)
    lit = runner.LitUniFIE(_kwargs(), model=model, detectors={"rn": w})
    with pytest.raises(ValueError, match="det"):
        lit.validation_step((batches[0][0], batches[0][1], batches[0][2], ["a", "b"], "ir"), tasks=["ir", "seg"])


def test_cli_validate_detect(tmp_path):
    from unirestore_amd import cli, ops
    lst, _ = write_pairs(str(tmp_path / "d"), n=4, hw=(64, 64), names=("person", "bicycle", "car", "motorbike"))
    wpath = str(tmp_path / "rn.pth")
    torch.save(detect.random_state_dict(R.ARCH, 7, 5), wpath)
    model = _tiny_model()
    keys = {"val_lq/rn", "val_input/rn", "det_nonfinite"}

    def cfg(cls, **args):
        return dict(seed_everything=3, trainer=dict(accelerator="gpu", devices=1, precision="bf16-mixed"),
                    model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=_kwargs())),
                    data=dict(class_path=f"unirestore_amd.data.{cls}", init_args=dict(batch_size=2, labels="boxes", **args)))
    files = cfg("ImageListFiles", list_file=lst)
    r0 = cli.validate(files, tasks=["ir", "det"], model=model)
    r1 = cli.validate(files, tasks=["ir", "det"], model=model, detect=f"rn={R.ARCH}:{wpath}")
    print({k: r1[k] for k in sorted(keys)})
    assert set(r1) == set(r0) | keys and r1["images"] == r0["images"] == 4 and r1["det_nonfinite"] == [0, 0]
    assert all(r1[k] == r0[k] for k in r0 if k != "images_per_s")                 # without --detect the result is what it was
    # the unrestored inputs by hand: the same files, the same weights, ops.detect + ops.mean_ap
    from unirestore_amd import data
    w = detect.load_weights(R.ARCH, wpath)
    dets, gts = [], []
    for lq, _hq, gt, _names, _task in data.ImageListFiles(lst, batch_size=2, labels="boxes").batches(device="cuda"):
        dets += ops.detect(lq.contiguous(), w)
        gts += gt
    assert r1["val_input/rn"] == ops.mean_ap(dets, gts, 0.5) and 0.0 <= r1["val_lq/rn"] <= 1.0
    r2 = cli.validate(files, tasks=["ir", "det"], model=model, detect={"rn": (R.ARCH, wpath)}, crop="64,64", det_score=0.05, det_iou=0.5)
    assert {k: r2[k] for k in keys} == {k: r1[k] for k in keys}
    r3 = cli.validate(files, tasks=["ir", "det"], model=model, detect={"rn": w}, det_score=0.3, det_iou=0.75)
    assert r3["val_input/rn"] == ops.mean_ap([d for lq, *_ in data.ImageListFiles(lst, batch_size=2).batches(device="cuda")
                                              for d in ops.detect(lq.contiguous(), w, score_thresh=0.3)], gts, 0.75)
    # a degrading dataset: every by_corruption entry gains the pair of keys
    fog = cfg("CorruptedImageFiles", source=lst, corruptions="fog", severity=3)
    r4 = cli.validate(fog, tasks=["ir", "det"], model=model, detect={"rn": w})
    assert list(r4["by_corruption"]) == ["fog/3"] and {"rn", "input/rn"} <= set(r4["by_corruption"]["fog/3"])
    assert r4["by_corruption"]["fog/3"]["rn"] == r4["val_lq/rn"] and r4["by_corruption"]["fog/3"]["input/rn"] == r4["val_input/rn"]
    json.dumps(r4)
