"""RetinaNet scoring of the `det` output on the GPU in exact fp32: the reference's `DetectionEvaluator` in `eval_mode: single`,
torchvision's `retinanet_resnet50_fpn_v2` in eval mode, on the fp32 layers and the ResNet-50 trunk of f32net.py and the kernels of
csrc/detect.hip.  Quantised image -> `GeneralizedRCNNTransform` (ImageNet Normalize, half-pixel bilinear resize to min_size /
max_size, a zero canvas padded to multiples of 32) -> ResNet-50 (FrozenBatchNorm folded) -> FPN on C3..C5 with P6 from C5 and P7
from relu(P6) -> the two heads (four 3x3 conv + GroupNorm(32) + ReLU each, shared by the five levels) -> per level the candidates
above the score threshold, at most `topk_candidates` of them, decoded against the anchors and clipped -> class-aware NMS ->
`detections_per_img` boxes in the original image's coordinates.  In NHWC the heads' outputs [N,H,W,9K] and [N,H,W,36] already are
torchvision's [N, HWA, K] and [N, HWA, 4]: the channel index is a * K + k.

The mean average precision (`MeanAP`) is host fp64 numpy: pycocotools' algorithm at one IoU threshold, area range `all`, no crowd.

The key layout and the forward are torchvision's source as recalled - the package is not installed where this is developed - and
unchecked against it and against published mAP, as is the metric against torchmetrics / pycocotools.  The project ships NO
weights.  `load_weights` reads the checkpoint a user of the metric already has; `random_weights` makes seeded stand-ins for tests
and timing, which say nothing about any published mAP.
"""
import functools
import math

import numpy as np
import torch

from . import f32net
from .capi import check, lib
from .f32net import PackedConvF32, conv2d_f32, stream, take

ARCHS = {"retinanet_resnet50_fpn_v2": (3, 4, 6, 3)}
FPN_CH, GN_GROUPS, GN_EPS = 256, 32, 1e-5
LEVELS = 5
ANCHOR_SIZES = tuple((x, int(x * 2 ** (1.0 / 3)), int(x * 2 ** (2.0 / 3))) for x in (32, 64, 128, 256, 512))
ASPECT_RATIOS = (0.5, 1.0, 2.0)
NUM_ANCHORS = len(ANCHOR_SIZES[0]) * len(ASPECT_RATIOS)
BBOX_XFORM_CLIP = math.log(1000.0 / 16)
SIZE_DIVISIBLE = 32
SCORE_THRESH, TOPK_CANDIDATES, NMS_THRESH, DETECTIONS_PER_IMG = 0.05, 1000, 0.5, 300      # torchvision's own defaults
TRUNK_CH = (512, 1024, 2048)                              # C3, C4, C5


def depths_of(arch):
    if not isinstance(arch, str) or arch not in ARCHS:
        raise ValueError(f"unknown detector arch {arch!r}: choose from {sorted(ARCHS)}")
    return ARCHS[arch]


# ---- host geometry: anchors, the nearest table, the resize ---------------------------------------------------------------------

def base_anchors(level: int) -> torch.Tensor:
    """The nine zero-centred anchors of a level, fp32 [9, 4] (x1, y1, x2, y2), as `AnchorGenerator.generate_anchors` builds them:
    fp32 arithmetic, ratio-major and scale-minor, rounded half to even."""
    scales = torch.tensor(ANCHOR_SIZES[level], dtype=torch.float32)
    h_ratios = torch.sqrt(torch.tensor(ASPECT_RATIOS, dtype=torch.float32))
    w_ratios = 1 / h_ratios
    ws = (w_ratios[:, None] * scales[None, :]).view(-1)
    hs = (h_ratios[:, None] * scales[None, :]).view(-1)
    return (torch.stack([-ws, -hs, ws, hs], dim=1) / 2).round()


def nearest_table(n_in: int, n_out: int) -> torch.Tensor:
    """One axis of `F.interpolate(size=n_out, mode="nearest")`: int32 [n_out], the source min(floor(dst * fp32(n_in / n_out)),
    n_in - 1), the product in fp32 as torch forms it."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"nearest_table: sizes must be >= 1, got {n_in} -> {n_out}")
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(src, n_in - 1).astype(np.int32))


def resized_size(h: int, w: int, min_size: int, max_size: int):
    """`GeneralizedRCNNTransform`'s output size of an h x w image: s = min(min_size / min(h, w), max_size / max(h, w)) in fp32,
    (floor(h s), floor(w s)) - `interpolate(scale_factor=s, recompute_scale_factor=True)`."""
    s = float(min(np.float32(min_size) / np.float32(min(h, w)), np.float32(max_size) / np.float32(max(h, w))))
    return max(int(math.floor(h * s)), 1), max(int(math.floor(w * s)), 1)


def canvas_size(rh: int, rw: int):
    return -(-rh // SIZE_DIVISIBLE) * SIZE_DIVISIBLE, -(-rw // SIZE_DIVISIBLE) * SIZE_DIVISIBLE


def level_sizes(hp: int, wp: int):
    """The five feature sizes of an hp x wp canvas: C3, C4, C5 of the trunk, then two 3x3 / stride 2 / pad 1 convolutions."""
    def half(v):
        return (v - 1) // 2 + 1
    h, w = half(half(hp)), half(half(wp))                  # conv1 and the max-pool
    out = []
    for _ in range(LEVELS):
        h, w = half(h), half(w)
        out.append((h, w))
    return out


@functools.lru_cache(maxsize=None)                       # never evicted: a captured graph keeps reading the tables it was captured with
def _nearest_tables(h, w, oh, ow, dev_index):
    dev = torch.device("cuda", dev_index)
    return nearest_table(h, oh).to(dev), nearest_table(w, ow).to(dev)


@functools.lru_cache(maxsize=None)
def _base_anchors_dev(dev_index):
    return torch.stack([base_anchors(l) for l in range(LEVELS)]).contiguous().to(torch.device("cuda", dev_index))


# ---- weights -------------------------------------------------------------------------------------------------------------------

def backbone_plan(arch):
    return [(f"backbone.body.{c}", f"backbone.body.{b}", *rest) for c, b, *rest in f32net.resnet_plan("bottleneck", depths_of(arch))]


def fpn_plan():
    """[(key, Cout, Cin, kernel, stride, pad)] of the FPN's biased convolutions, in state-dict order."""
    plan = [(f"backbone.fpn.inner_blocks.{i}.0", FPN_CH, c, 1, 1, 0) for i, c in enumerate(TRUNK_CH)]
    plan += [(f"backbone.fpn.layer_blocks.{i}.0", FPN_CH, FPN_CH, 3, 1, 1) for i in range(3)]
    plan += [("backbone.fpn.extra_blocks.p6", FPN_CH, TRUNK_CH[2], 3, 2, 1), ("backbone.fpn.extra_blocks.p7", FPN_CH, FPN_CH, 3, 2, 1)]
    return plan


CLS_KEY, REG_KEY = "head.classification_head.cls_logits", "head.regression_head.bbox_reg"
TOWERS = ("head.classification_head.conv", "head.regression_head.conv")


def strip_prefix(sd: dict) -> dict:
    """A state dict whose keys carry something in front of `backbone.` (a Lightning module's attribute path) without it."""
    probe = next((k for k in sd if k.endswith("backbone.body.conv1.weight")), None)
    prefix = "" if probe is None else probe[:-len("backbone.body.conv1.weight")]
    if not prefix:
        return sd
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


class DetectorWeights:
    """One RetinaNet ready for the fp32 kernels: the trunk's convolutions with their FrozenBatchNorm folded in (fp64 fold), the FPN's
    and the heads' convolutions repacked, the GroupNorm parameters, all on the device.  `cpu` keeps the UNFUSED state dict (fp32
    tensors under torchvision's keys): what a host restatement of the network needs."""

    def __init__(self, arch, sd: dict, *, min_size: int = 800, max_size: int = 1333, dev=None, source: str = "state dict"):
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        self.arch, self.device, self.depths = arch, dev, depths_of(arch)
        if not (isinstance(min_size, int) and isinstance(max_size, int) and 1 <= min_size <= max_size):
            raise ValueError(f"min_size and max_size must be integers with 1 <= min_size <= max_size, got {min_size!r}, {max_size!r}")
        self.min_size, self.max_size = min_size, max_size
        sd = strip_prefix(sd)
        self.cpu = {}
        wkey = f"{CLS_KEY}.weight"
        if wkey not in sd or not torch.is_tensor(sd[wkey]) or sd[wkey].ndim != 4 or sd[wkey].shape[0] % NUM_ANCHORS or sd[wkey].shape[0] < NUM_ANCHORS:
            raise ValueError(f"{source}: {wkey!r} is missing or no [9 K, 256, 3, 3] tensor: the number of classes is read from it")
        self.num_classes = k = sd[wkey].shape[0] // NUM_ANCHORS
        ready = f32net.fold_convs(backbone_plan(arch), sd, source, self.cpu)                      # every check first
        geometry = {}
        for key, cout, cin, ks, stride, pad in fpn_plan() + [(CLS_KEY, NUM_ANCHORS * k, FPN_CH, 3, 1, 1), (REG_KEY, NUM_ANCHORS * 4, FPN_CH, 3, 1, 1)]:
            ready.append((key, take(sd, source, f"{key}.weight", (cout, cin, ks, ks), keep=self.cpu),
                          take(sd, source, f"{key}.bias", (cout,), keep=self.cpu), stride, pad))
        norms = {}
        for tower in TOWERS:
            for i in range(4):
                ready.append((f"{tower}.{i}.0", take(sd, source, f"{tower}.{i}.0.weight", (FPN_CH, FPN_CH, 3, 3), keep=self.cpu),
                              torch.zeros(FPN_CH), 1, 1))
                norms[f"{tower}.{i}.1"] = (take(sd, source, f"{tower}.{i}.1.weight", (FPN_CH,), keep=self.cpu),
                                           take(sd, source, f"{tower}.{i}.1.bias", (FPN_CH,), keep=self.cpu))
        self.convs = {key: PackedConvF32(w, b, stride, pad, dev) for key, w, b, stride, pad in ready}
        self.norms = {key: (g.contiguous().to(dev), b.contiguous().to(dev)) for key, (g, b) in norms.items()}
        self.backbone = {key[len("backbone.body."):]: v for key, v in self.convs.items() if key.startswith("backbone.body.")}
        self.stages = f32net.resnet_stages("bottleneck", self.depths, self.backbone)


def read_state_dict(path) -> dict:
    """A bare state dict, or a Lightning checkpoint's `state_dict`; whatever stands in front of `backbone.` in the keys is stripped."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(ckpt, dict) and isinstance(ckpt.get("state_dict"), dict):
        ckpt = ckpt["state_dict"]
    if not isinstance(ckpt, dict):
        raise ValueError(f"{path}: not a state dict")
    return strip_prefix(ckpt)


def load_weights(arch, path, dev=None, *, min_size: int = 800, max_size: int = 1333) -> DetectorWeights:
    """arch: one of ARCHS; path: the user's torchvision RetinaNet state dict (`backbone.body.*`, `backbone.fpn.*`, `head.*`).  The
    number of classes is cls_logits.weight's rows / 9.  ValueError (file and key named) for a missing key, a wrong shape or a
    non-finite value - before anything is uploaded."""
    depths_of(arch)
    return DetectorWeights(arch, read_state_dict(path), min_size=min_size, max_size=max_size, dev=dev, source=str(path))


def random_state_dict(arch, seed: int, num_classes: int = 91) -> dict:
    """A seeded stand-in in torchvision's key layout, for tests and timing ONLY: f32net.random_backbone's recipe for the trunk
    (without `num_batches_tracked`: FrozenBatchNorm2d has none), Kaiming-scaled FPN and tower convolutions - those that read a trunk
    stage scaled down by 1.2 per block in front of them beyond one per stage, the rate at which the stand-in residual sums grow -
    GroupNorm gamma in [0.5, 1.5] and small beta.  The class logits come out roughly N(-4.4, 1) on the largest level and narrower
    on the small ones: about one in fourteen passes the 0.05 threshold (logit -2.94) there and next to none on the smallest, so
    with a few dozen candidates wanted a large level is cut and a small one is not.  NOT trained weights."""
    g = torch.Generator().manual_seed(seed)
    depths = depths_of(arch)
    sd = {k: v for k, v in f32net.random_backbone(backbone_plan(arch), "bottleneck", g).items() if not k.endswith("num_batches_tracked")}
    growth = {0: sum(depths[:2]) - 2, 1: sum(depths[:3]) - 3, 2: sum(depths) - 4}
    for key, cout, cin, ks, _s, _p in fpn_plan():
        gain = 1.0
        if "inner_blocks" in key:
            gain = 1.2 ** -growth[int(key.split(".")[3])]
        elif key.endswith("p6"):
            gain = 1.2 ** -growth[2]
        sd[f"{key}.weight"] = torch.randn(cout, cin, ks, ks, generator=g) * (gain * math.sqrt(2.0 / (cin * ks * ks)))
        sd[f"{key}.bias"] = 0.1 * torch.randn(cout, generator=g)
    for tower in TOWERS:
        for i in range(4):
            sd[f"{tower}.{i}.0.weight"] = torch.randn(FPN_CH, FPN_CH, 3, 3, generator=g) * math.sqrt(2.0 / (FPN_CH * 9))
            sd[f"{tower}.{i}.1.weight"] = 0.5 + torch.rand(FPN_CH, generator=g)
            sd[f"{tower}.{i}.1.bias"] = 0.1 * torch.randn(FPN_CH, generator=g)
    sd[f"{CLS_KEY}.weight"] = torch.randn(NUM_ANCHORS * num_classes, FPN_CH, 3, 3, generator=g) * (1.5 * math.sqrt(1.0 / (FPN_CH * 9)))
    sd[f"{CLS_KEY}.bias"] = torch.full((NUM_ANCHORS * num_classes,), -4.4) + 0.1 * torch.randn(NUM_ANCHORS * num_classes, generator=g)
    sd[f"{REG_KEY}.weight"] = torch.randn(NUM_ANCHORS * 4, FPN_CH, 3, 3, generator=g) * (0.5 * math.sqrt(1.0 / (FPN_CH * 9)))
    sd[f"{REG_KEY}.bias"] = 0.05 * torch.randn(NUM_ANCHORS * 4, generator=g)
    return sd


def random_weights(arch, seed: int = 0, num_classes: int = 91, dev=None, *, min_size: int = 800, max_size: int = 1333) -> DetectorWeights:
    """The structure `load_weights` returns, with `random_state_dict`'s values.  For tests and timing ONLY."""
    return DetectorWeights(arch, random_state_dict(arch, seed, num_classes), min_size=min_size, max_size=max_size, dev=dev,
                           source=f"random_state_dict({arch!r}, {seed})")


# ---- launch wrappers of csrc/detect.hip ----------------------------------------------------------------------------------------

def _need(who, t, dtype, ndim=None):
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or (ndim is not None and t.ndim != ndim):
        raise ValueError(f"{who}: needs a contiguous {dtype} device tensor{'' if ndim is None else f' of {ndim} dimensions'}, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', 'the host')}")


def prep(images: torch.Tensor, wts_or_sizes):
    """fp32 NCHW [N,3,H,W] in [0,1] -> (canvas NHWC [N,HP,WP,3], (RH, RW)): Normalize, the half-pixel bilinear resize to
    `resized_size`, zeros up to the next multiples of 32.  wts_or_sizes: a DetectorWeights or (min_size, max_size)."""
    _need("detect.prep", images, torch.float32, 4)
    n, c, h, w = images.shape
    if c != 3 or n < 1 or h < 1 or w < 1:
        raise ValueError(f"detect.prep: needs a non-empty [N,3,H,W] batch, got {tuple(images.shape)}")
    mn, mx = (wts_or_sizes.min_size, wts_or_sizes.max_size) if isinstance(wts_or_sizes, DetectorWeights) else wts_or_sizes
    rh, rw = resized_size(h, w, mn, mx)
    hp, wp = canvas_size(rh, rw)
    dev = images.device.index
    iy, wy = f32net._device_tables_hp(((h, rh),), dev)
    ix, wx = f32net._device_tables_hp(((w, rw),), dev)
    y = torch.empty(n, hp, wp, 3, dtype=torch.float32, device=images.device)
    check(lib.ur_det_prep(images.data_ptr(), y.data_ptr(), n, h, w, rh, rw, hp, wp, iy.data_ptr(), wy.data_ptr(), ix.data_ptr(), wx.data_ptr(),
                          stream()))
    return y, (rh, rw)


def upsample_nearest_add_f32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [N,OH,OW,C] + F.interpolate(b [N,h,w,C], size=(OH, OW), mode="nearest") on NHWC fp32, any size pair."""
    _need("upsample_nearest_add_f32", a, torch.float32, 4)
    _need("upsample_nearest_add_f32", b, torch.float32, 4)
    n, oh, ow, c = a.shape
    if b.shape[0] != n or b.shape[3] != c or b.device != a.device or a.numel() < 1 or b.numel() < 1:
        raise ValueError(f"upsample_nearest_add_f32: a {tuple(a.shape)} and b {tuple(b.shape)} must share N, C and the device")
    iy, ix = _nearest_tables(b.shape[1], b.shape[2], oh, ow, a.device.index)
    y = torch.empty_like(a)
    check(lib.ur_upsample_nearest_add_f32(a.data_ptr(), b.data_ptr(), y.data_ptr(), n, oh, ow, c, b.shape[1], b.shape[2], iy.data_ptr(),
                                          ix.data_ptr(), stream()))
    return y


def groupnorm_relu_f32(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float = GN_EPS, relu: bool = True) -> torch.Tensor:
    """F.group_norm(groups) of NHWC fp32 [N,H,W,C] (+ ReLU): per (image, group) the mean first, then the biased variance of the
    centred values, in fp64 in a fixed order; the affine in fp64, rounded to fp32 once.  A non-finite value makes its own (image,
    group) NaN and leaves every other one its bits.  Any 4-byte aligned storage offset."""
    if not torch.is_tensor(x) or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous() or x.ndim != 4 or x.numel() < 1:
        raise ValueError(f"groupnorm_relu_f32: needs a non-empty contiguous fp32 [N,H,W,C] device tensor, got {tuple(getattr(x, 'shape', ()))}")
    n, h, w, c = x.shape
    for name, t in (("gamma", gamma), ("beta", beta)):
        if not torch.is_tensor(t) or tuple(t.shape) != (c,) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"groupnorm_relu_f32: {name} must be a contiguous fp32 ({c},) tensor on {x.device}")
    if groups < 1 or c % groups:
        raise ValueError(f"groupnorm_relu_f32: {c} channels do not split into {groups} groups")
    y = torch.empty_like(x)
    check(lib.ur_groupnorm_relu_f32(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), n, h * w, c, groups, float(eps), int(relu), stream()))
    return y


def logit_threshold(score_thresh: float) -> float:
    """fp32(log(t / (1 - t))): `sigmoid(x) > t` decided in the logit domain.  t <= 0 passes every logit that is no NaN but -inf,
    t >= 1 none."""
    t = float(score_thresh)
    if t <= 0.0:
        return float("-inf")
    if t >= 1.0:
        return float("inf")
    return float(np.float32(math.log(t / (1.0 - t))))


def det_select(logits: torch.Tensor, reg, k: int, lt: float, out=None, want_index: bool = False):
    """logits [N, HWA, K] (reg [N, HWA, 4] or None) -> (scores fp32, anchors int32, labels int32, counts int32 [N], nonfinite int32
    [N][, index int32]), the first three [N, k]: per image the first min(k, count) logits > lt in the order (logit descending, flat
    index ascending).  out = (scores, anchors, labels, counts, nonfinite, column): the rows of wider [N, ld] buffers from `column`
    on are written instead."""
    _need("det_select", logits, torch.float32, 3)
    n, hwa, kk = logits.shape
    if reg is not None:
        _need("det_select", reg, torch.float32, 3)
        if tuple(reg.shape) != (n, hwa, 4):
            raise ValueError(f"det_select: reg must be [{n}, {hwa}, 4], got {tuple(reg.shape)}")
    dev = logits.device
    if out is None:
        scores = torch.empty(n, k, dtype=torch.float32, device=dev)
        anchors, labels = torch.empty(n, k, dtype=torch.int32, device=dev), torch.empty(n, k, dtype=torch.int32, device=dev)
        counts, bad, col = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev), 0
    else:
        scores, anchors, labels, counts, bad, col = out
    ld = scores.shape[1]
    index = torch.empty(n, ld, dtype=torch.int32, device=dev) if want_index else None
    ws_bytes = lib.ur_det_select_ws_bytes(n, hwa * kk)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    check(lib.ur_det_select(logits.data_ptr(), None if reg is None else reg.data_ptr(), n, hwa, kk, float(lt), int(k),
                            scores.data_ptr() + 4 * col, anchors.data_ptr() + 4 * col, labels.data_ptr() + 4 * col,
                            None if index is None else index.data_ptr() + 4 * col, ld, counts.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws_bytes,
                            stream()))
    res = (scores, anchors, labels, counts, bad)
    return res + (index,) if want_index else res


def det_decode(reg: torch.Tensor, anchors: torch.Tensor, counts: torch.Tensor, base: torch.Tensor, wf: int, strides, img_size, ratios,
               k: int = None, col: int = 0, out=None, want_raw: bool = False):
    """The boxes of the candidates `anchors` [N, ld] (from column `col`, k of them, counts [N] valid) of one level: reg [N, HWA, 4],
    base fp32 [A, 4], wf the level's width, strides (sh, sw), img_size (h, w) the resized image, ratios (rh, rw) original / resized.
    -> (clipped [N, ld, 4], scaled [N, ld, 4][, raw]); out = (clipped, scaled): written in place."""
    n, hwa, _ = reg.shape
    ld = anchors.shape[1]
    k = ld if k is None else k
    dev = reg.device
    clipped, scaled = (torch.zeros(n, ld, 4, dtype=torch.float32, device=dev), torch.zeros(n, ld, 4, dtype=torch.float32, device=dev)) if out is None else out
    raw = torch.zeros(n, ld, 4, dtype=torch.float32, device=dev) if want_raw else None
    check(lib.ur_det_decode(reg.data_ptr(), anchors.data_ptr() + 4 * col, counts.data_ptr(), base.data_ptr(),
                            None if raw is None else raw.data_ptr() + 16 * col, clipped.data_ptr() + 16 * col, scaled.data_ptr() + 16 * col,
                            n, hwa, k, ld, base.shape[0], wf, strides[0], strides[1], float(img_size[0]), float(img_size[1]),
                            float(ratios[0]), float(ratios[1]), stream()))
    return (clipped, scaled, raw) if want_raw else (clipped, scaled)


def det_nms(boxes, out_boxes, scores, labels, counts, flags, seg: int, nms_thresh: float, detections_per_img: int):
    """Class-aware greedy NMS per image over positions [N, M]: counts int32 [levels, N] (position p is a candidate when p % seg <
    counts[p // seg, n]), flags int32 [levels, N] or None -> (boxes [N,D,4], scores [N,D], labels int64 [N,D], keep int32 [N,D]
    (the kept positions, -1 beyond the count), counts int32 [N], nonfinite int32 [N])."""
    n, m = scores.shape
    dev, d = scores.device, int(detections_per_img)
    levels = counts.shape[0]
    yb = torch.empty(n, d, 4, dtype=torch.float32, device=dev)
    ys = torch.empty(n, d, dtype=torch.float32, device=dev)
    yl = torch.empty(n, d, dtype=torch.int64, device=dev)
    yk = torch.empty(n, d, dtype=torch.int32, device=dev)
    yc, yf = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    ws_bytes = lib.ur_det_nms_ws_bytes(n, m)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    check(lib.ur_det_nms(boxes.data_ptr(), out_boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), counts.data_ptr(),
                         None if flags is None else flags.data_ptr(), n, m, int(seg), levels, float(nms_thresh), d, yb.data_ptr(), ys.data_ptr(),
                         yl.data_ptr(), yk.data_ptr(), yc.data_ptr(), yf.data_ptr(), ws.data_ptr(), ws_bytes, stream()))
    return yb, ys, yl, yk, yc, yf


# ---- the network ---------------------------------------------------------------------------------------------------------------

def fpn(canvas: torch.Tensor, wts: DetectorWeights):
    """The five pyramid levels P3..P7 (NHWC fp32, 256 channels) of a normalised canvas [N,HP,WP,3]."""
    cv = wts.convs
    _c2, c3, c4, c5 = f32net.resnet_trunk(canvas, wts.backbone, wts.stages)
    inner = conv2d_f32(c5, cv["backbone.fpn.inner_blocks.2.0"], relu=False)
    feats = [None, None, conv2d_f32(inner, cv["backbone.fpn.layer_blocks.2.0"], relu=False)]
    for i, c in ((1, c4), (0, c3)):
        inner = upsample_nearest_add_f32(conv2d_f32(c, cv[f"backbone.fpn.inner_blocks.{i}.0"], relu=False), inner)
        feats[i] = conv2d_f32(inner, cv[f"backbone.fpn.layer_blocks.{i}.0"], relu=False)
    p6 = conv2d_f32(c5, cv["backbone.fpn.extra_blocks.p6"], relu=False)
    # relu(P6) is the same convolution with the ReLU in its epilogue: max(bits, 0) of the same sums (C5 is the smallest map)
    p7 = conv2d_f32(conv2d_f32(c5, cv["backbone.fpn.extra_blocks.p6"], relu=True), cv["backbone.fpn.extra_blocks.p7"], relu=False)
    return feats + [p6, p7]


def _tower(x, tower, last, wts):
    for i in range(4):
        g, b = wts.norms[f"{tower}.{i}.1"]
        x = groupnorm_relu_f32(conv2d_f32(x, wts.convs[f"{tower}.{i}.0"], relu=False), g, b, GN_GROUPS)
    return conv2d_f32(x, wts.convs[last], relu=False)


def head_outputs(images: torch.Tensor, wts: DetectorWeights):
    """(logits, regressions, geometry): per level the class logits [N, HWA, K] and box regressions [N, HWA, 4] of fp32 NCHW images
    in [0,1]; geometry = dict(resized=(RH, RW), canvas=(HP, WP), sizes=[(h, w)] per level)."""
    canvas, resized = prep(images, wts)
    n = canvas.shape[0]
    feats = fpn(canvas, wts)
    logits = [_tower(f, TOWERS[0], CLS_KEY, wts).view(n, -1, wts.num_classes) for f in feats]
    regs = [_tower(f, TOWERS[1], REG_KEY, wts).view(n, -1, 4) for f in feats]
    return logits, regs, dict(resized=resized, canvas=tuple(canvas.shape[1:3]), sizes=[tuple(f.shape[1:3]) for f in feats])


def postprocess(logits, regs, geometry, orig_size, score_thresh=SCORE_THRESH, topk_candidates=TOPK_CANDIDATES, nms_thresh=NMS_THRESH,
                detections_per_img=DETECTIONS_PER_IMG, want_candidates: bool = False):
    """torchvision's `postprocess_detections` and the transform's rescale on the heads' outputs: the padded `raw` tensors.
    want_candidates: also the per-image candidate buffers (scores, anchors, labels [N, 5k], counts [5, N], clipped boxes)."""
    n, dev = logits[0].shape[0], logits[0].device
    k = int(topk_candidates)
    if not 1 <= k <= lib.ur_det_select_kmax():
        raise ValueError(f"topk_candidates must be in [1, {lib.ur_det_select_kmax()}], got {topk_candidates}")
    if int(detections_per_img) < 1:
        raise ValueError(f"detections_per_img must be >= 1, got {detections_per_img}")
    nl = len(logits)
    lt = logit_threshold(score_thresh)
    scores = torch.empty(n, nl * k, dtype=torch.float32, device=dev)
    anchors, labels = torch.empty(n, nl * k, dtype=torch.int32, device=dev), torch.empty(n, nl * k, dtype=torch.int32, device=dev)
    counts, flags = torch.empty(nl, n, dtype=torch.int32, device=dev), torch.empty(nl, n, dtype=torch.int32, device=dev)
    clipped, scaled = torch.empty(n, nl * k, 4, dtype=torch.float32, device=dev), torch.empty(n, nl * k, 4, dtype=torch.float32, device=dev)
    (rh, rw), (hp, wp) = geometry["resized"], geometry["canvas"]
    ratios = (float(np.float32(orig_size[0]) / np.float32(rh)), float(np.float32(orig_size[1]) / np.float32(rw)))
    base = _base_anchors_dev(dev.index)
    for l, (lg, rg, (fh, fw)) in enumerate(zip(logits, regs, geometry["sizes"])):
        det_select(lg, rg, k, lt, out=(scores, anchors, labels, counts[l], flags[l], l * k))
        det_decode(rg, anchors, counts[l], base[l], fw, (hp // fh, wp // fw), (rh, rw), ratios, k=k, col=l * k, out=(clipped, scaled))
    res = det_nms(clipped, scaled, scores, labels, counts, flags, k, nms_thresh, detections_per_img)
    out = (res[0], res[1], res[2], res[4], res[5])
    return out + (dict(scores=scores, anchors=anchors, labels=labels, counts=counts, clipped=clipped, scaled=scaled, keep=res[3]),) if want_candidates else out


def raw(images: torch.Tensor, wts: DetectorWeights, score_thresh=SCORE_THRESH, topk_candidates=TOPK_CANDIDATES, nms_thresh=NMS_THRESH,
        detections_per_img=DETECTIONS_PER_IMG):
    """fp32 NCHW images [N,3,H,W] in [0,1] -> (boxes [N,D,4] in the images' own coordinates, scores [N,D], labels int64 [N,D], counts
    int32 [N], nonfinite int32 [N]) with D = detections_per_img, zeros beyond an image's count.  nonfinite[n] = 1: a logit or a
    regression of image n was not finite - it has no detections then.  No host synchronisation: capturable in a torch.cuda.graph
    once a shape has run eagerly (the first call uploads its tables)."""
    if not isinstance(wts, DetectorWeights):
        raise ValueError(f"detect.raw: weights must be a detect.DetectorWeights, got {type(wts).__name__}")
    logits, regs, geometry = head_outputs(images, wts)
    return postprocess(logits, regs, geometry, images.shape[2:], score_thresh, topk_candidates, nms_thresh, detections_per_img)


def forward(images: torch.Tensor, wts: DetectorWeights, **params):
    """torchvision's result: per image {boxes [n,4], scores [n], labels int64 [n]}, after one read of the counts.  The flags are
    returned as the second value: int32 [N] on the host."""
    boxes, scores, labels, counts, bad = raw(images, wts, **params)
    cb = torch.stack([counts, bad]).cpu()
    return [dict(boxes=boxes[i, :c], scores=scores[i, :c], labels=labels[i, :c]) for i, c in enumerate(cb[0].tolist())], cb[1]


# ---- the metric ----------------------------------------------------------------------------------------------------------------

def box_iou_np(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """fp64 IoU matrix [len(a), len(b)] of x1 y1 x2 y2 boxes (pycocotools' for non-crowd boxes)."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 4), np.asarray(b, dtype=np.float64).reshape(-1, 4)
    iw = np.clip(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0, None)
    inter = iw * ih
    union = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] + ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(union > 0, inter / union, 0.0)


RECALL_POINTS = np.linspace(0.0, 1.0, 101)


class MeanAP:
    """pycocotools' average precision at ONE IoU threshold, area range `all`, no crowd, `max_dets` detections per image and class:
    what torchmetrics' `MeanAveragePrecision(iou_thresholds=[t])` reports as `map`.  Matching is per image, so the state is the
    per-class (score, tp) lists and ground-truth counts; `merge` concatenates the lists of another instance (another rank)."""

    def __init__(self, iou_threshold: float = 0.5, max_dets: int = 100):
        if not 0.0 < float(iou_threshold) <= 1.0 or int(max_dets) < 1:
            raise ValueError(f"MeanAP: iou_threshold must be in (0, 1] and max_dets >= 1, got {iou_threshold!r}, {max_dets!r}")
        self.iou_threshold, self.max_dets = float(iou_threshold), int(max_dets)
        self.scores, self.tps, self.n_gt = {}, {}, {}

    @staticmethod
    def _np(t, dtype):
        return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(dtype)

    def update(self, detections, targets):
        """detections: per image {boxes [n,4], scores [n], labels [n]}; targets: per image {boxes [m,4], labels [m]}."""
        if len(detections) != len(targets):
            raise ValueError(f"MeanAP.update: {len(detections)} detections for {len(targets)} targets")
        thr = min(self.iou_threshold, 1 - 1e-10)
        for det, tgt in zip(detections, targets):
            db, ds, dl = self._np(det["boxes"], np.float64).reshape(-1, 4), self._np(det["scores"], np.float64).reshape(-1), \
                self._np(det["labels"], np.int64).reshape(-1)
            gb, gl = self._np(tgt["boxes"], np.float64).reshape(-1, 4), self._np(tgt["labels"], np.int64).reshape(-1)
            for c in sorted(set(dl.tolist()) | set(gl.tolist())):
                g = gb[gl == c]
                self.n_gt[c] = self.n_gt.get(c, 0) + len(g)
                sel = np.flatnonzero(dl == c)
                sel = sel[np.argsort(-ds[sel], kind="stable")][:self.max_dets]
                if not len(sel):
                    continue
                ious = box_iou_np(db[sel], g)
                taken = np.zeros(len(g), dtype=bool)
                tp = np.zeros(len(sel), dtype=bool)
                for i in range(len(sel)):
                    best, m = thr, -1
                    for j in range(len(g)):                   # cocoeval's loop: `<` skips, so an equal IoU moves on to the later one
                        if taken[j] or ious[i, j] < best:
                            continue
                        best, m = ious[i, j], j
                    if m >= 0:
                        taken[m] = tp[i] = True
                self.scores.setdefault(c, []).append(ds[sel])
                self.tps.setdefault(c, []).append(tp)

    def merge(self, other: "MeanAP"):
        if (other.iou_threshold, other.max_dets) != (self.iou_threshold, self.max_dets):
            raise ValueError("MeanAP.merge: the two states were built with different parameters")
        for c, n in other.n_gt.items():
            self.n_gt[c] = self.n_gt.get(c, 0) + n
        for c in other.scores:
            self.scores.setdefault(c, []).extend(other.scores[c])
            self.tps.setdefault(c, []).extend(other.tps[c])
        return self

    def average_precision(self, c) -> float:
        n_gt = self.n_gt.get(c, 0)
        if n_gt == 0:
            return -1.0
        if c not in self.scores:
            return 0.0
        s, tp = np.concatenate(self.scores[c]), np.concatenate(self.tps[c])
        order = np.argsort(-s, kind="stable")
        tp = tp[order]
        ctp, cfp = np.cumsum(tp).astype(np.float64), np.cumsum(~tp).astype(np.float64)
        recall = ctp / n_gt
        prec = ctp / (ctp + cfp + np.spacing(1))
        for i in range(len(prec) - 1, 0, -1):
            if prec[i] > prec[i - 1]:
                prec[i - 1] = prec[i]
        idx = np.searchsorted(recall, RECALL_POINTS, side="left")
        q = np.zeros(len(RECALL_POINTS))
        ok = idx < len(prec)
        q[ok] = prec[idx[ok]]
        return float(q.mean())

    def compute(self) -> dict:
        per_class = {int(c): self.average_precision(c) for c in sorted(self.n_gt) if self.n_gt[c] > 0}
        return {"map": float(np.mean(list(per_class.values()))) if per_class else -1.0, "per_class": per_class}
