"""LPIPS (AlexNet, v0.1 linear layers) on the GPU in exact fp32: weight loading, the layer plan and the launch wrappers of
csrc/lpips.hip, on the fp32 layers of f32net.py.  What the reference's evaluator builds as `LPIPS(net_type="alex", normalize=True)`
(eval_image_restoration.py:181-185), run with autocast off.

The project ships NO weights.  `load_weights` reads the two files a user of the metric already has (torchvision's AlexNet state
dict and the LPIPS v0.1 `alex.pth` linear layers); `random_weights` makes seeded stand-ins for tests and timing.
"""
import ctypes as C
import math

import torch

from . import f32net
from .capi import check, lib
from .f32net import PackedConvF32, stream, take

# (state-dict index, Cout, Cin, kernel, stride, pad) of AlexNet's five convolutions; every ReLU output is a tap
CONVS = ((0, 64, 3, 11, 4, 2), (3, 192, 64, 5, 1, 2), (6, 384, 192, 3, 1, 1), (8, 256, 384, 3, 1, 1), (10, 256, 256, 3, 1, 1))
POOL_BEFORE = (False, True, True, False, False)          # a 3x3 / stride-2 max-pool in front of conv2 and conv3
MIN_HW = 31                                              # the smallest input at which the fifth tap still has one pixel


class LpipsWeights:
    """AlexNet's five convolutions (repacked, on the device) and the five non-negative linear-layer vectors.  `cpu` keeps the
    tensors as they were given (conv{i}.weight OIHW, conv{i}.bias, lin{i}): what a host restatement of the metric needs."""

    def __init__(self, convs, lins, dev=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        self.device = dev
        self.cpu = {}
        self.convs, self.lins = [], []
        for i, ((w, b), lin, (_, cout, cin, k, stride, pad)) in enumerate(zip(convs, lins, CONVS)):
            self.cpu[f"conv{i}.weight"], self.cpu[f"conv{i}.bias"], self.cpu[f"lin{i}"] = w.float(), b.float(), lin.float().reshape(-1)
            self.convs.append(PackedConvF32(w, b, stride, pad, dev))
            self.lins.append(lin.float().reshape(-1).contiguous().to(dev))


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def load_weights(alexnet_path, lin_path, dev=None) -> LpipsWeights:
    """alexnet_path: torchvision's AlexNet state dict (`features.{0,3,6,8,10}.{weight,bias}`; `classifier.*` is ignored);
    lin_path: the LPIPS v0.1 linear layers (`lin{0..4}.model.1.weight`, [1,C,1,1]).  Both are user-supplied: none ship here.
    ValueError (file and key named) for a missing key, a wrong shape or a negative linear weight - LPIPS's linear weights are
    non-negative by construction, so a negative one means a wrong file."""
    asd, lsd = _load(alexnet_path), _load(lin_path)
    convs, lins = [], []
    for i, (idx, cout, cin, k, _s, _p) in enumerate(CONVS):
        convs.append((take(asd, alexnet_path, f"features.{idx}.weight", (cout, cin, k, k), finite=False),
                      take(asd, alexnet_path, f"features.{idx}.bias", (cout,), finite=False)))
        key = f"lin{i}.model.1.weight"
        lin = take(lsd, lin_path, key, (1, cout, 1, 1), finite=False)
        if bool((lin < 0).any()) or not bool(torch.isfinite(lin).all()):
            raise ValueError(f"{lin_path}: {key!r} holds a negative or non-finite weight: not an LPIPS linear layer")
        lins.append(lin)
    return LpipsWeights(convs, lins, dev)


def random_state_dicts(seed: int):
    """Seeded stand-ins in the two real key layouts: (alexnet state dict, lin state dict).  Kaiming-scaled convolutions
    (std sqrt(2 / fan_in)), small biases, non-negative linear weights.  NOT the published weights."""
    g = torch.Generator().manual_seed(seed)
    asd, lsd = {}, {}
    for i, (idx, cout, cin, k, _s, _p) in enumerate(CONVS):
        asd[f"features.{idx}.weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
        asd[f"features.{idx}.bias"] = 0.1 * torch.randn(cout, generator=g)
        lsd[f"lin{i}.model.1.weight"] = torch.rand(1, cout, 1, 1, generator=g) / cout
    return asd, lsd


def random_weights(seed: int = 0, dev=None) -> LpipsWeights:
    """The structure `load_weights` returns, with seeded random values.  For tests and timing ONLY: no real weights exist where
    this project is developed, so its values say nothing about published LPIPS numbers - no parity with them is claimed."""
    asd, lsd = random_state_dicts(seed)
    return LpipsWeights([(asd[f"features.{c[0]}.weight"], asd[f"features.{c[0]}.bias"]) for c in CONVS],
                        [lsd[f"lin{i}.model.1.weight"] for i in range(len(CONVS))], dev)


# ---- launch wrappers of csrc/lpips.hip (fp32 NHWC device tensors) --------------------------------------------------------------

def tap_hw(h: int, w: int, tap: int):
    oh, ow = C.c_int(), C.c_int()
    check(lib.ur_lpips_tap_hw(h, w, tap, oh, ow))
    return oh.value, ow.value


def prep(x: torch.Tensor) -> torch.Tensor:
    """fp32 NCHW [N,3,H,W] in [0,1] -> NHWC [N,H,W,3], scaled as LPIPS's ScalingLayer does after normalize=True."""
    n, c, h, w = x.shape
    y = torch.empty(n, h, w, 3, dtype=torch.float32, device=x.device)
    check(lib.ur_lpips_prep(x.data_ptr(), y.data_ptr(), n, c, h, w, stream()))
    return y


def layer_parts(pixels: int) -> int:
    r = lib.ur_lpips_layer_parts(pixels)
    if r < 0:
        check(int(r))
    return int(r)


def layer(feat: torch.Tensor, lin: torch.Tensor, part: torch.Tensor = None) -> torch.Tensor:
    """One tap: feat [2N,OH,OW,C] (predictions first) -> fp64 [N, parts] partial sums over pixels (into `part` when given)."""
    n2, oh, ow, c = feat.shape
    n, p = n2 // 2, oh * ow
    if n2 % 2 or lin.numel() != c:
        raise ValueError(f"lpips layer: feat {tuple(feat.shape)} needs an even batch and {c} linear weights, got {lin.numel()}")
    if part is None:
        part = torch.empty(n, layer_parts(p), dtype=torch.float64, device=feat.device)
    check(lib.ur_lpips_layer(feat.data_ptr(), lin.data_ptr(), n, p, c, part.data_ptr(), part.numel() * 8, stream()))
    return part


def features(x2: torch.Tensor, wts: LpipsWeights):
    """The five taps (NHWC fp32) of a [2N,3,H,W] batch."""
    taps, f = [], prep(x2)
    for pc, pool in zip(wts.convs, POOL_BEFORE):
        if pool:
            f = f32net.maxpool2d_f32(f)
        f = f32net.conv2d_f32(f, pc, relu=True)
        taps.append(f)
    return taps


def forward(pred: torch.Tensor, target: torch.Tensor, wts: LpipsWeights) -> torch.Tensor:
    """ops.lpips after its argument checks: fp64 [N]."""
    n, _c, h, w = pred.shape
    dev = pred.device
    ws_bytes = lib.ur_lpips_ws_size(n, h, w)
    if ws_bytes < 0:
        check(int(ws_bytes))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    off = 0
    for feat, lin in zip(features(torch.cat([pred, target]), wts), wts.lins):
        cnt = n * layer_parts(feat.shape[1] * feat.shape[2])
        layer(feat, lin, ws[off:off + cnt])
        off += cnt
    check(lib.ur_lpips_finish(ws.data_ptr(), ws_bytes, n, h, w, out.data_ptr(), stream()))
    return out
