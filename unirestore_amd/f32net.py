"""The fp32 NHWC layer format of the scoring networks (LPIPS's AlexNet, the classifier's ResNet, the segmenters' RefineNet-LW and
DeepLabV3+), stated once: the `[Kpad][Cout_pad]` weight repack and `PackedConvF32`, the launch wrappers of csrc/f32_layers.hip
(the table-driven bilinear resize with either table, dense or into a channel slice, among them) and of the two generic layers of
csrc/vit.hip (LayerNorm and the exact-erf GELU, which the ViT scorer of vit.py brought), the state-dict checks with the
conv + BatchNorm fold, and the torchvision-layout ResNet backbone that three of the networks share.  What belongs to one metric
alone (its preprocess, its head, its formula) stays in lpips.py, classify.py, segment.py and deeplab.py; the next scoring network
is written against this module.
"""
import ctypes as C
import functools
import math

import torch

from .capi import check, lib

PLANES = (64, 128, 256, 512)
EXPANSION = {"basic": 1, "bottleneck": 4}
BN_EPS = 1e-5


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the packed convolution ----------------------------------------------------------------------------------------------------

def wpack_dims(cin, cout, kh, kw):
    """(Kpad, Cout_pad) of the kernel's weight layout."""
    kpad, cpad = C.c_int(), C.c_int()
    check(lib.ur_conv2d_f32_wpack_dims(cin, cout, kh, kw, kpad, cpad))
    return kpad.value, cpad.value


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 filter -> the kernel's [Kpad][Cout_pad] layout (CPU tensor): row k = (kh * KW + kw) * Cin + cin, zero-filled."""
    cout, cin, kh, kw = w.shape
    kpad, cpad = wpack_dims(cin, cout, kh, kw)
    out = torch.zeros(kpad, cpad, dtype=torch.float32)
    out[:cin * kh * kw, :cout] = w.float().permute(2, 3, 1, 0).reshape(kh * kw * cin, cout)
    return out


class PackedConvF32:
    """One fp32 convolution ready for ur_conv2d_f32_res (ur_dlv3_conv2d_f32 when dilated): the repacked filter and the bias on the
    device, and its geometry."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, stride: int, pad: int, dev, dilation: int = 1):
        self.cout, self.cin, self.kh, self.kw = weight.shape
        self.stride, self.pad, self.dilation = stride, pad, dilation
        self.w = pack_conv_weight(weight).to(dev)
        self.bias = bias.float().contiguous().to(dev)


# ---- launch wrappers (each one kernel family; fp32 NHWC device tensors) -------------------------------------------------------

def conv2d_f32(x: torch.Tensor, pc: PackedConvF32, res: torch.Tensor = None, relu: bool = True, out=None) -> torch.Tensor:
    """act(conv(x) + bias + res) on NHWC fp32; res None: no residual.  out = (buffer, channel_offset): the result goes to channels
    channel_offset .. channel_offset + Cout - 1 of `buffer`, a contiguous fp32 [N,OH,OW,C >= offset + Cout] tensor whose other
    channels stay as they are, and `buffer` is returned.  An undilated convolution without `out` is ur_conv2d_f32_res; a dilated
    one, or one with `out`, is ur_dlv3_conv2d_f32 - the same kernel.
    Non-finite inputs: every output is finite, +inf, -inf or NaN exactly where torch's F.conv2d (+ res) and torch.relu are in fp64
    (relu keeps NaN and +inf and turns -inf into 0); a value no filter tap reads reaches no output; an image without a non-finite
    value gets the bits it gets in a clean batch (tests/test_nonfinite_gpu.py)."""
    n, h, w, cin = x.shape
    if cin != pc.cin:
        raise ValueError(f"conv2d_f32: input has {cin} channels, the filter {pc.cin}")
    dil = pc.dilation
    oh, ow = (h + 2 * pc.pad - dil * (pc.kh - 1) - 1) // pc.stride + 1, (w + 2 * pc.pad - dil * (pc.kw - 1) - 1) // pc.stride + 1
    shape = (n, max(oh, 0), max(ow, 0), pc.cout)
    if res is not None and (tuple(res.shape) != shape or res.dtype != torch.float32 or not res.is_contiguous() or res.device != x.device):
        raise ValueError(f"conv2d_f32: the residual must be a contiguous fp32 {shape} tensor on {x.device}, got "
                         f"{res.dtype} {tuple(res.shape)} on {res.device}")
    if out is None and dil == 1:
        y = torch.empty(shape, dtype=torch.float32, device=x.device)
        check(lib.ur_conv2d_f32_res(x.data_ptr(), pc.w.data_ptr(), pc.bias.data_ptr(), None if res is None else res.data_ptr(), y.data_ptr(),
                                    n, h, w, cin, pc.cout, pc.kh, pc.kw, pc.stride, pc.pad, int(relu), stream()))
        return y
    buf, off = (torch.empty(shape, dtype=torch.float32, device=x.device), 0) if out is None else out
    if (buf.ndim != 4 or tuple(buf.shape[:3]) != shape[:3] or buf.dtype != torch.float32 or not buf.is_contiguous() or buf.device != x.device
            or not 0 <= off <= buf.shape[3] - pc.cout):
        raise ValueError(f"conv2d_f32: out must be a contiguous fp32 [{n}, {shape[1]}, {shape[2]}, C] tensor on {x.device} with "
                         f"offset + {pc.cout} <= C, got {buf.dtype} {tuple(buf.shape)} on {buf.device}, offset {off}")
    check(lib.ur_dlv3_conv2d_f32(x.data_ptr(), pc.w.data_ptr(), pc.bias.data_ptr(), None if res is None else res.data_ptr(),
                                 buf.data_ptr() + 4 * off, n, h, w, cin, pc.cout, pc.kh, pc.kw, pc.stride, pc.pad, dil, buf.shape[3], int(relu),
                                 stream()))
    return buf


def maxpool2d_f32(x: torch.Tensor) -> torch.Tensor:
    """3x3 / stride 2 / no padding, floor mode, on NHWC fp32.  As torch.max_pool2d, a NaN in any tap of a window is the window's
    maximum (the three max-pools share this: a non-finite pixel is not dropped on the way to a score); a window of -inf gives
    -inf; the rows and columns the floor drops are not read."""
    n, h, w, c = x.shape
    y = torch.empty(n, max((h - 3) // 2 + 1, 0), max((w - 3) // 2 + 1, 0), c, dtype=torch.float32, device=x.device)
    check(lib.ur_maxpool2d_f32(x.data_ptr(), y.data_ptr(), n, h, w, c, stream()))
    return y


def maxpool2d_pad_f32(x: torch.Tensor) -> torch.Tensor:
    """3x3 / stride 2 / padding 1 (-inf) on NHWC fp32.  NaN and -inf as in maxpool2d_f32."""
    n, h, w, c = x.shape
    y = torch.empty(n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c, dtype=torch.float32, device=x.device)
    check(lib.ur_maxpool2d_pad_f32(x.data_ptr(), y.data_ptr(), n, h, w, c, stream()))
    return y


def maxpool5_f32(x: torch.Tensor) -> torch.Tensor:
    """5x5 / stride 1 / padding 2 (-inf) on NHWC fp32.  NaN and -inf as in maxpool2d_f32, with C % 4 == 0 (float4) or not."""
    n, h, w, c = x.shape
    y = torch.empty_like(x)
    check(lib.ur_maxpool5_f32(x.data_ptr(), y.data_ptr(), n, h, w, c, stream()))
    return y


def avgpool_f32(x: torch.Tensor) -> torch.Tensor:
    """[N,H,W,C] -> [N,C], the mean over the map."""
    n, h, w, c = x.shape
    y = torch.empty(n, c, dtype=torch.float32, device=x.device)
    check(lib.ur_avgpool_f32(x.data_ptr(), y.data_ptr(), n, h * w, c, stream()))
    return y


def add_f32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a + b on contiguous fp32 tensors of one shape."""
    y = torch.empty_like(a)
    check(lib.ur_add_f32(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), stream()))
    return y


def _check_rows(who, x):
    if not torch.is_tensor(x) or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous() or x.ndim < 1 or x.numel() < 1:
        raise ValueError(f"{who}: needs a non-empty contiguous fp32 device tensor, got {getattr(x, 'dtype', type(x))} "
                         f"{tuple(getattr(x, 'shape', ()))} on {getattr(x, 'device', 'the host')}")


def layernorm_f32(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, first_row_of: int = 1) -> torch.Tensor:
    """F.layer_norm over the last axis of a contiguous fp32 [..., D] tensor: (x - mean) / sqrt(var + eps) * gamma + beta, the mean
    first and then the biased variance of the centred values, in fp64, rounded to fp32 once.  first_row_of = S > 1: x is [N, S, D]
    and only row 0 of every image is normalised (a ViT's class token) -> [N, D].
    Non-finite inputs: a row that holds a NaN or an infinity is all NaN, as F.layer_norm; the other rows keep their bits."""
    _check_rows("layernorm_f32", x)
    d = x.shape[-1]
    for name, t in (("gamma", gamma), ("beta", beta)):
        if not torch.is_tensor(t) or tuple(t.shape) != (d,) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"layernorm_f32: {name} must be a contiguous fp32 ({d},) tensor on {x.device}, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if first_row_of == 1:
        rows, ldx, shape = x.numel() // d, d, x.shape
    else:
        if x.ndim != 3 or x.shape[1] != first_row_of:
            raise ValueError(f"layernorm_f32: first_row_of={first_row_of} needs an [N, {first_row_of}, D] tensor, got {tuple(x.shape)}")
        rows, ldx, shape = x.shape[0], first_row_of * d, (x.shape[0], d)
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    check(lib.ur_layernorm_f32(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), rows, d, float(eps), ldx, stream()))
    return y


def gelu_f32(x: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """The exact-erf GELU 0.5 x (1 + erf(x / sqrt 2)) of a contiguous fp32 tensor, with libm's erff; inplace: x is overwritten and
    returned.  Non-finite inputs: NaN -> NaN, +inf -> +inf, -inf -> NaN (-inf * 0, the formula's own result and torch's in fp64)."""
    _check_rows("gelu_f32", x)
    y = x if inplace else torch.empty_like(x)
    check(lib.ur_gelu_f32(x.data_ptr(), y.data_ptr(), x.numel(), stream()))
    return y


def ac_table(n_in: int, n_out: int):
    """One axis of `interpolate(mode="bilinear", align_corners=True)`: (idx [n_out] int32, wt [n_out, 2] fp64).  Output o reads
    sources idx[o] and idx[o] + 1 with weights wt[o]; its source coordinate o * (n_in - 1) / (n_out - 1) (0 when n_out == 1) is
    split into index and fraction in integers, so the fraction is the correctly rounded fp64 value."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"ac_table: sizes must be >= 1, got {n_in} -> {n_out}")
    idx, wt = [], []
    for o in range(n_out):
        q, rem = divmod(o * (n_in - 1), n_out - 1) if n_out > 1 else (0, 0)
        frac = rem / (n_out - 1) if rem else 0.0                     # (rem == 0 also where the last output sits on the last source)
        idx.append(q)
        wt.append((1.0 - frac, frac))
    return torch.tensor(idx, dtype=torch.int32), torch.tensor(wt, dtype=torch.float64)


def hp_table(n_in: int, n_out: int):
    """One axis of `interpolate(mode="bilinear", align_corners=False)` (half-pixel centres), in ac_table's layout: output o has the
    source coordinate max(0, (o + 0.5) * n_in / n_out - 0.5) = max(0, (2 o + 1) n_in - n_out) / (2 n_out), split into index and
    fraction in integers, so the fraction is the correctly rounded fp64 value.  idx[o] + 1 may be n_in: the kernels clamp it to the
    axis, as torch does (both taps then read the last source)."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"hp_table: sizes must be >= 1, got {n_in} -> {n_out}")
    idx, wt = [], []
    for o in range(n_out):
        q, rem = divmod(max((2 * o + 1) * n_in - n_out, 0), 2 * n_out)      # q <= n_in - 1: the coordinate is below n_in - 1/2
        frac = rem / (2 * n_out) if rem else 0.0
        idx.append(q)
        wt.append((1.0 - frac, frac))
    return torch.tensor(idx, dtype=torch.int32), torch.tensor(wt, dtype=torch.float64)


@functools.lru_cache(maxsize=None)                       # never evicted: a captured graph keeps reading the tables it was captured with
def _device_tables_hp(pairs: tuple, dev_index: int):
    """The half-pixel tables of several (n_in, n_out) axes, one after the other: (idx [sum n_out], wt [sum n_out, 2] fp32)."""
    tabs = [hp_table(n_in, n_out) for n_in, n_out in pairs]
    dev = torch.device("cuda", dev_index)
    return torch.cat([t[0] for t in tabs]).to(dev), torch.cat([t[1] for t in tabs]).float().contiguous().to(dev)


@functools.lru_cache(maxsize=None)                       # never evicted: a captured graph keeps reading the tables it was captured with
def _device_tables(n_ins: tuple, n_out: int, dev_index: int):
    """The tables of several source axes to one output axis, one after the other: (idx [len(n_ins) * n_out], wt [.., 2] fp32)."""
    tabs = [ac_table(n_in, n_out) for n_in in n_ins]
    dev = torch.device("cuda", dev_index)
    return torch.cat([t[0] for t in tabs]).to(dev), torch.cat([t[1] for t in tabs]).float().contiguous().to(dev)


def _upsample_bilinear(who, x, size, tables_h, tables_w, out, entry):
    """The table-driven resize of NHWC fp32 x to `size` with the (idx, wt) device tables of the two axes.  out = (buffer,
    channel_offset) or None for a new dense tensor; entry(x ptr, y ptr, n, h, w, c, oh, ow, ldy, *table ptrs, stream) launches."""
    n, h, w, c = x.shape
    oh, ow = size
    buf, off = (torch.empty(n, oh, ow, c, dtype=torch.float32, device=x.device), 0) if out is None else out
    if (buf.ndim != 4 or tuple(buf.shape[:3]) != (n, oh, ow) or buf.dtype != torch.float32 or not buf.is_contiguous() or buf.device != x.device
            or not 0 <= off <= buf.shape[3] - c):
        raise ValueError(f"{who}: out must be a contiguous fp32 [{n}, {oh}, {ow}, >= offset + {c}] tensor on {x.device}, got "
                         f"{buf.dtype} {tuple(buf.shape)} on {buf.device}, offset {off}")
    check(entry(x.data_ptr(), buf.data_ptr() + 4 * off, n, h, w, c, oh, ow, buf.shape[3], *(t.data_ptr() for t in (*tables_h, *tables_w)),
                stream()))
    return buf


def upsample_bilinear_ac_f32(x: torch.Tensor, size) -> torch.Tensor:
    """NHWC fp32 [N,h,w,C] -> [N,H,W,C], bilinear with align_corners=True; the same size is the identity, bit for bit, while the
    values are finite (0 x inf from a neighbour is NaN, as in torch; a -0.0 may come out as +0.0)."""
    def dense(xp, yp, n, h, w, c, oh, ow, _ldy, *tables_and_stream):          # the dense export has no ldy: it is C
        return lib.ur_upsample_bilinear_ac_f32(xp, yp, n, h, w, c, oh, ow, *tables_and_stream)
    dev = x.device.index
    return _upsample_bilinear("upsample_bilinear_ac_f32", x, size, _device_tables((x.shape[1],), size[0], dev),
                              _device_tables((x.shape[2],), size[1], dev), None, dense)


def upsample_bilinear_hp_f32(x: torch.Tensor, size, out=None) -> torch.Tensor:
    """NHWC fp32 [N,h,w,C] -> [N,H,W,C], bilinear with align_corners=False (half-pixel centres, hp_table).  out = (buffer,
    channel_offset): the result goes to that channel slice of a contiguous fp32 [N,H,W,C_all] buffer, which is returned."""
    dev = x.device.index
    return _upsample_bilinear("upsample_bilinear_hp_f32", x, size, _device_tables_hp(((x.shape[1], size[0]),), dev),
                              _device_tables_hp(((x.shape[2], size[1]),), dev), out, lib.ur_dlv3_upsample_f32)


def broadcast_f32(v: torch.Tensor, out, channel_offset: int) -> torch.Tensor:
    """v fp32 [N,C] -> channels channel_offset .. channel_offset + C - 1 of every pixel of `out` (contiguous fp32 [N,H,W,C_all]);
    returns `out`.  The bilinear resize of a 1 x 1 map, which is the value itself whatever align_corners says."""
    n, c = v.shape
    if (out.ndim != 4 or out.shape[0] != n or out.dtype != torch.float32 or not out.is_contiguous() or out.device != v.device
            or not v.is_contiguous() or v.dtype != torch.float32 or not 0 <= channel_offset <= out.shape[3] - c):
        raise ValueError(f"broadcast_f32: needs a contiguous fp32 [{n}, C] vector and a contiguous fp32 [{n}, H, W, >= offset + C] buffer on one "
                         f"device, got {v.dtype} {tuple(v.shape)} and {out.dtype} {tuple(out.shape)}, offset {channel_offset}")
    check(lib.ur_dlv3_broadcast_f32(v.data_ptr(), out.data_ptr() + 4 * channel_offset, n, out.shape[1] * out.shape[2], c, out.shape[3], stream()))
    return out


# ---- state dicts: checks, and the conv + BatchNorm fold ------------------------------------------------------------------------

def read_state_dict(path) -> dict:
    """A torchvision state dict, or a Lightning checkpoint: its ["state_dict"] with a leading `model.` stripped from every key,
    as the reference's `_load_ckpt` does."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd["state_dict"].items()}
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state dict")
    return sd


def take(sd, source, key, shape, finite=True, keep=None):
    """sd[key] as an fp32 CPU tensor: ValueError (`source` and key named) when it is missing, has another shape or - with `finite` -
    holds a non-finite value.  `keep`: a dict that receives the tensor under its key."""
    if key not in sd:
        raise ValueError(f"{source}: key {key!r} is missing")
    t = sd[key]
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{source}: {key!r} has shape {tuple(getattr(t, 'shape', ()))}, expected {tuple(shape)}")
    t = t.detach().float().cpu()
    if finite and not bool(torch.isfinite(t).all()):
        raise ValueError(f"{source}: {key!r} holds a non-finite value")
    if keep is not None:
        keep[key] = t
    return t


def fold_bn(w, gamma, beta, mean, var, eps: float = BN_EPS):
    """conv (no bias) followed by eval-mode BatchNorm as one convolution, folded in fp64: (weight fp64, bias fp64)."""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * scale.view(-1, 1, 1, 1), beta.double() - mean.double() * scale


def fold_convs(plan, sd, source, keep):
    """Every (conv, BatchNorm) pair of `plan` taken from sd, checked and folded: [(conv key, weight fp32, bias fp32, stride, pad)].
    Host only - the caller uploads once every check of the file has passed."""
    folded = []
    for ckey, bkey, cout, cin, k, stride, pad in plan:
        w = take(sd, source, f"{ckey}.weight", (cout, cin, k, k), keep=keep)
        bn = [take(sd, source, f"{bkey}.{n}", (cout,), keep=keep) for n in ("weight", "bias", "running_mean", "running_var")]
        if not bool((bn[3].double() + BN_EPS > 0).all()):
            raise ValueError(f"{source}: {bkey + '.running_var'!r} + eps is not positive: not a trained BatchNorm")
        fw, fb = fold_bn(w, *bn)
        if not (bool(torch.isfinite(fw).all()) and bool(torch.isfinite(fb).all())):
            raise ValueError(f"{source}: folding {bkey!r} into {ckey!r} gives a non-finite value")
        folded.append((ckey, fw.float(), fb.float(), stride, pad))
    return folded


# ---- the ResNet backbone (torchvision's layout, the stride on the 3x3 convolution: ResNet v1.5) --------------------------------

def resnet_plan(kind, depths):
    """[(conv key, bn key, Cout, Cin, kernel, stride, pad)] of every convolution of a "basic" or "bottleneck" ResNet with `depths`
    blocks per stage, in state-dict order."""
    exp = EXPANSION[kind]
    plan = [("conv1", "bn1", 64, 3, 7, 2, 3)]
    cin = 64
    for li, (planes, depth) in enumerate(zip(PLANES, depths), 1):
        for bi in range(depth):
            stride = 2 if (li > 1 and bi == 0) else 1
            p = f"layer{li}.{bi}"
            if kind == "basic":
                plan += [(f"{p}.conv1", f"{p}.bn1", planes, cin, 3, stride, 1), (f"{p}.conv2", f"{p}.bn2", planes, planes, 3, 1, 1)]
            else:
                plan += [(f"{p}.conv1", f"{p}.bn1", planes, cin, 1, 1, 0), (f"{p}.conv2", f"{p}.bn2", planes, planes, 3, stride, 1),
                         (f"{p}.conv3", f"{p}.bn3", planes * exp, planes, 1, 1, 0)]
            if stride != 1 or cin != planes * exp:
                plan.append((f"{p}.downsample.0", f"{p}.downsample.1", planes * exp, cin, 1, stride, 0))
            cin = planes * exp
    return plan


def resnet_stages(kind, depths, convs):
    """The blocks in execution order, by stage: (conv keys of the main path, downsample key or None)."""
    per_block = 2 if kind == "basic" else 3
    return [[([f"layer{li}.{bi}.conv{j}" for j in range(1, per_block + 1)],
              f"layer{li}.{bi}.downsample.0" if f"layer{li}.{bi}.downsample.0" in convs else None) for bi in range(depth)]
            for li, depth in enumerate(depths, 1)]


def resnet_trunk(x: torch.Tensor, convs, stages):
    """Stem and the four stages on an NHWC fp32 input [N,H,W,3]: the four stage outputs.  Per block: the downsample first, then
    the main path, the residual sum and the ReLU in the last convolution's epilogue."""
    f = maxpool2d_pad_f32(conv2d_f32(x, convs["conv1"]))
    feats = []
    for blocks in stages:
        for main, down in blocks:
            identity = f if down is None else conv2d_f32(f, convs[down], relu=False)
            y = f
            for key in main[:-1]:
                y = conv2d_f32(y, convs[key])
            f = conv2d_f32(y, convs[main[-1]], res=identity)
        feats.append(f)
    return feats


def random_backbone(plan, kind, g, conv1_gain=1.0):
    """The backbone part of a seeded stand-in state dict, drawn from generator `g` in plan order: Kaiming-scaled convolutions (std
    sqrt(2 / fan_in); conv1 times `conv1_gain`), BatchNorm gamma in [0.5, 1.5] (halved on the last BatchNorm of every block, so the
    residual sums do not grow), running_var in [0.5, 1.5], small beta and running_mean."""
    sd = {}
    for ckey, bkey, cout, cin, k, _s, _p in plan:
        gain = conv1_gain if ckey == "conv1" else 1.0
        sd[f"{ckey}.weight"] = torch.randn(cout, cin, k, k, generator=g) * (gain * math.sqrt(2.0 / (cin * k * k)))
        last = ckey.endswith("conv3") or (kind == "basic" and ckey.endswith("conv2"))
        sd[f"{bkey}.weight"] = (0.5 + torch.rand(cout, generator=g)) * (0.5 if last else 1.0)
        sd[f"{bkey}.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{bkey}.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{bkey}.running_var"] = 0.5 + torch.rand(cout, generator=g)
        sd[f"{bkey}.num_batches_tracked"] = torch.tensor(0)
    return sd
