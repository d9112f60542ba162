"""Torch-tensor front end of the HIP kernels (device pointers + current HIP stream -> C ABI).

Activations are NHWC bf16 tensors ([N,H,W,C] or [rows, C]); C is always a multiple of 8 (thin tensors such as
images / latents are zero-padded to 8 channels).  PyTorch only owns memory and the stream here.
"""
from dataclasses import dataclass
from typing import Optional

import torch

from . import capi
from .capi import (UR_ACT_GATE, UR_ACT_GEGLU, UR_ACT_GELU, UR_ACT_NONE, UR_ACT_RELU, UR_ACT_SILU, UR_ACT_TANH, UR_DT_BF16,
                   UR_DT_F16, ConvDesc, ConvPlan, check, lib)

BF16 = torch.bfloat16
F16 = torch.float16
_ws = {}

# ---- compute dtype: the 16-bit type activations / weights are stored in and fed to the matrix cores ----------------------
_DTYPES = {"bf16": BF16, "bfloat16": BF16, BF16: BF16, "fp16": F16, "float16": F16, "f16": F16, "16": F16, F16: F16}
_act = BF16


def set_dtype(dt) -> torch.dtype:
    """Select the 16-bit activation / weight type ("bf16" | "fp16") for subsequent ops; returns the torch dtype."""
    global _act
    if dt not in _DTYPES:
        raise ValueError(f"unsupported compute dtype {dt!r}: choose 'bf16' or 'fp16'")
    _act = _DTYPES[dt]
    return _act


def act_dtype() -> torch.dtype:
    return _act


def _dt(t: Optional[torch.Tensor] = None) -> int:
    """UR_DT_* code of tensor `t` (or of the current compute dtype)."""
    d = _act if t is None else t.dtype
    if d == BF16:
        return UR_DT_BF16
    if d == F16:
        return UR_DT_F16
    raise TypeError(f"expected a bf16 / fp16 tensor, got {d}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def workspace(dev, nbytes=192 << 20) -> torch.Tensor:
    """Split-K partial planes: ONE fixed-size buffer per device (every launch of a forward is ordered on one stream).  Allocated
    once and never regrown (captured graphs keep its address); the library falls back to fewer splits when a launch would not fit."""
    key = (dev, "splitk")
    if key not in _ws:
        _ws[key] = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    return _ws[key]


def ln_of(t):
    """Per-row (sum, sum of squares) attached to `t` by its producer GEMM (or None)."""
    return getattr(t, "_ln", None)


def gn_of(t):
    """(partial plane fp32 [N][P][C][2], P) attached to tensor `t` by its producer (or None): its GroupNorm statistics."""
    return getattr(t, "_gn", None)


def carry(src, dst):
    """Propagate the producer's statistics across a reshape / view."""
    g = getattr(src, "_gn", None)
    if g is not None:
        dst._gn = g
    r = getattr(src, "_ln", None)
    if r is not None:
        dst._ln = r
    return dst


def round_up(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ weights
@dataclass
class PackedConv:
    """16-bit [Cout][KH*KW*Cin] weight (K runs tap-major, channel-minor) + fp32 bias, padded for the kernel."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    cin: int          # padded input channels (multiple of 8)
    cout: int         # GEMM N (multiple of 4; for pair activations the interleaved a|g row count)
    cout_out: int     # channels actually produced (cout/2 for pair activations)
    k: int            # kernel size (1 or 3)
    groups: int = 1
    pair: bool = False
    ln_colsum: Optional[torch.Tensor] = None   # LayerNorm-fused GEMM: fp32 [cout] row sums of the folded bf16 weight
    ln_eps: float = 0.0
    kcm: bool = False  # K order (64-ch chunk, tap, ch) instead of (tap, ch): consecutive K tiles re-read the same pixels (L2)
    w_frag: Optional[torch.Tensor] = None      # MFMA-fragment-major copy for the weight-streaming kernel (built on first use)

    def frag(self) -> torch.Tensor:
        """ur_conv_desc.w_frag: [Cout/128][Cin/64][tap][k-step][row block][lane][8] from the chunk-major rows (csrc/conv_wstream.hip)."""
        if self.w_frag is None:
            nt, nc = self.cout // 128, self.cin // 64
            w = self.w.view(nt, 4, 32, nc, 9, 4, 2, 8)                    # [nt][row block][row][chunk][tap][k-step][half][8]
            self.w_frag = w.permute(0, 3, 4, 5, 1, 6, 2, 7).contiguous()  # lane = half * 32 + row
        return self.w_frag

    w_up4: Optional[torch.Tensor] = None       # the four 2x2 phase convs of "nearest-2x upsample, then this 3x3 conv" (built on first use)

    def up4(self, weight: torch.Tensor) -> torch.Tensor:
        """ur_conv_desc.w_up4 from the fp32 master `weight` [Cout, Cin, 3, 3] of these packed weights: folded in fp32, rounded once
        (up4_fold / up4_pack).  Call it once the plan has taken the folded path (ConvPlan.up4): it is a second copy of the weights."""
        if self.w_up4 is None:
            w = weight.detach().to(self.w.device, torch.float32).permute(0, 2, 3, 1)
            if w.shape[0] != self.cout or w.shape[3] != self.cin:              # the padding pack_conv added (zero rows / channels)
                w = torch.nn.functional.pad(w, (0, self.cin - w.shape[3], 0, 0, 0, 0, 0, self.cout - w.shape[0]))
            self.w_up4 = up4_pack(up4_fold(w), self.w.dtype)
        return self.w_up4


def up4_fold(w: torch.Tensor) -> torch.Tensor:
    """w [Cout][3][3][Cin] (fp32 / fp64) -> W4 [py][px][Cout][a][b][Cin]: a nearest-2x upsample followed by the 3x3 conv (pad 1) is,
    for the output pixels of parity (py, px), a 2x2 conv over the source image - the 3x3 window of output row 2y + py covers the
    source rows y - 1 + py + a, a in {0, 1}, and the taps that fall on one source row add up:
    py = 0: {ky 0} -> a 0, {ky 1, 2} -> a 1;  py = 1: {ky 0, 1} -> a 0, {ky 2} -> a 1;  the columns likewise with px."""
    sel = w.new_tensor([[[1, 0, 0], [0, 1, 1]], [[1, 1, 0], [0, 0, 1]]])       # [parity][a][k]
    return torch.einsum("pay,qbx,oyxc->pqoabc", sel, sel, w)


def up4_pack(w4: torch.Tensor, dtype) -> torch.Tensor:
    """W4 [py][px][Cout][a][b][Cin] -> 16-bit [phase = 2 py + px][Cout][4 Cin], K chunk-major like the halo kernels' weights with four
    taps per 64-channel chunk: K tile = chunk * 4 + (2 a + b)."""
    _, _, cout, _, _, cin = w4.shape
    assert cin % 64 == 0
    return w4.to(dtype).reshape(4, cout, 4, cin // 64, 64).permute(0, 1, 3, 2, 4).reshape(4, cout, 4 * cin).contiguous()


def up4_unpack(packed: torch.Tensor, cin: int) -> torch.Tensor:
    """Inverse of up4_pack: [4][Cout][4 Cin] -> [py][px][Cout][a][b][Cin]."""
    cout = packed.shape[1]
    return packed.reshape(2, 2, cout, cin // 64, 2, 2, 64).permute(0, 1, 2, 4, 5, 3, 6).reshape(2, 2, cout, 2, 2, cin)


def wants_up4(pc: "PackedConv", n, h, w_, c1, c2, stride, upsample, groups, pad=(1, 1)) -> bool:
    """The upsampling launches csrc/igemm.hip can run folded (it also checks, and ConvPlan.up4 says what it chose): 3x3, pad 1, one
    source of whole 64-channel chunks, and a source image of whole 8 x 32 patches."""
    return (pc.k == 3 and pc.kcm and groups == 1 and stride == 1 and bool(upsample) and tuple(pad) == (1, 1) and not pc.pair
            and c2 == 0 and c1 % 64 == 0 and w_ % 32 == 0 and h % 8 == 0)


def wants_frag(pc: "PackedConv", n, h, w_, c1, c2, stride, upsample, groups) -> bool:
    """The launches csrc/igemm.hip sends to the weight-streaming kernel (it also checks): 3x3 on 8 x 8 maps of <= 16 images."""
    return (pc.k == 3 and pc.kcm and groups == 1 and stride == 1 and not upsample and h == 8 and w_ == 8 and n <= 16 and not pc.pair
            and pc.cout % 128 == 0 and (c1 + c2) % 256 == 0 and (c1 + c2) >= 512 and (c2 == 0 or c1 % 64 == 0))


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor], dev, *, pair=False, groups=1, cin_pad=None, c1=None, group_halo=False) -> PackedConv:
    """weight: [Cout, Cin/groups, k, k] (nn.Conv2d) or [N, K] (nn.Linear), fp32 master on any device.
    The repack (OIHW -> O,kh,kw,I; zero padding; a|g interleave; bf16 cast) runs on `dev` with torch copies.
    group_halo: a grouped 3x3 conv whose groups are halo-kernel sized (>= 64 channels in, a multiple of 128 out) - chunk-major
    weights, one halo launch per group on its channel slice (csrc/igemm.hip conv_impl)."""
    w = weight.detach().to(dev, torch.float32)
    if w.dim() == 2:
        w = w[:, :, None, None]
    cout, cin_g, kh, kw = w.shape
    assert kh == kw and kh in (1, 3)
    cin_p = cin_pad or round_up(cin_g, 8)
    cout_p = round_up(cout, 8)           # outputs feed the next conv: keep C % 8 == 0 (padded rows are zero)
    if groups > 1:
        assert cin_g % 8 == 0 and (cout // groups) % 4 == 0
    if cin_p == cin_g and cout_p == cout:
        wp = w.permute(0, 2, 3, 1).contiguous()
    else:
        wp = torch.zeros(cout_p, kh, kw, cin_p, dtype=torch.float32, device=dev)
        wp[:cout, :, :, :cin_g] = w.permute(0, 2, 3, 1)
    b = None
    if bias is not None:
        b = torch.zeros(cout_p, dtype=torch.float32, device=dev)
        b[:cout] = bias.detach().to(dev, torch.float32)
    cout_out = cout_p
    if pair:
        half = cout // 2
        if cout % 2 or half % 32:
            raise NotImplementedError(f"UR_E_UNSUPPORTED: pair activations (GEGLU / SimpleGate) need (Cout/2) % 32 == 0, got {half}")
        idx = torch.arange(cout, device=dev).view(2, half // 32, 32).permute(1, 0, 2).reshape(-1)   # [blk][a|g][32]
        wp = wp[idx]
        b = b[idx] if b is not None else None
        cout_out = half
    # chunk-major K for 3x3 kernels: [Cout][kh*kw][Cin/64][64] -> [Cout][Cin/64][kh*kw][64]; c1 = channels of the first
    # source when the input is a virtual concat (chunks must not straddle it)
    # (grouped convs too when every group is chunk-sized: each group then runs the halo kernel on its channel slice)
    kcm = kh == 3 and (groups == 1 or (group_halo and cout_p == cout)) and cin_p % 64 == 0 and (c1 is None or c1 % 64 == 0)
    if kcm:
        wp = wp.reshape(cout_p, kh * kw, cin_p // 64, 64).permute(0, 2, 1, 3)
    return PackedConv(wp.reshape(cout_p, kh * kw * cin_p).to(_act).contiguous(),
                      None if b is None else b.contiguous(), cin_p, cout_p, cout_out, kh, groups, pair, kcm=kcm)


# ------------------------------------------------------------------------------------------------ conv / gemm
def _conv_desc(x, pc: PackedConv, x2, stride, pad, upsample, out_hw, plan_only) -> ConvDesc:
    """ur_conv_desc of `pc` over x (| x2): input and weight pointers, geometry, weight layout, workspace, ldy = dense output.
    The caller adds outputs, epilogue inputs and activation.  plan_only: placeholder pointers (ur_conv2d_plan reads no data)."""
    n, h, w_, c1 = x.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    k, g = pc.k, pc.groups
    if pad is None:
        pad = (k // 2, k // 2)
    if out_hw is None:
        hin, win = (h * 2, w_ * 2) if upsample else (h, w_)
        out_hw = ((hin + 2 * pad[0] - k) // stride + 1, (win + 2 * pad[1] - k) // stride + 1)
    d = ConvDesc()
    d.dtype = _dt(x)
    if plan_only:
        d.x, d.x2, d.w = 16, (16 if c2 else None), 16
    else:
        d.x, d.x2, d.w = _ptr(x), _ptr(x2), _ptr(pc.w)
    ws = workspace(x.device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    d.N, d.H, d.W = n, h, w_
    d.C1, d.ldx, d.C2, d.ldx2 = (c1 // g if g > 1 else c1), c1, c2, c2
    d.Cout, d.ldw, d.ldy = pc.cout // g, pc.w.shape[1], pc.cout_out
    d.KH = d.KW = k
    d.stride, d.pad_t, d.pad_l = stride, pad[0], pad[1]
    d.OH, d.OW = out_hw
    d.upsample2x, d.out_scale = int(upsample), 1.0
    d.k_chunk_major = int(pc.kcm and (c2 == 0 or c1 % 64 == 0))
    if wants_frag(pc, n, h, w_, c1, c2, stride, upsample, g) and pad == (1, 1):
        d.w_frag = 16 if plan_only else pc.frag().data_ptr()
    d.nbatch = g
    if g > 1:
        d.bs_x, d.bs_w, d.bs_bias, d.bs_y, d.bs_r = c1 // g, (pc.cout // g) * pc.w.shape[1], pc.cout // g, pc.cout_out // g, pc.cout_out // g
    return d


def conv(x: torch.Tensor, pc: PackedConv, *, x2=None, residual=None, bias=None, act=UR_ACT_NONE, stride=1, pad=None,
         out_hw=None, upsample=False, out_f32=False, out_scale=1.0, out=None, yt=None, n_split=0, t_rows=0,
         gn=False, store=True, rows=False, ln_stats=None, gn_ab=None, gn_silu=False, up4=None):
    """x: [N,H,W,C1] 16-bit (x2 optional [N,H,W,C2], virtual concat).  Returns [N,OH,OW,cout_out].
    gn=True: the consumer of the output is a GroupNorm / InstanceNorm / global average pool - leave its partial statistics
    (out._gn); store=False (with gn): only the statistics are wanted, the output tensor is not written (returns the plane).
    rows=True: leave per-row sums for a LayerNorm-folded consumer GEMM (out._ln).
    gn_ab / gn_silu: read act(a*x+b) instead of x (GroupNorm apply fused into the loader; only where conv_plan says so).
    up4 (with upsample): pc.up4(...) - the folded weights of the four 2x2 phase convs; taken where conv_plan(..., up4=True).up4."""
    if x.dtype not in (BF16, F16) or x.dtype != pc.w.dtype or not x.is_contiguous() or x.dim() != 4:
        raise ValueError(f"conv: x must be a contiguous 4-d {pc.w.dtype} tensor, got {x.dtype} {tuple(x.shape)}")
    n, h, w_, c1 = x.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    if (c1 + c2) != pc.cin * pc.groups:
        raise ValueError(f"conv: Cin mismatch: {c1}+{c2} vs {pc.cin}*{pc.groups}")
    d = _conv_desc(x, pc, x2, stride, pad, upsample, out_hw, plan_only=False)
    assert not pc.kcm or d.k_chunk_major, "chunk-major weights need a 64-aligned concat boundary"
    oh, ow = d.OH, d.OW
    co_total = pc.cout_out
    if out is None and store:
        out = torch.empty((n, oh, ow, co_total), dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    bias_t = pc.bias if bias is None else bias          # override: per-step (time-embedding) or per-image bias rows
    d.bias = _ptr(bias_t)
    if bias is not None and bias.dim() == 2 and bias.shape[0] > 1:
        d.bias_img_stride = bias.shape[1]
    d.residual, d.y, d.yt = _ptr(residual), _ptr(out), _ptr(yt)
    if ln_stats is not None:
        assert pc.ln_colsum is not None, "weights were not packed with pack_linear_ln"
        st, parts = ln_stats
        d.ln_stats, d.ln_colsum, d.ln_eps, d.ln_dim, d.ln_parts = st.data_ptr(), pc.ln_colsum.data_ptr(), pc.ln_eps, pc.cin, parts
    if gn_ab is not None:
        d.gn_ab, d.gn_silu = gn_ab.data_ptr(), int(gn_silu)
    if up4 is not None:
        d.w_up4 = up4.data_ptr()
    if out is not None:
        d.ldy = out.shape[-1]
    d.ldr = residual.shape[-1] if residual is not None else 0
    d.act, d.out_f32, d.out_scale = act, int(out_f32), out_scale
    d.n_split, d.t_rows = n_split, t_rows
    d.t_ld = yt.shape[-1] if yt is not None else 0
    stats = rstats = None
    if gn or rows:      # the consumer is a norm: plan the launch, then hand it the planes to fill (plain stores, no atomics)
        if gn:
            d.gn_part = 16      # dummy non-null values: the plan must see what the real launch will see
        if rows:
            d.row_stats = 16
        plan = ConvPlan()
        check(lib.ur_conv2d_plan(d, plan))
        if gn:
            if not store and not plan.gn_fused:
                raise NotImplementedError("store=False needs a launch whose epilogue writes the statistics (conv_plan().gn_fused)")
            stats = (torch.empty((n, plan.gn_parts, co_total, 2), dtype=torch.float32, device=x.device), plan.gn_parts)
            d.gn_part = stats[0].data_ptr()
        if rows:
            rstats = (torch.empty((plan.row_stat_parts, n * oh * ow, 2), dtype=torch.float32, device=x.device), plan.row_stat_parts)
            d.row_stats = rstats[0].data_ptr()
    check(lib.ur_conv2d_nhwc(d, _stream()))
    if not store:
        return stats
    if stats is not None:
        out._gn = stats
    if rstats is not None:
        out._ln = rstats
    return out


def conv_plan(x: torch.Tensor, pc: PackedConv, *, x2=None, stride=1, pad=None, upsample=False, gn=False, gn_ab=False, up4=False,
              act=UR_ACT_NONE, residual=False, store=True) -> ConvPlan:
    """What `conv` would do for this (shape, weights) - used to decide whether the GroupNorm apply can ride in the conv."""
    d = _conv_desc(x, pc, x2, stride, pad, upsample, None, plan_only=True)
    d.y = 16 if store else None
    d.residual = 16 if residual else None
    d.gn_part = 16 if gn else None
    d.gn_ab = 16 if gn_ab else None
    d.w_up4 = 16 if up4 else None
    d.ldr = pc.cout_out if residual else 0
    d.act = act
    plan = ConvPlan()
    check(lib.ur_conv2d_plan(d, plan))
    return plan


def conv_launch(x: torch.Tensor, pc: PackedConv, *, x2=None, stride=1, pad=None, upsample=False, gn=False, gn_ab=False, up4=False,
                act=UR_ACT_NONE, residual=False, store=True):
    """Which launcher `conv` would run for this (shape, weights), and its split (capi.ConvLaunchInfo; name: capi.launcher_names())."""
    d = _conv_desc(x, pc, x2, stride, pad, upsample, None, plan_only=True)
    d.y = 16 if store else None
    d.residual = 16 if residual else None
    d.gn_part = 16 if gn else None
    d.gn_ab = 16 if gn_ab else None
    d.w_up4 = 16 if up4 else None
    d.ldr = pc.cout_out if residual else 0
    d.act = act
    return capi.plan_launch(d)


def pack_linear_ln(weight, bias, gamma, beta, eps, dev, *, pair=False) -> PackedConv:
    """Linear(LayerNorm(x)) folded for the LN-fused GEMM epilogue: w' = W*gamma (bf16), bias' = W.beta + b,
    ln_colsum[n] = sum_k bf16(w'[n,k]).  The kernel computes rstd*(w'.x - mean*ln_colsum) + bias'."""
    w = weight.detach().to(dev, torch.float32)
    g, b0 = gamma.detach().to(dev, torch.float32), beta.detach().to(dev, torch.float32)
    wf = w * g[None, :]
    t = w @ b0 + (bias.detach().to(dev, torch.float32) if bias is not None else 0.0)
    pc = pack_conv(wf, t, dev, pair=pair)
    pc.ln_colsum = pc.w.float().sum(dim=1).contiguous()          # of the ROUNDED weights, in packed (possibly a|g interleaved) row order
    pc.ln_eps = float(eps)
    return pc


def linear(x: torch.Tensor, pc: PackedConv, **kw):
    """x: [..., K] bf16 -> [..., N]; runs as a 1x1 conv over a [1,1,rows,K] image."""
    shp = x.shape
    rows = x.numel() // shp[-1]
    res = kw.pop("residual", None)
    if res is not None:
        res = res.reshape(1, 1, rows, res.shape[-1])
    gn = kw.pop("gn", False)
    gn_hw = kw.pop("gn_hw", None)       # (N, HW): how the rows split into images for the fused GroupNorm sums
    if kw.get("ln_stats") is None and getattr(pc, "ln_colsum", None) is not None:
        raise ValueError("LayerNorm-folded weights need ln_stats")
    if gn:
        n_img, hw = gn_hw
        y = conv(x.reshape(n_img, 1, hw, shp[-1]), pc, residual=None if res is None else res.reshape(n_img, 1, hw, -1), gn=True, **kw)
    else:
        y = conv(x.reshape(1, 1, rows, shp[-1]), pc, residual=res, **kw)
    return None if y is None else carry(y, y.reshape(*shp[:-1], y.shape[-1]))


def bmm_nt(a: torch.Tensor, bmat: torch.Tensor, *, out_f32=False, out_scale=1.0):
    """Batched C[b] = A[b] @ B[b]^T with A:[B,M,K], B:[B,N,K] bf16 (last dim contiguous; row strides free)."""
    B, M, K = a.shape
    N = bmat.shape[1]
    if a.dtype != bmat.dtype or a.dtype not in (BF16, F16):
        raise ValueError(f"bmm_nt: both operands must share one 16-bit type, got {a.dtype} and {bmat.dtype}")
    assert a.stride(2) == 1 and bmat.stride(2) == 1 and K % 8 == 0 and N % 4 == 0
    out = torch.empty((B, M, N), dtype=torch.float32 if out_f32 else a.dtype, device=a.device)
    d = ConvDesc()
    d.dtype = _dt(a)
    d.x, d.w, d.y = a.data_ptr(), bmat.data_ptr(), out.data_ptr()
    ws = workspace(a.device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    d.N, d.H, d.W, d.C1, d.ldx, d.Cout, d.ldw, d.ldy = 1, 1, M, K, a.stride(1), N, bmat.stride(1), N
    d.KH = d.KW = 1
    d.stride, d.OH, d.OW, d.out_f32, d.out_scale, d.nbatch = 1, 1, M, int(out_f32), out_scale, B
    d.bs_x, d.bs_w, d.bs_y = a.stride(0), bmat.stride(0), M * N
    check(lib.ur_conv2d_nhwc(d, _stream()))
    return out


# ------------------------------------------------------------------------------------------------ norms
def gn_partials(x: torch.Tensor):
    """(plane, P) of x: the producer's, or from a statistics pass over x (deterministic partial planes, no atomics)."""
    pre = gn_of(x)
    if pre is not None:
        return pre
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    parts = lib.ur_groupnorm_stats_parts(n, hw, c)
    if parts <= 0:
        check(parts if parts < 0 else -1)
    plane = torch.empty((n, parts, c, 2), dtype=torch.float32, device=x.device)
    check(lib.ur_groupnorm_stats(x.data_ptr(), plane.data_ptr(), n, hw, c, _dt(x), _stream()))
    return plane, parts


def gn_finalize(x: torch.Tensor, gamma, beta, groups: int, eps: float, x2=None, use_pre=True, want_mean=False):
    """GroupNorm statistics of x (| x2, virtually concatenated) -> fp32 ab [N][2][C] with GroupNorm(x) = a*x + b
    (want_mean: the [N][groups] group means instead)."""
    n, c1 = x.shape[0], x.shape[-1]
    c2 = 0 if x2 is None else x2.shape[-1]
    hw = x.numel() // (n * c1)
    if not use_pre:
        x = x.view(x.shape)          # fresh tensor object: no producer attributes
        x2 = None if x2 is None else x2.view(x2.shape)
    p1, n1 = gn_partials(x)
    p2, n2 = gn_partials(x2) if x2 is not None else (None, 0)
    out = torch.empty((n, groups) if want_mean else (n, 2, c1 + c2), dtype=torch.float32, device=x.device)
    check(lib.ur_groupnorm_finalize(p1.data_ptr(), n1, c1, _ptr(p2), n2, c2, _ptr(gamma), _ptr(beta), n, hw, groups, eps,
                                    None if want_mean else out.data_ptr(), out.data_ptr() if want_mean else None, _stream()))
    return out


def gn_finalize_planes(plane: torch.Tensor, parts: int, hw: int):
    """Channel means [N][C] straight from a partial plane [N][P][C][2] (statistics-only conv launch)."""
    n, c = plane.shape[0], plane.shape[2]
    out = torch.empty((n, c), dtype=torch.float32, device=plane.device)
    check(lib.ur_groupnorm_finalize(plane.data_ptr(), parts, c, None, 0, 0, None, None, n, hw, c, 0.0, None, out.data_ptr(), _stream()))
    return out


def gn_apply(x: torch.Tensor, ab: torch.Tensor, silu=False, x2=None):
    n, c1 = x.shape[0], x.shape[-1]
    c2 = 0 if x2 is None else x2.shape[-1]
    hw = x.numel() // (n * c1)
    out = torch.empty((*x.shape[:-1], c1 + c2), dtype=x.dtype, device=x.device)
    check(lib.ur_groupnorm_apply_act(x.data_ptr(), _ptr(x2), out.data_ptr(), ab.data_ptr(), n, hw, c1, c2, int(silu), _dt(x), _stream()))
    return out


def group_norm(x: torch.Tensor, gamma, beta, groups: int, eps: float, silu=False, x2=None, use_pre=True):
    """x: [N,H,W,C1] 16-bit (+ optional x2 [N,H,W,C2], normalised as one concatenated tensor) -> [N,H,W,C1+C2].
    gamma/beta fp32 [C] or None (InstanceNorm when groups == C)."""
    assert x.dtype in (BF16, F16) and x.is_contiguous()
    return gn_apply(x, gn_finalize(x, gamma, beta, groups, eps, x2=x2, use_pre=use_pre), silu, x2=x2)


def layer_norm(x: torch.Tensor, gamma, beta, eps: float):
    assert x.dtype in (BF16, F16) and x.is_contiguous()
    c = x.shape[-1]
    out = torch.empty_like(x)
    check(lib.ur_layernorm_rows(x.data_ptr(), out.data_ptr(), _ptr(gamma), _ptr(beta), x.numel() // c, c, eps, _dt(x), _stream()))
    return out


def softmax_rows(s: torch.Tensor, ldp=None):
    """s: [..., cols] fp32 -> 16-bit probabilities [..., ldp] (columns >= cols are zero)."""
    cols = s.shape[-1]
    ldp = ldp or round_up(cols, 8)
    p = torch.empty((*s.shape[:-1], ldp), dtype=_act, device=s.device)
    check(lib.ur_softmax_rows_f32(s.data_ptr(), p.data_ptr(), s.numel() // cols, cols, ldp, _dt(), _stream()))
    return p


# ------------------------------------------------------------------------------------------------ attention
def attention(q, k, vt, heads: int, head_dim: int, tq: int, tk: int, scale: float, *, ldq, ldk, bs_q, bs_k, bs_vt,
              batch: int, out=None):
    """q:[B,Tq,ldq] k:[B?,Tk,ldk] vt:[B?,H*D,ldvt] (raw tensors; strides given explicitly) -> o [B,Tq,H*D]."""
    c = heads * head_dim
    if not (q.dtype == k.dtype == vt.dtype) or q.dtype not in (BF16, F16):
        raise ValueError(f"attention: q, k, v^T must share one 16-bit type, got {q.dtype}, {k.dtype}, {vt.dtype}")
    out = torch.empty((batch, tq, c), dtype=q.dtype, device=q.device) if out is None else out
    nws = lib.ur_attention_workspace_bytes(batch, heads, tq, tk, head_dim)       # key-split last round of the d = 64 kernel (0: none)
    ws = torch.empty(nws, dtype=torch.uint8, device=q.device) if nws else None
    check(lib.ur_attention_fwd_ws(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), batch, heads, tq, tk, head_dim,
                                  ldq, ldk, vt.shape[-1], c, bs_q, bs_k, bs_vt, tq * c, scale, _ptr(ws), nws, _dt(q), _stream()))
    return out


# ------------------------------------------------------------------------------------------------ misc
def dwconv3x3(x, w9c, bias, gate=False):
    n, h, w_, c = x.shape
    out = torch.empty((n, h, w_, c // 2 if gate else c), dtype=x.dtype, device=x.device)
    check(lib.ur_dwconv3x3_nhwc(x.data_ptr(), w9c.data_ptr(), bias.data_ptr(), out.data_ptr(), n, h, w_, c, int(gate), _dt(x), _stream()))
    return out


def avgpool(x):
    """Mean over HW -> fp32 [N][C]: a finalize over the tensor's (producer-side or freshly computed) partial sums."""
    return gn_finalize(x, None, None, x.shape[-1], 0.0, want_mean=True)


def scale_channels(x, s, residual=None):
    n, c = x.shape[0], x.shape[-1]
    out = torch.empty_like(x)
    check(lib.ur_scale_channels(x.data_ptr(), s.data_ptr(), _ptr(residual), out.data_ptr(), n, x.numel() // (n * c), c, _dt(x), _stream()))
    return out


FANOUT_MAX_K = 8


def scale_channels_fanout(x, s, k):
    """Task fan-out of `scale_channels`: x [B,...,C] shared by k tasks, s fp32 [k*B, C] (or None: k copies of x) ->
    [k*B,...,C], task-major (task j's image b is row j*B + b).  x is read once."""
    b, c = x.shape[0], x.shape[-1]
    if s is not None and (s.dtype != torch.float32 or tuple(s.shape) != (k * b, c) or not s.is_contiguous()):
        raise ValueError(f"scale_channels_fanout: s must be a contiguous fp32 [{k * b}, {c}] tensor, got {s.dtype} {tuple(s.shape)}")
    if not x.is_contiguous():
        raise ValueError("scale_channels_fanout: x must be contiguous")
    out = torch.empty((k * b, *x.shape[1:]), dtype=x.dtype, device=x.device)
    for k0 in range(0, k, FANOUT_MAX_K):                   # the kernel keeps up to 8 results per thread in flight
        check(lib.ur_scale_channels_fanout(x.data_ptr(), None if s is None else s[k0 * b:].data_ptr(), out[k0 * b:].data_ptr(), b,
                                           min(FANOUT_MAX_K, k - k0), x.numel() // (b * c), c, _dt(x), _stream()))
    return out


def spade_modulate(n, gb, residual=None):
    """y = n * (1 + gamma) + beta (+ residual); gb [..., 2C] = gamma | beta (spade.py:69)."""
    c = n.shape[-1]
    out = torch.empty_like(n)
    check(lib.ur_spade_modulate(n.data_ptr(), gb.data_ptr(), gb.shape[-1], _ptr(residual), out.data_ptr(), n.numel() // c, c, _dt(n), _stream()))
    return out


def axpy_channels(a, b, s):
    c = a.shape[-1]
    out = torch.empty_like(a)
    check(lib.ur_axpy_channels(a.data_ptr(), b.data_ptr(), s.data_ptr(), out.data_ptr(), a.numel() // c, c, _dt(a), _stream()))
    return out


def linear_f32(x, w, bias, act=UR_ACT_NONE, groups=1):
    """x [M,K] fp32, w [N,K/groups] fp32 -> [M,N] fp32."""
    m, k = x.shape
    n = w.shape[0]
    out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    check(lib.ur_linear_f32(x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), m, n, k, groups, act, _stream()))
    return out


def tfa_prompt_update(pooled, cond):
    b, t, d = cond.shape
    upd = torch.empty_like(cond)
    check(lib.ur_tfa_prompt_update(pooled.data_ptr(), cond.data_ptr(), upd.data_ptr(), b, t, d, _stream()))
    return upd


def tfa_prompt_update_fanout(pooled, cond, b, k, cond_per_row):
    """Task fan-out of `tfa_prompt_update`: pooled fp32 [b,3,T*D] shared by k tasks; cond fp32 [k,T,D] (one prompt per task,
    cond_per_row=False) or [k*b,T,D] (cond_per_row=True) -> upd [k*b,T,D], row j*b + i from pooled row i."""
    rows, t, d = cond.shape
    if rows != (k * b if cond_per_row else k) or pooled.shape[0] != b or pooled.numel() != b * 3 * t * d:
        raise ValueError(f"tfa_prompt_update_fanout: pooled {tuple(pooled.shape)} / cond {tuple(cond.shape)} do not fit b={b}, k={k}")
    if not (pooled.is_contiguous() and cond.is_contiguous() and pooled.dtype == cond.dtype == torch.float32):
        raise ValueError("tfa_prompt_update_fanout: pooled and cond must be contiguous fp32 tensors")
    upd = torch.empty((k * b, t, d), dtype=torch.float32, device=cond.device)
    check(lib.ur_tfa_prompt_update_fanout(pooled.data_ptr(), cond.data_ptr(), upd.data_ptr(), b, k, t, d, int(bool(cond_per_row)), _stream()))
    return upd


def vec_mul_group(a, b, groups):
    out = torch.empty_like(a)
    check(lib.ur_vec_mul_group(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.shape[0], a.shape[1], groups, _stream()))
    return out


def nchw_to_nhwc(x: torch.Tensor, cpad=None, image=False):
    """fp32 NCHW -> 16-bit NHWC (channels zero-padded to a multiple of 8); image=True applies x*2-1."""
    x = x.contiguous().float()
    n, c, h, w_ = x.shape
    cpad = cpad or round_up(c, 8)
    out = torch.empty((n, h, w_, cpad), dtype=_act, device=x.device)
    fn = lib.ur_image_to_nhwc if image else lib.ur_nchw_f32_to_nhwc
    check(fn(x.data_ptr(), out.data_ptr(), n, c, h, w_, cpad, _dt(), _stream()))
    return out


def image_resize_pad(img: torch.Tensor, rh: int, rw: int, ph: int, pw: int, mul=2.0, add=-1.0, cpad=None):
    """DiffUIE.forward pre-processing (unifie.py:124-134) + x*2-1 + layout: fp32 NCHW -> bf16 NHWC [N, rh+ph, rw+pw, cpad]."""
    img = img.contiguous().float()
    n, c, h, w_ = img.shape
    cpad = cpad or round_up(c, 8)
    out = torch.empty((n, rh + ph, rw + pw, cpad), dtype=_act, device=img.device)
    check(lib.ur_image_resize_pad_nhwc(img.data_ptr(), out.data_ptr(), n, c, h, w_, rh, rw, ph, pw, cpad, mul, add, _dt(), _stream()))
    return out


def image_unpad_resize(x: torch.Tensor, c: int, crop_hw, out_hw, mul=1.0, add=0.0, quantize=False):
    """Post-processing (unifie.py:164-168 [+ eval_image_restoration.py:71 when quantize]): NHWC -> crop -> bicubic -> fp32 NCHW."""
    n, xh, xw, ld = x.shape
    out = torch.empty((n, c, out_hw[0], out_hw[1]), dtype=torch.float32, device=x.device)
    check(lib.ur_image_unpad_resize_nchw(x.data_ptr(), int(x.dtype == torch.float32), out.data_ptr(), n, c, xh, xw, ld, crop_hw[0],
                                         crop_hw[1], out_hw[0], out_hw[1], mul, add, int(quantize), _dt() if x.dtype == torch.float32 else _dt(x), _stream()))
    return out


def ragged_geometry(sizes, canvas):
    """Host int32 [N,4] table (H, W, RH, RW) of a ragged 8-bit batch from [(H, W, RH, RW), ...] and the canvas (CH, CW); ValueError
    for a row that does not fit the canvas (the kernels never follow such a row, they cannot report which)."""
    ch, cw = int(canvas[0]), int(canvas[1])
    rows = []
    for n, row in enumerate(sizes):
        h, w, rh, rw = (int(v) for v in row)
        if not (0 < h <= rh <= ch and 0 < w <= rw <= cw and ch - rh < rh and cw - rw < rw):
            raise ValueError(f"ragged geometry: image {n} (H, W, RH, RW) = {(h, w, rh, rw)} does not fit the canvas {(ch, cw)}: "
                             "needs H <= RH <= CH, W <= RW <= CW and a reflect padding smaller than the resized image")
        rows.append((h, w, rh, rw))
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)


def _check_ragged(name, slots, geom, n, canvas, validate):
    dev = torch.device("cuda", torch.cuda.current_device())
    ch, cw = int(canvas[0]), int(canvas[1])
    if not isinstance(slots, torch.Tensor) or slots.dtype != torch.uint8 or slots.ndim != 2 or slots.shape[0] != n or n == 0:
        raise ValueError(f"{name}: the slot buffer must be a uint8 tensor [N = {n}, slot_bytes], got "
                         f"{getattr(slots, 'dtype', type(slots))} {tuple(getattr(slots, 'shape', ()))}")
    if slots.shape[1] < ch * cw * 3:
        raise ValueError(f"{name}: slot_bytes = {slots.shape[1]} is smaller than a canvas-sized image ({ch} * {cw} * 3)")
    if not isinstance(geom, torch.Tensor) or geom.dtype != torch.int32 or tuple(geom.shape) != (n, 4):
        raise ValueError(f"{name}: geom must be an int32 tensor [N = {n}, 4] of (H, W, RH, RW), got "
                         f"{getattr(geom, 'dtype', type(geom))} {tuple(getattr(geom, 'shape', ()))}")
    for what, t in (("slot buffer", slots), ("geom", geom)):
        if t.device != dev:
            raise ValueError(f"{name}: the {what} is on {t.device}, not on the current device {dev}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: the {what} must be contiguous")
    if validate:
        ragged_geometry(geom.tolist(), canvas)


def image_u8_ingest(slots: torch.Tensor, geom: torch.Tensor, canvas, mul=2.0, add=-1.0, cpad=8, validate=True):
    """Ragged 8-bit batch -> 16-bit NHWC [N, CH, CW, cpad]: per image u8 / 255, then what `image_resize_pad` does.  slots uint8
    [N, slot_bytes] (image n dense HWC at the start of row n), geom device int32 [N,4] (H, W, RH, RW), canvas (CH, CW).
    validate reads the table back (a sync) and raises for a row that does not fit; a caller that built the table with
    `ragged_geometry` - or runs inside a graph capture, where a read-back is impossible - passes validate=False."""
    n = int(slots.shape[0]) if isinstance(slots, torch.Tensor) and slots.ndim == 2 else 0
    _check_ragged("image_u8_ingest", slots, geom, n, canvas, validate)
    out = torch.empty((n, int(canvas[0]), int(canvas[1]), cpad), dtype=_act, device=slots.device)
    check(lib.ur_image_u8_ingest(slots.data_ptr(), slots.shape[1], geom.data_ptr(), out.data_ptr(), n, int(canvas[0]), int(canvas[1]),
                                 cpad, mul, add, _dt(), _stream()))
    return out


def image_u8_egress(x: torch.Tensor, c: int, geom: torch.Tensor, mul=1.0, add=0.0, out=None, nonfinite=None, validate=True):
    """x NHWC (16-bit | fp32) [N, CH, CW, ld] -> ragged 8-bit batch: per image what `image_unpad_resize(..., quantize=True)` does,
    stored as uint8 code values, HWC.  Returns (slots uint8 [N, CH*CW*c], nonfinite int32 [N]): flag n is 1 when image n met a
    non-finite sample (stored as code 0).  `out` / `nonfinite` are written in place when given (nonfinite must come zeroed)."""
    if not isinstance(x, torch.Tensor) or x.ndim != 4 or x.dtype not in (torch.float32, BF16, F16) or not x.is_contiguous():
        raise ValueError(f"image_u8_egress: x must be a contiguous 4-d NHWC tensor (fp32 or 16-bit), got "
                         f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    n, xh, xw, ld = x.shape
    if c != 3 or ld < c:
        raise ValueError(f"image_u8_egress: c must be 3 (RGB) and at most ld = {ld}, got {c}")
    if out is None:
        out = torch.empty((n, xh * xw * c), dtype=torch.uint8, device=x.device)
    _check_ragged("image_u8_egress", out, geom, n, (xh, xw), validate)
    if nonfinite is None:
        nonfinite = torch.zeros(n, dtype=torch.int32, device=x.device)
    elif nonfinite.dtype != torch.int32 or tuple(nonfinite.shape) != (n,) or nonfinite.device != x.device or not nonfinite.is_contiguous():
        raise ValueError(f"image_u8_egress: nonfinite must be a contiguous int32 tensor [{n}] on {x.device}")
    check(lib.ur_image_u8_egress(x.data_ptr(), int(x.dtype == torch.float32), out.data_ptr(), out.shape[1], geom.data_ptr(),
                                 nonfinite.data_ptr(), n, c, xh, xw, ld, mul, add, _dt() if x.dtype == torch.float32 else _dt(x),
                                 _stream()))
    return out, nonfinite


COLOR_FIX_MODES = ("wavelet", "adain")


def check_color_fix_mode(mode):
    """None (off) or one of COLOR_FIX_MODES -> the mode; ValueError for anything else."""
    if mode is not None and mode not in COLOR_FIX_MODES:
        raise ValueError(f"color fix mode must be None, 'wavelet' or 'adain', got {mode!r}")
    return mode


def color_fix(c: torch.Tensor, src: torch.Tensor, mode: str, src_n=None):
    """Colour correction of restored images against the images the encoder saw, in the decoder's domain (about [-1, 1]):
    c fp32 NHWC [N, H, W, ld_c] (the conv_out output), src 16-bit NHWC [>= src_n, H, W, ld_s] (x0), image n is corrected against
    source n % src_n (src_n defaults to src.shape[0] and must divide N).  mode "wavelet": c + L(src - c), the restored detail on the
    source's level-5 a-trous low band; "adain": c's per-channel mean / standard deviation replaced by the source's.
    -> fp32 NHWC [N, H, W, ld_c], RGB in channels 0..2 and zeros behind them."""
    if mode not in COLOR_FIX_MODES:
        raise ValueError(f"color_fix: mode must be 'wavelet' or 'adain', got {mode!r}")
    if not isinstance(c, torch.Tensor) or c.ndim != 4 or c.dtype != torch.float32 or not c.is_contiguous():
        raise ValueError(f"color_fix: c must be a contiguous 4-d fp32 NHWC tensor, got {getattr(c, 'dtype', type(c))} "
                         f"{tuple(getattr(c, 'shape', ()))}")
    if not isinstance(src, torch.Tensor) or src.ndim != 4 or src.dtype not in (BF16, F16) or not src.is_contiguous():
        raise ValueError(f"color_fix: src must be a contiguous 4-d 16-bit NHWC tensor, got {getattr(src, 'dtype', type(src))} "
                         f"{tuple(getattr(src, 'shape', ()))}")
    dev = torch.device("cuda", torch.cuda.current_device())
    for name, t in (("c", c), ("src", src)):
        if t.device != dev:
            raise ValueError(f"color_fix: {name} is on {t.device}, not on the current device {dev}")
    n, h, w_, ld_c = c.shape
    src_n = int(src.shape[0] if src_n is None else src_n)
    if tuple(src.shape[1:3]) != (h, w_):
        raise ValueError(f"color_fix: c is {h} x {w_} but src is {src.shape[1]} x {src.shape[2]}: both live on one canvas")
    if not 1 <= src_n <= src.shape[0] or n % src_n:
        raise ValueError(f"color_fix: src_n = {src_n} must be in [1, {src.shape[0]}] and divide N = {n}")
    if ld_c < 3 or src.shape[3] < 3:
        raise ValueError(f"color_fix: both tensors need at least 3 channels (RGB), got ld_c = {ld_c}, ld_s = {src.shape[3]}")
    if n == 0 or h == 0 or w_ == 0:
        raise ValueError(f"color_fix: empty tensor {tuple(c.shape)}")
    out = torch.empty_like(c)
    if mode == "wavelet":
        check(lib.ur_color_fix_wavelet(c.data_ptr(), ld_c, src.data_ptr(), src.shape[3], out.data_ptr(), n, src_n, h, w_, _dt(src), _stream()))
    else:
        if h * w_ < 2:
            raise ValueError("color_fix: adain needs at least 2 pixels per image (unbiased variance)")
        ws_bytes = lib.ur_color_fix_adain_ws_bytes(n, h, w_)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
        check(lib.ur_color_fix_adain(c.data_ptr(), ld_c, src.data_ptr(), src.shape[3], out.data_ptr(), n, src_n, h, w_, _dt(src),
                                     ws.data_ptr(), ws_bytes, _stream()))
    return out


def nhwc_to_nchw(x: torch.Tensor, c=None, mul=1.0, add=0.0):
    n, h, w_, ld = x.shape
    c = c or ld
    out = torch.empty((n, c, h, w_), dtype=torch.float32, device=x.device)
    check(lib.ur_nhwc_to_nchw_f32(x.data_ptr(), int(x.dtype == torch.float32), out.data_ptr(), n, c, h, w_, ld, mul, add,
                                  _dt() if x.dtype == torch.float32 else _dt(x), _stream()))
    return out


def vae_sample(moments_f32, noise_nchw, clat, scale):
    n, h, w_, ld = moments_f32.shape
    z = torch.empty((n, h, w_, 8), dtype=torch.float32, device=moments_f32.device)
    zb = torch.empty((n, h, w_, 8), dtype=_act, device=moments_f32.device)
    check(lib.ur_vae_sample(moments_f32.data_ptr(), ld, noise_nchw.data_ptr(), z.data_ptr(), zb.data_ptr(), n, h * w_, clat, 8,
                            scale, _dt(), _stream()))
    return z, zb


def add_noise(z0, noise_nchw, clat, sa, sb):
    n, h, w_, cp = z0.shape
    zt, zb = torch.empty_like(z0), torch.empty(z0.shape, dtype=_act, device=z0.device)
    check(lib.ur_add_noise(z0.data_ptr(), noise_nchw.data_ptr(), zt.data_ptr(), zb.data_ptr(), n, h * w_, clat, cp, sa, sb, _dt(), _stream()))
    return zt, zb


def noise_keys(seeds):
    """Per-image seeds (ints in [0, 2^64)) -> the host int32 [N,2] key table of `keyed_noise`: row n holds (seed_n & 0xffffffff,
    seed_n >> 32) as two's-complement words.  ValueError for an empty sequence, a non-integer or a seed outside the range."""
    rows = []
    for n, sd in enumerate(seeds):
        if isinstance(sd, bool) or not hasattr(sd, "__index__"):
            raise ValueError(f"noise_keys: seed {n} must be an integer, got {sd!r}")
        sd = sd.__index__()
        if not 0 <= sd < 1 << 64:
            raise ValueError(f"noise_keys: seed {n} = {sd} is outside [0, 2^64)")
        rows.append([w - (1 << 32) if w >= 1 << 31 else w for w in (sd & 0xffffffff, sd >> 32)])
    if not rows:
        raise ValueError("noise_keys: needs at least one seed")
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 2)


NOISE_KINDS = {"normal": (0, torch.float32), "bits": (1, torch.int32)}


def keyed_noise(keys_dev: torch.Tensor, draw: int, shape, kind="normal", out=None):
    """Counter-based noise keyed per image (Philox4x32-10, csrc/noise.hip; the specification is ur_keyed_noise's comment in the
    header): keys_dev device int32 / uint32 [N,2] (`noise_keys(seeds)` on the device), draw 0 (the VAE posterior draw) or 1 (the
    t=999 draw) or any other uint32, shape = (C, H, W) -> [N,C,H,W] on the device: fp32 standard normals for kind "normal", int32
    holding the raw words for "bits".  Image n's values depend on (key n, draw, element) only - not on N or on n.  The keys are
    read by the kernel, so a captured launch follows later changes of the table.  out: a contiguous tensor of the result's
    dtype and element count to write instead of a new one (4-byte aligned; any offset)."""
    if kind not in NOISE_KINDS:
        raise ValueError(f"keyed_noise: kind must be 'normal' or 'bits', got {kind!r}")
    code, dtype = NOISE_KINDS[kind]
    if not isinstance(keys_dev, torch.Tensor) or keys_dev.dtype not in (torch.int32, torch.uint32) or keys_dev.ndim != 2 or \
            keys_dev.shape[1] != 2 or keys_dev.shape[0] == 0 or not keys_dev.is_contiguous():
        raise ValueError(f"keyed_noise: keys must be a contiguous int32 / uint32 tensor [N, 2], got "
                         f"{getattr(keys_dev, 'dtype', type(keys_dev))} {tuple(getattr(keys_dev, 'shape', ()))}")
    dev = torch.device("cuda", torch.cuda.current_device())
    if keys_dev.device != dev:
        raise ValueError(f"keyed_noise: the keys are on {keys_dev.device}, not on the current device {dev}")
    if len(shape) != 3 or any(int(v) < 1 for v in shape):
        raise ValueError(f"keyed_noise: shape must be (C, H, W) with positive extents, got {tuple(shape)}")
    if not 0 <= int(draw) < 1 << 32:
        raise ValueError(f"keyed_noise: draw = {draw} is outside [0, 2^32)")
    n, (c, h, w_) = keys_dev.shape[0], (int(v) for v in shape)
    if out is None:
        out = torch.empty((n, c, h, w_), dtype=dtype, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != dtype or out.numel() != n * c * h * w_ or out.device != dev or \
            not out.is_contiguous():
        raise ValueError(f"keyed_noise: out must be a contiguous {dtype} tensor of {n * c * h * w_} elements on {dev}")
    check(lib.ur_keyed_noise(keys_dev.data_ptr(), int(draw), out.data_ptr(), n, c * h * w_, code, _stream()))
    return out.view(n, c, h, w_)


# ---- corruptions of u8 images (csrc/corrupt.hip; the specification is the ur_corrupt_* comment in the header; the planner that
# builds the tables is unirestore_amd.corrupt) ----------------------------------------------------------------------------------
def check_u8_images(who: str, x, min_side: int = 32):
    """x must be a contiguous uint8 [N, H, W, 3] tensor on the current device with N >= 1 and H, W >= min_side."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.ndim != 4 or x.shape[3] != 3 or not x.is_contiguous():
        raise ValueError(f"{who}: images must be a contiguous uint8 tensor [N, H, W, 3], got {getattr(x, 'dtype', type(x))} "
                         f"{tuple(getattr(x, 'shape', ()))}")
    dev = torch.device("cuda", torch.cuda.current_device())
    if x.device != dev:
        raise ValueError(f"{who}: the images are on {x.device}, not on the current device {dev}")
    if x.shape[0] < 1 or x.shape[1] < min_side or x.shape[2] < min_side:
        raise ValueError(f"{who}: needs N >= 1 and H, W >= {min_side}, got {tuple(x.shape)}")


def _corrupt_table(who: str, t, dtype, numel=None):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.device.type != "cuda" or \
            (numel is not None and t.numel() != numel) or t.numel() == 0:
        raise ValueError(f"{who}: expected a contiguous device {dtype} table" + (f" of {numel} elements" if numel is not None else "") +
                         f", got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    return t


def _corrupt_out(x, out_kind):
    if out_kind not in (0, 1):
        raise ValueError(f"out_kind must be 0 (uint8) or 1 (fp32 before the floor), got {out_kind!r}")
    return torch.empty(x.shape, dtype=torch.float32 if out_kind else torch.uint8, device=x.device)


def _corrupt_ws(x, nbytes):
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=x.device), nbytes


def corrupt_noise(x, keys_dev, mode: int, c: float, table=None, out_kind=0):
    """Keyed pointwise noise: mode 0 gaussian (c = 255 sigma), 1 speckle (c = sigma), 2 impulse (c = amount), 3 shot (c = the
    reference's constant; table = the int32 view of corrupt.poisson_table(c) on the device).  keys_dev as for `keyed_noise`."""
    check_u8_images("corrupt_noise", x)
    n, h, w_, _ = x.shape
    _corrupt_table("corrupt_noise: keys", keys_dev, torch.int32, 2 * n)
    if mode == 3:
        _corrupt_table("corrupt_noise: table", table, torch.int32, 256 * 128)
    out = _corrupt_out(x, out_kind)
    check(lib.ur_corrupt_noise(x.data_ptr(), keys_dev.data_ptr(), out.data_ptr(), n, h, w_, int(mode), float(c), _ptr(table), out_kind, _stream()))
    return out


def corrupt_filter_sep(x, taps, out_kind=0):
    """Separable filter with a replicate border: taps = device fp32 [2 r + 1], applied along the rows, then along the columns."""
    check_u8_images("corrupt_filter_sep", x)
    _corrupt_table("corrupt_filter_sep: taps", taps, torch.float32)
    if taps.numel() % 2 != 1:
        raise ValueError(f"corrupt_filter_sep: needs an odd number of taps, got {taps.numel()}")
    n, h, w_, _ = x.shape
    out = _corrupt_out(x, out_kind)
    ws, nbytes = _corrupt_ws(x, lib.ur_corrupt_filter_sep_ws_bytes(n, h, w_))
    check(lib.ur_corrupt_filter_sep(x.data_ptr(), taps.data_ptr(), taps.numel() // 2, out.data_ptr(), n, h, w_, ws.data_ptr(), nbytes, out_kind,
                                    _stream()))
    return out


def corrupt_taps(x, taps, border=0, out_kind=0):
    """Tap-list sum: taps = device int32 [T, 3] (one list) or [N, T, 3] (one per image) of (tx, ty, fp32 bits of the weight)
    (corrupt.pack_taps); border 0 = replicate, 1 = reflect-101."""
    check_u8_images("corrupt_taps", x)
    _corrupt_table("corrupt_taps: taps", taps, torch.int32)
    n, h, w_, _ = x.shape
    if taps.shape[-1] != 3 or taps.ndim not in (2, 3) or (taps.ndim == 3 and taps.shape[0] != n):
        raise ValueError(f"corrupt_taps: taps must be [T, 3] or [{n}, T, 3], got {tuple(taps.shape)}")
    out = _corrupt_out(x, out_kind)
    check(lib.ur_corrupt_taps(x.data_ptr(), taps.data_ptr(), taps.shape[-2], int(taps.ndim == 3), int(border), out.data_ptr(), n, h, w_, out_kind,
                              _stream()))
    return out


def corrupt_zoom(x, layers, out_kind=0):
    """(x + the bilinear zoom layers) / (K + 1): layers = device int32 [K, 6] (corrupt.zoom_layers)."""
    check_u8_images("corrupt_zoom", x)
    _corrupt_table("corrupt_zoom: layers", layers, torch.int32)
    if layers.ndim != 2 or layers.shape[1] != 6:
        raise ValueError(f"corrupt_zoom: layers must be [K, 6], got {tuple(layers.shape)}")
    n, h, w_, _ = x.shape
    out = _corrupt_out(x, out_kind)
    check(lib.ur_corrupt_zoom(x.data_ptr(), layers.data_ptr(), layers.shape[0], out.data_ptr(), n, h, w_, out_kind, _stream()))
    return out


def corrupt_color(x, mode: int, a: float, b: float = 0.0, out_kind=0):
    """mode 0 contrast (a = the factor), 1 brightness (V + a, a on the 0-255 scale), 2 saturate (S * a + b)."""
    check_u8_images("corrupt_color", x)
    n, h, w_, _ = x.shape
    out = _corrupt_out(x, out_kind)
    ws, nbytes = _corrupt_ws(x, lib.ur_corrupt_color_ws_bytes(n, h, w_))
    check(lib.ur_corrupt_color(x.data_ptr(), out.data_ptr(), n, h, w_, int(mode), float(a), float(b), ws.data_ptr(), nbytes, out_kind, _stream()))
    return out


def corrupt_pixelate(x, small_h: int, small_w: int, hbox, vbox, ymap, xmap, out_kind=0):
    """Box reduction to small_h x small_w and nearest-neighbour enlargement by the device int32 tables of corrupt.pixelate_tables."""
    check_u8_images("corrupt_pixelate", x)
    n, h, w_, _ = x.shape
    for name, t, numel in (("hbox", hbox, 2 * small_w), ("vbox", vbox, 2 * small_h), ("ymap", ymap, h), ("xmap", xmap, w_)):
        _corrupt_table(f"corrupt_pixelate: {name}", t, torch.int32, numel)
    out = _corrupt_out(x, out_kind)
    ws, nbytes = _corrupt_ws(x, lib.ur_corrupt_pixelate_ws_bytes(n, h, small_w))
    check(lib.ur_corrupt_pixelate(x.data_ptr(), out.data_ptr(), n, h, w_, int(small_h), int(small_w), hbox.data_ptr(), vbox.data_ptr(),
                                  ymap.data_ptr(), xmap.data_ptr(), ws.data_ptr(), nbytes, out_kind, _stream()))
    return out


def corrupt_fog(x, keys_dev, c: float, decay: float, out_kind=0):
    """Fog: a keyed diamond-square map per image blended into it; c = 255 * the reference's constant, decay = its wibble decay."""
    check_u8_images("corrupt_fog", x)
    n, h, w_, _ = x.shape
    _corrupt_table("corrupt_fog: keys", keys_dev, torch.int32, 2 * n)
    out = _corrupt_out(x, out_kind)
    ws, nbytes = _corrupt_ws(x, lib.ur_corrupt_fog_ws_bytes(n, h, w_))
    check(lib.ur_corrupt_fog(x.data_ptr(), keys_dev.data_ptr(), out.data_ptr(), n, h, w_, float(c), float(decay), ws.data_ptr(), nbytes, out_kind,
                             _stream()))
    return out


# ---- JPEG compression as a degradation (csrc/jpeg.hip; the specification is the ur_jpeg_roundtrip comment in the header; the
# planner is unirestore_amd.jpeg) ----------------------------------------------------------------------------------------------
def jpeg_roundtrip(x, quality: int, subsampling: int = 2, out=None):
    """The bytes a baseline JPEG of x (device uint8 [N, H, W, 3], H, W >= 16) decodes to: quality 1..100, subsampling 0 (4:4:4) or
    2 (4:2:0), Pillow's codes.  out: a contiguous uint8 tensor of x's shape on x's device, not x (default: a new one)."""
    check_u8_images("jpeg_roundtrip", x, min_side=16)
    if subsampling not in (0, 2):
        raise ValueError(f"jpeg_roundtrip: subsampling must be 0 (4:4:4) or 2 (4:2:0), got {subsampling!r}")
    n, h, w_, _ = x.shape
    if out is None:
        out = torch.empty_like(x)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != x.shape or out.device != x.device or \
            not out.is_contiguous():
        raise ValueError(f"jpeg_roundtrip: out must be a contiguous uint8 tensor {tuple(x.shape)} on {x.device}")
    ws, nbytes = _corrupt_ws(x, lib.ur_jpeg_roundtrip_ws_bytes(n, h, w_, int(subsampling)))
    check(lib.ur_jpeg_roundtrip(x.data_ptr(), out.data_ptr(), n, h, w_, int(quality), int(subsampling), ws.data_ptr(), nbytes, _stream()))
    return out


# ---- antialiased resize of u8 images (csrc/resize.hip; the specification is the ur_resize_u8 comment in the header; the planner
# that builds the tables is unirestore_amd.resize) -----------------------------------------------------------------------------
def resize_u8(x, size, xaxis, yaxis, out=None):
    """x: device uint8 [N, H, W, 3] (H, W >= 2) -> uint8 [N, oh, ow, 3], size = (oh, ow), both >= 2.  xaxis / yaxis = (bounds, weights,
    K, p) of the width / height axis: device int32 tables [n_out, 2] and [n_out, K] (resize.axis_tables, uploaded).  out: a
    contiguous uint8 tensor [N, oh, ow, 3] on x's device, not x (default: a new one)."""
    check_u8_images("resize_u8", x, min_side=2)
    n, h, w_, _ = x.shape
    if not isinstance(size, (tuple, list)) or len(size) != 2 or any(isinstance(s, bool) or not hasattr(s, "__index__") for s in size) or \
            min(int(s) for s in size) < 2:
        raise ValueError(f"resize_u8: size must be two integers (oh, ow), both >= 2, got {size!r}")
    oh, ow = int(size[0]), int(size[1])
    for who, axis, n_out in (("width", xaxis, ow), ("height", yaxis, oh)):
        if not isinstance(axis, (tuple, list)) or len(axis) != 4:
            raise ValueError(f"resize_u8: the {who} axis must be (bounds, weights, K, p)")
        bounds, weights, k, p = axis
        if isinstance(k, bool) or not hasattr(k, "__index__") or not 1 <= int(k) <= 65536:
            raise ValueError(f"resize_u8: {who} K must be an integer in [1, 65536], got {k!r}")
        if isinstance(p, bool) or not hasattr(p, "__index__") or not 1 <= int(p) <= 22:
            raise ValueError(f"resize_u8: {who} p must be an integer in [1, 22], got {p!r}")
        _corrupt_table(f"resize_u8: {who} bounds", bounds, torch.int32, 2 * n_out)
        _corrupt_table(f"resize_u8: {who} weights", weights, torch.int32, int(k) * n_out)
    shape = (n, oh, ow, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != x.device or \
            not out.is_contiguous() or out.data_ptr() == x.data_ptr():
        raise ValueError(f"resize_u8: out must be a contiguous uint8 tensor {shape} on {x.device}, not the input")
    ws, nbytes = _corrupt_ws(x, lib.ur_resize_u8_ws_bytes(n, h, w_, oh, ow))
    check(lib.ur_resize_u8(x.data_ptr(), out.data_ptr(), n, h, w_, oh, ow, xaxis[0].data_ptr(), xaxis[1].data_ptr(), int(xaxis[2]), int(xaxis[3]),
                           yaxis[0].data_ptr(), yaxis[1].data_ptr(), int(yaxis[2]), int(yaxis[3]), ws.data_ptr(), nbytes, _stream()))
    return out


# ---- glass blur, snow and elastic transform (csrc/distort.hip; the specification is the ur_distort_* comment in the header; the
# planner is unirestore_amd.distort) --------------------------------------------------------------------------------------------
def _distort_field(who: str, f, shape, dev):
    if not isinstance(f, torch.Tensor) or f.dtype != torch.float32 or tuple(f.shape) != tuple(shape) or not f.is_contiguous() or f.device != dev:
        raise ValueError(f"{who}: the field must be a contiguous fp32 tensor {tuple(shape)} on {dev}, got "
                         f"{getattr(f, 'dtype', type(f))} {tuple(getattr(f, 'shape', ()))}")
    return f


def _distort_shape(who: str, n, h, w_):
    if any(isinstance(v, bool) or not hasattr(v, "__index__") for v in (n, h, w_)) or n < 1 or h < 32 or w_ < 32:
        raise ValueError(f"{who}: needs integers N >= 1 and H, W >= 32, got {(n, h, w_)!r}")
    return torch.device("cuda", torch.cuda.current_device())


def distort_shuffle(x, keys_dev, delta: int, draw: int):
    """One iteration of glass blur's local shuffle, u8 -> u8: every interior pixel takes the pixel at (y + dy, x + dx), dy / dx
    keyed integers in [-delta, delta) of draws `draw` / `draw + 1`; delta in 1..4."""
    check_u8_images("distort_shuffle", x)
    n, h, w_, _ = x.shape
    _corrupt_table("distort_shuffle: keys", keys_dev, torch.int32, 2 * n)
    if isinstance(delta, bool) or not hasattr(delta, "__index__") or not 1 <= delta <= 4:
        raise ValueError(f"distort_shuffle: delta must be an integer in [1, 4], got {delta!r}")
    if isinstance(draw, bool) or not hasattr(draw, "__index__") or not 0 <= draw < (1 << 32) - 1:
        raise ValueError(f"distort_shuffle: draw = {draw!r} must be an integer in [0, 2^32 - 1)")
    out = torch.empty_like(x)
    check(lib.ur_distort_shuffle(x.data_ptr(), keys_dev.data_ptr(), out.data_ptr(), n, h, w_, int(delta), int(draw), _stream()))
    return out


def distort_snow_layer(keys_dev, n: int, h: int, w_: int, geometry, loc: float, scale: float, thr: float):
    """The snow layer fp32 [N, oh, ow]: the keyed normal field loc + scale n of an H x W image, its crop geometry = (top, left, ch,
    cw, oh, ow) (distort.snow_geometry) enlarged bilinearly to oh x ow, values < thr zeroed, the rest clamped to [0, 1]."""
    dev = _distort_shape("distort_snow_layer", n, h, w_)
    _corrupt_table("distort_snow_layer: keys", keys_dev, torch.int32, 2 * n)
    if len(geometry) != 6 or any(isinstance(v, bool) or not hasattr(v, "__index__") for v in geometry):
        raise ValueError(f"distort_snow_layer: geometry must be six integers (top, left, ch, cw, oh, ow), got {geometry!r}")
    top, left, ch, cw, oh, ow = (int(v) for v in geometry)
    if oh < h or ow < w_:
        raise ValueError(f"distort_snow_layer: the enlarged layer {oh} x {ow} must cover the image {h} x {w_}")
    field = torch.empty((n, oh, ow), dtype=torch.float32, device=dev)
    check(lib.ur_distort_snow_layer(keys_dev.data_ptr(), field.data_ptr(), n, h, w_, top, left, ch, cw, oh, ow, float(loc), float(scale),
                                    float(thr), _stream()))
    return field


def distort_snow(x, field, taps, keep: float, out_kind=0):
    """Snow from its layer: the motion blur of `field` fp32 [N, oh, ow] by the per-image tap lists int32 [N, T, 3]
    (corrupt.pack_taps), rounded to bytes, added to the whitened image with its own 180-degree rotation."""
    check_u8_images("distort_snow", x)
    n, h, w_, _ = x.shape
    if not isinstance(field, torch.Tensor) or field.ndim != 3 or field.shape[1] < h or field.shape[2] < w_:
        raise ValueError(f"distort_snow: the field must be fp32 [{n}, oh >= {h}, ow >= {w_}], got {tuple(getattr(field, 'shape', ()))}")
    _distort_field("distort_snow", field, (n, field.shape[1], field.shape[2]), x.device)
    _corrupt_table("distort_snow: taps", taps, torch.int32)
    if taps.ndim != 3 or taps.shape[0] != n or taps.shape[2] != 3 or taps.shape[1] > 64:
        raise ValueError(f"distort_snow: taps must be [{n}, T <= 64, 3], got {tuple(taps.shape)}")
    out = _corrupt_out(x, out_kind)
    ws, nbytes = _corrupt_ws(x, lib.ur_distort_snow_ws_bytes(n, h, w_))
    check(lib.ur_distort_snow(x.data_ptr(), field.data_ptr(), taps.data_ptr(), taps.shape[1], out.data_ptr(), n, h, w_, field.shape[1],
                              field.shape[2], float(keep), ws.data_ptr(), nbytes, out_kind, _stream()))
    return out


def distort_field(keys_dev, n: int, h: int, w_: int, taps_y, taps_x, m: float, alpha: float):
    """The elastic displacement field fp32 [N, 2, H, W] (dy, dx): keyed uniforms m (2u - 1) smoothed by the separable filter taps_y
    (along the rows' axis) / taps_x (device fp32, odd lengths) with a reflect border, times alpha."""
    dev = _distort_shape("distort_field", n, h, w_)
    _corrupt_table("distort_field: keys", keys_dev, torch.int32, 2 * n)
    for name, t in (("taps_y", taps_y), ("taps_x", taps_x)):
        _corrupt_table(f"distort_field: {name}", t, torch.float32)
        if t.numel() % 2 != 1:
            raise ValueError(f"distort_field: {name} needs an odd number of taps, got {t.numel()}")
    field = torch.empty((n, 2, h, w_), dtype=torch.float32, device=dev)
    ws, nbytes = _corrupt_ws(field, lib.ur_distort_field_ws_bytes(n, h, w_))
    check(lib.ur_distort_field(keys_dev.data_ptr(), taps_y.data_ptr(), taps_y.numel() // 2, taps_x.data_ptr(), taps_x.numel() // 2,
                               field.data_ptr(), n, h, w_, float(m), float(alpha), ws.data_ptr(), nbytes, _stream()))
    return field


def distort_warp(x, field, out_kind=0):
    """x sampled bilinearly at (y + field[n, 0], x + field[n, 1]), indices reflected at the edges (map_coordinates' "reflect")."""
    check_u8_images("distort_warp", x)
    n, h, w_, _ = x.shape
    _distort_field("distort_warp", field, (n, 2, h, w_), x.device)
    out = _corrupt_out(x, out_kind)
    check(lib.ur_distort_warp(x.data_ptr(), field.data_ptr(), out.data_ptr(), n, h, w_, out_kind, _stream()))
    return out


def ddim_step_(zt, zt_bf16, eps_f32, clat, c_x, c_e):
    cp = zt.shape[-1]
    check(lib.ur_ddim_step(zt.data_ptr(), eps_f32.data_ptr(), eps_f32.shape[-1], zt_bf16.data_ptr(), zt.numel() // cp, clat, cp,
                           c_x, c_e, _dt(zt_bf16), _stream()))


def latent_tiles_gather(z, origins_dev, th, tw):
    """z fp32 NHWC [N,LH,LW,Cpad] -> 16-bit tile batch [N*T,th,tw,Cpad] (origins_dev: device int32 [T,2])."""
    n, lh, lw, cp = z.shape
    t = origins_dev.shape[0]
    out = torch.empty((n * t, th, tw, cp), dtype=_act, device=z.device)
    check(lib.ur_latent_tiles_gather(z.data_ptr(), out.data_ptr(), n, lh, lw, cp, t, th, tw, origins_dev.data_ptr(), _dt(), _stream()))
    return out


def latent_tiles_blend_ddim_(zt, zt_tiles, eps_tiles, wn, origins_dev, clat, c_x, c_e):
    """Blended DDIM step of tiled sampling: zt (fp32 [N,LH,LW,Cpad]) and zt_tiles (16-bit [N*T,th,tw,Cpad]) updated in place from
    the per-tile eps (fp32 [N*T,th,tw,ld]) and the normalised weights wn (fp32 [T,th,tw])."""
    n, lh, lw, cp = zt.shape
    t, th, tw = wn.shape
    check(lib.ur_latent_tiles_blend_ddim(zt.data_ptr(), eps_tiles.data_ptr(), eps_tiles.shape[-1], zt_tiles.data_ptr(), wn.data_ptr(),
                                         n, lh, lw, clat, cp, t, th, tw, origins_dev.data_ptr(), c_x, c_e, _dt(zt_tiles), _stream()))


def f32_to_bf16(x, c, mul=1.0, cpad=8):
    ld = x.shape[-1]
    out = torch.empty((*x.shape[:-1], cpad), dtype=_act, device=x.device)
    check(lib.ur_f32_to_bf16_scaled(x.data_ptr(), ld, out.data_ptr(), x.numel() // ld, c, cpad, mul, _dt(), _stream()))
    return out


def _check_images(who, name, t):
    """t must be a contiguous 4-d fp32 NCHW tensor on the current device."""
    dev = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.ndim != 4:
        raise ValueError(f"{who}: {name} must be a 4-d fp32 NCHW tensor, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if t.device != dev:
        raise ValueError(f"{who}: {name} is on {t.device}, not on the current device {dev}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")


def _check_scorer(who, what, obj, cls, makers):
    """obj (a scorer's `what`: its weights or params) must be a `cls`, which `makers` return, on the current device."""
    dev = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(obj, cls):
        raise ValueError(f"{who}: {what} must come from {makers}, got {type(obj).__name__}")
    if obj.device != dev:
        raise ValueError(f"{who}: the {what} are on {obj.device}, not on the current device {dev}")


def image_metrics(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, win: int = 7):
    """Per-image PSNR and SSIM of fp32 NCHW batches on the GPU -> (psnr, ssim), fp64 [N] device tensors.  Same semantics as
    runner.psnr_per_image / runner.ssim per image (skimage defaults: uniform win x win window, K1 0.01, K2 0.03, sample
    covariance, valid interior); fp64 moments and fixed-order sums, so two calls give the same bits.  No host sync."""
    dev = torch.device("cuda", torch.cuda.current_device())
    for name, t in (("pred", pred), ("target", target)):
        _check_images("image_metrics", name, t)
    if pred.shape != target.shape:
        raise ValueError(f"image_metrics: shapes differ: {tuple(pred.shape)} vs {tuple(target.shape)}")
    n, c, h, w = pred.shape
    if not data_range > 0:
        raise ValueError(f"image_metrics: data_range must be > 0, got {data_range}")
    ws_bytes = lib.ur_image_metrics_ws_size(n, c, h, w, int(win))
    if ws_bytes < 0:
        check(int(ws_bytes))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    psnr = torch.empty(n, dtype=torch.float64, device=dev)
    ssim = torch.empty(n, dtype=torch.float64, device=dev)
    check(lib.ur_image_metrics(pred.data_ptr(), target.data_ptr(), n, c, h, w, int(win), float(data_range), psnr.data_ptr(),
                               ssim.data_ptr(), ws.data_ptr(), ws_bytes, _stream()))
    return psnr, ssim


def lpips(pred: torch.Tensor, target: torch.Tensor, weights) -> torch.Tensor:
    """LPIPS (AlexNet, normalize=True: inputs in [0,1]) of fp32 NCHW batches on the GPU -> fp64 [N] device tensor.  weights: what
    lpips.load_weights / lpips.random_weights return.  Predictions and targets go through the network as one batch of 2N; exact
    fp32 (fp32-input MFMA convolutions), fixed-order sums, so two calls give the same bits.  No host sync.  A NaN or an infinity
    in an image of either batch makes that image's distance NaN, as the fp64 restatement of the metric in torch does; the other
    images' distances are the bits a clean batch gives."""
    from . import lpips as _lpips
    for name, t in (("pred", pred), ("target", target)):
        _check_images("lpips", name, t)
    if pred.shape != target.shape:
        raise ValueError(f"lpips: shapes differ: {tuple(pred.shape)} vs {tuple(target.shape)}")
    n, c, h, w = pred.shape
    if n < 1 or c != 3 or h < _lpips.MIN_HW or w < _lpips.MIN_HW:
        raise ValueError(f"lpips: needs [N>=1, 3, H>={_lpips.MIN_HW}, W>={_lpips.MIN_HW}] images, got {tuple(pred.shape)}")
    _check_scorer("lpips", "weights", weights, _lpips.LpipsWeights, "lpips.load_weights / lpips.random_weights")
    return _lpips.forward(pred, target, weights)


def niqe(images: torch.Tensor, params, color_space: str = "yiq") -> torch.Tensor:
    """NIQE (no reference; lower is better) of fp32 NCHW images in [0,1] -> fp64 [N] device tensor.  params: what niqe.load_params /
    niqe.random_params / niqe.fit_params return.  The block features are fp64 HIP kernels with fixed-order sums (two calls give
    the same bits); the 36-dimensional algebra of the score runs on the host (one device-to-host copy).  The top-left
    (H // 96 * 96, W // 96 * 96) crop must hold at least two 96 x 96 blocks."""
    from . import niqe as _niqe
    _check_images("niqe", "images", images)
    n, c, h, w = images.shape
    if n < 1 or c != 3:
        raise ValueError(f"niqe: needs [N>=1, 3, H, W] images, got {tuple(images.shape)}")
    if h < _niqe.BLOCK or w < _niqe.BLOCK or (h // _niqe.BLOCK) * (w // _niqe.BLOCK) < _niqe.MIN_BLOCKS:
        raise ValueError(f"niqe: images of shape {tuple(images.shape)} hold {(h // _niqe.BLOCK) * (w // _niqe.BLOCK)} block(s) of "
                         f"{_niqe.BLOCK} x {_niqe.BLOCK}; the score needs at least {_niqe.MIN_BLOCKS}")
    _check_scorer("niqe", "params", params, _niqe.NiqeParams, "niqe.load_params / niqe.random_params / niqe.fit_params")
    if color_space not in _niqe.COLOR_SPACES:
        raise ValueError(f"niqe: unknown color_space {color_space!r}, choose from {_niqe.COLOR_SPACES}")
    return _niqe.forward(images, params, color_space)


def classify(images: torch.Tensor, weights) -> torch.Tensor:
    """Logits [N, classes] (fp32, on the device) of fp32 NCHW images in [0,1], any H, W >= 1: the classification evaluator's
    preprocess (antialiased bilinear resize to 224 x 224, ImageNet normalisation) and a ResNet, in exact fp32 on the GPU.  weights:
    what classify.load_weights / classify.random_weights return.  An image's logits do not depend on its place in the batch, and
    two calls give the same bits.  No host sync.  A non-finite pixel is not erased on the way: every logit is finite, infinite or
    NaN exactly where the fp64 restatement in torch is (one NaN pixel: every logit of that image is NaN, and `top1`, as
    torch.argmax, then predicts the first NaN's class); the other images' logits are the bits a clean batch gives."""
    from . import classify as _classify
    _check_images("classify", "images", images)
    n, c, h, w = images.shape
    if n < 1 or c != 3 or h < 1 or w < 1:
        raise ValueError(f"classify: needs [N>=1, 3, H>=1, W>=1] images, got {tuple(images.shape)}")
    _check_scorer("classify", "weights", weights, _classify.ClassifierWeights, "classify.load_weights / classify.random_weights")
    return _classify.forward(images, weights)


def vit(images: torch.Tensor, weights) -> torch.Tensor:
    """`classify` with a VisionTransformer: logits [N, classes] (fp32, on the device) of fp32 NCHW images in [0,1], any H, W >= 1 -
    the classification evaluator's preprocess (antialiased bilinear resize to 224 x 224, ImageNet normalisation) and a torchvision-
    layout ViT in exact fp32 on the GPU (the fp32 convolution as every Linear; LayerNorm, GELU and attention of csrc/vit.hip).
    weights: what vit.load_weights / vit.random_weights return; `top1` takes the logits as it takes `classify`'s.  An image's
    logits do not depend on its place in the batch, and two calls give the same bits.  No host sync.  A non-finite pixel is not
    erased on the way: every logit of that image is NaN, as in the fp64 restatement in torch (LayerNorm of a row with a NaN or an
    infinity is NaN); the other images' logits are the bits a clean batch gives."""
    from . import vit as _vit
    _check_images("vit", "images", images)
    n, c, h, w = images.shape
    if n < 1 or c != 3 or h < 1 or w < 1:
        raise ValueError(f"vit: needs [N>=1, 3, H>=1, W>=1] images, got {tuple(images.shape)}")
    _check_scorer("vit", "weights", weights, _vit.ViTWeights, "vit.load_weights / vit.random_weights")
    return _vit.forward(images, weights)


def swin(images: torch.Tensor, weights) -> torch.Tensor:
    """`classify` with a Swin-V2: logits [N, classes] (fp32, on the device) of fp32 NCHW images in [0,1], any H, W >= 1 - the
    classification evaluator's preprocess (antialiased bilinear resize to 224 x 224, ImageNet normalisation) and a torchvision-
    layout SwinTransformer V2 in exact fp32 on the GPU (the fp32 convolution as every Linear, patch embedding and patch merging;
    LayerNorm and GELU of csrc/vit.hip; the fused shifted-window cosine attention of csrc/swin.hip).  weights: what
    swin.load_weights / swin.random_weights return; `top1` takes the logits as it takes `classify`'s.  An image's logits do not
    depend on its place in the batch, and two calls give the same bits.  No host sync.  A non-finite pixel is not erased on the
    way: every logit of that image is NaN, as in the fp64 restatement in torch; the other images' logits are the bits a clean
    batch gives."""
    from . import swin as _swin
    _check_images("swin", "images", images)
    n, c, h, w = images.shape
    if n < 1 or c != 3 or h < 1 or w < 1:
        raise ValueError(f"swin: needs [N>=1, 3, H>=1, W>=1] images, got {tuple(images.shape)}")
    _check_scorer("swin", "weights", weights, _swin.SwinWeights, "swin.load_weights / swin.random_weights")
    return _swin.forward(images, weights)


def rvt(images: torch.Tensor, weights) -> torch.Tensor:
    """`classify` with a Robust Vision Transformer: logits [N, classes] (fp32, on the device) of fp32 NCHW images in [0,1], any H,
    W >= 1 - the classification evaluator's preprocess (antialiased bilinear resize to 224 x 224, ImageNet normalisation) and the
    reference's own PoolingTransformer (rvt_tiny / rvt_small / rvt_base and their `_plus` variants) in exact fp32 on the GPU (the
    fp32 convolution as the stem, every Linear and every 1 x 1 convolution, BatchNorm folded in; LayerNorm and GELU of csrc/vit.hip;
    the gated attention and the depthwise 3 x 3 convolution of csrc/rvt.hip).  weights: what rvt.load_weights / rvt.random_weights
    return; `top1` takes the logits as it takes `classify`'s.  An image's logits do not depend on its place in the batch, and two
    calls give the same bits.  No host sync.  A non-finite pixel is not erased on the way: every logit of that image is NaN, as in
    the fp64 restatement in torch; the other images' logits are the bits a clean batch gives."""
    from . import rvt as _rvt
    _check_images("rvt", "images", images)
    n, c, h, w = images.shape
    if n < 1 or c != 3 or h < 1 or w < 1:
        raise ValueError(f"rvt: needs [N>=1, 3, H>=1, W>=1] images, got {tuple(images.shape)}")
    _check_scorer("rvt", "weights", weights, _rvt.RVTWeights, "rvt.load_weights / rvt.random_weights")
    return _rvt.forward(images, weights)


def vgg(images: torch.Tensor, weights) -> torch.Tensor:
    """`classify` with a VGG: logits [N, classes] (fp32, on the device) of fp32 NCHW images in [0,1], any H, W >= 1 - the
    classification evaluator's preprocess (antialiased bilinear resize to 224 x 224, ImageNet normalisation) and a torchvision-
    layout VGG 11 / 13 / 16 / 19 (with or without BatchNorm) in exact fp32 on the GPU (the fp32 convolution with the BatchNorm
    folded in; the 2 x 2 max-pool, the adaptive average pool and the split-K Linear of csrc/vgg.hip).  weights: what
    vgg.load_weights / vgg.random_weights return; `top1` takes the logits as it takes `classify`'s.  An image's logits do not
    depend on its place in the batch, and two calls give the same bits.  No host sync.  A non-finite pixel is not erased on the
    way: it reaches its image's logits as in the fp64 restatement in torch (one NaN pixel: every logit of that image is NaN); the
    other images' logits are the bits a clean batch gives."""
    from . import vgg as _vgg
    _check_images("vgg", "images", images)
    n, c, h, w = images.shape
    if n < 1 or c != 3 or h < 1 or w < 1:
        raise ValueError(f"vgg: needs [N>=1, 3, H>=1, W>=1] images, got {tuple(images.shape)}")
    _check_scorer("vgg", "weights", weights, _vgg.VGGWeights, "vgg.load_weights / vgg.random_weights")
    return _vgg.forward(images, weights)


def top1(logits: torch.Tensor, labels: torch.Tensor):
    """(pred, tp, targets, predicted) of one batch: pred int64 [N] = the argmax of logits fp32 [N,C] (ties to the lowest index, as
    torch.argmax), and the three int64 [C] per-class counts of classify.accuracy - tp_c (pred = label = c), targets_c, predicted_c.
    labels: an integer [N] tensor, on the host or the device; a label outside [0, C) is a ValueError raised before any launch
    (checking device labels reads them back: one host sync)."""
    from . import classify as _classify
    dev = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.ndim != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"top1: logits must be a non-empty fp32 [N, C] tensor, got "
                         f"{getattr(logits, 'dtype', type(logits))} {tuple(getattr(logits, 'shape', ()))}")
    if logits.device != dev:
        raise ValueError(f"top1: logits is on {logits.device}, not on the current device {dev}")
    if not logits.is_contiguous():
        raise ValueError("top1: logits must be contiguous")
    if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int64, torch.int32) or labels.shape != (logits.shape[0],):
        raise ValueError(f"top1: labels must be an int64 / int32 [{logits.shape[0]}] tensor, got "
                         f"{getattr(labels, 'dtype', type(labels))} {tuple(getattr(labels, 'shape', ()))}")
    if labels.is_cuda and labels.device != dev:
        raise ValueError(f"top1: labels is on {labels.device}, not on the host or the current device {dev}")
    host = labels.cpu()
    if int(host.min()) < 0 or int(host.max()) >= logits.shape[1]:
        bad = [int(v) for v in host.tolist() if not 0 <= v < logits.shape[1]]
        raise ValueError(f"top1: label {bad[0]} is outside [0, {logits.shape[1]}), the logits' classes")
    pred, counts = _classify.top1_counts(logits, labels.to(device=dev, dtype=torch.int64).contiguous())
    return pred, counts[0], counts[1], counts[2]


def _segmenter(who, images, weights, cls, size, scales):
    """`segment` and `deeplab` behind their names: the checks on images, weights (a `cls` of module `who`), size and scales, then
    the one test-time augmentation of segment.py."""
    from . import segment as _segment
    _check_images(who, "images", images)
    n, c, h, w = images.shape
    if n < 1 or c != 3 or h < 1 or w < 1:
        raise ValueError(f"{who}: needs [N>=1, 3, H>=1, W>=1] images, got {tuple(images.shape)}")
    _check_scorer(who, "weights", weights, cls, f"{who}.load_weights / {who}.random_weights")
    if size is not None and not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and v >= 1 for v in size)):
        raise ValueError(f"{who}: size must be (H, W) with H, W >= 1, got {size!r}")
    if not (isinstance(scales, (tuple, list)) and 1 <= len(scales) <= 3 and all(isinstance(v, (int, float)) and 0 < v <= 8 for v in scales)):
        raise ValueError(f"{who}: scales must be 1 to 3 numbers in (0, 8], got {scales!r}")
    return _segment.segment(images, weights, size, scales)


def segment(images: torch.Tensor, weights, size=None, scales=(1, 0.8, 0.6)) -> torch.Tensor:
    """Predicted classes uint8 [N,H,W] (on the device) of fp32 NCHW images in [0,1]: the segmentation evaluator's test-time
    augmentation in exact fp32 on the GPU - for each scale a bilinear align_corners=True resize to floor(size * scale), RefineNet-LW's
    preprocess and network; then every scale's logits resized to `size` (default: the images' own H, W), averaged, argmax (ties to
    the lowest class).  weights: what segment.load_weights / segment.random_weights return.  ValueError when the smallest scale's
    input falls below 32 px on a side.  An image's result does not depend on its place in the batch, and two calls give the same
    bytes.  No host sync - except on the FIRST call for a new image size, target size or set of scales, which builds that shape's
    tap tables on the host and uploads them with a blocking copy: run a shape once eagerly before capturing it in a graph.  The
    tables (a few KB per shape) stay on the device for the life of the process, so a captured graph never loses the ones it reads.
    A non-finite pixel is not erased on the way: the averaged logits are finite, infinite or NaN exactly where the fp64 restatement
    in torch is, a pixel whose class vector holds a NaN is given its first NaN's class (torch.argmax), and the other images'
    predictions are the bytes a clean batch gives."""
    from .segment import SegmenterWeights
    return _segmenter("segment", images, weights, SegmenterWeights, size, scales)


def deeplab(images: torch.Tensor, weights, size=None, scales=(1, 0.8, 0.6)) -> torch.Tensor:
    """`segment` with the reference's other segmenter, DeepLabV3+ on ResNet-50 / 101 at output stride 16: predicted classes uint8
    [N,H,W] (on the device) of fp32 NCHW images in [0,1].  For each scale a bilinear align_corners=True resize to floor(size *
    scale), the ImageNet Normalize and the network; then one kernel takes every scale's classifier map through the model's own
    half-pixel resize to that scale's input and the evaluator's align_corners=True resize to `size` (default: the images' own H,
    W), averages and takes the argmax (ties to the lowest class).  weights: what deeplab.load_weights / deeplab.random_weights
    return.  ValueError when the smallest scale's input falls below 16 px on a side.  The same guarantees - for non-finite pixels
    too - and the same first-call table upload as `segment`: run a shape once eagerly before capturing it in a graph."""
    from .deeplab import DeepLabWeights
    return _segmenter("deeplab", images, weights, DeepLabWeights, size, scales)


def checked_targets(target: torch.Tensor, classes: int = 19, ignore_index: int = 255) -> torch.Tensor:
    """A uint8 / int64 target tensor on the current device, after checking that every value lies in [0, classes) or is
    ignore_index (ValueError otherwise; one flag is read back: one host sync).  What `confusion` does to its targets; a caller
    that scores several predictions against the same targets checks them once with this and calls segment.confusion."""
    target = target.to(torch.device("cuda", torch.cuda.current_device()))
    wrong = (target != ignore_index) & ((target < 0) | (target >= classes)) if target.dtype == torch.int64 else \
        (target != ignore_index) & (target >= classes)
    if bool(wrong.any()):
        raise ValueError(f"confusion: target {int(target[wrong][0])} is neither in [0, {classes}) nor ignore_index {ignore_index}")
    return target


def confusion(pred: torch.Tensor, target: torch.Tensor, classes: int = 19, ignore_index: int = 255) -> torch.Tensor:
    """The confusion matrix int64 [classes, classes] (on the device) of one batch, conf[target][pred], over the pixels whose target
    is not ignore_index: pred uint8 on the device, target uint8 / int64 of the same shape, on the host or the device.  A target
    outside [0, classes) that is not ignore_index, or a prediction >= classes, is a ValueError raised before any launch (checking
    device tensors reads one flag back: one host sync).  segment.miou turns the summed matrices into mIoU and pixel accuracy."""
    from . import segment as _segment
    dev = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(classes, int) or not 1 <= classes <= 255 or not isinstance(ignore_index, int):
        raise ValueError(f"confusion: classes must be an int in [1, 255] and ignore_index an int, got {classes!r}, {ignore_index!r}")
    if not isinstance(pred, torch.Tensor) or pred.dtype != torch.uint8 or pred.numel() < 1:
        raise ValueError(f"confusion: pred must be a non-empty uint8 tensor, got {getattr(pred, 'dtype', type(pred))} {tuple(getattr(pred, 'shape', ()))}")
    if pred.device != dev:
        raise ValueError(f"confusion: pred is on {pred.device}, not on the current device {dev}")
    if not isinstance(target, torch.Tensor) or target.dtype not in (torch.uint8, torch.int64) or target.shape != pred.shape:
        raise ValueError(f"confusion: target must be a uint8 / int64 {tuple(pred.shape)} tensor, got "
                         f"{getattr(target, 'dtype', type(target))} {tuple(getattr(target, 'shape', ()))}")
    if target.is_cuda and target.device != dev:
        raise ValueError(f"confusion: target is on {target.device}, not on the host or the current device {dev}")
    if not pred.is_contiguous() or not target.is_contiguous():
        raise ValueError("confusion: pred and target must be contiguous")
    target = checked_targets(target, classes, ignore_index)
    if bool((pred >= classes).any()):
        raise ValueError(f"confusion: prediction {int(pred.max())} is outside [0, {classes})")
    return _segment.confusion(pred, target, classes, ignore_index)


def detect(images: torch.Tensor, weights, score_thresh: float = 0.05, topk_candidates: int = 1000, nms_thresh: float = 0.5,
           detections_per_img: int = 300) -> list:
    """RetinaNet detections of fp32 NCHW images [N,3,H,W] in [0,1] (one size per batch), torchvision's result: per image {boxes
    [n,4] (x1, y1, x2, y2 in the image's own pixels), scores [n] descending, labels int64 [n]} on the device.  weights: what
    detect.load_weights / detect.random_weights return.  The defaults are torchvision's own.  An image whose logits or regressions
    were not finite has no detections (detect.forward also returns that flag; detect.raw is the padded, sync-free form)."""
    from . import detect as _detect
    if not isinstance(weights, _detect.DetectorWeights):
        raise ValueError(f"detect: weights must be a detect.DetectorWeights, got {type(weights).__name__}")
    if not isinstance(images, torch.Tensor) or images.dtype != torch.float32 or images.ndim != 4 or images.shape[1] != 3 or images.numel() < 1:
        raise ValueError(f"detect: images must be a non-empty fp32 [N,3,H,W] tensor, got {getattr(images, 'dtype', type(images))} "
                         f"{tuple(getattr(images, 'shape', ()))}")
    if images.device != weights.device:
        raise ValueError(f"detect: images are on {images.device}, the weights on {weights.device}")
    return _detect.forward(images.contiguous(), weights, score_thresh=score_thresh, topk_candidates=topk_candidates, nms_thresh=nms_thresh,
                           detections_per_img=detections_per_img)[0]


def mean_ap(detections, targets, iou: float = 0.5) -> float:
    """The mean average precision at one IoU threshold of per-image detections against per-image targets {boxes, labels}: one
    detect.MeanAP update (host fp64; pycocotools' algorithm, area range all, 100 detections per image and class)."""
    from .detect import MeanAP
    m = MeanAP(iou)
    m.update(detections, targets)
    return m.compute()["map"]


def profile_enable(on: bool):
    check(lib.ur_profile_enable(int(on)))


def profile_report() -> dict:
    import ctypes
    import json
    buf = ctypes.create_string_buffer(1 << 20)
    check(lib.ur_profile_report(buf, len(buf)))
    return json.loads(buf.value.decode())
