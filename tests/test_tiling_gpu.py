"""Tiled latent sampling on the GPU: the tile gather / blended DDIM kernels against fp64 torch, the single-tile identity with
whole-latent sampling, the tiled forward against a tiled CPU oracle (composed here from the oracle's classes, with its own tile
plan and fp64 weights computed from the spec, so it checks the product's plan too), and graph-replay determinism."""
import math

import pytest
import torch
import torch.nn.functional as F

from golden_util import rel_l2
from tiny_cfg import TINY, model_kwargs, randomise_

pytestmark = pytest.mark.gpu

# rel-L2 tolerances of the whole tiny forward (tests/test_modules_gpu.py TOL fwd_*: 1.5 x measured for whole-latent sampling)
FWD_TOL = {"bf16": dict(z0=8.5e-3, zt=6e-3, img=5.5e-3), "fp16": dict(z0=1.05e-3, zt=7.6e-4, img=7e-4)}
TILE, STRIDE = 32, 24           # 96x80 input -> 768x640 after resize + pad -> 80x64 latent -> 3 x 3 tiles of 32x32


@pytest.fixture(scope="module")
def M():
    import unirestore_amd.modules as m
    return m


def _pair(M, seed=0, steps=2, dtype="bf16", kw=None):
    from oracle.model import DiffUIE as ODiffUIE
    torch.manual_seed(seed)
    kw = kw or model_kwargs(steps)
    o = randomise_(ODiffUIE(**kw, **TINY).eval(), seed)
    p = M.DiffUIE(**kw, **TINY, use_graph=False, dtype=dtype).eval()
    p.load_state_dict(o.state_dict())
    return o, p


# ---- the tiled CPU oracle -------------------------------------------------------------------------------------------------
def _spec_origins(length, n, s):
    if length <= n:
        return [0], length
    out, pos = [], 0
    while pos + n < length:
        out.append(pos)
        pos += s
    if length - n not in out:
        out.append(length - n)
    return out, n


def _spec_plan(lh, lw, n, s):
    """Origins (row-major) and fp64 normalised weights [T, th, tw] from the spec."""
    ys, th = _spec_origins(lh, n, s)
    xs, tw = _spec_origins(lw, n, s)
    origins = [(y, x) for y in ys for x in xs]

    def g(m):
        i = torch.arange(m, dtype=torch.float64)
        return torch.exp(-(i - (m - 1) / 2) ** 2 / (2 * (0.1 * m) ** 2))
    w = g(th)[:, None] * g(tw)[None, :]
    acc = torch.zeros(lh, lw, dtype=torch.float64)
    for y, x in origins:
        acc[y:y + th, x:x + tw] += w
    return origins, (th, tw), torch.stack([w / acc[y:y + th, x:x + tw] for y, x in origins])


def _tiles(z, origins, th, tw):
    """NCHW [N,C,H,W] -> tile batch [N*T,C,th,tw], image-major (image n's tile k at n*T+k)."""
    return torch.stack([z[:, :, y:y + th, x:x + tw] for y, x in origins], 1).flatten(0, 1)


def tiled_oracle(o, images, noise, tile, stride):
    """oracle.model.DiffUIE.forward with its denoise loop tiled: per-step eps of the tile batch blended with the spec's weights."""
    from oracle import schedule
    from oracle.model import resize_pad_plan
    org_h, org_w = images.shape[-2:]
    h, w, pad_h, pad_w = resize_pad_plan(org_h, org_w)
    x = F.interpolate(images, (h, w), mode="bicubic", align_corners=False, antialias=False) if (h, w) != (org_h, org_w) else images
    if pad_h or pad_w:
        x = F.pad(x, (0, pad_w, 0, pad_h), mode="reflect")
    n_vae, n_t = noise
    with torch.no_grad():
        z0, mids = o.ae.encode(x, enable_fr=True, noise=n_vae)
        nb, c, lh, lw = z0.shape
        origins, (th, tw), wn = _spec_plan(lh, lw, tile, stride)
        nt = len(origins)
        zt, _, _ = o.diffuse(z0, torch.full((nb,), 999, dtype=torch.int64), n_t)
        z0t = _tiles(z0, origins, th, tw)
        for t in o.timesteps:
            ts = torch.tensor([int(t)], dtype=torch.int64)
            eps_t = o.base_model(_tiles(zt, origins, th, tw), o.controller(z0t, ts), ts).double().view(nb, nt, c, th, tw)
            eps = torch.zeros(nb, c, lh, lw, dtype=torch.float64)
            for k, (y, x0) in enumerate(origins):
                eps[:, :, y:y + th, x0:x0 + tw] += wn[k] * eps_t[:, k]
            zt = schedule.ddim_step(eps.float(), int(t), zt, o.num_inference_steps)
        preds = o.ae.decode(zt, mids, "ir")[..., :h, :w]
        preds = F.interpolate(preds, (org_h, org_w), mode="bicubic", align_corners=False, antialias=False)
    return preds, z0, zt


@pytest.fixture(scope="module")
def case(M):
    """Oracle weights, inputs and the tiled CPU reference of the 96x80 forward (2 steps), shared by the parity tests."""
    o, _ = _pair(M, 3, steps=2)
    g = torch.Generator().manual_seed(11)
    img = torch.rand(1, 3, 96, 80, generator=g)
    noise = (torch.randn(1, 4, 80, 64, generator=g), torch.randn(1, 4, 80, 64, generator=g))
    ref = tiled_oracle(o, img, noise, TILE, STRIDE)
    return o, img, noise, ref


# ---- 1. kernels vs fp64 torch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gather_and_blend_kernels(dtype):
    from unirestore_amd import ops, schedule
    from unirestore_amd.tiling import latent_tile_plan
    ops.set_dtype(dtype)
    try:
        g = torch.Generator().manual_seed(5)
        n, lh, lw, clat, cp = 2, 80, 64, 4, 8
        origins, (th, tw), wn = latent_tile_plan(lh, lw, TILE, STRIDE)
        nt = len(origins)
        org_d = torch.tensor(origins, dtype=torch.int32).cuda()
        wn_d = torch.from_numpy(wn).cuda()
        z = torch.zeros(n, lh, lw, cp)
        z[..., :clat] = torch.randn(n, lh, lw, clat, generator=g)
        eps = torch.randn(n * nt, th, tw, cp, generator=g)                # padding channels carry garbage: must not leak
        zd, epsd = z.cuda(), eps.cuda()
        tiles = ops.latent_tiles_gather(zd, org_d, th, tw)
        tdt = ops.act_dtype()
        ref_tiles = torch.stack([z[:, y:y + th, x:x + tw] for y, x in origins], 1).flatten(0, 1).to(tdt)
        assert tiles.shape == (n * nt, th, tw, cp) and tiles.dtype == tdt
        assert torch.equal(tiles.cpu(), ref_tiles)                         # gather is exact

        c_x, c_e = schedule.ddim_coefficients(int(schedule.ddim_timesteps(4)[1]), 4)
        ops.latent_tiles_blend_ddim_(zd, tiles, epsd, wn_d, org_d, clat, c_x, c_e)
        torch.cuda.synchronize()
        out, out_tiles = zd.cpu(), tiles.cpu()

        e64 = torch.zeros(n, lh, lw, clat, dtype=torch.float64)
        mag = torch.zeros(n, lh, lw, clat, dtype=torch.float64)
        ev = eps.double().view(n, nt, th, tw, cp)[..., :clat]
        for k, (y, x) in enumerate(origins):
            wk = torch.from_numpy(wn[k]).double()[None, :, :, None]
            e64[:, y:y + th, x:x + tw] += wk * ev[:, k]
            mag[:, y:y + th, x:x + tw] += (wk * ev[:, k]).abs()
        z64 = z[..., :clat].double()
        ref = c_x * z64 + c_e * e64
        bound = 8 * 2.0 ** -24 * (abs(c_x) * z64.abs() + abs(c_e) * mag) + 1e-30      # a few fp32 roundings of the sum
        err = (out[..., :clat].double() - ref).abs()
        assert (err <= bound).all(), float((err / bound).max())
        assert (out[..., clat:] == 0).all()
        for b in range(n):
            for k, (y, x) in enumerate(origins):
                slot = out_tiles[b * nt + k]
                assert torch.equal(slot, out[b, y:y + th, x:x + tw].to(tdt)), (b, k)
    finally:
        ops.set_dtype("bf16")


def test_kernels_reject_bad_arguments():
    from unirestore_amd import capi
    s = torch.cuda.current_stream().cuda_stream
    z = torch.zeros(1, 16, 16, 8, device="cuda")
    t = torch.zeros(1, 16, 16, 8, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(1, 2, dtype=torch.int32, device="cuda")
    assert capi.lib.ur_latent_tiles_gather(z.data_ptr(), t.data_ptr(), 1, 16, 16, 8, 1, 32, 16, o.data_ptr(), 0, s) == capi.UR_E_INVALID
    assert capi.lib.ur_latent_tiles_blend_ddim(z.data_ptr(), z.data_ptr(), 8, t.data_ptr(), None, 1, 16, 16, 4, 8, 1, 16, 16,
                                               o.data_ptr(), 1.0, 0.0, 0, s) == capi.UR_E_INVALID


# ---- 2. single-tile identity ---------------------------------------------------------------------------------------------
def test_single_tile_is_bit_identical(M):
    _, p = _pair(M, 1, steps=2)
    p.use_graph = True
    g = torch.Generator().manual_seed(2)
    img = torch.rand(1, 3, 512, 512, generator=g)
    noise = (torch.randn(1, 4, 64, 64, generator=g), torch.randn(1, 4, 64, 64, generator=g))
    y0 = p(img, "ir", noise=noise, return_latents=True)
    p.set_latent_tiling(64, 48)
    assert p._tile_plan(64, 64) is None                                   # one tile: the whole-latent loop runs
    y1 = p(img, "ir", noise=noise, return_latents=True)
    p.set_latent_tiling(None)
    y2 = p(img, "ir", noise=noise, return_latents=True)
    for a, b, c in zip(y0, y1, y2):
        assert torch.equal(a.cpu(), b.cpu()) and torch.equal(a.cpu(), c.cpu())


# ---- 3. tiled forward vs the tiled CPU oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("use_graph", [False, True])
def test_tiled_forward_matches_tiled_oracle(M, case, dtype, use_graph):
    o, img, noise, (oy, oz0, ozt) = case
    p = M.DiffUIE(**model_kwargs(2), **TINY, use_graph=use_graph, dtype=dtype).eval()
    p.load_state_dict(o.state_dict())
    p.set_latent_tiling(TILE, STRIDE)
    assert p._tile_plan(80, 64)[0] == 9
    py, pz0, pzt = p(img, "ir", noise=noise, return_latents=True)
    e = dict(z0=rel_l2(pz0.cpu(), oz0), zt=rel_l2(pzt.cpu(), ozt), img=rel_l2(py.cpu(), oy))
    print(f"tiled forward rel-L2 [{dtype}, graph={use_graph}]:", e)
    t = FWD_TOL[dtype]
    assert py.shape == img.shape
    assert e["z0"] < t["z0"] and e["zt"] < t["zt"] and e["img"] < t["img"], e


def test_chunked_controller_matches_oracle(M, case, monkeypatch):
    """Large tile batches: limit 9 (= N*T) runs the Controller one step at a time, 18 as one chunk of both steps (run_steps)."""
    import unirestore_amd.modules.model as mm
    o, img, noise, (oy, _, ozt) = case
    p = M.DiffUIE(**model_kwargs(2), **TINY, use_graph=False, dtype="bf16").eval()
    p.load_state_dict(o.state_dict())
    p.set_latent_tiling(TILE, STRIDE)
    for limit in (18, 9):
        monkeypatch.setattr(mm, "TILE_CONTROLLER_MAX_IMAGES", limit)
        py, _, pzt = p(img, "ir", noise=noise, return_latents=True)
        e = dict(zt=rel_l2(pzt.cpu(), ozt), img=rel_l2(py.cpu(), oy))
        assert e["zt"] < FWD_TOL["bf16"]["zt"] and e["img"] < FWD_TOL["bf16"]["img"], (limit, e)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------
def test_tiled_graph_replays_are_bit_identical(M, case):
    o, img, noise, _ = case
    p = M.DiffUIE(**model_kwargs(2), **TINY, use_graph=True, dtype="bf16").eval()
    p.load_state_dict(o.state_dict())
    p.set_latent_tiling(TILE, STRIDE)
    a = [t.cpu() for t in p(img, "ir", noise=noise, return_latents=True)]
    b = [t.cpu() for t in p(img, "ir", noise=noise, return_latents=True)]
    c = [t.cpu() for t in p(img, "ir", noise=noise, return_latents=True)]
    assert len(p._graphs) == 1
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(y, z)
    assert all(math.isfinite(float(x.abs().max())) for x in a)
