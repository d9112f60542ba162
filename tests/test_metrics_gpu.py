"""GPU PSNR / SSIM (ops.image_metrics, csrc/metrics.hip) against the host fp64 yardstick (runner.psnr_per_image, runner.ssim per
image), bit-reproducibility (eager and hipGraph replay), and the `metrics_device="gpu"` caller path (LitUniFIE, cli.validate)."""
import math
import os

import pytest
import torch

from tiny_cfg import TINY, model_kwargs, randomise_

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# fp64 on both sides, only the summation order differs
PSNR_TOL, SSIM_TOL = 1e-9, 1e-10


def _gpu(pred, target, data_range=1.0, win=7):
    from unirestore_amd import ops
    ps, ss = ops.image_metrics(pred.cuda(), target.cuda(), data_range=data_range, win=win)
    assert ps.dtype == ss.dtype == torch.float64 and ps.is_cuda and ss.is_cuda and ps.shape == ss.shape == (pred.shape[0],)
    return ps.cpu(), ss.cpu()


def _cpu(pred, target, data_range=1.0, win=7):
    from unirestore_amd import runner
    ps = runner.psnr_per_image(pred, target, data_range)
    ss = torch.tensor([runner.ssim(pred[i:i + 1], target[i:i + 1], data_range, win) for i in range(pred.shape[0])], dtype=torch.float64)
    return ps, ss


def _check(pred, target, data_range=1.0, win=7):
    gp, gs = _gpu(pred, target, data_range, win)
    cp, cs = _cpu(pred, target, data_range, win)
    dp, ds = float((gp - cp).abs().max()), float((gs - cs).abs().max())
    print(f"{tuple(pred.shape)} win {win} range {data_range}: |dPSNR| {dp:.2e} dB, |dSSIM| {ds:.2e}")
    assert dp <= PSNR_TOL and ds <= SSIM_TOL, (dp, ds)
    return gp, gs


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * scale, torch.rand(shape, generator=g) * scale


CASES = {
    "rgb_67x91": ((3, 3, 67, 91), 7, 1.0),            # odd, not a tile multiple in either direction
    "gray_c1": ((2, 1, 80, 130), 7, 1.0),
    "min_7x7": ((2, 3, 7, 7), 7, 1.0),
    "narrow_tall": ((2, 3, 300, 20), 7, 1.0),        # W below one tile width, H many tiles
    "win11": ((2, 3, 70, 150), 11, 1.0),
    "win3": ((1, 2, 33, 65), 3, 1.0),
    "range255": ((2, 3, 45, 77), 7, 255.0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_cpu_yardstick(name):
    shape, win, dr = CASES[name]
    _check(*_rand(shape, len(name), dr), data_range=dr, win=win)


def test_production_batch_quantised_512():
    """B = 8, 512 x 512, both images on the 8-bit grid - what DiffUIE.forward(quantize=True) returns and the batch carries."""
    g = torch.Generator().manual_seed(7)
    tgt = torch.rand(8, 3, 512, 512, generator=g)
    pred = (tgt + 0.08 * torch.randn(tgt.shape, generator=g)).clamp(0, 1)
    q = lambda x: torch.round(x * 255) / 255
    _check(q(pred), q(tgt))


def test_identical_images():
    x, _ = _rand((2, 3, 40, 50), 3)
    gp, gs = _gpu(x, x.clone())
    assert torch.isinf(gp).all() and (gp > 0).all()
    assert float((gs - 1).abs().max()) <= 1e-12
    cp, _ = _cpu(x, x.clone())
    assert torch.isinf(cp).all()


def test_constant_against_noisy():
    """Flat image: E[x^2] - E[x]^2 cancels to ~0, against c2 = 9e-4 - where an fp32 moment would be ~1e-4 off in SSIM."""
    g = torch.Generator().manual_seed(5)
    flat = torch.full((2, 3, 64, 96), 0.7)
    noisy = (0.7 + 0.05 * torch.randn(flat.shape, generator=g)).clamp(0, 1)
    _check(flat, noisy)
    _check(noisy, flat)
    _check(flat, torch.full_like(flat, 0.3))


def test_deterministic_eager_and_graph_replay():
    from unirestore_amd import ops
    p, t = (x.cuda() for x in _rand((4, 3, 129, 257), 9))
    a = ops.image_metrics(p, t)
    b = ops.image_metrics(p, t)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.image_metrics(p, t)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = ops.image_metrics(p, t)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z)


def test_op_rejects_bad_inputs():
    from unirestore_amd import ops
    p, t = (x.cuda() for x in _rand((2, 3, 20, 24), 1))
    bad = [
        (p, t[:1]),                                   # shapes differ
        (p.double(), t.double()),                     # not fp32
        (p.half(), t),
        (p.cpu(), t),                                 # not on the current device
        (p[0], t[0]),                                 # not 4-d
        (p.transpose(2, 3), t.transpose(2, 3)),       # not contiguous
        (p[:, :, :6], t[:, :, :6].contiguous()),      # H < win (and a non-contiguous view)
        (p[:, :, :6].contiguous(), t[:, :, :6].contiguous()),
    ]
    for a, b in bad:
        with pytest.raises(ValueError):
            ops.image_metrics(a, b)
    for kw in (dict(win=8), dict(win=1), dict(win=25), dict(data_range=0.0), dict(data_range=-1.0)):
        with pytest.raises(ValueError):
            ops.image_metrics(p, t, **kw)


def _tiny_model():
    import unirestore_amd.modules as M
    from oracle.model import DiffUIE as ODiffUIE
    torch.manual_seed(0)
    o = randomise_(ODiffUIE(**model_kwargs(2), **TINY).eval(), 0)
    p = M.DiffUIE(**model_kwargs(2), **TINY).eval()
    p.load_state_dict(o.state_dict())
    return p


def test_validation_step_gpu_metrics_match_cpu():
    from unirestore_amd import runner
    model = _tiny_model()
    out = {}
    for dev in ("cpu", "gpu"):
        lit = runner.LitUniFIE(model_kwargs(2), model=model, metrics_device=dev)
        preds = []
        for b in range(2):                           # two batches: the totals accumulate
            gb = torch.Generator().manual_seed(100 + b)
            hq = torch.rand(2, 3, 96, 80, generator=gb).cuda()
            lq = (hq + 0.1 * torch.randn(hq.shape, generator=gb).cuda()).clamp(0, 1)
            torch.manual_seed(40 + b)                # the forward's noise draws: the same for both instances
            preds.append(lit.validation_step((lq, hq, None, ["a", "b"], "ir"))[-1].cpu())
        if dev == "gpu":
            assert torch.is_tensor(lit.totals["psnr"]) and lit.totals["psnr"].is_cuda and lit.totals["psnr"].dtype == torch.float64
        out[dev] = (lit.metrics(), preds)
    (mc, pc), (mg, pg) = out["cpu"], out["gpu"]
    for a, b in zip(pc, pg):
        assert torch.equal(a, b)                     # the restored images do not depend on where the metrics run
    assert mc["images"] == mg["images"] == 4 and set(mc) == set(mg)
    assert abs(mc["val_lq/psnr"] - mg["val_lq/psnr"]) <= PSNR_TOL and math.isfinite(mg["val_lq/psnr"])
    assert abs(mc["val_lq/ssim"] - mg["val_lq/ssim"]) <= SSIM_TOL


def test_cli_validate_gpu_metrics():
    from unirestore_amd import cli
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))
    rc = cli.validate(cfg, max_batches=2)
    rg = cli.validate(cfg, max_batches=2, metrics_device="gpu")
    print({k: (rc[k], rg[k]) for k in ("val_lq/psnr", "val_lq/ssim", "images")})
    assert set(rc) == set(rg) and rc["images"] == rg["images"] == 2 and rg["output_finite"]
    assert abs(rc["val_lq/psnr"] - rg["val_lq/psnr"]) <= PSNR_TOL
    assert abs(rc["val_lq/ssim"] - rg["val_lq/ssim"]) <= SSIM_TOL
