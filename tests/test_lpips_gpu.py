"""LPIPS on the GPU (ops.lpips, unirestore_amd/lpips.py, csrc/lpips.hip): every launcher of its own against the fp64 restatement element by
element (the shared fp32 layers: test_f32net_gpu.py), the whole metric on the end-to-end cases, bit-reproducibility (eager and hipGraph replay), argument checks, and the
caller path (LitUniFIE, cli.validate).  Every bound is 8 x fp32's own measured error (lpips_reference.py: E32_* / *_TOL, kept
honest by test_lpips_cpu.py::test_tolerances_follow_the_measured_fp32_error); the weights are seeded stand-ins - no real LPIPS
weights exist where this runs, so nothing here says anything about published LPIPS values."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import lpips_reference as R
from tiny_cfg import TINY, model_kwargs, randomise_

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_W = {}


def _weights():
    from unirestore_amd import lpips
    if "w" not in _W:
        _W["w"] = lpips.random_weights(R.WEIGHT_SEED)
    return _W["w"]


# ---- the launchers ------------------------------------------------------------------------------------------------------------

def test_prep_matches_fp64_and_writes_nhwc():
    from unirestore_amd import lpips
    x, _ = R.images((2, 3, 33, 47), 8)
    y = lpips.prep(x.cuda()).cpu()
    assert tuple(y.shape) == (2, 33, 47, 3) and y.dtype == torch.float32
    err = float((R.nchw(y).double() - R.scale_input(x)).abs().max())
    print(f"prep: max |err| {err:.2e} (bound {R.PREP_TOL:.2e})")
    assert err <= R.PREP_TOL


LAYER_CASES = {"c64_1px": (2, 64, 1, 1), "c64_15x11": (2, 64, 15, 11), "c384_1px": (1, 384, 1, 1), "c384_15x11": (3, 384, 15, 11)}


def _layer_gpu(fp, ft, lin):
    from unirestore_amd import lpips
    part = lpips.layer(R.nhwc(torch.cat([fp, ft])).cuda(), lin.cuda())
    assert part.dtype == torch.float64 and part.shape == (fp.shape[0], lpips.layer_parts(fp.shape[2] * fp.shape[3]))
    return part.cpu().sum(dim=1) / (fp.shape[2] * fp.shape[3])


@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_lpips_layer_matches_fp64(name):
    n, c, h, w_ = LAYER_CASES[name]
    g = torch.Generator().manual_seed(len(name) + c)
    fp, ft = F.relu(torch.randn(n, c, h, w_, generator=g)), F.relu(torch.randn(n, c, h, w_, generator=g))
    lin = torch.rand(c, generator=g) / c
    if h * w_ > 2:
        fp[0, :, 0, 0] = 0.0                                 # all zero in one image
        fp[0, :, 0, 1] = 0.0                                 # ... and in both
        ft[0, :, 0, 1] = 0.0
    got, want = _layer_gpu(fp, ft, lin), R.layer(fp, ft, lin)
    ratio = float(((got - want).abs() / R.layer_abs(fp, ft, lin)).max())
    print(f"{name}: max |err| / layer_abs {ratio:.2e} (bound {R.LAYER_TOL:.2e})")
    assert bool(torch.isfinite(got).all()) and ratio <= R.LAYER_TOL


def test_lpips_layer_zero_feature_vectors_give_the_references_value():
    """One pixel: zero against a vector gives sum_c lin_c u_c^2 (the eps is added to the norm: 0 / 1e-10 = 0, no NaN); zero against
    zero gives exactly 0."""
    lin = torch.rand(64, generator=torch.Generator().manual_seed(2)) / 64
    f = F.relu(torch.randn(1, 64, 1, 1, generator=torch.Generator().manual_seed(3)))
    z = torch.zeros_like(f)
    for fp, ft in ((z, f), (f, z)):
        got, want = _layer_gpu(fp, ft, lin), R.layer(fp, ft, lin)
        assert float(want) > 0 and abs(float(got - want)) <= R.LAYER_TOL * float(R.layer_abs(fp, ft, lin))
    assert float(_layer_gpu(z, z, lin)) == 0.0 and float(R.layer(z, z, lin)) == 0.0


# ---- the whole metric ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(R.E2E_CASES), ids=["x".join(map(str, s)) for s in R.E2E_CASES])
def test_end_to_end_matches_fp64(shape):
    """Images on the 8-bit grid, random stand-in weights.  lpips(x, x) is exactly 0 (both copies of an image take the same fma
    chains: a GEMM row depends on nothing but its own pixels).  Swapping the arguments gives the SAME BITS: an image's features
    do not depend on its place in the batch, and u_pred - u_tgt only changes sign before it is squared."""
    from unirestore_amd import ops
    pred, tgt = (t.cuda() for t in R.images(shape, R.E2E_CASES[shape]))
    got = ops.lpips(pred, tgt, _weights())
    assert got.dtype == torch.float64 and got.is_cuda and got.shape == (shape[0],)
    want = R.e2e_reference(shape)
    err = float((got.cpu() - want).abs().max())
    print(f"{shape}: lpips {got.cpu().tolist()} max |err| {err:.2e} (bound {R.METRIC_TOL:.2e})")
    assert err <= R.METRIC_TOL
    assert bool((got > 0).all())
    assert torch.equal(ops.lpips(tgt, pred, _weights()), got)
    same = ops.lpips(pred, pred.clone(), _weights())
    assert bool((same == 0).all())


def test_deterministic_eager_and_graph_replay():
    from unirestore_amd import ops
    p, t = (x.cuda() for x in R.images((3, 3, 75, 101), 9))
    w = _weights()
    a = ops.lpips(p, t, w)
    b = ops.lpips(p, t, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.lpips(p, t, w)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = ops.lpips(p, t, w)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a).all())


def test_op_rejects_bad_inputs():
    from unirestore_amd import ops
    w = _weights()
    p, t = (x.cuda() for x in R.images((2, 3, 40, 44), 1))
    bad = [
        (p, t[:1]),                                   # shapes differ
        (p.double(), t.double()),                     # not fp32
        (p.half(), t),
        (p.cpu(), t),                                 # not on the current device
        (p[0], t[0]),                                 # 3-d
        (p.transpose(2, 3), t.transpose(2, 3)),       # not contiguous
        (p[:, :1].contiguous(), t[:, :1].contiguous()),                 # C = 1
        (p[:, :, :30].contiguous(), t[:, :, :30].contiguous()),         # H = 30
        (p[:, :, :, :30].contiguous(), t[:, :, :, :30].contiguous()),   # W = 30
    ]
    for a, b in bad:
        with pytest.raises(ValueError):
            ops.lpips(a, b, w)
    with pytest.raises(ValueError):
        ops.lpips(p, t, None)
    assert ops.lpips(p[:, :, :31, :31].contiguous(), t[:, :, :31, :31].contiguous(), w).shape == (2,)      # 31 is legal


# ---- the caller ---------------------------------------------------------------------------------------------------------------

def _tiny_model():
    import unirestore_amd.modules as M
    from oracle.model import DiffUIE as ODiffUIE
    torch.manual_seed(0)
    o = randomise_(ODiffUIE(**model_kwargs(2), **TINY).eval(), 0)
    p = M.DiffUIE(**model_kwargs(2), **TINY).eval()
    p.load_state_dict(o.state_dict())
    return p


def test_litunifie_accumulates_lpips_and_leaves_the_rest_alone():
    from unirestore_amd import ops, runner
    model = _tiny_model()
    out = {}
    for on in (False, True):
        lit = runner.LitUniFIE(model_kwargs(2), model=model, lpips_weights=_weights() if on else None)
        preds, tgts = [], []
        for b in range(2):                           # two batches: the totals accumulate
            gb = torch.Generator().manual_seed(100 + b)
            hq = torch.rand(2, 3, 96, 80, generator=gb).cuda()
            lq = (hq + 0.1 * torch.randn(hq.shape, generator=gb).cuda()).clamp(0, 1)
            torch.manual_seed(40 + b)                # the forward's noise draws: the same for both instances
            preds.append(lit.validation_step((lq, hq, None, ["a", "b"], "ir"))[-1])
            tgts.append(hq)
        out[on] = (lit, lit.metrics(), preds, tgts)
    (lit0, m0, p0, _), (lit1, m1, p1, t1) = out[False], out[True]
    assert set(m0) == {"val_lq/psnr", "val_lq/ssim", "images"} and set(lit0.totals) == {"psnr", "ssim", "images"}      # today's keys
    assert set(m1) == set(m0) | {"val_lq/lpips"} and set(lit1.totals) == set(lit0.totals) | {"lpips"}
    tot = lit1.totals["lpips"]
    assert torch.is_tensor(tot) and tot.is_cuda and tot.dtype == torch.float64 and tot.ndim == 0
    for a, b in zip(p0, p1):
        assert torch.equal(a, b)                     # the restored images do not depend on the metric
    assert m0["val_lq/psnr"] == m1["val_lq/psnr"] and m0["val_lq/ssim"] == m1["val_lq/ssim"] and m1["images"] == 4
    per_image = torch.cat([ops.lpips(p.contiguous(), t.contiguous(), _weights()) for p, t in zip(p1, t1)])
    assert per_image.shape == (4,)
    want = float(per_image.mean())
    assert math.isfinite(want) and want > 0 and abs(m1["val_lq/lpips"] - want) <= 1e-12 * want
    lit1.update_metrics(p1[0], t1[0])                # the path cli.validate takes
    assert abs(lit1.metrics()["val_lq/lpips"] - float((per_image.sum() + per_image[:2].sum()) / 6)) <= 1e-12 * want


def test_cli_validate_lpips(tmp_path):
    from unirestore_amd import cli, lpips
    asd, lsd = lpips.random_state_dicts(R.WEIGHT_SEED)
    a, l = str(tmp_path / "alexnet.pth"), str(tmp_path / "alex_lin.pth")
    torch.save(asd, a)
    torch.save(lsd, l)
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))
    r0 = cli.validate(cfg, max_batches=2)
    r1 = cli.validate(cfg, max_batches=2, lpips=f"{a},{l}")
    print({k: r1[k] for k in ("val_lq/psnr", "val_lq/ssim", "val_lq/lpips", "images")})
    assert "val_lq/lpips" not in r0 and set(r1) == set(r0) | {"val_lq/lpips"}
    assert math.isfinite(r1["val_lq/lpips"]) and r1["val_lq/lpips"] >= 0
    assert r1["images"] == r0["images"] == 2 and r1["val_lq/psnr"] == r0["val_lq/psnr"] and r1["val_lq/ssim"] == r0["val_lq/ssim"]
