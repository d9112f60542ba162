"""NIQE on the GPU: every kernel of csrc/niqe.hip against the fp64 host yardstick (tests/niqe_reference.py) on the cases and at
the tolerances of tests/niqe_cases.py - counts, alpha indices and NaN masks exactly - then ops.niqe, its determinism, its
argument errors, and the evaluator / validate path on the tiny config."""
import math
import os

import pytest
import torch

import niqe_cases as C
import niqe_reference as R
from tiny_cfg import TINY, model_kwargs, randomise_

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(got, want, column_dims, what, tol):
    d = C.column_rel(got.cpu(), want, column_dims)
    print(f"{what}: {d:.3e} (tolerance {tol:.3e})")
    assert d <= tol, (what, d, tol)


def _params():
    from unirestore_amd import niqe
    return niqe.NiqeParams(*C.params_host())


# ---- every kernel against the yardstick, fed with the yardstick's own input -----------------------------------------------------

@pytest.mark.parametrize("case", C.CASES)
def test_kernels_match_the_yardstick(case):
    from unirestore_amd import niqe
    ref = C.reference(case)
    x = C.images(case).cuda()
    y = niqe.luma(x, C.color_space(case))
    assert y.dtype == torch.float64 and torch.equal(y.cpu(), ref["luma"])                      # integral: equal
    for scale, bs in ((1, 96), (2, 48)):
        src = ref["luma"] if scale == 1 else ref["halve"]
        _rel(niqe.mscn(src.cuda()), ref[f"mscn{scale}"], 0, f"{case} mscn{scale}", C.tolerance(case, "mscn"))
        mom = niqe.block_moments(ref[f"mscn{scale}"].cuda(), bs)
        want = ref[f"moments{scale}"]
        assert tuple(mom.shape) == tuple(want.shape)
        assert torch.equal(mom[..., 0].cpu(), want[..., 0]) and torch.equal(mom[..., 2].cpu(), want[..., 2])       # the counts
        _rel(mom, want, 2, f"{case} moments{scale}", C.tolerance(case, "moments"))
        feat, idx = niqe.fit(want.cuda(), bs * bs, want_index=True)
        assert torch.equal(idx.cpu().long(), ref[f"index{scale}"])                                 # the alpha indices
        assert torch.equal(torch.isnan(feat).cpu(), torch.isnan(ref[f"features{scale}"]))
        _rel(feat, ref[f"features{scale}"], 1, f"{case} features{scale}", C.tolerance(case, "features"))
    _rel(niqe.halve(ref["luma"].cuda()), ref["halve"], 0, f"{case} halve", C.tolerance(case, "halve"))
    # and chained: the features of the whole pipeline, the indices through the alpha column
    feats = niqe.block_features(x, C.color_space(case))
    assert tuple(feats.shape) == tuple(ref["features"].shape)
    _rel(feats, ref["features"], 1, f"{case} block_features", C.tolerance(case, "features"))
    alpha = R.tables()[0]
    for scale, cols in ((1, [0, 2, 6, 10, 14]), (2, [18, 20, 24, 28, 32])):
        assert torch.equal(feats[..., cols].cpu(), alpha[ref[f"index{scale}"]])


# ---- fields fed to block_moments directly -----------------------------------------------------------------------------------------

def test_flat_and_one_signed_blocks():
    from unirestore_amd import niqe
    g = torch.Generator().manual_seed(2)
    field = torch.zeros(1, 96, 192, dtype=torch.float64)
    field[0, :, 96:] = 0.5 + torch.rand(96, 96, generator=g, dtype=torch.float64)                # all positive
    mom = niqe.block_moments(field.cuda(), 96)
    want = R.block_moments(field, 96)
    assert torch.equal(mom[0, 0].cpu(), torch.zeros(5, 6, dtype=torch.float64))                  # exact zeros: every count 0
    assert torch.equal(mom[..., 0].cpu(), want[..., 0]) and torch.equal(mom[..., 2].cpu(), want[..., 2])
    assert mom[0, 1, :, 0].tolist() == [0.0] * 5 and mom[0, 1, :, 2].tolist() == [9216.0] * 5
    assert C.column_rel(mom.cpu(), want, 2) <= 1e-12
    feat, idx = niqe.fit(mom, 96 * 96, want_index=True)
    assert bool(torch.isnan(feat).all()) and bool((idx == -1).all())                               # no negative entry anywhere
    rfeat, ridx = R.fit(want, 96 * 96)
    assert bool(torch.isnan(rfeat).all()) and bool((ridx == -1).all())


@pytest.mark.parametrize("bs", (96, 48))
@pytest.mark.parametrize("corner", ((0, 0), (0, -1), (-1, 0), (-1, -1)))
def test_roll_wraps_inside_the_block(bs, corner):
    """All entries positive but one negative corner of block 0: a product field counts a negative entry exactly where the rolled
    block meets that corner - two per shift - and block 1, next to it, none.  A roll that read the neighbour block instead of
    wrapping would lose block 0's and give block 1 some."""
    from unirestore_amd import niqe
    g = torch.Generator().manual_seed(7)
    field = 0.5 + torch.rand(2, bs, 2 * bs, generator=g, dtype=torch.float64)
    r, c = corner[0] % bs, corner[1] % bs
    field[:, r, c] = -field[:, r, c]                                                               # block 0 of both images
    mom = niqe.block_moments(field.cuda(), bs).cpu()
    want = R.block_moments(field, bs)
    assert torch.equal(mom[..., 0], want[..., 0]) and torch.equal(mom[..., 2], want[..., 2])
    assert mom[:, 0, :, 0].tolist() == [[1.0, 2.0, 2.0, 2.0, 2.0]] * 2 and mom[:, 1, :, 0].tolist() == [[0.0] * 5] * 2
    assert C.column_rel(mom, want, 2) <= 1e-12


def test_halve_on_a_ramp_of_mirrored_indices():
    from unirestore_amd import niqe
    yy, xx = torch.meshgrid(torch.arange(6, dtype=torch.float64), torch.arange(10, dtype=torch.float64), indexing="ij")
    ramp = torch.stack([3.0 * yy + 17.0 * xx + 1.0, 255.0 - (yy * xx)])                            # [2, 6, 10]: every output reads a mirrored row
    got = niqe.halve(ramp.cuda()).cpu()
    want = R.halve(ramp)
    assert tuple(got.shape) == (2, 3, 5)
    assert C.column_rel(got, want, 0) <= 1e-12


# ---- the operator -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.CASES)
def test_op_matches_the_yardstick_score(case):
    from unirestore_amd import ops
    mu, cov = C.params_host()
    want = R.score(C.reference(case)["features"], mu, cov)
    x = C.images(case).cuda()
    got = ops.niqe(x, _params(), C.color_space(case))
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (x.shape[0],)
    assert bool(torch.isfinite(want).all()) and bool((want > 0).all())
    _rel(got, want, 0, f"{case} score", C.tolerance(case, "score"))
    assert torch.equal(got, ops.niqe(x, _params(), C.color_space(case)))                           # two calls: the same bits


def test_block_features_graph_replay_is_bit_equal():
    from unirestore_amd import niqe
    x = C.images("ragged").cuda()
    a = niqe.block_features(x)                                                                     # eager first: uploads the tables
    b = niqe.block_features(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        niqe.block_features(x)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = niqe.block_features(x)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a).all())


def test_op_rejects_bad_inputs():
    from unirestore_amd import niqe, ops
    p = _params()
    x = C.images("two_blocks").cuda()
    wide = torch.rand(1, 3, 95, 400).cuda()
    bad = [x.double(), x.half(), x.cpu(), x[0], x.transpose(2, 3), x[:, :2].contiguous(), x[:0],
           wide,                                                                                   # 95 x 400: H < 96
           wide.transpose(2, 3).contiguous(),                                                      # 400 x 95: W < 96
           x[:, :, :, :191].contiguous()]                                                          # 96 x 191: one block
    for t in bad:
        with pytest.raises(ValueError):
            ops.niqe(t, p)
    for t, words in ((wide, "(1, 3, 95, 400)"), (x[:, :, :, :191].contiguous(), "(2, 3, 96, 191)")):
        with pytest.raises(ValueError, match="block") as e:
            ops.niqe(t, p)
        assert words in str(e.value)
    with pytest.raises(ValueError, match="params"):
        ops.niqe(x, None)
    with pytest.raises(ValueError, match="params are on"):
        ops.niqe(x, niqe.NiqeParams(*C.params_host(), dev="cpu"))
    with pytest.raises(ValueError, match="color_space"):
        ops.niqe(x, p, "hsv")
    assert ops.niqe(x, p).shape == (2,)


# ---- the caller ---------------------------------------------------------------------------------------------------------------

def _tiny_model():
    import unirestore_amd.modules as M
    from oracle.model import DiffUIE as ODiffUIE
    torch.manual_seed(0)
    o = randomise_(ODiffUIE(**model_kwargs(2), **TINY).eval(), 0)
    p = M.DiffUIE(**model_kwargs(2), **TINY).eval()
    p.load_state_dict(o.state_dict())
    return p


def _files(tmp_path, n=4, hw=(256, 256)):
    """n textured 8-bit images (a smooth pattern under noise: no flat block) and an `lq hq` list of them."""
    from PIL import Image
    g = torch.Generator().manual_seed(31)
    yy, xx = torch.meshgrid(torch.arange(hw[0], dtype=torch.float32), torch.arange(hw[1], dtype=torch.float32), indexing="ij")
    lines = []
    for i in range(n):
        base = torch.stack([0.5 + 0.25 * torch.sin(yy / (9.0 + i + c) + xx / (14.0 - c)) for c in range(3)])
        img = (base + 0.08 * torch.randn(3, *hw, generator=g)).clamp(0, 1)
        Image.fromarray((img * 255).round().byte().permute(1, 2, 0).numpy()).save(str(tmp_path / f"im{i}.png"))
        lines.append(f"im{i}.png im{i}.png\n")
    lst = tmp_path / "list.txt"
    lst.write_text("".join(lines))
    return str(lst)


def _tiny_cli_cfg(data):
    return dict(seed_everything=3, trainer=dict(accelerator="gpu", devices=1, precision="bf16-mixed"),
                model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=model_kwargs(2))), data=data)


def test_cli_validate_niqe(tmp_path):
    from unirestore_amd import cli, data, niqe
    lst = _files(tmp_path)
    model = _tiny_model()
    mu, cov = C.params_host()
    ppath = str(tmp_path / "pris.npz")
    import numpy as np
    np.savez(ppath, mu_prisparam=mu.numpy()[None], cov_prisparam=cov.numpy())
    args = dict(class_path="unirestore_amd.data.ImageListFiles", init_args=dict(list_file=lst, batch_size=2))
    cfg = _tiny_cli_cfg(args)
    r0 = cli.validate(cfg, model=model)
    r1 = cli.validate(cfg, model=model, niqe=niqe.random_params(3))
    new = {"val_lq/niqe", "val_input/niqe", "niqe_skipped"}
    print({k: r1[k] for k in sorted(new)})
    assert set(r1) == set(r0) | new and not new & set(r0)                                          # without niqe: the parent's keys
    assert r1["images"] == r0["images"] == 4 and r1["val_lq/psnr"] == r0["val_lq/psnr"] and r1["val_lq/ssim"] == r0["val_lq/ssim"]
    assert math.isfinite(r1["val_lq/niqe"]) and math.isfinite(r1["val_input/niqe"]) and r1["niqe_skipped"] == [0, 0]
    # the inputs' score against the yardstick on the same (cropped) inputs, with the parameters read from a file
    r2 = cli.validate(cfg, model=model, niqe=ppath)
    from unirestore_amd import runner
    lqs = torch.cat([runner.crop_tensor(b[0]).cpu() for b in data.ImageListFiles(**args["init_args"]).batches(0, 1, torch.device("cuda"))])
    assert tuple(lqs.shape) == (4, 3, 256, 256)
    want = R.score(R.pipeline(lqs)["features"], mu, cov)
    assert bool(torch.isfinite(want).all())
    print(f"val_input/niqe {r2['val_input/niqe']!r} vs the yardstick's {float(want.mean())!r}")
    assert abs(r2["val_input/niqe"] - float(want.mean())) <= C.FLOOR * float(want.mean()), (r2["val_input/niqe"], float(want.mean()))
    assert r2["niqe_skipped"] == [0, 0] and math.isfinite(r2["val_lq/niqe"])
    # clean files corrupted on the GPU: every entry of the table carries the two keys, and they recombine by image count
    cfg = _tiny_cli_cfg(dict(class_path="unirestore_amd.data.CorruptedImageFiles",
                             init_args=dict(source=lst, corruptions="fog,contrast", severity=3, batch_size=2, seed=2)))
    r3 = cli.validate(cfg, model=model, niqe=ppath)
    table = r3["by_corruption"]
    print(table)
    assert len(table) == 2 and sum(v["images"] for v in table.values()) == r3["images"] == 4
    for v in table.values():
        assert {"niqe", "input/niqe", "psnr", "ssim", "images"} <= set(v) and math.isfinite(v["niqe"]) and math.isfinite(v["input/niqe"])
    if r3["niqe_skipped"] == [0, 0]:
        for side, key in (("", "val_lq/niqe"), ("input/", "val_input/niqe")):
            assert sum(v[f"{side}niqe"] * v["images"] for v in table.values()) / 4 == pytest.approx(r3[key], rel=1e-12)


def test_litunifie_niqe_states_and_skipped_images():
    from unirestore_amd import niqe, ops, runner
    model = _tiny_model()
    p = _params()
    lit = runner.LitUniFIE(model_kwargs(2), model=model, niqe_params=p, eval_mode="NR")
    assert set(lit.totals) == {"psnr", "ssim", "images", "niqe", "niqe_input"}
    for k in lit.NIQE_KEYS:
        assert lit.totals[k].is_cuda and lit.totals[k].dtype == torch.float64 and tuple(lit.totals[k].shape) == (2,)
    x = C.images("unquantised")[:2, :, :, :].cuda()
    flat = x.clone()
    flat[1] = 0.0                                                                                  # a black input: every MSCN entry is exactly 0, no finite score
    before = lit.totals["niqe_input"]
    lit.update_niqe(x, flat)                                                                       # needs no hq
    assert before.tolist() == [0.0, 0.0]                                                           # replaced, not changed in place
    want = ops.niqe(x, p)
    assert lit.totals["niqe"].tolist() == [float(want.sum()), 2.0]
    assert lit.totals["niqe_input"].tolist() == [float(want[0]), 1.0]
    m = lit.metrics()
    assert m["val_lq/niqe"] == float(want.sum()) / 2 and m["val_input/niqe"] == float(want[0]) and m["niqe_skipped"] == [0, 1]
    off = runner.LitUniFIE(model_kwargs(2), model=model)
    off.update_niqe(x, x)                                                                          # off: nothing
    assert set(off.totals) == {"psnr", "ssim", "images"} and set(off.metrics()) == {"val_lq/psnr", "val_lq/ssim", "images"}
    # validation_step with metrics on calls it on both of its paths, hq or not
    lq = torch.nn.functional.interpolate(x, size=(256, 256), mode="bilinear").contiguous()
    for tasks in (None, ["ir"]):
        lit = runner.LitUniFIE(model_kwargs(2), model=model, niqe_params=p)
        lit.validation_step((lq, None, None, ["a", "b"], "ir"), tasks=tasks)
        assert lit.niqe_seen == 2 and sum(lit.metrics()["niqe_skipped"]) + int(lit.totals["niqe"][1]) + int(lit.totals["niqe_input"][1]) == 4
