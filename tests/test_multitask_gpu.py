"""DiffUIE.forward_tasks on the GPU: restore once, decode for several tasks.

Op level: the two fan-out kernels against the single-task kernels they generalise (bit for bit) and against fp64.
Module level (tiny model): K = 1 is `forward`, parity with the CPU oracle per task on weights whose tasks MATTER, the work is
really shared (call counts), graphs, chunking, errors, tiling, the config entry point.  Full size: the N = 24 decode.

Tolerances are the existing ones: TOL of test_modules_gpu.py (tiny model vs the fp32 oracle) and the full-size bounds of
test_configs_gpu.py.
"""
import itertools
import math
import os
import sys
import time

import pytest
import torch

from golden_util import rel_l2
from test_modules_gpu import TOL
from tiny_cfg import TINY, model_kwargs, randomise_

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["bf16", "fp16"]
TASKS = ["ir", "cls", "seg"]
# Multipliers of the recipe below.  Prompt std 50 with gate gain 4 separates the tasks on the decode alone (ae.decode of a
# 2 x 3 x 64 x 128 input: 0.14-0.15 pairwise rel-L2), but through the whole forward at 640 x 512 the oracle's three images then differ
# by 1.5e-3 only.  Measured on the CPU oracle (seed 3, the input of _inputs): gain 16 -> 8.0-8.9e-3, 64 -> 3.5-3.9e-2,
# 128 -> 7.1-7.8e-2, 256 -> 0.134-0.149.  256 clears the 10 x fwd_img bar (5.5e-2) by 2.4x; outputs stay within |x| <= 1.4.
PROMPT_STD, GATE_GAIN = 50.0, 256.0


@pytest.fixture(scope="module")
def M():
    import unirestore_amd.modules as m
    return m


@pytest.fixture(scope="module")
def ops():
    from unirestore_amd import ops as o
    yield o
    o.set_dtype("bf16")


def tasks_matter_(model, seed, gain=GATE_GAIN):
    """With randomise_'s default weights the tiny oracle's ir / cls / seg images differ by 4e-7 rel-L2: a decode that ignored
    the task would pass any parity test.  After randomise_: task prompts from N(0, 50^2) (own generator, names in sorted
    order) and the out_gate / t_gate2 weights of every task editor x GATE_GAIN (values and what they give: above)."""
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for name, p in sorted(model.ae.vae.decoder.task_prompts.items()):
            p.copy_((torch.randn(p.shape, generator=g) * PROMPT_STD).to(p.device))
        for ed in model.ae.vae.decoder.task_editors:
            ed.out_gate["0"].weight.mul_(gain)
            ed.t_gate2.weight.mul_(gain)
    return model


def _pair(M, seed=3, steps=2, dtype="bf16", kw=None, use_graph=False):
    from oracle.model import DiffUIE as ODiffUIE
    torch.manual_seed(seed)
    kw = kw or model_kwargs(steps)
    o = randomise_(ODiffUIE(**kw, **TINY).eval(), seed)
    if kw.get("tedit"):
        tasks_matter_(o, seed)
    p = M.DiffUIE(**kw, **TINY, use_graph=use_graph, dtype=dtype).eval()
    p.load_state_dict(o.state_dict())
    return o, p


def _inputs(b=2, seed=7):
    """The 96 x 80 input of test_full_forward_tiny (upscaled to 614 x 512, padded to 640 x 512), b images."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(b, 3, 96, 80, generator=g)
    noise = (torch.randn(b, 4, 80, 64, generator=g), torch.randn(b, 4, 80, 64, generator=g))
    return img, noise


_ORACLE = {}


def _oracle(o, task, img, noise):
    """(image, z0, zt) of the oracle; _pair's oracle is the same model for the same (seed, steps), so results are kept."""
    key = (task, tuple(img.shape), float(img.sum()), float(noise[0].sum()), o.num_inference_steps)
    if key not in _ORACLE:
        _ORACLE[key] = o(img, task, noise=noise, return_latents=True)
    return _ORACLE[key]


# ---- op level ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,k,hw,c", [(2, 1, 35, 64), (1, 3, 63, 8), (3, 2, 17 * 3, 512), (2, 3, 16 * 16, 128), (8, 3, 1, 32),
                                      (1, 8, 77, 24), (2, 11, 9, 16)])
def test_scale_channels_fanout_equals_scale_channels(ops, dtype, b, k, hw, c):
    dt = ops.set_dtype(dtype)
    g = torch.Generator().manual_seed(b * 1000 + k * 100 + c)
    x = torch.randn(b, hw, 1, c, generator=g).to(dt).cuda()
    s = (torch.randn(k * b, c, generator=g) * 3).cuda()
    y = ops.scale_channels_fanout(x, s, k)
    assert y.shape == (k * b, hw, 1, c) and y.dtype == dt
    for j in range(k):
        assert torch.equal(y[j * b:(j + 1) * b], ops.scale_channels(x, s[j * b:(j + 1) * b].contiguous())), (j, "scaled")
    r = ops.scale_channels_fanout(x, None, k)
    for j in range(k):
        assert torch.equal(r[j * b:(j + 1) * b], x), (j, "replicated")
    assert torch.equal(ops.scale_channels_fanout(x, s, k), y)                # a second call: the same bits
    graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ops.scale_channels_fanout(x, s, k)
    torch.cuda.current_stream().wait_stream(st)
    with torch.cuda.graph(graph):
        yg = ops.scale_channels_fanout(x, s, k)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y)                                                 # and a graph replay


def test_scale_channels_fanout_rejects_bad_scale_shape(ops):
    ops.set_dtype("bf16")
    x = torch.zeros(2, 4, 4, 16, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        ops.scale_channels_fanout(x, torch.zeros(2, 16, device="cuda"), 3)


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("d", [16, 128, 512])
@pytest.mark.parametrize("per_row", [False, True])
def test_tfa_prompt_update_fanout(ops, t, d, per_row):
    b, k = 3, 3
    g = torch.Generator().manual_seed(t * 1000 + d + int(per_row))
    pooled = (torch.randn(b, 3, t * d, generator=g) * 2).cuda()
    cond = (torch.randn(k * b if per_row else k, t, d, generator=g) * 5).cuda()
    upd = ops.tfa_prompt_update_fanout(pooled, cond, b, k, per_row)
    assert upd.shape == (k * b, t, d)
    for j, i in itertools.product(range(k), range(b)):
        n = j * b + i
        row = cond[n:n + 1] if per_row else cond[j:j + 1]
        assert torch.equal(upd[n:n + 1], ops.tfa_prompt_update(pooled[i:i + 1].contiguous(), row.contiguous())), (j, i)
    # fp64 restatement of taskeditor.py:80-91 (bound: the one the tfa_prompt_update op test uses)
    p64, c64 = pooled.double().cpu(), cond.double().cpu()
    f, iv, cc = (p64[:, q].view(b, t, d).repeat(k, 1, 1) for q in range(3))
    c_rows = c64 if per_row else c64.repeat_interleave(b, dim=0)
    ref = torch.softmax(f, -1) * c_rows + torch.softmax(iv, -1) * torch.tanh(cc)
    assert rel_l2(upd.double().cpu(), ref) < 1e-5


# ---- module level, tiny model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_graph", [False, True])
def test_one_task_is_forward(M, use_graph, dtype):
    _, p = _pair(M, dtype=dtype, use_graph=use_graph)
    img, noise = _inputs()
    for t, q in itertools.product(("ir", "seg"), (False, True)):
        ref, z0, zt = p(img, t, noise=noise, quantize=q, return_latents=True)
        got, gz0, gzt = p.forward_tasks(img, [t], noise=noise, quantize=q, return_latents=True)
        assert list(got) == [t] and torch.equal(got[t], ref) and torch.equal(gz0, z0) and torch.equal(gzt, zt), (t, q)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_graph", [False, True])
def test_oracle_parity_per_task(M, use_graph, dtype):
    """Measured on MI355X with the sharpened weights (graph on and off alike): bf16 z0 5.62e-3, zt 3.99e-3, images 4.24 / 4.28 / 4.25e-3
    (single-task forward, same weights: 4.24 / 4.30 / 4.28e-3); fp16 7.04e-4, 5.02e-4, 5.34 / 5.41 / 5.38e-4 - inside the existing
    fwd_* bounds, which therefore stand."""
    o, p = _pair(M, dtype=dtype, use_graph=use_graph)
    img, noise = _inputs()
    ref = {t: _oracle(o, t, img, noise) for t in TASKS}
    sep = {(a, b): rel_l2(ref[a][0], ref[b][0]) for a, b in itertools.combinations(TASKS, 2)}
    print(f"oracle images, pairwise rel-L2 between tasks (prompt std {PROMPT_STD}, gate gain {GATE_GAIN}):", sep)
    assert min(sep.values()) > 10 * TOL["bf16"]["fwd_img"], sep            # the tasks matter: a task-blind decode cannot pass
    got, z0, zt = p.forward_tasks(img, TASKS, noise=noise, return_latents=True)
    assert list(got) == TASKS
    tol = TOL[dtype]
    e = dict(z0=rel_l2(z0.cpu(), ref["ir"][1]), zt=rel_l2(zt.cpu(), ref["ir"][2]),
             **{t: rel_l2(got[t].cpu(), ref[t][0]) for t in TASKS})
    single = {t: rel_l2(p(img, t, noise=noise).cpu(), ref[t][0]) for t in TASKS}      # the existing path, same weights
    print(f"forward_tasks rel-L2 vs oracle [{dtype}, graph={use_graph}]:", e, "| single-task forward:", single)
    assert all(got[t].shape == img.shape for t in TASKS)
    assert e["z0"] < tol["fwd_z0"] and e["zt"] < tol["fwd_zt"], e
    assert all(e[t] < tol["fwd_img"] for t in TASKS), e
    if use_graph:                                               # replay with a second image tracks the oracle too
        img2, _ = _inputs(seed=8)
        got2 = p.forward_tasks(img2, TASKS, noise=noise)
        for t in TASKS:
            assert rel_l2(got2[t].cpu(), _oracle(o, t, img2, noise)[0]) < tol["fwd_img"], t


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_tasks_operator_level(M, ops, dtype):
    o, p = _pair(M, seed=2, dtype=dtype)
    ops.set_dtype(dtype)
    g = torch.Generator().manual_seed(6)
    img, noise = torch.rand(2, 3, 64, 128, generator=g), torch.randn(2, 4, 8, 16, generator=g)
    with torch.no_grad():
        oz, ores = o.ae.encode(img, enable_fr=True, noise=noise)
        oimg = {t: o.ae.decode(oz, ores, t) for t in TASKS}
    got = p.ae.decode_tasks(oz, ores, TASKS)
    e = {t: rel_l2(got[t].cpu(), oimg[t]) for t in TASKS}
    print(f"decode_tasks rel-L2 [{dtype}]:", e, "| oracle ir-seg:", rel_l2(oimg["ir"], oimg["seg"]))
    assert list(got) == TASKS and all(v < TOL[dtype]["img"] for v in e.values()), e
    assert torch.equal(p.ae.decode_tasks(oz, ores, ["seg"])["seg"], p.ae.decode(oz, ores, "seg"))
    with pytest.raises(KeyError):
        p.ae.decode_tasks(oz, ores, ["ir", "nope"])


def test_work_is_shared(M, monkeypatch):
    """Eager run with counting wrappers: one encode, exactly `steps` UNet runs, and every conv of a single-task forward is
    issued exactly once - at batch B up to and including each task editor's gate convs and t_gate1, at K*B from t_gate2 on."""
    from unirestore_amd import ops
    steps, b, k = 2, 2, 3
    _, p = _pair(M, steps=steps)
    img, noise = _inputs(b)
    p(img, "ir", noise=noise)                                  # (builds the schedule tables and packs weights: not counted)
    calls = dict(encode=0, unet=0)
    convs = []
    enc, unet, conv = p.ae.encode_run, p.base_model.run, ops.conv

    def count(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapped

    def conv_counted(x, pc, **kw):
        convs.append((id(pc.w), x.shape[0]))
        return conv(x, pc, **kw)
    monkeypatch.setattr(p.ae, "encode_run", count("encode", enc))
    monkeypatch.setattr(p.base_model, "run", count("unet", unet))
    monkeypatch.setattr(ops, "conv", conv_counted)
    p(img, "ir", noise=noise)
    single, calls["encode"], calls["unet"] = list(convs), 0, 0
    convs.clear()
    p.trace_zt = []
    p.forward_tasks(img, TASKS, noise=noise)
    assert calls == dict(encode=1, unet=steps) and len(p.trace_zt) == steps
    assert [w for w, _ in convs] == [w for w, _ in single]                  # the same convs in the same order, each once
    eds = p.ae.vae.decoder.task_editors
    first_fanned = [w for w, _ in convs].index(id(eds[0].t_gate2.packed().w))
    shared_later = {id(pc.w) for ed in eds for pc in (*ed._fused(), ed.t_gate1.packed())}
    for i, ((w, n), (_, n1)) in enumerate(zip(convs, single)):           # (n1: the single-task batch - B, or S*B in the Controller)
        assert n == (n1 if i < first_fanned or w in shared_later else k * n1), (i, n, n1)
    fanned = {id(ed.t_gate2.packed().w) for ed in eds} | {id(ed.conv_out.packed().w) for ed in eds}
    assert all(n == k * b for w, n in convs if w in fanned) and all(n == b for w, n in convs if w in shared_later)
    assert convs[-1][1] == k * b and len(convs) - first_fanned > 20        # the decoder behind the first adapter ran fanned out


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replays_and_keys(M, dtype):
    """A second call is bit-identical; a `forward` between two forward_tasks calls disturbs neither (separate graph keys,
    outputs are copies)."""
    _, p = _pair(M, dtype=dtype, use_graph=True)
    img, noise = _inputs()
    a = p.forward_tasks(img, TASKS, noise=noise)
    keep = {t: v.clone() for t, v in a.items()}
    ir = p(img, "ir", noise=noise)
    ir_keep = ir.clone()
    b = p.forward_tasks(img, TASKS, noise=noise)
    assert all(torch.equal(a[t], keep[t]) and torch.equal(b[t], keep[t]) for t in TASKS)
    assert torch.equal(ir, ir_keep) and torch.equal(p(img, "ir", noise=noise), ir_keep)
    assert len({v.data_ptr() for v in list(a.values()) + list(b.values())}) == 2 * len(TASKS)
    keys = [k[1] for k in p._graphs]
    assert tuple(TASKS) in keys and "ir" in keys


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_graph", [False, True])
def test_chunked_tasks(M, monkeypatch, use_graph, dtype):
    """Chunk bound lowered so that K = 3 splits into 2 + 1: each chunk equals a forward_tasks call on just its tasks."""
    from unirestore_amd import tiling
    o, p = _pair(M, dtype=dtype, use_graph=use_graph)
    img, noise = _inputs()
    b = img.shape[0]
    extent = p.ae.fanout_extent(80, 64)
    per_task = b * extent[0] * extent[1] * extent[2]
    whole, z0, zt = p.forward_tasks(img, TASKS, noise=noise, return_latents=True)
    monkeypatch.setattr(tiling, "TASK_CHUNK_MAX_ELEMS", 2 * per_task + 1)
    assert tiling.task_chunks(b, 3, *extent) == [(0, 2), (2, 1)]
    p._graphs.clear()
    split, sz0, szt = p.forward_tasks(img, TASKS, noise=noise, return_latents=True)
    monkeypatch.undo()
    p._graphs.clear()
    assert tiling.task_chunks(b, 3, *extent) == [(0, 3)]
    assert torch.equal(sz0, z0) and torch.equal(szt, zt)
    first = p.forward_tasks(img, TASKS[:2], noise=noise)
    last = p.forward_tasks(img, TASKS[2:], noise=noise)
    assert list(split) == TASKS
    assert all(torch.equal(split[t], first[t]) for t in TASKS[:2]) and torch.equal(split[TASKS[2]], last[TASKS[2]])
    for t in TASKS:
        assert rel_l2(split[t].cpu(), _oracle(o, t, img, noise)[0]) < TOL[dtype]["fwd_img"], t
        assert whole[t].shape == split[t].shape


def test_errors_and_model_without_task_editor(M):
    _, p = _pair(M)
    img, noise = _inputs(1)
    with pytest.raises(ValueError):
        p.forward_tasks(img, [], noise=noise)
    with pytest.raises(ValueError):
        p.forward_tasks(img, ["ir", "seg", "ir"], noise=noise)
    with pytest.raises(KeyError):
        p.forward_tasks(img, ["ir", "nope"], noise=noise)
    with pytest.raises(TypeError):
        p.forward_tasks(img, "ir", noise=noise)
    with pytest.raises(ValueError):
        p.forward_tasks(img, ["ir"], noise=(noise[0], noise[1][:, :, :8]))
    kw = dict(frenc=dict(type="CFRM"), cnet=dict(type="scedit", num_inference_steps=2), tedit=None)
    for use_graph in (False, True):
        _, q = _pair(M, kw=kw, use_graph=use_graph)
        got = q.forward_tasks(img, ["a", "b"], noise=noise)
        assert list(got) == ["a", "b"] and torch.equal(got["a"], got["b"]) and got["a"].data_ptr() != got["b"].data_ptr()
        assert torch.equal(got["a"], q(img, "anything", noise=noise))


def test_tiled_latent_sampling_composes(M):
    _, p = _pair(M, use_graph=True)
    p.set_latent_tiling(32, 24)
    img, noise = _inputs()                                     # latent 80 x 64: 3 x 3 tiles of 32
    assert p._tile_plan(80, 64) is not None
    ref = p(img, "seg", noise=noise)
    assert torch.equal(p.forward_tasks(img, ["seg"], noise=noise)["seg"], ref)
    got = p.forward_tasks(img, TASKS, noise=noise)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    # the loop is shared; the two decodes differ in batch (6 vs 2) only: each within fwd_img of the exact decode of the same latent
    assert rel_l2(got["seg"].cpu(), ref.cpu()) < 2 * TOL["bf16"]["fwd_img"]


def test_runner_and_cli_validate_tasks(M):
    from unirestore_amd import cli, runner
    _, p = _pair(M, use_graph=True)
    img, noise = _inputs()
    torch.manual_seed(5)
    outs = runner.forward_tasks(p, [img, img], ["ir", "seg"], quantize=True)
    assert len(outs) == 2 and all(list(d) == ["ir", "seg"] for d in outs)
    assert float((outs[0]["ir"] * 255 - (outs[0]["ir"] * 255).round()).abs().max()) < 1e-3
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))
    base = cli.validate(cfg, max_batches=3)
    one = cli.validate(cfg, max_batches=3, tasks=["ir"])
    assert one["val_lq/psnr"] == base["val_lq/psnr"] and one["val_lq/ssim"] == base["val_lq/ssim"] and one["tasks"] == ["ir"]
    assert "tasks" not in base
    three = cli.validate(cfg, max_batches=3, tasks=["seg", "ir", "cls"])
    print("cli validate psnr: forward", base["val_lq/psnr"], "forward_tasks x3", three["val_lq/psnr"], three["images_per_s"])
    assert three["output_finite"] and three["images"] == 3 and three["tasks"] == ["seg", "ir", "cls"] and three["images_per_s"] > 0
    # the "ir" image of a K*B = 3 batch and of a B = 1 batch agree to 16-bit rounding: rms difference d <= the full-size bf16 image
    # bound (images are in [0, 1]) + one 8-bit level, so a PSNR of P dB (rms error 10^(-P/20)) moves by <= 20 log10(1 + d 10^(P/20))
    from test_configs_gpu import TOL as FULL_TOL
    d = FULL_TOL["bf16"][2] + 1.0 / 255
    bound = 20 * math.log10(1 + d * 10 ** (base["val_lq/psnr"] / 20))
    assert abs(three["val_lq/psnr"] - base["val_lq/psnr"]) < bound, (three["val_lq/psnr"], base["val_lq/psnr"], bound)
    with pytest.raises(ValueError, match="ir"):
        cli.validate(cfg, max_batches=1, tasks=["cls", "seg"])


# ---- full size ---------------------------------------------------------------------------------------------------------------
def test_full_size_three_tasks_batch8():
    """Real architecture, random weights, B = 8, 512 x 512, 1 step, three tasks: the N = 24 decode.  Finite, bit-identical on a
    second call, and each task's image agrees with the single-task forward of the same noise under the bound
    test_config1_batch8_one_step applies between a batched run and its own B = 1 runs.  No CPU oracle here (host time).
    Measured on MI355X: 2.9 s for the two dtypes (under 5 s with the sharpened-prompt pass; budget 60 s); rel-L2 0.0 for every
    task and type - the per-image work of the decode kernels does not depend on the batch at this size."""
    sys.path.insert(0, ROOT)
    import bench
    from test_configs_gpu import TOL as FULL_TOL
    t0 = time.time()
    m = bench.build_model(1, torch.device("cuda", 0), 0, 1)
    m.set_num_inference_steps(1)
    g = torch.Generator().manual_seed(61)
    img = torch.rand(8, 3, 512, 512, generator=g)
    noise = (torch.randn(8, 4, 64, 64, generator=g), torch.randn(8, 4, 64, 64, generator=g))
    for dt, lim in (("bf16", FULL_TOL["bf16"][2]), ("fp16", 8e-4)):
        m.set_dtype(dt)
        got, z0, zt = m.forward_tasks(img, TASKS, noise=noise, return_latents=True)
        assert all(v.shape == img.shape and bool(torch.isfinite(v).all()) for v in got.values())
        again = m.forward_tasks(img, TASKS, noise=noise)
        assert all(torch.equal(again[t], got[t]) for t in TASKS)
        for t in TASKS:
            one, oz0, ozt = m(img, t, noise=noise, return_latents=True)
            e = rel_l2(got[t].cpu(), one.cpu())
            print(f"full size B=8 x 3 tasks [{dt}] task {t}: rel-L2 vs single-task forward {e:.2e} (bound {lim:.1e})")
            assert e < lim, (dt, t, e)
            assert torch.equal(oz0, z0) and torch.equal(ozt, zt)
        m._graphs.clear()
    # init_random_ draws the prompts from N(0, 0.02^2): the three tasks then decode to nearly the same image.  Once more (bf16) with
    # the prompts of the recipe at its base strength (std 50, gain 4), so that the agreement above is not one image checked thrice.
    tasks_matter_(m, 0, gain=4.0)
    m.refresh()
    m.set_dtype("bf16")
    got = m.forward_tasks(img, TASKS, noise=noise)
    sep = {(a, b): rel_l2(got[a].cpu(), got[b].cpu()) for a, b in itertools.combinations(TASKS, 2)}
    print("full size, sharpened prompts: pairwise rel-L2 between the tasks' images", sep)
    assert all(bool(torch.isfinite(v).all()) for v in got.values()) and min(sep.values()) > 0.0
    for t in TASKS:
        e = rel_l2(got[t].cpu(), m(img, t, noise=noise).cpu())
        print(f"full size B=8 x 3 tasks [bf16, sharpened prompts] task {t}: rel-L2 vs single-task forward {e:.2e}")
        assert e < FULL_TOL["bf16"][2], (t, e)
    print(f"full-size multi-task test took {time.time() - t0:.1f} s")
