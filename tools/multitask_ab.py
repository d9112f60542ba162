"""A/B of DiffUIE.forward_tasks against one DiffUIE.forward per task (one MI355X, one process, graph replay).

  python tools/multitask_ab.py [--reps 7] [--steps 20] [--dtype bf16] [--only-forward]

Full-size model with bench.py's seeded random weights.  Per case (B = 8 at 512 x 512 with K = 3 and K = 2, B = 1 at 1024 x 1024
with K = 3): warm-up (capture + one replay), then the median of `--reps` timed calls of
  (a) `forward` for each task in turn (K graph replays),
  (b) one `forward_tasks(tasks)`,
alternated rep by rep so that clock drift hits both alike.  Also the decode phase alone (ae.decode_run / decode_run_tasks,
eager, on a fixed latent) at N = K * 8 = 8 / 16 / 24 images.  Prints one JSON line per measurement.
--only-forward measures (a) alone: it also runs on a tree without forward_tasks (the parent commit, for the "forward did
not get slower" comparison on the same box).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

TASKS = ["ir", "cls", "seg"]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--only-forward", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multitask_ab.py needs a GPU: it measures, it does not estimate")
    dev = torch.device("cuda", 0)
    m = bench.build_model(a.steps, dev, 0, 1, dtype=a.dtype)
    from unirestore_amd.modules import resize_pad_plan
    g = torch.Generator().manual_seed(11)
    for b, res, k in ((8, 512, 3), (8, 512, 2), (1, 1024, 3)):
        tasks = TASKS[:k]
        img = torch.rand(b, 3, res, res, generator=g).to(dev)
        noise = tuple(torch.randn(b, 4, res // 8, res // 8, generator=g).to(dev) for _ in range(2))
        run_a = lambda: [m(img, t, noise=noise) for t in tasks]
        run_b = None if a.only_forward else (lambda: m.forward_tasks(img, tasks, noise=noise))
        for fn in (run_a, run_b):
            if fn is not None:
                fn(), fn()                                           # capture, then one warm replay
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(timed(run_a))
            if run_b is not None:
                tb.append(timed(run_b))
        rec = dict(case=f"B={b} {res}x{res} K={k}", steps=a.steps, dtype=a.dtype, reps=a.reps,
                   forward_x_k_ms=round(statistics.median(ta), 2), forward_x_k_minmax=[round(min(ta), 2), round(max(ta), 2)])
        if tb:
            rec.update(forward_tasks_ms=round(statistics.median(tb), 2), forward_tasks_minmax=[round(min(tb), 2), round(max(tb), 2)],
                       ratio=round(statistics.median(tb) / statistics.median(ta), 3))
        rec["peak_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)
        print(json.dumps(rec), flush=True)
        m._graphs.clear()
    # decode phase alone, eager, B = 8 at 512 x 512: N = 8 (decode_run), 16, 24 (decode_run_tasks)
    b, res = 8, 512
    img = torch.rand(b, 3, res, res, generator=g).to(dev)
    n_vae = torch.randn(b, 4, res // 8, res // 8, generator=g).to(dev)
    from unirestore_amd import ops
    ops.set_dtype(a.dtype)
    with torch.no_grad():
        z0, _, mids = m.ae.encode_run(img, n_vae, enable_fr=True, plan=resize_pad_plan(res, res))
        out_plan = ((res, res), (res, res), False)
        cases = [(1, lambda: m.ae.decode_run(z0, mids, "ir", out_plan=out_plan))]
        if not a.only_forward:
            cases += [(k, (lambda k=k: m.ae.decode_run_tasks(z0, mids, TASKS[:k], out_plan=out_plan))) for k in (1, 2, 3)]
        for k, fn in cases:
            fn(), fn()
            ts = [timed(fn) for _ in range(a.reps)]
            print(json.dumps(dict(case=f"decode phase, eager, N={k * b} ({'decode_run' if fn is cases[0][1] else 'decode_run_tasks'})",
                                  dtype=a.dtype, ms=round(statistics.median(ts), 2), minmax=[round(min(ts), 2), round(max(ts), 2)])), flush=True)


if __name__ == "__main__":
    main()
