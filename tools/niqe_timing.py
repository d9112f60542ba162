"""Time NIQE (`ops.niqe`, csrc/niqe.hip) for one batch on cuda:0 against the fp64 host yardstick (tests/niqe_reference.py) on the
same batch.  Seeded 8-bit images and seeded stand-in parameters (niqe.random_params: no pristine model is needed to time it).

  python tools/niqe_timing.py [--batch 8 --res 512 --reps 200] [--out profiles/niqe_timing.txt]

Prints JSON lines: ops.niqe per call (host clock around the call; it ends in the device-to-host copy of the features, so it is
synchronised), its two halves - the eight launches of niqe.block_features (device events around `reps` back-to-back calls) and
the host algebra of niqe.score - every kernel alone (device events around `reps` back-to-back launches on its own input, with
the bytes it has to move over that time), and the yardstick's wall time for the block features and the score.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def _device_ms(fn, reps):
    """ms per call of `reps` back-to-back calls between two device events (after a warm-up)."""
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("niqe_timing: needs a GPU (nothing is timed on the host in its place)")
    from unirestore_amd import niqe, ops
    import niqe_reference as R
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(3)
    x_host = torch.round(torch.rand(a.batch, 3, a.res, a.res, generator=g) * 255) / 255
    x = x_host.to(dev)
    p = niqe.random_params(0)
    lines = []

    for _ in range(3):
        ops.niqe(x, p)
    calls = []
    for _ in range(max(a.reps // 4, 10)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.niqe(x, p)
        torch.cuda.synchronize()
        calls.append((time.perf_counter() - t0) * 1e3)
    feats = niqe.block_features(x)
    t0 = time.perf_counter()
    for _ in range(10):
        niqe.score(feats, p)
    score_ms = (time.perf_counter() - t0) * 1e3 / 10
    lines.append(json.dumps(dict(what="ops.niqe", batch=a.batch, res=a.res, blocks=feats.shape[1], ms_median=round(statistics.median(calls), 4),
                                 ms_min=round(min(calls), 4), block_features_ms=round(_device_ms(lambda: niqe.block_features(x), a.reps), 4),
                                 score_host_ms=round(score_ms, 4))))

    y = niqe.luma(x)
    m1 = niqe.mscn(y)
    y2 = niqe.halve(y)
    m2 = niqe.mscn(y2)
    mom1, mom2 = niqe.block_moments(m1, 96), niqe.block_moments(m2, 48)
    px, px2 = y.numel(), y2.numel()
    kernels = [("ur_niqe_luma", lambda: niqe.luma(x), 12 * px + 8 * px), ("ur_niqe_mscn (scale 1)", lambda: niqe.mscn(y), 16 * px),
               ("ur_niqe_block_moments (96)", lambda: niqe.block_moments(m1, 96), 8 * px), ("ur_niqe_fit", lambda: niqe.fit(mom1), 240 * mom1.shape[0] * mom1.shape[1]),
               ("ur_niqe_halve", lambda: niqe.halve(y), 8 * px + 8 * px2), ("ur_niqe_mscn (scale 2)", lambda: niqe.mscn(y2), 16 * px2),
               ("ur_niqe_block_moments (48)", lambda: niqe.block_moments(m2, 48), 8 * px2)]
    for name, fn, nbytes in kernels:
        ms = _device_ms(fn, a.reps)
        lines.append(json.dumps(dict(kernel=name, ms=round(ms, 5), bytes=nbytes, GBps=round(nbytes / ms / 1e6, 1),
                                     note="wrapper call: one launch and its output allocation")))

    t0 = time.perf_counter()
    ref = R.pipeline(x_host)
    feat_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = R.score(ref["features"], p.mu, p.cov)
    ref_score_s = time.perf_counter() - t0
    got = ops.niqe(x, p).cpu()
    lines.append(json.dumps(dict(what="host yardstick (tests/niqe_reference.py, fp64 torch on the CPU)", block_features_ms=round(feat_s * 1e3, 1),
                                 score_ms=round(ref_score_s * 1e3, 2), max_rel_score_diff=float(((got - want).abs() / want).max()))))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# python tools/niqe_timing.py --batch {a.batch} --res {a.res} --reps {a.reps}  ({torch.cuda.get_device_name(0)})\n{text}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
