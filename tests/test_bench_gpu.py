"""bench.py's two kinds of run (-m gpu): a plain run prints the headline and none of what --full adds, and the files its
--dump-outputs writes are the ones a --full run writes, bit for bit (its fp16 image comes from one call, not a timed loop)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"fp16", "other_configs", "roofline", "families", "cpu_baseline", "parity_vs_oracle"}


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]          # (libdrm prints a notice line of its own)
    assert lines, (p.stdout[-1000:], p.stderr[-2000:])
    return json.loads(lines[-1])


def test_plain_run_prints_the_headline_and_dumps_what_full_dumps(tmp_path):
    plain, full = tmp_path / "plain", tmp_path / "full"
    v = _bench("--dump-outputs", str(plain))
    assert v["unit"] == "images/s" and v["higher_is_better"] is True and v["dtype"] == "bf16" and v["output_finite"], v
    assert abs(v["value"] - 8 * 1e3 / v["ms_per_step"]) < 1e-6 * v["value"], v
    assert not FULL_ONLY & v.keys(), v
    # --full with every extra but the fp16 loop skipped: the loop whose last step the plain run's restored_fp16 stands for
    f = _bench("--full", "--no-cpu-baseline", "--no-profile", "--no-other-configs", "--dump-outputs", str(full))
    assert f["fp16"]["output_finite"] and f["fp16"]["ms_per_step"] > 0, f
    names = sorted(os.listdir(full))
    assert names == ["restored_bf16.npy", "restored_fp16.npy"] and sorted(os.listdir(plain)) == names
    for n in names:
        a, b = np.load(plain / n), np.load(full / n)
        assert a.shape == (8, 3, 512, 512) and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n
