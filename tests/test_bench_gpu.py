"""bench.py without --full: the headline's steps only, its result line, and --dump-outputs of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(d):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
                        "--height", "128", "--width", "192", "--prealloc-gb", "0", "--dump-outputs", d],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert len(r.stdout.strip().splitlines()) == 1, r.stdout[-2000:]
    return json.loads(r.stdout)


def test_plain_run_line_and_dumped_outputs(tmp_path):
    d = str(tmp_path / "out")
    out = _plain_run(d)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "image-pairs/s" and out["higher_is_better"] is True
    assert out["value"] > 0 and out["ms_per_step"] == pytest.approx(2 * 1e3 / out["value"], rel=2e-3)
    assert out["dtype"].startswith("f32") and out["metric"].startswith("image-pairs/sec")
    # nothing that needs work of its own
    for k in ("secondary", "cpu_baseline", "reference_harness", "forward_only", "without_kernel_timer", "launches_per_step"):
        assert k not in out, k
    assert out["roofline"] is None
    # the dump: the last timed step's losses (== the line's) and outputs; float32, within the budget
    files = sorted(os.listdir(d))
    assert set(out["dumped_outputs"]["elements"]) == {f[:-4] for f in files}
    assert {"loss_total_loss.npy", "flow_0_0.npy", "occ_0_0.npy"} <= set(files), files
    arrs = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 * 2 ** 20
    for k, v in out["loss"].items():
        assert float(arrs["loss_" + k]) == pytest.approx(v, rel=1e-6), k
    # a second run with the same arguments computes the same outputs
    d2 = str(tmp_path / "again")
    _plain_run(d2)
    assert sorted(os.listdir(d2)) == files
    for f in files:
        np.testing.assert_allclose(np.load(os.path.join(d2, f)), arrs[f[:-4]], rtol=1e-6, atol=1e-7, err_msg=f)
