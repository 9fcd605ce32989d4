"""bench.py on the device: a plain run prints the headline figure alone, ``--full`` adds what takes runs of its own."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config", "dump_outputs")
FULL_ONLY = ("device_ms_per_step", "kernel_ms_per_step", "end_to_end", "roofline", "roofline_hbm", "configs", "cpu_baseline")


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "2", "--warmup", "1", "--structures", "64", *argv],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--full", "--no-configs", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    for line in (plain, full):
        assert all(k in line for k in HEADLINE), sorted(line)
        assert line["unit"] == "structures/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["steps"] == 2 and line["warmup"] == 1 and line["config"]["structures_per_gpu"] == 64
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(64 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert not any(k in plain for k in FULL_ONLY), sorted(plain)
    assert all(k in full for k in FULL_ONLY), sorted(full)
    assert full["device_ms_per_step"] > 0 and full["kernel_ms_per_step"] and full["roofline"]["kernel"] in full["kernel_ms_per_step"]
    assert full["roofline_hbm"]["stream_copy_gbs"] > 0 and full["end_to_end"]["ms"] > 0
    assert full["configs"] == {} and full["cpu_baseline"] is None
    # both runs time the same seeded batch through the same path: the same outputs
    for name, tol in (("e", 1e-5), ("f", 2e-5), ("s", 2e-4)):
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a.shape == b.shape and np.abs(a - b).max() < tol, name
