"""bench.py --dump-outputs: what the last timed step returned, written as float32 .npy files under a size cap."""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_step(n_struct=64, n_atoms=40):
    rng = np.random.default_rng(1)
    res = {"e": rng.standard_normal(n_struct).astype(np.float32),
           "f": rng.standard_normal((n_struct * n_atoms, 3)).astype(np.float32),
           "s": rng.standard_normal((n_struct, 3, 3)).astype(np.float32)}
    return res, np.arange(n_struct + 1) * n_atoms


def test_dump_outputs_writes_every_array(tmp_path):
    import bench

    res, off = _fake_step()
    shapes = bench.dump_outputs(str(tmp_path / "out"), res, off)
    assert shapes == {"e": [64], "f": [2560, 3], "s": [64, 3, 3]}
    for k, v in res.items():
        got = np.load(tmp_path / "out" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, v)


def test_dump_outputs_samples_whole_structures_past_the_cap(tmp_path, monkeypatch):
    import bench

    res, off = _fake_step()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8192)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, off)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["e.npy", "f.npy", "s.npy"]
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in files) <= 8192
    e = np.load(tmp_path / "a" / "e.npy")
    keep = np.flatnonzero(np.isin(res["e"], e))          # energies are distinct: they identify the sampled structures
    assert 0 < len(keep) < 64
    assert np.array_equal(np.load(tmp_path / "a" / "f.npy"), res["f"].reshape(64, 40, 3)[keep].reshape(-1, 3))
    assert np.array_equal(np.load(tmp_path / "a" / "s.npy"), res["s"][keep])
    for f in files:                                      # the sample is fixed
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
