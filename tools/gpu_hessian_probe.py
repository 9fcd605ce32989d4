"""Cost and accuracy of the exact device Hessian (CHGNet.predict_hessian, chg_hessian_vector) against a central-difference
Hessian from batched force evaluations (CHGNet.predict_structure), on the 40-atom LiMnO2 cell (tests/golden/case_s40.npz) and the
256-atom 2x2x2 Li9Co7O16 cell (case_li9co7o16.npz, rattled by 0.02 A as in gpu_md_device_probe.py).  Trained-like golden weights.
One JSON line per cell, appended to --out:

  hessian_s / hvp_per_s     wall time of predict_hessian (3n HVPs) after a warm-up, and HVPs per second
  fd_forces_s               wall time of the 6n force evaluations a central-difference Hessian needs (one predict_structure call)
  max_abs_fd_minus_exact    max|H_fd - H| at delta = 0.01 A and 0.001 A (eV/A^2), with max|H| for scale

Run each cell under its own time limit.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _cell(name: str):
    from chgnet_amd.graph.structure import Lattice, Structure

    d = np.load(os.path.join(REPO, "tests", "golden", f"case_{name}.npz"))
    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"])
    if name != "li9co7o16":
        return s
    s = s.make_supercell((2, 2, 2))
    rng = np.random.default_rng(100)
    cart = s.frac_coords @ s.lattice.matrix + 0.02 * rng.normal(size=(len(s), 3))
    return Structure(s.lattice, s.atomic_numbers, cart @ np.linalg.inv(s.lattice.matrix))


def _displaced(s, atom: int, axis: int, delta: float):
    from chgnet_amd.graph.structure import Structure

    cart = s.frac_coords @ s.lattice.matrix
    cart[atom, axis] += delta
    return Structure(s.lattice, s.atomic_numbers, cart @ np.linalg.inv(s.lattice.matrix))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", choices=("s40", "li9co7o16"), required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hessian_probe.jsonl"))
    args = ap.parse_args()

    from chgnet_amd import CHGNet

    W = dict(np.load(os.path.join(REPO, "tests", "golden", "weights_trained_like.npz")))
    model = CHGNet(state_dict=W)
    s = _cell(args.cell)
    n = len(s.atomic_numbers)
    model.predict_hessian(s)                                                   # warm-up: engine, workspaces
    t0 = time.perf_counter()
    h = model.predict_hessian(s, symmetrize=False)
    t_h = time.perf_counter() - t0
    out = {"cell": args.cell, "atoms": n, "hessian_s": t_h, "hvp_per_s": 3 * n / t_h,
           "max_abs_H": float(np.abs(h).max()), "max_abs_asym": float(np.abs(h - h.T).max()),
           "max_abs_acoustic_sum": float(np.abs(h.reshape(3 * n, n, 3).sum(1)).max())}
    for delta in (0.01, 0.001):
        jobs = [_displaced(s, i, a, sg * delta) for i in range(n) for a in range(3) for sg in (1.0, -1.0)]
        model.predict_structure(jobs[:2], task="ef")
        t0 = time.perf_counter()
        preds = model.predict_structure(jobs, task="ef")
        t_fd = time.perf_counter() - t0
        cols = [-(np.asarray(preds[2 * c]["f"], np.float64) - np.asarray(preds[2 * c + 1]["f"], np.float64)).reshape(-1) / (2 * delta)
                for c in range(3 * n)]
        h_fd = np.stack(cols, axis=1)
        out[f"fd_forces_s_{delta:g}"] = t_fd
        out[f"max_abs_fd_minus_exact_{delta:g}"] = float(np.abs(h_fd - h).max())
    out["force_evals"] = 6 * n
    line = json.dumps(out)
    print(line, flush=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
