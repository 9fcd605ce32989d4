"""Cost and accuracy of the device elastic tensor (CHGNet.predict_elastic_tensor, chg_hessian_vector_strain), on the 40-atom LiMnO2
cell (tests/golden/case_s40.npz), the 256-atom 2x2x2 Li9Co7O16 cell (case_li9co7o16.npz, rattled by 0.02 A as in
gpu_hessian_probe.py) and a batch of 1024 rattled 40-atom cells.  Trained-like golden weights.  One JSON line per run, appended to
--out:

  clamped_s / relaxed_s     wall time of predict_elastic_tensor with relaxed_ion False / True, after a warm-up of each
  hessian_s                 wall time of predict_hessian on the same cell (the 3n position columns alone), for the ratio
  max_abs_fd_minus_C_<h>    max|C_fd - C_clamped| (GPa), C_fd from central differences of the engine's own stress
                            (predict_structure, cell strained by +-h along each Voigt unit strain, atoms at fixed fractional
                            coordinates, neighbour list rebuilt), with max|C| for scale
  --cell batch: tensors_per_s, clamped-only tensors per second for 1024 rattled 40-atom cells (6 strain products each)

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

GPA = 160.21766208


def _cell(name: str, rattle: float = 0.0, seed: int = 100):
    from chgnet_amd.graph.structure import Lattice, Structure

    d = np.load(os.path.join(REPO, "tests", "golden", f"case_{name}.npz"))
    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"])
    if name == "li9co7o16":
        s, rattle = s.make_supercell((2, 2, 2)), 0.02
    if not rattle:
        return s
    rng = np.random.default_rng(seed)
    cart = s.frac_coords @ s.lattice.matrix + rattle * rng.normal(size=(len(s), 3))
    return Structure(s.lattice, s.atomic_numbers, cart @ np.linalg.inv(s.lattice.matrix))


def _fd_clamped(model, s, h: float) -> np.ndarray:
    """C_fd[i][j] = (1/V) W_i : d(dE/deps)/deps : W_j by central differences of the engine's stress (GPa)."""
    from chgnet_amd.elastic import voigt_strains
    from chgnet_amd.graph.structure import Structure

    wv = voigt_strains()
    lat = s.lattice.matrix
    vol = abs(float(np.linalg.det(lat)))
    jobs = [Structure(lat @ (np.eye(3) + sg * h * w), s.atomic_numbers, s.frac_coords) for w in wv for sg in (1.0, -1.0)]
    preds = model.predict_structure(jobs, task="efs")
    grads = []
    for k, p in enumerate(preds):
        eps = (1.0 if k % 2 == 0 else -1.0) * h * wv[k // 2]
        g_strained = np.asarray(p["s"], np.float64).reshape(3, 3) * np.linalg.det(lat @ (np.eye(3) + eps)) / GPA
        grads.append(np.linalg.inv(np.eye(3) + eps).T @ g_strained)     # dE/deps of this parameterisation (tests/elastic_ref.py)
    cols = [(grads[2 * j] - grads[2 * j + 1]) / (2 * h) for j in range(6)]
    c = np.array([[float((wv[i] * cols[j]).sum()) for j in range(6)] for i in range(6)]) * GPA / vol
    return 0.5 * (c + c.T)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", choices=("s40", "li9co7o16", "batch"), required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "elastic_probe.jsonl"))
    args = ap.parse_args()

    from chgnet_amd import CHGNet

    W = dict(np.load(os.path.join(REPO, "tests", "golden", "weights_trained_like.npz")))
    model = CHGNet(state_dict=W)
    if args.cell == "batch":
        cells = [_cell("s40", 0.01, seed) for seed in range(1024)]
        model.predict_elastic_tensor(cells[:64], relaxed_ion=False)           # warm-up: engine, workspaces
        t0 = time.perf_counter()
        res = model.predict_elastic_tensor(cells, relaxed_ion=False)
        t = time.perf_counter() - t0
        out = {"cell": "batch_s40_rattled", "structures": len(cells), "atoms": 40, "clamped_s": t, "tensors_per_s": len(cells) / t,
               "hvp_per_s": 6 * len(cells) / t, "max_abs_C": float(max(np.abs(r["clamped_ion"]).max() for r in res))}
    else:
        s = _cell(args.cell)
        n = len(s.atomic_numbers)
        model.predict_elastic_tensor(s, relaxed_ion=False)                   # warm-up
        t0 = time.perf_counter()
        clamped = model.predict_elastic_tensor(s, relaxed_ion=False)
        t_c = time.perf_counter() - t0
        model.predict_elastic_tensor(s)
        t0 = time.perf_counter()
        relaxed = model.predict_elastic_tensor(s)
        t_r = time.perf_counter() - t0
        model.predict_hessian(s)
        t0 = time.perf_counter()
        model.predict_hessian(s)
        t_h = time.perf_counter() - t0
        c = relaxed["clamped_ion"]
        out = {"cell": args.cell, "atoms": n, "clamped_s": t_c, "relaxed_s": t_r, "hessian_s": t_h, "relaxed_over_hessian": t_r / t_h,
               "max_abs_C": float(np.abs(c).max()), "max_abs_C_relaxed": float(np.abs(relaxed["relaxed_ion"]).max()),
               "max_abs_clamped_run_minus_relaxed_run": float(np.abs(clamped["clamped_ion"] - c).max()),
               "max_abs_stress_gpa": float(np.abs(relaxed["stress"]).max()), "min_phonon_eigenvalue": relaxed["min_phonon_eigenvalue"]}
        for h in (1e-3, 1e-4):
            out[f"max_abs_fd_minus_C_{h:g}"] = float(np.abs(_fd_clamped(model, s, h) - c).max())
    line = json.dumps(out)
    print(line, flush=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
