"""Throughput of the batched relaxation (StructOptimizer, chgnet_amd/relax.py) on one GPU; prints one JSON line per leg.

  --leg batch   1024 strained, rattled 40-atom LiMnO2 cells through relax_batch
  --leg single  one 256-atom Li9Co7O16 cell through relax
  --leg host    the same relaxations through CHGNetCalculator + a host NumPy optimizer (tests/relax_ref.py, tests/lbfgs_ref.py), one
                structure at a time (the first --host-structures of the 1024 cells, then the 256-atom cell)

  --optimizer FIRE (default) or LBFGS: the optimizer_class of StructOptimizer, with its defaults.
  --fixed-fraction F: hold every atom whose index is below F n in every structure of the batch leg (fixed_atoms; 0: no mask at all).

Weights: the trained-like golden set (tests/golden/weights_trained_like.npz).  Run every leg under its own time limit.
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
sys.path.insert(0, os.path.join(REPO, "tests"))


def _structure(d, supercell, rattle, strain, seed):
    from chgnet_amd.graph.structure import Lattice, Structure

    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]).make_supercell(supercell)
    rng = np.random.default_rng(seed)
    lat = s.lattice.matrix @ (np.eye(3) + strain * rng.normal(size=(3, 3)))
    cart = s.frac_coords @ s.lattice.matrix + rattle * rng.normal(size=(len(s), 3))
    return Structure(Lattice(lat), s.atomic_numbers, cart @ np.linalg.inv(lat))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("batch", "single", "host"), required=True)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--fmax", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-structures", type=int, default=8)
    ap.add_argument("--optimizer", choices=("FIRE", "LBFGS"), default="FIRE")
    ap.add_argument("--fixed-fraction", type=float, default=0.0)
    args = ap.parse_args()

    from chgnet_amd import CHGNet
    from chgnet_amd.relax import StructOptimizer

    W = dict(np.load(os.path.join(REPO, "tests", "golden", "weights_trained_like.npz")))
    limno2 = np.load(os.path.join(REPO, "tests", "golden", "case_limno2.npz"))
    lco = np.load(os.path.join(REPO, "tests", "golden", "case_li9co7o16.npz"))
    model = CHGNet(state_dict=W)
    opt = StructOptimizer(model=model, optimizer_class=args.optimizer)
    cells = [_structure(limno2, (5, 1, 1), 0.05, 0.02, 1000 + i) for i in range(args.n)]
    big = _structure(lco, (2, 2, 2), 0.03, 0.01, 7)
    kw = dict(fmax=args.fmax, steps=args.steps)
    opt.relax_batch(cells[:4], fmax=args.fmax, steps=3)          # warm-up: engine creation, first builds
    out = {"leg": args.leg, "optimizer": args.optimizer, "fmax": args.fmax, "max_steps": args.steps}
    if args.leg == "batch":
        if args.fixed_fraction > 0:
            kw.update(fixed_atoms=[list(range(int(args.fixed_fraction * len(c)))) for c in cells])
            out.update(fixed_fraction=args.fixed_fraction)
        t0 = time.perf_counter()
        res = opt.relax_batch(cells, **kw)
        wall = time.perf_counter() - t0
        steps = np.array([r["n_steps"] for r in res])
        out.update(structures=len(cells), atoms_each=len(cells[0]), wall_s=wall, relaxations_per_s=len(cells) / wall,
                   steps_total=int(steps.sum()), structure_steps_per_s=float(steps.sum() / wall), batch_evaluations=int(steps.max() + 1),
                   converged=int(sum(r["converged"] for r in res)), mean_steps=float(steps.mean()),
                   mean_final_energy_per_atom=float(np.mean([r["energy"] / len(c) for r, c in zip(res, cells)])))
    elif args.leg == "single":
        t0 = time.perf_counter()
        res = opt.relax_batch([big], **kw)[0]
        wall = time.perf_counter() - t0
        out.update(atoms=len(big), wall_s=wall, steps=res["n_steps"], status=res["status"], steps_per_s=(res["n_steps"] + 1) / wall,
                   mean_final_energy_per_atom=res["energy"] / len(big))
    else:
        from chgnet_amd import CHGNetCalculator
        from chgnet_amd.graph.structure import Lattice, Structure
        from lbfgs_ref import relax_host_lbfgs
        from relax_ref import relax_host

        host_loop = relax_host_lbfgs if args.optimizer == "LBFGS" else relax_host

        calc = CHGNetCalculator(model=model)

        def run(s):
            def predict(frac, lat):
                calc.calculate(Structure(Lattice(lat), s.atomic_numbers, frac), task="efsm")
                return calc.results["forces"], calc.results["stress"] / calc.stress_weight
            t0 = time.perf_counter()
            r, frames = host_loop(s, predict, **kw)
            return time.perf_counter() - t0, len(frames)

        small = [run(s) for s in cells[:args.host_structures]]
        wall40, evals40 = sum(w for w, _ in small), sum(e for _, e in small)
        w256, e256 = run(big)
        out.update(structures_40=len(small), wall_40_s=wall40, relaxations_per_s_40=len(small) / wall40, evaluations_per_s_40=evals40 / wall40,
                   wall_256_s=w256, evaluations_256=e256, evaluations_per_s_256=e256 / w256)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
