"""Throughput of the device nudged elastic band (NudgedElasticBand.run_batch, chgnet_amd/neb.py) on one GPU: image-steps/s of
1, 8 and 64 bands of 7 images of the 40-atom 5x1x1 LiMnO2 cell, beside its ceiling -- bare ``ef`` predictions of the same batches,
graph build included (chg_batch_build_predict, one synchronisation each: every image once, then the interior images) -- and beside
``relax_batch(relax_cell=False)`` of the same structures (structure-steps/s).  The three legs alternate in one process, --repeats
times each; one JSON line per leg, band count and repeat, then one summary line per band count with the range of every leg and of
the run-by-run ratio to the ceiling, appended to --out (profiles/neb_probe.jsonl).

An image-step is one structure evaluated for a band: 7 per band at the first evaluation, 5 at every later one.

Weights: the trained-like golden set (tests/golden/weights_trained_like.npz).
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

IMAGES = 7


def _band(d, seed):
    """7 images between two rattled copies of the cell, every interior image rattled a little on top of the line."""
    from chgnet_amd.graph.structure import Lattice, Structure

    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]).make_supercell((5, 1, 1))
    rng = np.random.default_rng(seed)
    lat = s.lattice.matrix
    a = s.frac_coords @ lat + 0.05 * rng.normal(size=(len(s), 3))
    b = a + 0.3 * rng.normal(size=(len(s), 3))
    out = []
    for i in range(IMAGES):
        cart = a + (b - a) * i / (IMAGES - 1) + (0.02 * rng.normal(size=a.shape) if 0 < i < IMAGES - 1 else 0.0)
        out.append(Structure(Lattice(lat), s.atomic_numbers, cart @ np.linalg.inv(lat)))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bands", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "neb_probe.jsonl"))
    args = ap.parse_args()

    from chgnet_amd import CHGNet, CHGNetCalculator, NudgedElasticBand
    from chgnet_amd.relax import StructOptimizer

    W = dict(np.load(os.path.join(REPO, "tests", "golden", "weights_trained_like.npz")))
    lmo = np.load(os.path.join(REPO, "tests", "golden", "case_limno2.npz"))
    model = CHGNet(state_dict=W)
    calc = CHGNetCalculator(model=model)
    opt = StructOptimizer(model=calc)
    eng, conv = model.engine, model.graph_converter
    n = args.steps
    lines = []

    def emit(**kw):
        lines.append(json.dumps({"atoms_each": 40, "images": IMAGES, "steps": n, **kw}))
        print(lines[-1], flush=True)

    for R in args.bands:
        images = [_band(lmo, 100 + k) for k in range(R)]
        structs = [s for band in images for s in band]
        prep_all = eng.prepare_structures(structs)
        prep_int = eng.prepare_structures([s for band in images for s in band[1:-1]])
        work = R * (IMAGES + n * (IMAGES - 2))           # image-steps of a NEB run of n steps (n + 1 evaluations) and of the ceiling

        def neb_leg(steps=n):
            bands = [NudgedElasticBand(band, model=calc) for band in images]
            t0 = time.perf_counter()
            res = NudgedElasticBand.run_batch(bands, fmax=1e-6, steps=steps, climb=True)
            wall = time.perf_counter() - t0
            done = sum(r["n_evaluated"] for r in res)
            return wall, done, {"stopped_early": int(sum(r["status"] != "MAX_STEPS" for r in res))}

        def ceiling_leg():
            t0 = time.perf_counter()
            for i in range(n + 1):
                batch = eng.build_prepared(prep_all if i == 0 else prep_int, conv.atom_graph_cutoff, conv.bond_graph_cutoff, predict_task="ef")
                eng.synchronize()
                batch.free()
            return time.perf_counter() - t0, work, {}

        def relax_leg(steps=n):
            t0 = time.perf_counter()
            res = opt.relax_batch(structs, fmax=1e-6, steps=steps, relax_cell=False)
            wall = time.perf_counter() - t0
            return wall, sum(r["n_steps"] + 1 for r in res), {"stopped_early": int(sum(r["status"] != "MAX_STEPS" for r in res))}

        legs = {"neb": neb_leg, "ef_ceiling": ceiling_leg, "relax_fixed_cell": relax_leg}
        neb_leg(5)                                        # warm-up: first builds, both step kernels
        relax_leg(5)
        rates = {name: [] for name in legs}
        for rep in range(args.repeats):
            for name, leg in legs.items():
                wall, done, extra = leg()
                rates[name].append(done / wall)
                emit(leg=name, bands=R, repeat=rep, wall_s=wall, structures=done, per_s=done / wall, **extra)
        ratio = [x / c for x, c in zip(rates["neb"], rates["ef_ceiling"])]
        emit(leg="summary", bands=R, **{f"{name}_per_s": [min(v), max(v)] for name, v in rates.items()},
             neb_over_ceiling_run_by_run=[min(ratio), max(ratio)])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
