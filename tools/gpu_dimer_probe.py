"""Throughput of the device dimer saddle search (DimerSearch.run_batch, chgnet_amd/dimer.py) on one GPU: evaluated structures/s of
1, 8 and 64 searches on the 40-atom 5x1x1 LiMnO2 cell for --steps translations, beside its ceiling -- bare ``ef`` predictions of
batches of the same sizes, graph build included (chg_batch_build_predict, one synchronisation each).  A search stages two structures
for a translation decision and one for a rotation, so the ceiling of a run that made r rotations per search on average predicts
steps + 1 batches of two structures per search and round(r) batches of one: the batches the searches would have formed in lockstep.
The two legs alternate in one process, --repeats times each; one JSON line per leg, search count and repeat, then one summary line
per search count with the range of every leg and of the run-by-run ratio to the ceiling, appended to --out
(profiles/dimer_probe.jsonl).

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


def _start(d, seed):
    """A rattled copy of the cell and a random mode."""
    from chgnet_amd.graph.structure import Lattice, Structure

    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]).make_supercell((5, 1, 1))
    rng = np.random.default_rng(seed)
    lat = s.lattice.matrix
    cart = s.frac_coords @ lat + 0.05 * rng.normal(size=(len(s), 3))
    return Structure(Lattice(lat), s.atomic_numbers, cart @ np.linalg.inv(lat)), rng.normal(size=(len(s), 3))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--searches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dimer_probe.jsonl"))
    args = ap.parse_args()

    from chgnet_amd import CHGNet, CHGNetCalculator, DimerSearch

    W = dict(np.load(os.path.join(REPO, "tests", "golden", "weights_trained_like.npz")))
    lmo = np.load(os.path.join(REPO, "tests", "golden", "case_limno2.npz"))
    model = CHGNet(state_dict=W)
    calc = CHGNetCalculator(model=model)
    eng, conv = model.engine, model.graph_converter
    n = args.steps
    lines = []

    def emit(**kw):
        lines.append(json.dumps({"atoms_each": 40, "steps": n, **kw}))
        print(lines[-1], flush=True)

    for S in args.searches:
        starts = [_start(lmo, 200 + k) for k in range(S)]
        structs = [s for s, _ in starts]
        prep_two = eng.prepare_structures([s for s in structs for _ in range(2)])
        prep_one = eng.prepare_structures(structs)
        last = {"rotations": 0.0}

        def dimer_leg(steps=n):
            searches = [DimerSearch(s, m, calc) for s, m in starts]
            t0 = time.perf_counter()
            res = DimerSearch.run_batch(searches, fmax=1e-6, steps=steps)
            wall = time.perf_counter() - t0
            last["rotations"] = float(np.mean([r["n_rotations"] for r in res]))
            return wall, sum(r["n_evaluated"] for r in res), {"rotations_per_search": last["rotations"], "stopped_early": int(
                sum(r["status"] != "MAX_STEPS" for r in res))}

        def ceiling_leg():
            trials = int(round(last["rotations"]))
            t0 = time.perf_counter()
            for i in range(n + 1 + trials):
                batch = eng.build_prepared(prep_two if i <= n else prep_one, conv.atom_graph_cutoff, conv.bond_graph_cutoff, predict_task="ef")
                eng.synchronize()
                batch.free()
            return time.perf_counter() - t0, S * (2 * (n + 1) + trials), {"trial_batches": trials}

        legs = {"dimer": dimer_leg, "ef_ceiling": ceiling_leg}
        dimer_leg(5)                                      # warm-up: first builds, both instantiations' code objects
        rates = {name: [] for name in legs}
        for rep in range(args.repeats):
            for name, leg in legs.items():
                wall, done, extra = leg()
                rates[name].append(done / wall)
                emit(leg=name, searches=S, repeat=rep, wall_s=wall, structures=done, per_s=done / wall, **extra)
        ratio = [x / c for x, c in zip(rates["dimer"], rates["ef_ceiling"])]
        emit(leg="summary", searches=S, **{f"{name}_per_s": [min(v), max(v)] for name, v in rates.items()},
             dimer_over_ceiling_run_by_run=[min(ratio), max(ratio)])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
