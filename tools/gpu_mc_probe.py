"""Throughput of the device Monte Carlo (MonteCarlo.run_batch, chgnet_amd/montecarlo.py) on one GPU: replica-trials/s of R = 1, 8, 64
replicas of the 256-atom 2x2x2 Li9Co7O16 cell of tools/gpu_md_device_probe.py (Li / Co swaps and displacements, half each, 1000 K),
beside its ceiling -- bare energy-only predictions of the same batch, graph build included (chg_batch_build_predict, CHG_TASK_E, one
synchronisation each) -- and beside the NVT Berendsen replica-steps/s of MolecularDynamics.run_batch (task ef).  The three legs
alternate in one process, --repeats times each; one JSON line per leg, replica count and repeat, appended to --out
(profiles/mc_probe.jsonl).  With --profile one more Monte Carlo run per replica count goes through the engine's profile counters
(device time per label) to show where a trial's time outside the prediction goes.

With --exchange-interval K the probe measures what replica exchange costs instead: every replica count R >= 2 runs as one tempering
ladder (600 K to 1500 K, geometric) with an exchange event after every K-th trial (leg ``mc_exchange``), alternating in the same process
with the same batch at the same temperatures without a ladder (leg ``mc``), --repeats times each, then one summary line per R with the
range of both legs and of their run-by-run ratio.  Default output: profiles/mc_tempering_probe.jsonl.

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


def _cell(d, seed):
    from chgnet_amd.graph.structure import Lattice, Structure

    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]).make_supercell((2, 2, 2))
    rng = np.random.default_rng(seed)
    cart = s.frac_coords @ s.lattice.matrix + 0.02 * rng.normal(size=(len(s), 3))
    return Structure(s.lattice, s.atomic_numbers, cart @ np.linalg.inv(s.lattice.matrix))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--trials", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--exchange-interval", type=int, default=0, help="K > 0: measure replica exchange every K trials against the same leg without")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "mc_tempering_probe.jsonl" if args.exchange_interval > 0 else "mc_probe.jsonl")

    from chgnet_amd import CHGNet, CHGNetCalculator
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.montecarlo import MonteCarlo, temperature_ladder

    W = dict(np.load(os.path.join(REPO, "tests", "golden", "weights_trained_like.npz")))
    lco = np.load(os.path.join(REPO, "tests", "golden", "case_li9co7o16.npz"))
    model = CHGNet(state_dict=W)
    calc = CHGNetCalculator(model=model)
    eng, conv = model.engine, model.graph_converter
    n = args.trials
    lines = []

    def emit(**kw):
        lines.append(json.dumps({"atoms_each": 256, "count": n, **kw}))
        print(lines[-1], flush=True)

    for R in args.replicas:
        cells = [_cell(lco, 100 + i) for i in range(R)]
        mc_kw = dict(model=model, temperatures=1000.0, seeds=list(range(R)), swap_species=("Li", "Co"), swap_probability=0.5,
                     max_displacement=0.1, loginterval=n)
        md_kw = dict(model=calc, ensemble="nvt", temperature=300.0, starting_temperature=300.0, timestep=2.0, loginterval=n)
        prep = eng.prepare_structures(cells)

        def mc_leg(**extra_kw):
            t0 = time.perf_counter()
            res = MonteCarlo.run_batch(cells, n, **{**mc_kw, **extra_kw})
            wall = time.perf_counter() - t0
            acc = [r["counts"][[1, 3]].sum() / n for r in res]
            out = {"nonfinite": int(sum(r["status"] != "RUNNING" for r in res)), "acceptance_mean": float(np.mean(acc))}
            if extra_kw:
                tried, took = sum(r["exchange_attempts"] for r in res), sum(r["exchange_accepts"] for r in res)
                out.update(exchange_interval=args.exchange_interval, exchange_attempts=tried, exchange_accepts=took,
                           round_trips=int(sum(r["round_trips"] for r in res)))
            return wall, out

        if args.exchange_interval > 0:   # the cost of exchanging: the same batch at the same temperatures with and without the ladder
            if R < 2:
                continue
            mc_kw["temperatures"] = temperature_ladder(600.0, 1500.0, R).tolist()
            ladder_kw = dict(ladders=[0] * R, exchange_interval=args.exchange_interval)
            MonteCarlo.run_batch(cells, 5, **mc_kw)                               # warm-up: first builds, graph capture, both kernels
            MonteCarlo.run_batch(cells, 5, **{**mc_kw, **ladder_kw, "exchange_interval": 1})
            rates = {"mc": [], "mc_exchange": []}
            for rep in range(args.repeats):
                for name, kw in (("mc", {}), ("mc_exchange", ladder_kw)):
                    wall, extra = mc_leg(**kw)
                    rates[name].append(R * n / wall)
                    emit(leg=name, replicas=R, repeat=rep, wall_s=wall, per_s=n / wall, replica_per_s=R * n / wall, **extra)
            ratio = [x / p for x, p in zip(rates["mc_exchange"], rates["mc"])]
            emit(leg="summary", replicas=R, exchange_interval=args.exchange_interval,
                 mc_replica_per_s=[min(rates["mc"]), max(rates["mc"])], mc_exchange_replica_per_s=[min(rates["mc_exchange"]), max(rates["mc_exchange"])],
                 ratio_run_by_run=[min(ratio), max(ratio)])
            continue

        def ceiling_leg():
            t0 = time.perf_counter()
            for _ in range(n):
                batch = eng.build_prepared(prep, conv.atom_graph_cutoff, conv.bond_graph_cutoff, predict_task="e")
                eng.synchronize()
                batch.free()
            return time.perf_counter() - t0, {}

        def md_leg():
            t0 = time.perf_counter()
            res = MolecularDynamics.run_batch(cells, n, seeds=list(range(R)), **md_kw)
            return time.perf_counter() - t0, {"nonfinite": int(sum(r["status"] != "RUNNING" for r in res))}

        legs = {"mc": mc_leg, "e_only_ceiling": ceiling_leg, "md_nvt_berendsen": md_leg}
        MonteCarlo.run_batch(cells, 5, **mc_kw)                                   # warm-up: first builds, graph capture
        MolecularDynamics.run_batch(cells, 5, seeds=list(range(R)), **md_kw)
        for rep in range(args.repeats):
            for name, leg in legs.items():
                wall, extra = leg()
                emit(leg=name, replicas=R, repeat=rep, wall_s=wall, per_s=n / wall, replica_per_s=R * n / wall, **extra)
        if args.profile:
            eng.profile(True)
            eng.profile_reset()
            wall, _ = mc_leg()
            prof = eng.profile_read()
            eng.profile(False)
            top = sorted(prof.items(), key=lambda kv: -kv[1][1])
            emit(leg="mc_profiled", replicas=R, wall_s=wall, device_ms_total=sum(v[1] for v in prof.values()),
                 mc_step=prof.get("mc_step"), top=[(k, v[0], round(v[1], 3)) for k, v in top[:12]])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
