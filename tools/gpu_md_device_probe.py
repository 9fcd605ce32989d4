"""Throughput of the device molecular dynamics (MolecularDynamics.run_batch, chgnet_amd/dynamics.py) on one GPU: replica-steps/s
of R = 1, 8, 64 replicas of the 256-atom 2x2x2 Li9Co7O16 cell, NVT Berendsen at 300 K, 2 fs, against the host BerendsenNVT
(chgnet_amd/md.py) through CHGNetCalculator on the same machine.  One JSON line per leg, appended to --out.

  --leg device --replicas R   one chg_md handle over R replicas (wall clock of run_batch: create, steps, download)
      --thermostat langevin   the same leg with the Langevin thermostat (BAOAB, 0.01 / fs, noise generated in the step kernel)
      --thermostat nhc        the same leg with Nose-Hoover chains (3 thermostats); with --ensemble npt the isotropic barostat too
                              (task efs: the stress is evaluated every step, so compare it with Berendsen NVT only as an upper bound)
      --cell-dof flexible|axes  with --thermostat nhc --ensemble npt: the flexible-cell barostat (symmetric strain-rate matrix, all six
                              components or the three diagonal ones) instead of the isotropic one; compare it with --cell-dof isotropic
      --repeats K             K timed runs in one process, one JSON line each (their spread is the run-to-run noise)
      --fixed-fraction F      hold every atom whose index is below F n in every replica (fixed_atoms; 0: no mask at all)
      --observe               accumulate observables on the device while the run goes on (MDObservers: every step, 256 MSD / VACF
                              lags, RDF with 200 bins up to 6 A); lines go to profiles/md_observe_probe.jsonl unless --out is given.
                              Compare it with the same leg without the flag: their ratio is the cost of observing
      --observe --transport   the same leg with the transport accumulators on top (collective displacements and currents, the
                              non-Gaussian parameter, van Hove histograms of 64 bins up to 4 A at every 16th lag); lines go to
                              profiles/md_transport_probe.jsonl unless --out is given.  Compare it with --observe alone
      --magmoms               evaluate the site moments every step and keep those of the logged frames (log_magmoms=True: task M plus
                              one gather launch per step); lines go to profiles/md_magmom_probe.jsonl unless --out is given.  Compare
                              it with the plain leg of the same session
      --observe --charge-states  the --observe leg with the charge-state observers on top (Co states split at 0.5 and 1.0 mu_B, O at
                              0.1, a moment histogram of 64 bins up to 2 mu_B, the Co-centred state-resolved RDF with 100 bins up to
                              6 A); same file.  Compare it with --observe alone
  --leg host                  one replica, BerendsenNVT + CHGNetCalculator.calculate per step

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


def _cell(d, seed):
    from chgnet_amd.graph.structure import Structure, Lattice

    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]).make_supercell((2, 2, 2))
    rng = np.random.default_rng(seed)
    cart = s.frac_coords @ s.lattice.matrix + 0.02 * rng.normal(size=(len(s), 3))
    return Structure(s.lattice, s.atomic_numbers, cart @ np.linalg.inv(s.lattice.matrix))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("device", "host"), required=True)
    ap.add_argument("--replicas", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--thermostat", choices=("berendsen", "langevin", "nhc"), default="berendsen")
    ap.add_argument("--ensemble", choices=("nvt", "npt"), default="nvt", help="npt: --thermostat nhc only")
    ap.add_argument("--cell-dof", choices=("isotropic", "flexible", "axes"), default="isotropic", help="--thermostat nhc --ensemble npt only")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--fixed-fraction", type=float, default=0.0)
    ap.add_argument("--observe", action="store_true")
    ap.add_argument("--transport", action="store_true", help="with --observe")
    ap.add_argument("--magmoms", action="store_true")
    ap.add_argument("--charge-states", action="store_true", help="with --observe")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.transport and not args.observe:
        ap.error("--transport belongs to --observe")
    if args.charge_states and not args.observe:
        ap.error("--charge-states belongs to --observe")
    if args.magmoms and args.leg != "device":
        ap.error("--magmoms belongs to --leg device")
    if args.out is None:
        name = ("md_magmom_probe.jsonl" if args.magmoms or args.charge_states else "md_transport_probe.jsonl" if args.transport
                else "md_observe_probe.jsonl" if args.observe else "md_device_probe.jsonl")
        args.out = os.path.join(REPO, "profiles", name)
    if args.observe and args.leg != "device":
        ap.error("--observe belongs to --leg device")
    if args.ensemble == "npt" and args.thermostat != "nhc":
        ap.error("--ensemble npt is probed with --thermostat nhc only")
    if args.cell_dof != "isotropic" and args.ensemble != "npt":
        ap.error("--cell-dof belongs to --thermostat nhc --ensemble npt")

    from chgnet_amd import CHGNet, CHGNetCalculator

    W = dict(np.load(os.path.join(REPO, "tests", "golden", "weights_trained_like.npz")))
    lco = np.load(os.path.join(REPO, "tests", "golden", "case_li9co7o16.npz"))
    calc = CHGNetCalculator(model=CHGNet(state_dict=W))
    out = {"leg": args.leg, "ensemble": args.ensemble, "thermostat": args.thermostat, "atoms_each": 256, "steps": args.steps, "timestep_fs": 2.0}
    lines = []
    if args.leg == "device":
        from chgnet_amd.dynamics import MolecularDynamics

        R = args.replicas
        cells = [_cell(lco, 100 + i) for i in range(R)]
        kw = dict(model=calc, ensemble="nvt", temperature=300.0, starting_temperature=300.0, timestep=2.0, loginterval=args.steps)
        if args.thermostat == "langevin":
            kw.update(thermostat="Langevin", friction=0.01)
        if args.thermostat == "nhc":
            kw.update(ensemble=args.ensemble, thermostat="Nose-Hoover-Chain", chain_length=3)
        if args.ensemble == "npt":
            kw.update(cell_dof=args.cell_dof)
            out.update(cell_dof=args.cell_dof)
        if args.fixed_fraction > 0:
            kw.update(fixed_atoms=[list(range(int(args.fixed_fraction * len(c)))) for c in cells])
            out.update(fixed_fraction=args.fixed_fraction)
        if args.observe:
            from chgnet_amd.observables import MDObservers

            observe = {"sample_interval": 1, "msd_lags": 256, "rdf_bins": 200, "rdf_rmax": 6.0}
            if args.transport:
                observe.update(collective=True, non_gaussian=True, vanhove_bins=64, vanhove_rmax=4.0, vanhove_stride=16)
            if args.charge_states:
                observe.update(magmom_states={27: [0.5, 1.0], 8: [0.1]}, magmom_bins=64, magmom_max=2.0, state_rdf_center=27, state_rdf_bins=100,
                               state_rdf_rmax=6.0)
            kw.update(observers=MDObservers(**observe))
            out.update(observe={k: ({str(z): b for z, b in v.items()} if isinstance(v, dict) else v) for k, v in observe.items()})
        if args.magmoms:
            kw.update(log_magmoms=True)
            out.update(magmoms=True)
        MolecularDynamics.run_batch(cells, 5, seeds=list(range(R)), **kw)          # warm-up: engine creation, first builds
        for rep in range(args.repeats):
            t0 = time.perf_counter()
            res = MolecularDynamics.run_batch(cells, args.steps, seeds=list(range(R)), **kw)
            wall = time.perf_counter() - t0
            out.update(replicas=R, repeat=rep, wall_s=wall, replica_steps_per_s=R * args.steps / wall, steps_per_s=args.steps / wall,
                       nonfinite=int(sum(r["status"] != "RUNNING" for r in res)),
                       final_T_mean=float(np.mean([r["trajectory"].temperatures[-1] for r in res])))
            if args.observe:                     # what a user reads off: Li MSD at the longest lag every replica has reached
                ob = res[0]["observables"]
                reached = int(np.flatnonzero(ob.cnt > 0)[-1])
                out.update(li_msd_A2=float(ob.msd(3)[reached]), li_msd_lag_fs=float(ob.lag_times_fs[reached]),
                           rdf_samples=int(ob.rdf_samples), o_around_co=ob.coordination_number(27, 8, 2.4))
            if args.transport:                   # the Li-Li collective displacement and alpha_2 at that lag, and the van Hove mass inside 4 A
                out.update(li_collective_msd_A2=float(ob.collective_msd(3, 3)[reached]), li_alpha2=float(ob.non_gaussian_parameter(3)[reached]),
                           transport_samples=int(ob.transport_samples),
                           li_vanhove_inside=float(ob.vanhove_hist[0, ob._s(3)].sum() / (ob.cnt[0] * ob.n_per_species[ob._s(3)])))
            if args.charge_states:               # what a user reads off: the Co moments and how the Co atoms spread over their states
                out.update(co_mean_magmom=ob.mean_magmom(27), co_magmom_std=ob.magmom_std(27), co_state_populations=ob.state_populations(27).tolist(),
                           co_transitions=int(ob.transition_counts(27).sum() - np.trace(ob.transition_counts(27))),
                           charge_samples=int(ob.charge.samples))
            if args.magmoms:
                out.update(co_last_magmom_mean=float(np.mean(res[0]["magmoms"][np.asarray(cells[0].atomic_numbers) == 27])),
                           frames_with_magmoms=len(res[0]["trajectory"].magmoms))
            lines.append(json.dumps(out))
    else:
        from chgnet_amd.md import BerendsenNVT

        md = BerendsenNVT(_cell(lco, 100), calc, temperature_K=300.0, timestep_fs=2.0, taut_fs=200.0, seed=0)
        md.run(5)
        r = md.run(args.steps)
        out.update(replicas=1, wall_s=r["wall_s"], replica_steps_per_s=r["steps_per_s"], steps_per_s=r["steps_per_s"])
        lines.append(json.dumps(out))
    print("\n".join(lines), flush=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
