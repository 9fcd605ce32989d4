"""``StructOptimizer`` -- batched structure relaxation on the device (reference chgnet/model/dynamics.py:184-400).

The reference relaxes one structure at a time through ASE: ``FIRE(FrechetCellFilter(atoms)).run(fmax, steps)`` with
``CHGNetCalculator`` evaluating every step.  ASE is absent offline, and one Python round trip per step leaves the batch
engine idle.  Here the whole optimizer runs behind the C-ABI (``chg_relax_*``, include/chgnet_hip.h): every structure
is an independent optimizer whose float64 state stays in HBM, one step kernel advances all active structures at once,
and structures that have stopped drop out of the next graph build.  A batch gives every structure the result it would
get alone.  Two optimizers: ``"FIRE"`` (the default, csrc/kernels_relax.h) and ``"LBFGS"`` (csrc/kernels_lbfgs.h), with
the semantics of ASE's FIRE and LBFGS (no line search) through FrechetCellFilter, with their defaults; tests/relax_ref.py
and tests/lbfgs_ref.py restate them in float64 NumPy / SciPy.

Deviations: a structure whose energy, forces or stress are non-finite even on the engine's wide-range sweep stops with
status ``NONFINITE`` without moving (ASE would carry the NaN on).  L-BFGS skips the history triple of a step whose
curvature ``y . s`` is exactly zero or non-finite (ASE would divide by zero); a triple with ``y . s < 0`` is kept, as
ASE keeps it.

Constraints (DESIGN.md "Constraints"): ``fixed_atoms`` -- atom indices, a bool [n] array or a bool [n, 3] array with True = held --
or, without the keyword, the ``selective_dynamics`` site property (True = free) and the ``FixAtoms`` / ``FixCartesian`` constraints of
an ASE ``Atoms``.  The force on a held component counts as zero everywhere, the reported forces included (ASE's ``get_forces``
returns the masked forces too); with ``relax_cell`` a held atom keeps its fractional coordinates and follows the cell, and a mask
that holds only some components of an atom is refused.
"""

from __future__ import annotations

import contextlib
import ctypes
import io
import pickle
import sys

import numpy as np

from chgnet_amd import _lib
from chgnet_amd.calculator import (GPA_TO_EV_A3, CHGNetCalculator, atoms_to_structure, check_fixed, join_fixed, report_isolated_atoms,
                                   structure_fixed, voigt)
from chgnet_amd.graph.structure import Lattice, Structure

OPTIMIZERS = ("FIRE",)
FILTERS = ("FrechetCellFilter",)
STATUS_NAMES = ("RUNNING", "CONVERGED", "MAX_STEPS", "NONFINITE")
FIRE_DEFAULTS = {"dt": 0.1, "maxstep": 0.2, "dtmax": 1.0, "Nmin": 5, "finc": 1.1, "fdec": 0.5, "astart": 0.1, "fa": 0.99}
LBFGS = "LBFGS"                # the alternative to the default: ASE's LBFGS without line search
LBFGS_DEFAULTS = {"maxstep": 0.2, "memory": 100, "damping": 1.0, "alpha": 70.0}


class TrajectoryObserver:
    """Frames of one relaxation (reference dynamics.py:349-405): total energy (eV), forces (eV/A), stress (Voigt 6, eV/A^3),
    magnetic moments, cartesian positions and cells, one per logged evaluation plus the final one once more."""

    def __init__(self, atomic_numbers) -> None:
        self.atomic_numbers = np.asarray(atomic_numbers)
        self.energies: list[float] = []
        self.forces: list[np.ndarray] = []
        self.stresses: list[np.ndarray] = []
        self.magmoms: list[np.ndarray] = []
        self.atom_positions: list[np.ndarray] = []
        self.cells: list[np.ndarray] = []

    def append(self, energy, forces, stress, magmoms, positions, cell) -> None:
        self.energies.append(float(energy))
        self.forces.append(np.asarray(forces))
        self.stresses.append(np.asarray(stress))
        self.magmoms.append(np.asarray(magmoms))
        self.atom_positions.append(np.asarray(positions))
        self.cells.append(np.asarray(cell))

    def __len__(self) -> int:
        return len(self.energies)

    def save(self, filename: str) -> None:
        """Pickle with the reference's keys."""
        out_pkl = {"energy": self.energies, "forces": self.forces, "stresses": self.stresses, "magmoms": self.magmoms,
                   "atom_positions": self.atom_positions, "cell": self.cells, "atomic_number": self.atomic_numbers}
        with open(filename, "wb") as file:
            pickle.dump(out_pkl, file)


class StructOptimizer:
    """Relax crystal structures with FIRE (the default) or L-BFGS (through the Frechet cell filter) on the device."""

    def __init__(self, model=None, optimizer_class="FIRE", use_device: str | None = None, stress_weight: float = GPA_TO_EV_A3,
                 on_isolated_atoms: str = "warn") -> None:
        name = optimizer_class if isinstance(optimizer_class, str) else getattr(optimizer_class, "__name__", None)
        if name not in OPTIMIZERS and name != LBFGS:
            raise ValueError(f"Optimizer instance not found. Select from {list(OPTIMIZERS)} (default) or {LBFGS!r}")
        self.optimizer_class = name
        if isinstance(model, CHGNetCalculator):
            self.calculator = model
        else:
            self.calculator = CHGNetCalculator(model=model, stress_weight=stress_weight, use_device=use_device,
                                               on_isolated_atoms=on_isolated_atoms)

    @property
    def version(self) -> str | None:
        return self.calculator.model.version

    @property
    def n_params(self) -> int:
        return self.calculator.model.n_params

    # ------------------------------------------------------------------------------------------------------------------------
    def _params(self, fmax, steps, relax_cell, ase_filter, opt_kwargs: dict) -> dict:
        if ase_filter not in FILTERS:
            raise ValueError(f"Invalid {ase_filter=}, must be one of {list(FILTERS)}. ")
        if self.optimizer_class == LBFGS:
            unknown = set(opt_kwargs) - set(LBFGS_DEFAULTS) - {"use_line_search"}
            if unknown:
                raise TypeError(f"LBFGS got unexpected keyword argument(s) {sorted(unknown)}")
            if opt_kwargs.get("use_line_search"):
                raise ValueError("LBFGS(use_line_search=True) is not supported")
            lbfgs = {k: opt_kwargs.get(k, v) for k, v in LBFGS_DEFAULTS.items()}
            if int(lbfgs["memory"]) != lbfgs["memory"] or lbfgs["memory"] < 1:
                raise ValueError(f"LBFGS memory must be a positive integer, got {lbfgs['memory']!r}")
            for k in ("maxstep", "damping", "alpha"):
                if not float(lbfgs[k]) > 0.0:
                    raise ValueError(f"LBFGS {k} must be positive, got {lbfgs[k]!r}")
            fire = {**FIRE_DEFAULTS, "lbfgs": lbfgs}      # the binding passes FIRE's defaults; the engine ignores them
        else:
            unknown = set(opt_kwargs) - set(FIRE_DEFAULTS) - {"downhill_check"}
            if unknown:
                raise TypeError(f"FIRE got unexpected keyword argument(s) {sorted(unknown)}")
            if opt_kwargs.get("downhill_check"):
                raise ValueError("FIRE(downhill_check=True) is not supported")
            fire = {k: opt_kwargs.get(k, v) for k, v in FIRE_DEFAULTS.items()}
        fmax = 0.1 if fmax is None else float(fmax)
        steps = 500 if steps is None else int(steps)
        if fmax < 0 or steps < 0:
            raise ValueError(f"fmax and steps must be non-negative, got {fmax=}, {steps=}")
        return {"fmax": fmax, "steps": steps, "relax_cell": bool(relax_cell), **fire}

    def _structures(self, atoms) -> list[Structure]:
        structs = [atoms_to_structure(a) for a in atoms]
        for s in structs:
            if not hasattr(s, "frac_coords") or len(s) == 0:
                raise ValueError("every structure needs at least one site")
        return structs

    @staticmethod
    def _fixed(structs: list, fixed_atoms, relax_cell: bool) -> list:
        """One mask [n, 3] uint8 (1 = held) or None per structure, checked against the rules of ``chg_relax_set_fixed``."""
        if fixed_atoms is None:
            fixed_atoms = [None] * len(structs)
        elif len(fixed_atoms) != len(structs):
            raise ValueError(f"fixed_atoms has {len(fixed_atoms)} entries for {len(structs)} structures")
        masks = [structure_fixed(s, f) for s, f in zip(structs, fixed_atoms)]
        for i, m in enumerate(masks):
            check_fixed(m, moving_cell=relax_cell, needs_dof=False, what=f"structure {i}")
        return masks

    def _run(self, structures: list, p: dict, frame_every: int | None, verbose: bool, fixed: list | None = None):
        """Relax ``structures`` together: one ``chg_relax`` handle, frames every ``frame_every`` evaluations (None: none).  ``fixed``:
        one mask [n, 3] uint8 or None per structure."""
        model = self.calculator.model
        eng, conv = model.engine, model.graph_converter
        prep = eng.prepare_structures(structures)
        n_at = np.diff(prep.atom_off)
        params = _lib.RelaxParams(
            fmax=p["fmax"], max_steps=p["steps"], relax_cell=int(p["relax_cell"]), dt=p["dt"], maxstep=p["maxstep"], dtmax=p["dtmax"],
            finc=p["finc"], fdec=p["fdec"], astart=p["astart"], fa=p["fa"], nmin=int(p["Nmin"]), exp_cell_factor=0.0,
            r_atom=conv.atom_graph_cutoff, r_bond=conv.bond_graph_cutoff, numerical_tol=1e-8, stress_weight=self.calculator.stress_weight)
        host = prep.host()
        handle = ctypes.c_void_p()
        if "lbfgs" in p:
            lb = p["lbfgs"]
            lbfgs = _lib.LbfgsParams(maxstep=float(lb["maxstep"]), damping=float(lb["damping"]), alpha=float(lb["alpha"]), memory=int(lb["memory"]))
            eng._check(eng.lib.chg_relax_create_lbfgs(eng.handle, ctypes.byref(host), ctypes.byref(params), ctypes.byref(lbfgs), ctypes.byref(handle)))
        else:
            eng._check(eng.lib.chg_relax_create(eng.handle, ctypes.byref(host), ctypes.byref(params), ctypes.byref(handle)))
        B, N = prep.n_struct, int(prep.atom_off[-1])
        mask = join_fixed(fixed, n_at) if fixed is not None else None
        if mask is not None:
            rc = eng.lib.chg_relax_set_fixed(eng.handle, handle, mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
            if rc != 0:
                eng.lib.chg_relax_free(eng.handle, handle)
                eng._check(rc)
        scale = n_at.astype(np.float64) if model.is_intensive else np.ones(B)
        trajs = [TrajectoryObserver(prep.z[prep.atom_off[i]:prep.atom_off[i + 1]]) for i in range(B)] if frame_every else None

        def download() -> dict:
            out = {"frac": np.empty((N, 3)), "lattice": np.empty((B, 3, 3)), "energy": np.empty(B, np.float32),
                   "force": np.empty((N, 3), np.float32), "stress": np.empty((B, 3, 3), np.float32), "magmom": np.empty(N, np.float32),
                   "n_steps": np.empty(B, np.int32), "status": np.empty(B, np.int32)}
            eng._check(eng.lib.chg_relax_download(eng.handle, handle, ctypes.byref(_lib.fill_out(_lib.RelaxOutHost(), out))))
            return out

        def record(d: dict, which) -> None:
            for i in which:
                sl = slice(prep.atom_off[i], prep.atom_off[i + 1])
                trajs[i].append(d["energy"][i] * scale[i], d["force"][sl].astype(np.float64),
                                voigt(d["stress"][i].astype(np.float64)) * self.calculator.stress_weight, d["magmom"][sl].astype(np.float64),
                                d["frac"][sl] @ d["lattice"][i], d["lattice"][i].copy())

        def log(d: dict, active_before: np.ndarray) -> None:
            if not verbose:
                return
            for i in np.flatnonzero(active_before):
                sl = slice(prep.atom_off[i], prep.atom_off[i + 1])
                fmax_now = float(np.sqrt((d["force"][sl].astype(np.float64) ** 2).sum(1).max()))
                last = d["n_steps"][i] - (1 if d["status"][i] == 0 else 0)
                print(f"{self.optimizer_class}[{i}]: {last:4d}  E = {d['energy'][i] * scale[i]:.6f} eV  max|f| = {fmax_now:.6f} eV/A  {STATUS_NAMES[d['status'][i]]}")

        n_active = ctypes.c_int32(B)
        try:
            active = np.ones(B, bool)
            # the first call evaluates the initial configurations (frame 0); every later call takes `interval` more evaluations
            interval = frame_every or max(1, p["steps"] + 1)
            first = True
            while n_active.value > 0:
                eng._check(eng.lib.chg_relax_run(eng.handle, handle, 1 if first else interval, ctypes.byref(n_active)))
                first = False
                if trajs is not None or verbose:
                    d = download()
                    if trajs is not None:
                        # the evaluation just taken is frame number n_steps (stopped) or n_steps - 1 (still running)
                        idx = d["n_steps"] - (d["status"] == 0)
                        record(d, [i for i in np.flatnonzero(active) if idx[i] % frame_every == 0])
                    log(d, active)
                    active = d["status"] == 0
            d = download()
            if trajs is not None:
                record(d, range(B))           # the reference calls obs() once more after run()
        finally:
            eng.lib.chg_relax_free(eng.handle, handle)
        return prep, d, scale, trajs

    def _result(self, prep, d, scale, i: int, assign_magmoms: bool, fixed=None) -> dict:
        sl = slice(prep.atom_off[i], prep.atom_off[i + 1])
        struct = Structure(Lattice(d["lattice"][i]), prep.z[sl].copy(), d["frac"][sl].copy())
        if fixed is not None:
            struct.add_site_property("selective_dynamics", (fixed == 0).tolist())
        if assign_magmoms:
            struct.add_site_property("magmom", [float(m) for m in d["magmom"][sl]])
        return {"final_structure": struct, "energy": float(d["energy"][i] * scale[i]), "forces": d["force"][sl].astype(np.float64),
                "stress": voigt(d["stress"][i].astype(np.float64)) * self.calculator.stress_weight, "magmoms": d["magmom"][sl].astype(np.float64),
                "n_steps": int(d["n_steps"][i]), "status": STATUS_NAMES[d["status"][i]], "converged": bool(d["status"][i] == 1)}

    # ------------------------------------------------------------------------------------------------------------------------
    def relax(self, atoms, *, fmax: float | None = 0.1, steps: int | None = 500, relax_cell: bool | None = True,
              ase_filter: str | None = "FrechetCellFilter", save_path: str | None = None, loginterval: int | None = 1,
              crystal_feas_save_path: str | None = None, verbose: bool = True, assign_magmoms: bool = True, fixed_atoms=None,
              **kwargs) -> dict:
        """Relax one Structure / Atoms until the largest generalized force is below ``fmax`` (reference dynamics.py:246-346).
        ``fixed_atoms``: the atoms or components to hold (module docstring); ``final_structure`` carries them as
        ``selective_dynamics``.  Returns ``{"final_structure", "trajectory"}``."""
        if crystal_feas_save_path is not None:
            raise ValueError("crystal_feas_save_path is not supported by the device relaxation")
        p = self._params(fmax, steps, relax_cell, ase_filter, kwargs)
        loginterval = 1 if loginterval is None else int(loginterval)
        if loginterval < 1:
            raise ValueError(f"{loginterval=} must be positive")
        structs = self._structures([atoms])
        fixed = self._fixed(structs, None if fixed_atoms is None else [fixed_atoms], p["relax_cell"])
        report_isolated_atoms(self.calculator.model, structs)
        stream = sys.stdout if verbose else io.StringIO()
        with contextlib.redirect_stdout(stream):
            prep, d, scale, trajs = self._run(structs, p, loginterval, verbose, fixed)
        if save_path is not None:
            trajs[0].save(save_path)
        res = self._result(prep, d, scale, 0, assign_magmoms, fixed[0])
        return {"final_structure": res["final_structure"], "trajectory": trajs[0]}

    def relax_batch(self, structures, *, fmax: float | None = 0.1, steps: int | None = 500, relax_cell: bool | None = True,
                    ase_filter: str | None = "FrechetCellFilter", loginterval: int | None = 1, verbose: bool = False,
                    assign_magmoms: bool = True, trajectory: bool = False, fixed_atoms=None, **kwargs) -> list[dict]:
        """Relax many structures at once, each an independent optimizer (same result as ``relax`` on it alone).  Returns one
        dict per structure: ``final_structure``, ``energy`` (eV), ``forces``, ``stress`` (Voigt, eV/A^3), ``magmoms``, ``n_steps``,
        ``converged``, ``status`` (and ``trajectory`` when asked).  Chunked by atoms like ``predict_structure``; a chunk whose
        batch does not fit in device memory is split in two and relaxed again.  ``fixed_atoms``: one entry per structure (``None``:
        that structure's own ``selective_dynamics``, or nothing held)."""
        from chgnet_amd.model import _plan_chunks, _run_splitting  # noqa: PLC0415

        p = self._params(fmax, steps, relax_cell, ase_filter, kwargs)
        loginterval = 1 if loginterval is None else int(loginterval)
        if loginterval < 1:
            raise ValueError(f"{loginterval=} must be positive")
        structs = self._structures(list(structures))
        if not structs:
            return []
        model = self.calculator.model
        fixed = self._fixed(structs, None if fixed_atoms is None else list(fixed_atoms), p["relax_cell"])
        items = list(zip(structs, fixed))           # a chunk that is split keeps every structure with its mask

        def run(chunk):
            stream = sys.stdout if verbose else io.StringIO()
            with contextlib.redirect_stdout(stream):
                prep, d, scale, trajs = self._run([s for s, _ in chunk], p, loginterval if trajectory else None, verbose, [m for _, m in chunk])
            out = []
            for i in range(len(chunk)):
                r = self._result(prep, d, scale, i, assign_magmoms, chunk[i][1])
                if trajectory:
                    r["trajectory"] = trajs[i]
                out.append(r)
            return out

        results = []
        for a, b in _plan_chunks([len(s) for s in structs], 1, model.min_atoms_per_batch):
            report_isolated_atoms(model, structs[a:b])
            results.extend(_run_splitting(run, items[a:b]))
        return results
