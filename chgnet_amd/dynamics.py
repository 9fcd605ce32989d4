"""``MolecularDynamics`` -- batched molecular dynamics on the device (reference chgnet/model/dynamics.py:433-780).

The reference drives MD through ASE (VelocityVerlet, NVTBerendsen, Inhomogeneous_NPTBerendsen, NPTBerendsen) with
``CHGNetCalculator`` evaluating every step.  ASE is absent offline, and one host round trip per step leaves the engine idle.  Here
the integrator runs behind the C-ABI (``chg_md_*``, include/chgnet_hip.h): every replica's float64 state (positions, momenta,
masses, cell) stays in HBM, and one step kernel (csrc/kernels_md.h) advances all replicas after each device graph build and
prediction.  ``run_batch`` runs replicas of different sizes as one handle; each gets the trajectory it would get alone.
tests/md_ref.py restates the semantics in float64 NumPy.

Beyond the reference: ``ensemble="nvt", thermostat="Langevin"`` samples the canonical ensemble (Berendsen rescaling gives the right
mean temperature and the wrong fluctuations).  The integrator is BAOAB (half kick, half drift, p <- c1 p + sqrt((1 - c1^2) m kB T) xi
with c1 = exp(-friction dt), half drift, evaluation, half kick): one evaluation per step, fixed cell, ``friction`` in 1/fs.  The
noise is generated in the step kernel (csrc/philox.h, Philox4x32-10 + Box-Muller) as a pure function of (``thermostat_seed``, atom
index, steps completed in the device handle): nothing random is stored, so ``run(10); run(10)`` equals ``run(20)`` and a replica of
``run_batch`` gets the trajectory it would get alone.  ``set_atoms`` opens a new handle and so restarts the stream from step 0.  The
centre-of-mass momentum is removed after every noise step (mass-weighted, 3 degrees of freedom), while the reported temperature
stays ``T = 2 Ekin / (3 n kB)`` as for the other ensembles: it equilibrates at ``temperature * (n - 1) / n``.
tests/langevin_ref.py restates integrator and noise.

Also beyond the reference: ``thermostat="Nose-Hoover-Chain"`` is the deterministic canonical thermostat (``ensemble="nvt"``) and the
barostat that samples the isothermal-isobaric ensemble (``ensemble="npt"``; every Berendsen barostat only relaxes the mean pressure).
The integrator is Martyna-Tobias-Klein with Nose-Hoover chains of ``chain_length`` (1-4, default 3) thermostats on the particles
and, for NPT, on the barostat, in the reversible second-order factorisation of Tuckerman et al., J. Phys. A 39 (2006) 5629: one
evaluation per step, isotropic cell scaling that keeps any cell shape, ``taut`` / ``taup`` (fs) as the thermostat and barostat
periods, scalar ``pressure`` (GPa); ``bulk_modulus`` is not needed.  ``MDTrajectory.conserved`` holds the conserved extended energy
(eV) of every frame and ``thermostat_state`` the chain and barostat variables, which stay in the device handle, so ``run(10);
run(10)`` equals ``run(20)``; ``set_atoms`` opens a new handle with zeroed chains.  The centre-of-mass momentum is removed once,
mass-weighted, when the atoms are set, and never per step (the equations conserve it; N_f = 3 (n - 1)), while the reported
temperature stays ``T = 2 Ekin / (3 n kB)``: it equilibrates at ``temperature * (n - 1) / n``.  ``temperature <= 0`` and a
one-atom structure are refused.  tests/nhc_ref.py restates the integrator.  This is not ASE's ``NPT`` class, which the reference
calls "Nose-Hoover" (Melchionna leap-frog: upper-triangular cells only, conserved quantity of first order in the time step).

``cell_dof`` (``ensemble="npt", thermostat="Nose-Hoover-Chain"`` only) chooses what of the cell the barostat moves.  ``"isotropic"``
(default) is the scaling above.  ``"flexible"`` is the fully flexible form of the same equations: a symmetric strain-rate matrix
``Vg`` takes the place of ``veps``, all six components move, so lengths and angles follow the stress (layered/spinel transformations,
anisotropic expansion).  ``"axes"`` frees only the three cartesian diagonal components: independent axis lengths, angles kept for an
orthogonal cell -- the sampling counterpart of ``"Berendsen_inhomogeneous"``.  With d_b = 6 or 3 free components, W_g = W / 3 and
barostat chain masses d_b kT taup^2, kT taup^2, ...: ``Vg_ab += dt/2 (sum p_a p_b / m + (sum p^2/m / N_f - P V) delta_ab - V sym(sigma)_ab) / W_g``,
``p <- (p E + dt/2 F) E`` with ``E = exp(-(Vg + tr Vg / N_f) dt/4)``, ``r <- (r E + dt p/m) E`` with ``E = exp(Vg dt/2)``, ``h <- h exp(Vg dt)``
(3x3 matrix exponentials; rows of h are the lattice vectors).  ``pressure`` stays a scalar: an anisotropic target stress needs a
reference cell.  ``thermostat_state["vg"]`` is the [3, 3] strain-rate matrix (``veps`` stays 0); it continues over split runs like the
chains.  Held atoms follow the cell map ``r <- r exp(Vg dt)``.  tests/nhc_flex_ref.py restates the integrator.

Constraints (DESIGN.md "Constraints"): ``fixed_atoms`` -- atom indices, a bool [n] array or a bool [n, 3] array with True = held --
or, without the keyword, the ``selective_dynamics`` site property (True = free) and the ``FixAtoms`` / ``FixCartesian`` constraints of
an ASE ``Atoms``.  Held components get no force and no momentum (the initial momenta are masked after they are drawn, as ASE's
``set_momenta`` does), so they never drift; under a moving cell held atoms scale with it, and a mask that holds only some components
of an atom is refused there.  A replica that holds at least one component has ``dof`` = its free components: the reported
temperature is ``2 Ekin / (dof kB)`` (ASE >= 3.23), the Berendsen thermostat uses it, the Nose-Hoover chains take ``N_f = dof`` and
the one-time centre-of-mass removal is skipped (a pinned atom breaks momentum conservation).  A replica with nothing free is refused
except in NVE.

Observables (DESIGN.md "MD observables"): ``observers=MDObservers(...)`` (chgnet_amd/observables.py) accumulates the mean-squared
displacement and velocity autocorrelation per species and the pair histogram of the radial distribution function on the device
while the run goes on, whatever ``loginterval`` is; ``md.observables`` (``"observables"`` in the results of ``run_batch``) downloads
the sums as an ``MDObservables``.  ``set_atoms`` opens a new handle and so starts them from zero.  Without observers nothing changes.  The transport options of
``MDObservers`` (``collective``, ``non_gaussian``, ``vanhove_bins``) travel with the same object: ionic conductivity, Haven ratio,
non-Gaussian parameter and the self part of the van Hove function come out of the same ``MDObservables``.

Out of scope, refused with ``ValueError``: ``thermostat="Nose-Hoover"`` (ASE ``NPT``; use ``"Nose-Hoover-Chain"``), and NPT with a
Berendsen barostat without ``bulk_modulus`` (the reference then fits an equation of state).  Deviations from the reference:
  - ``starting_temperature`` draws from a seeded numpy ``Generator`` (``seed``), not ASE's global RNG: same distribution,
    different draws;
  - a replica whose energy or forces are non-finite even on the engine's wide-range sweep stops with status ``NONFINITE`` and
    its state untouched (ASE carries the NaN on);
  - there is no ASE ``.traj`` writer: ``trajectory`` names a pickle with ``TrajectoryObserver``'s keys plus ``momenta`` and
    ``temperature``; ``magmoms`` stay empty unless ``log_magmoms=True`` (the step evaluates energy and forces, plus stress for
    NPT; with ``log_magmoms`` or charge-state observers also the site moments).

Charge-informed MD (DESIGN.md "MD observables -> Charge states"): ``log_magmoms=True`` evaluates the site magnetic moments with every
step (``chg_md_set_magmoms``), puts one float32 ``[n]`` array per frame into ``MDTrajectory.magmoms`` (the reference's ``"magmoms"`` key
of the pickled trajectory) and keeps ``md.magmoms``, the moments of the last completed step.  The charge-state keywords of
``MDObservers`` (``magmom_states``, ``magmom_bins``, ``state_rdf_bins``) classify and accumulate them on the device at every sample,
with or without ``log_magmoms``.
"""

from __future__ import annotations

import ctypes
import pickle
import sys

import numpy as np

from chgnet_amd import _lib
from chgnet_amd.calculator import (CHGNetCalculator, atoms_to_structure, check_fixed, join_fixed, report_isolated_atoms, structure_fixed,
                                   voigt)
from chgnet_amd.graph.structure import Lattice, Structure
from chgnet_amd.observables import MDObservables, MDObservers
from chgnet_amd.observables import download as download_observables
from chgnet_amd.observables import ChargeStateSums, download_charge, download_transport

# ase.units (CODATA 2014)
_E, _AMU, _KB_J = 1.6021766208e-19, 1.660539040e-27, 1.38064852e-23
FS = 1e-15 * (1e10 * np.sqrt(_E / _AMU))   # units.fs = 1e-15 * second
KB = _KB_J / _E                             # units.kB, eV/K
GPA = 1e9 * ((1 / _E) / 1e30)               # units.GPa = 1e9 * Pascal, eV/A^3

ENSEMBLE_CODES = {"nve": 0, "nvt": 1, "npt_inhomogeneous": 2, "npt_berendsen": 3, "nvt_langevin": 4, "nvt_nhc": 5, "npt_nhc": 6}
NHC_KINDS = ("nvt_nhc", "npt_nhc")
CELL_DOFS = ("isotropic", "flexible", "axes")    # thermostat="Nose-Hoover-Chain", ensemble="npt"; the last two: chg_md_create_nhc_flex
STATUS_NAMES = ("RUNNING", "NONFINITE")
_U64 = (1 << 64) - 1

# ase.data.atomic_masses (IUPAC 2016 standard atomic weights), Z = 0..94
ATOMIC_MASSES = np.array([
    1.0, 1.008, 4.002602, 6.94, 9.0121831, 10.81, 12.011, 14.007, 15.999, 18.998403163, 20.1797, 22.98976928, 24.305, 26.9815385,
    28.085, 30.973761998, 32.06, 35.45, 39.948, 39.0983, 40.078, 44.955908, 47.867, 50.9415, 51.9961, 54.938044, 55.845, 58.933194,
    58.6934, 63.546, 65.38, 69.723, 72.630, 74.921595, 78.971, 79.904, 83.798, 85.4678, 87.62, 88.90584, 91.224, 92.90637, 95.95,
    97.90721, 101.07, 102.90550, 106.42, 107.8682, 112.414, 114.818, 118.710, 121.760, 127.60, 126.90447, 131.293, 132.90545196,
    137.327, 138.90547, 140.116, 140.90766, 144.242, 144.91276, 150.36, 151.964, 157.25, 158.92535, 162.500, 164.93033, 167.259,
    168.93422, 173.054, 174.9668, 178.49, 180.94788, 183.84, 186.207, 190.23, 192.217, 195.084, 196.966569, 200.592, 204.38,
    207.2, 208.98040, 208.98243, 209.98715, 222.01758, 223.01974, 226.02541, 227.02775, 232.0377, 231.03588, 238.02891,
    237.04817, 244.06421])


def maxwell_boltzmann(masses: np.ndarray, temperature_k: float, rng: np.random.Generator) -> np.ndarray:
    """ASE MaxwellBoltzmannDistribution(force_temp=True) then Stationary (mass-weighted, temperature preserved): momenta [n, 3]."""
    masses = np.asarray(masses, np.float64)
    kt = KB * temperature_k
    p = rng.standard_normal((len(masses), 3)) * np.sqrt(masses * kt)[:, None]

    def force_temperature(p, target_kt):
        cur = float(np.vdot(p, p / masses[:, None])) / (3 * len(masses))
        return p * np.sqrt(target_kt / cur) if cur > 0 else p

    p = force_temperature(p, kt)
    t0_kt = float(np.vdot(p, p / masses[:, None])) / (3 * len(masses))
    p = p - (p.sum(0) / masses.sum()) * masses[:, None]
    return force_temperature(p, t0_kt)


class MDTrajectory:
    """Frames of one replica, every ``loginterval`` steps from step 0: potential energy (eV), forces (eV/A), stress (Voigt, eV/A^3,
    when evaluated), cartesian positions, cells, momenta and temperature (K)."""

    def __init__(self, atomic_numbers) -> None:
        self.atomic_numbers = np.asarray(atomic_numbers)
        self.steps: list[int] = []
        self.energies: list[float] = []
        self.kinetic_energies: list[float] = []
        self.forces: list[np.ndarray] = []
        self.stresses: list[np.ndarray] = []
        self.magmoms: list[np.ndarray] = []
        self.atom_positions: list[np.ndarray] = []
        self.cells: list[np.ndarray] = []
        self.momenta: list[np.ndarray] = []
        self.temperatures: list[float] = []
        self.crystal_feas: list[np.ndarray] = []
        self.conserved: list[float] = []          # thermostat="Nose-Hoover-Chain": the conserved extended energy (eV) of every frame

    def __len__(self) -> int:
        return len(self.energies)

    def save(self, filename: str) -> None:
        """Pickle with TrajectoryObserver's keys (reference dynamics.py:389-405) plus momenta and temperature (and ``conserved``
        when the ensemble has one)."""
        out_pkl = {"energy": self.energies, "forces": self.forces, "stresses": self.stresses, "magmoms": self.magmoms,
                   "atom_positions": self.atom_positions, "cell": self.cells, "atomic_number": self.atomic_numbers,
                   "momenta": self.momenta, "temperature": self.temperatures}
        if self.conserved:
            out_pkl["conserved"] = self.conserved
        with open(filename, "wb") as file:
            pickle.dump(out_pkl, file)


class MDLogger:
    """ASE MDLogger's text format (header, then time in ps, Etot, Epot, Ekin in eV and T in K per logged step)."""

    def __init__(self, logfile: str, natoms: int) -> None:
        self.logfile = logfile
        digits = 4 if natoms <= 100 else 3 if natoms <= 1000 else 2
        self.hdr = "%-9s " % ("Time[ps]",) + "%12s %12s %12s  %6s" % ("Etot[eV]", "Epot[eV]", "Ekin[eV]", "T[K]")
        self.fmt = "%-10.4f " + 3 * ("%%12.%df " % (digits,)) + " %6.1f\n"
        self._write(self.hdr + "\n")

    def _write(self, text: str) -> None:
        if self.logfile == "-":
            sys.stdout.write(text)
            return
        with open(self.logfile, "a") as fh:
            fh.write(text)

    def rows(self, times_ps, epot, ekin, temp) -> None:
        self._write("".join(self.fmt % (t, e + k, e, k, tt) for t, e, k, tt in zip(times_ps, epot, ekin, temp)))


def _resolve(ensemble: str, thermostat: str, bulk_modulus) -> str:
    """Reference dynamics.py:598-760 -> the integrator name used here; out-of-scope choices raise ValueError."""
    ens = ensemble.lower()
    th = thermostat.lower()
    if ens == "nve":
        return "nve"
    if ens not in ("nvt", "npt"):
        raise ValueError(f"Ensemble {ensemble!r} not supported, choose in 'nve', 'nvt', 'npt'")
    if th == "nose-hoover":
        raise ValueError("thermostat='Nose-Hoover' (ASE NPT, upper-triangular cells) is not supported by the device MD; use "
                         "'Nose-Hoover-Chain' (another integrator: Martyna-Tobias-Klein chains, second order, any cell shape), "
                         "'Berendsen_inhomogeneous', 'Berendsen' (NVT) or 'npt_berendsen' (NPT)")
    if th == "nose-hoover-chain":
        return ens + "_nhc"
    if ens == "nvt":
        if th.startswith("berendsen"):
            return "nvt"
        if th == "langevin":
            return "nvt_langevin"
        raise ValueError("Thermostat not supported, choose in 'Nose-Hoover', 'Berendsen', 'Berendsen_inhomogeneous'")
    if th == "langevin":
        raise ValueError("Thermostat not supported for NPT: 'Langevin' keeps the cell fixed (ensemble='nvt')")
    if bulk_modulus is None:
        raise ValueError("NPT without bulk_modulus is not supported by the device MD (the reference fits an equation of state "
                         "there); pass bulk_modulus in GPa")
    if th == "berendsen_inhomogeneous":
        return "npt_inhomogeneous"
    if th == "npt_berendsen":
        return "npt_berendsen"
    raise ValueError("Thermostat not supported, choose in 'Nose-Hoover', 'Berendsen', 'Berendsen_inhomogeneous'")


class _DeviceRun:
    """One ``chg_md`` handle over R replicas; ``run`` returns the frames drained from the device ring."""

    RING = 32

    def __init__(self, calc: CHGNetCalculator, structures: list, masses: np.ndarray, momenta: np.ndarray, kind: str, cfg: dict,
                 seeds=None, fixed: list | None = None, observers: MDObservers | None = None, log_magmoms: bool = False) -> None:
        model = calc.model
        self.eng, self.model, self.calc = model.engine, model, calc
        conv = model.graph_converter
        self.prep = prep = self.eng.prepare_structures(structures)
        self.B, self.N = prep.n_struct, int(prep.atom_off[-1])
        self.n_at = np.diff(prep.atom_off)
        self.loginterval = int(cfg["loginterval"])
        self.cfea = bool(cfg["crystal_fea"])
        self.stress = kind.startswith("npt") or bool(cfg["log_stress"])
        self.masses = np.ascontiguousarray(masses, np.float64)
        mom = np.ascontiguousarray(momenta, np.float64)
        self.nhc = kind in NHC_KINDS
        self.cell_dof = cfg.get("cell_dof", "isotropic")
        params = _lib.MdParams(ensemble=ENSEMBLE_CODES[kind], fixcm=0 if self.nhc else 1, dt=cfg["dt"], temperature=cfg["temperature"], taut=cfg["taut"],
                               taup=cfg["taup"], pressure=cfg["pressure"], compressibility=cfg["compressibility"], kB=KB,
                               stress_weight=calc.stress_weight, loginterval=self.loginterval, ring_frames=self.RING,
                               log_stress=int(self.stress), log_crystal_fea=int(self.cfea), r_atom=conv.atom_graph_cutoff,
                               r_bond=conv.bond_graph_cutoff, numerical_tol=1e-8)
        dp = ctypes.POINTER(ctypes.c_double)
        host = prep.host()
        self.handle = ctypes.c_void_p()
        if kind == "nvt_langevin":       # friction and one noise key per replica travel beside the params struct
            keys = np.array([int(k) & _U64 for k in seeds], np.uint64)
            if len(keys) != self.B:
                raise ValueError("one thermostat seed per structure")
            self.eng._check(self.eng.lib.chg_md_create_langevin(
                self.eng.handle, ctypes.byref(host), self.masses.ctypes.data_as(dp), mom.ctypes.data_as(dp), ctypes.byref(params),
                cfg["friction"], keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(self.handle)))
        elif self.cell_dof != "isotropic":   # chain length and cell mode travel beside the params struct
            self.eng._check(self.eng.lib.chg_md_create_nhc_flex(
                self.eng.handle, ctypes.byref(host), self.masses.ctypes.data_as(dp), mom.ctypes.data_as(dp), ctypes.byref(params),
                int(cfg["chain_length"]), _lib.MD_CELL_MODES[self.cell_dof], ctypes.byref(self.handle)))
        elif self.nhc:                   # the chain length travels beside the params struct; the centre of mass is never touched
            self.eng._check(self.eng.lib.chg_md_create_nhc(
                self.eng.handle, ctypes.byref(host), self.masses.ctypes.data_as(dp), mom.ctypes.data_as(dp), ctypes.byref(params),
                int(cfg["chain_length"]), ctypes.byref(self.handle)))
        else:
            self.eng._check(self.eng.lib.chg_md_create(self.eng.handle, ctypes.byref(host), self.masses.ctypes.data_as(dp),
                                                       mom.ctypes.data_as(dp), ctypes.byref(params), ctypes.byref(self.handle)))
        mask = join_fixed(fixed, self.n_at) if fixed is not None else None
        if mask is not None:             # one mask [n, 3] uint8 or None per replica; the held momenta are zeroed there too
            rc = self.eng.lib.chg_md_set_fixed(self.eng.handle, self.handle, mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
            if rc != 0:
                self.free()
                self.eng._check(rc)
        self.log_magmoms = bool(log_magmoms)
        if self.log_magmoms:             # task M and a moment slot in every ring frame; without the keyword the call is never made
            rc = self.eng.lib.chg_md_set_magmoms(self.eng.handle, self.handle, 1)
            if rc != 0:
                self.free()
                self.eng._check(rc)
        self.observers = observers
        if observers is not None:        # species: the sorted unique atomic numbers of the batch
            try:
                self.species, self.species_index = observers.species_map(prep.z)
                tp = observers.transport_params(len(self.species))
                self.charge = observers.charge_params(self.species)
            except ValueError:
                self.free()
                raise
            op = observers.params(len(self.species))
            rc = self.eng.lib.chg_md_set_observers(self.eng.handle, self.handle, ctypes.byref(op),
                                                   self.species_index.ctypes.data_as(_lib.c_int_p))
            if rc == 0 and tp is not None:   # transport accumulators on the observers' ring; without them the call is never made
                rc = self.eng.lib.chg_md_set_transport(self.eng.handle, self.handle, ctypes.byref(tp))
            if rc == 0 and self.charge is not None:   # charge-state observers (they imply the moments); likewise never called without
                rc = self.eng.lib.chg_md_set_charge_states(self.eng.handle, self.handle, ctypes.byref(self.charge[0]),
                                                           self.charge[1].ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
            if rc != 0:
                self.free()
                self.eng._check(rc)
            self.transport = tp is not None
            self.sample_dt_fs = observers.sample_interval * cfg["dt"] / FS
        self.chain_length = int(cfg["chain_length"]) if self.nhc else 0
        self.started = False
        self.step = 0

    def free(self) -> None:
        if self.handle:
            self.eng.lib.chg_md_free(self.eng.handle, self.handle)
            self.handle = ctypes.c_void_p()

    def _download(self) -> dict:
        B, N, K = self.B, self.N, self.RING
        d = {"positions": np.empty((N, 3)), "momenta": np.empty((N, 3)), "cell": np.empty((B, 3, 3)), "n_steps": np.empty(B, np.int32),
             "status": np.empty(B, np.int32), "n_frames": np.zeros(1, np.int32), "frame_step": np.empty(K, np.int32),
             "frame_scalars": np.empty((K, B, 3)), "frame_positions": np.empty((K, N, 3)), "frame_momenta": np.empty((K, N, 3)),
             "frame_cell": np.empty((K, B, 3, 3)), "frame_force": np.empty((K, N, 3), np.float32), "frame_stress": np.empty((K, B, 3, 3), np.float32),
             "frame_crystal_fea": np.empty((K, B, 64), np.float32)}
        o = _lib.fill_out(_lib.MdOutHost(), d)
        o.frame_capacity = K
        extra = {}
        if self.nhc:                     # before chg_md_download drains the ring
            extra = {"nhc_state": np.empty((B, _lib.MD_NHC_STATE)), "frame_conserved": np.empty((K, B))}
            dp = ctypes.POINTER(ctypes.c_double)
            self.eng._check(self.eng.lib.chg_md_download_nhc(self.eng.handle, self.handle, extra["nhc_state"].ctypes.data_as(dp),
                                                             extra["frame_conserved"].ctypes.data_as(dp), K))
            if self.cell_dof != "isotropic":
                extra["vg"] = np.empty((B, 3, 3))
                self.eng._check(self.eng.lib.chg_md_download_vg(self.eng.handle, self.handle, extra["vg"].ctypes.data_as(dp)))
        if self.log_magmoms:             # likewise before the ring is drained
            extra["magmom"], extra["frame_magmom"] = np.empty(N, np.float32), np.empty((K, N), np.float32)
            self.eng._check(self.eng.lib.chg_md_download_magmoms(self.eng.handle, self.handle, extra["magmom"].ctypes.data_as(_lib.c_float_p),
                                                                 extra["frame_magmom"].ctypes.data_as(_lib.c_float_p), K))
        self.eng._check(self.eng.lib.chg_md_download(self.eng.handle, self.handle, ctypes.byref(o)))
        d.update(extra)
        return d

    def observables(self) -> list[MDObservables]:
        """The observers' sums as they stand, one ``MDObservables`` per replica (nothing is reset on the device)."""
        ob = self.observers
        d = download_observables(self.eng, self.handle, self.B, ob.msd_lags, len(self.species), ob.rdf_bins)
        t = (download_transport(self.eng, self.handle, self.B, ob.msd_lags, len(self.species), ob.vanhove_lags, ob.vanhove_bins)
             if self.transport else None)
        off = self.prep.atom_off
        charge = [None] * self.B
        if self.charge is not None:
            p, bounds = self.charge
            c = download_charge(self.eng, self.handle, self.B, self.N, ob.msd_lags, len(self.species), ob.magmom_bins, ob.state_rdf_bins)
            charge = [ChargeStateSums(c, i, slice(off[i], off[i + 1]), list(p.n_bounds)[:len(self.species)], bounds, ob.magmom_max,
                                      p.center_species, ob.state_rdf_rmax) for i in range(self.B)]
        return [MDObservables.from_download(d, i, self.species, self.species_index[off[i]:off[i + 1]], self.sample_dt_fs, ob.rdf_rmax,
                                            transport=t, observers=ob, charge=charge[i])
                for i in range(self.B)]

    def thermostat_state(self, d: dict, i: int) -> dict | None:
        """Chain and barostat variables of replica ``i`` from a download (ASE units): ``None`` for the other ensembles."""
        if not self.nhc:
            return None
        x, M = d["nhc_state"][i], self.chain_length
        st = {"v": x[0:M].copy(), "eta": x[4:4 + M].copy(), "vb": x[8:8 + M].copy(), "xi": x[12:12 + M].copy(), "veps": float(x[16])}
        if self.cell_dof != "isotropic":
            st["vg"] = d["vg"][i].copy()
        return st

    def run(self, steps: int, sink) -> dict:
        """``steps`` more steps in chunks whose frames fit the ring; every drained frame goes to ``sink(d, k)``.  Returns the final state."""
        li = self.loginterval
        left = int(steps)
        while True:
            chunk = min(left, li * (self.RING - 1))
            self.eng._check(self.eng.lib.chg_md_run(self.eng.handle, self.handle, chunk))
            self.started = True
            self.step += chunk
            left -= chunk
            d = self._download()
            for k in range(int(d["n_frames"][0])):
                sink(d, k)
            if left <= 0:
                return d


class MolecularDynamics:
    """Molecular dynamics on the device (reference MolecularDynamics: same arguments and defaults, plus ``seed``, and
    ``thermostat="Langevin"`` with ``friction`` in 1/fs for NVT and ``thermostat="Nose-Hoover-Chain"`` with ``chain_length`` for NVT and
    NPT and ``cell_dof`` ("isotropic", "flexible", "axes") for NPT, and ``log_magmoms`` for the site moments of every frame, see the
    module docstring)."""

    def __init__(self, atoms, *, model=None, ensemble: str = "nvt", thermostat: str = "Berendsen_inhomogeneous", temperature: float = 300,
                 starting_temperature: float | None = None, timestep: float = 2.0, pressure: float = 1.01325e-4, taut: float | None = None,
                 taup: float | None = None, bulk_modulus: float | None = None, trajectory: str | None = None, logfile: str | None = None,
                 loginterval: int = 1, crystal_feas_logfile: str | None = None, append_trajectory: bool = False,  # noqa: ARG002
                 on_isolated_atoms: str = "warn", return_site_energies: bool = False, use_device: str | None = None,
                 seed: int | None = None, friction: float | None = None, chain_length: int | None = None, fixed_atoms=None,
                 cell_dof: str = "isotropic", observers: MDObservers | None = None, log_magmoms: bool = False) -> None:
        self.ensemble, self.thermostat = ensemble, thermostat
        self.log_magmoms = bool(log_magmoms)
        self.magmoms: np.ndarray | None = None    # log_magmoms: float32 [n] of the last completed step
        if observers is not None and not isinstance(observers, MDObservers):
            raise ValueError(f"{observers=} must be an MDObservers")
        self.observers = observers
        self.fixed_atoms = fixed_atoms
        self.kind = _resolve(ensemble, thermostat, bulk_modulus)
        langevin = self.kind == "nvt_langevin"
        nhc = self.kind in NHC_KINDS
        if chain_length is not None and not nhc:
            raise ValueError(f"{chain_length=} belongs to thermostat='Nose-Hoover-Chain' (ensemble 'nvt' or 'npt')")
        if nhc:
            chain_length = 3 if chain_length is None else chain_length
            if isinstance(chain_length, bool) or chain_length != int(chain_length) or not 1 <= int(chain_length) <= 4:
                raise ValueError(f"{chain_length=} must be an integer from 1 to 4")
            if np.ndim(pressure) != 0:
                raise ValueError("pressure must be a scalar (GPa) with thermostat='Nose-Hoover-Chain': a tensor target needs a reference cell")
            if not (np.isfinite(temperature) and temperature > 0):
                raise ValueError(f"{temperature=} must be > 0 with thermostat='Nose-Hoover-Chain' (the thermostat masses are kB T taut^2)")
        self.chain_length = int(chain_length) if nhc else None
        if cell_dof not in CELL_DOFS:
            raise ValueError(f"{cell_dof=} must be one of {CELL_DOFS}")
        if cell_dof != "isotropic" and self.kind != "npt_nhc":
            raise ValueError(f"{cell_dof=} belongs to ensemble='npt', thermostat='Nose-Hoover-Chain'")
        self.cell_dof = cell_dof
        self.thermostat_state: dict | None = None
        if friction is not None and not langevin:
            raise ValueError(f"{friction=} belongs to ensemble='nvt', thermostat='Langevin'")
        friction = 0.01 if friction is None else float(friction)
        if langevin and not (np.isfinite(friction) and friction >= 0):
            raise ValueError(f"{friction=} must be >= 0 and finite (1/fs)")
        self.friction = friction if langevin else None
        # the key of the thermostat's noise stream: the given seed, else 64 fresh bits
        self.thermostat_seed = None if not langevin else (int(np.random.SeedSequence().entropy) if seed is None else int(seed)) & _U64
        if int(loginterval) < 1:
            raise ValueError(f"{loginterval=} must be positive")
        if not timestep > 0:
            raise ValueError(f"{timestep=} must be positive")
        if isinstance(model, CHGNetCalculator):
            self.calculator = model
        else:
            self.calculator = CHGNetCalculator(model=model, use_device=use_device, on_isolated_atoms=on_isolated_atoms,
                                               return_site_energies=return_site_energies)
        taut = 100 * timestep if taut is None else taut
        taup = 1000 * timestep if taup is None else taup
        self.bulk_modulus = bulk_modulus
        compressibility = 0.0 if bulk_modulus is None else 1.0 / (bulk_modulus / 160.2176)
        self.cfg = {"dt": timestep * FS, "temperature": float(temperature), "taut": taut * FS, "taup": taup * FS, "pressure": pressure * GPA,
                    "compressibility": compressibility, "loginterval": int(loginterval), "crystal_fea": crystal_feas_logfile is not None,
                    "log_stress": False, "friction": friction / FS, "chain_length": self.chain_length}
        if cell_dof != "isotropic":      # the isotropic configuration is what it was before the keyword existed
            self.cfg["cell_dof"] = cell_dof
        self.trajectory, self.logfile, self.loginterval, self.timestep = trajectory, logfile, int(loginterval), timestep
        self.crystal_feas_logfile = crystal_feas_logfile
        self.starting_temperature, self.seed = starting_temperature, seed
        self._run: _DeviceRun | None = None
        self.traj: MDTrajectory | None = None
        self._logger: MDLogger | None = None
        self.set_atoms(atoms)

    # ------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _initial(atoms, starting_temperature, rng):
        structure = atoms_to_structure(atoms)
        if not hasattr(structure, "frac_coords") or len(structure) == 0:
            raise ValueError("the structure needs at least one site")
        if hasattr(atoms, "get_masses"):
            masses = np.asarray(atoms.get_masses(), np.float64)
        else:
            masses = ATOMIC_MASSES[np.asarray(structure.atomic_numbers)]
        if starting_temperature is not None:
            momenta = maxwell_boltzmann(masses, float(starting_temperature), rng)
        elif hasattr(atoms, "get_momenta"):
            momenta = np.asarray(atoms.get_momenta(), np.float64)
        else:
            momenta = np.zeros((len(structure), 3))      # a Structure starts at 0 K (reference docstring)
        return structure, masses, momenta

    def set_atoms(self, atoms) -> None:
        """New atoms for the next ``run`` (the calculator and the integrator settings stay)."""
        self.close()
        rng = np.random.default_rng(self.seed)
        self._structure, self._masses, self._momenta = self._initial(atoms, self.starting_temperature, rng)
        self._fixed = structure_fixed(self._structure, self.fixed_atoms)
        check_fixed(self._fixed, moving_cell=self.kind.startswith("npt"), needs_dof=self.kind != "nve")
        constrained = self._fixed is not None and bool(self._fixed.any())
        if constrained:                  # ASE: set_momenta zeroes the held components after they are drawn
            self._momenta = np.where(self._fixed.astype(bool), 0.0, self._momenta)
            self._structure = self._with_fixed(self._structure)
        if self.kind in NHC_KINDS:
            if len(self._masses) < 2:
                raise ValueError("thermostat='Nose-Hoover-Chain' needs more than one atom: a single atom has no internal degree of freedom")
            # once, mass-weighted; the integrator conserves the total momentum and never removes it (unless an atom is pinned: then
            # the momentum is not conserved, N_f counts the free components and nothing is removed)
            if not constrained:
                self._momenta = self._momenta - self._masses[:, None] * (self._momenta.sum(axis=0) / self._masses.sum())
            self.thermostat_state = None
        self.magmoms = None              # a new handle: nothing has been evaluated yet
        self._step_offset = getattr(self, "nsteps", 0)
        self.nsteps = self._step_offset
        self.traj = MDTrajectory(self._structure.atomic_numbers)
        self._cfeas: list[np.ndarray] = []

    def _with_fixed(self, structure: Structure) -> Structure:
        """A copy of ``structure`` that carries the mask as ``selective_dynamics`` (True = free) beside the site properties it had; the
        caller's object is not touched."""
        out = Structure(Lattice(structure.lattice.matrix.copy()), np.asarray(structure.atomic_numbers).copy(), np.array(structure.frac_coords))
        for name, values in (getattr(structure, "site_properties", None) or {}).items():
            if name != "selective_dynamics":
                out.add_site_property(name, list(values))
        if self._fixed is not None and self._fixed.any():
            out.add_site_property("selective_dynamics", (self._fixed == 0).tolist())
        return out

    @property
    def atoms(self) -> Structure:
        """The current configuration as a ``Structure`` (unwrapped fractional coordinates)."""
        return self._structure

    @property
    def momenta(self) -> np.ndarray:
        return self._momenta

    def _observer_kw(self) -> dict:
        kw = {} if self.observers is None else {"observers": self.observers}   # without observers the handle is made as it always was
        if self.log_magmoms:
            kw["log_magmoms"] = True
        return kw

    @property
    def observables(self) -> MDObservables:
        """What the observers have accumulated since the atoms were set (downloaded on access)."""
        if self.observers is None:
            raise ValueError("the run has no observers: pass observers=MDObservers(...)")
        if self._run is None:
            raise ValueError("nothing has run yet")
        return self._run.observables()[0]

    def close(self) -> None:
        if getattr(self, "_run", None) is not None:
            self._run.free()
            self._run = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001, S110
            pass

    # ------------------------------------------------------------------------------------------------------------------------
    def _sinks(self, run: _DeviceRun, trajs: list[MDTrajectory], cfeas: list[list], step_offset: int):
        scale = run.n_at.astype(np.float64) if run.model.is_intensive else np.ones(run.B)
        sw = self.calculator.stress_weight
        pending = {"t": [], "e": [], "k": [], "T": []}

        def sink(d, k):
            step = int(d["frame_step"][k])
            for i in range(run.B):
                if d["status"][i] != 0 and step > d["n_steps"][i]:
                    continue                     # NONFINITE replica: no frames after it stopped
                sl = slice(run.prep.atom_off[i], run.prep.atom_off[i + 1])
                tr = trajs[i]
                e = float(d["frame_scalars"][k, i, 0] * scale[i])
                tr.steps.append(step + step_offset)
                tr.energies.append(e)
                tr.kinetic_energies.append(float(d["frame_scalars"][k, i, 1]))
                tr.temperatures.append(float(d["frame_scalars"][k, i, 2]))
                tr.forces.append(d["frame_force"][k, sl].astype(np.float64))
                if run.stress:
                    tr.stresses.append(voigt(d["frame_stress"][k, i].astype(np.float64)) * sw)
                tr.atom_positions.append(d["frame_positions"][k, sl].copy())
                tr.momenta.append(d["frame_momenta"][k, sl].copy())
                tr.cells.append(d["frame_cell"][k, i].copy())
                if run.nhc:
                    tr.conserved.append(float(d["frame_conserved"][k, i]) + e)
                if run.log_magmoms:
                    tr.magmoms.append(d["frame_magmom"][k, sl].copy())
                if run.cfea:
                    cfeas[i].append(d["frame_crystal_fea"][k, i].copy())
                if i == 0:
                    pending["t"].append((step + step_offset) * self.cfg["dt"] / (1000 * FS))
                    pending["e"].append(e)
                    pending["k"].append(tr.kinetic_energies[-1])
                    pending["T"].append(tr.temperatures[-1])
        return sink, pending

    def run(self, steps: int) -> MDTrajectory:
        """``steps`` MD steps (reference: ``self.dyn.run(steps)``).  Frames every ``loginterval`` steps (step 0 on the first call)
        go to the in-memory trajectory, ``logfile``, ``trajectory`` and ``crystal_feas_logfile``; returns the trajectory."""
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"{steps=} must be >= 0")
        if self._run is None:
            report_isolated_atoms(self.calculator.model, [self._structure])
            self._run = _DeviceRun(self.calculator, [self._structure], self._masses, self._momenta, self.kind, self.cfg,
                                   seeds=[self.thermostat_seed], fixed=[self._fixed], **self._observer_kw())
            if self.logfile is not None and self._logger is None:
                self._logger = MDLogger(self.logfile, len(self._structure))
        run = self._run
        sink, pending = self._sinks(run, [self.traj], [self._cfeas], self._step_offset)
        d = run.run(steps, sink)
        if self._logger is not None and pending["t"]:
            self._logger.rows(pending["t"], pending["e"], pending["k"], pending["T"])
        self._update_state(d)
        self.nsteps = self._step_offset + run.step
        if d["status"][0] != 0:
            print(f"MolecularDynamics: the run stopped at step {int(d['n_steps'][0])}: non-finite energy or forces")
        if self.trajectory is not None:
            self.traj.save(self.trajectory)
        if self.crystal_feas_logfile:
            with open(self.crystal_feas_logfile, "wb") as file:
                pickle.dump({"crystal_feas": self._cfeas}, file)
        return self.traj

    def _update_state(self, d: dict) -> None:
        lat = d["cell"][0]
        self._structure = self._with_fixed(Structure(Lattice(lat), self._structure.atomic_numbers, d["positions"] @ np.linalg.inv(lat)))
        self._momenta = d["momenta"].copy()
        self.thermostat_state = self._run.thermostat_state(d, 0)
        if self._run.log_magmoms:
            self.magmoms = d["magmom"].copy()

    # ------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def run_batch(cls, structures, steps: int, *, seeds=None, model=None, fixed_atoms=None, **kwargs) -> list[dict]:
        """Run R independent replicas (possibly of different sizes) as one device handle: each gets the trajectory it would get
        alone with ``MolecularDynamics(structures[i], seed=seeds[i], **kwargs).run(steps)`` (with the Langevin thermostat ``seeds[i]`` is
        also replica i's noise key; ``seeds=None`` draws one per replica).  Returns, per replica, ``{"trajectory",
        "final_structure", "momenta", "status", "n_steps", "thermostat_state"}`` (the last one ``None`` unless the thermostat is
        "Nose-Hoover-Chain"), plus ``"observables"`` when ``observers`` are given (one species map for the whole batch) and ``"magmoms"``
        (the last completed step's) with ``log_magmoms=True``.  ``trajectory`` / ``logfile`` / ``crystal_feas_logfile`` are not
        written here.  ``fixed_atoms``: one entry per structure (``None``: that structure's own ``selective_dynamics``, or nothing
        held)."""
        structures = list(structures)
        if not structures:
            return []
        fixed_atoms = [None] * len(structures) if fixed_atoms is None else list(fixed_atoms)
        if len(fixed_atoms) != len(structures):
            raise ValueError(f"fixed_atoms has {len(fixed_atoms)} entries for {len(structures)} structures")
        seeds = [None] * len(structures) if seeds is None else list(seeds)
        if len(seeds) != len(structures):
            raise ValueError("one seed per structure")
        for k in ("trajectory", "logfile", "crystal_feas_logfile"):
            if kwargs.get(k) is not None:
                raise ValueError(f"run_batch does not write {k}: save each returned trajectory instead")
        md, calc = [], model
        for s, sd, fx in zip(structures, seeds, fixed_atoms):      # one calculator for all replicas
            md.append(cls(s, model=calc, seed=sd, fixed_atoms=fx, **kwargs))
            calc = md[-1].calculator
        first = md[0]
        structs = [m._structure for m in md]
        report_isolated_atoms(first.calculator.model, structs)
        run = _DeviceRun(first.calculator, structs, np.concatenate([m._masses for m in md]), np.concatenate([m._momenta for m in md]),
                         first.kind, first.cfg, seeds=[m.thermostat_seed for m in md], fixed=[m._fixed for m in md], **first._observer_kw())
        try:
            trajs = [m.traj for m in md]
            sink, _ = first._sinks(run, trajs, [m._cfeas for m in md], 0)
            d = run.run(int(steps), sink)
            observed = run.observables() if run.observers is not None else None
        finally:
            run.free()
        out = []
        for i, tr in enumerate(trajs):
            sl = slice(run.prep.atom_off[i], run.prep.atom_off[i + 1])
            lat = d["cell"][i]
            fin = md[i]._with_fixed(Structure(Lattice(lat), structs[i].atomic_numbers, d["positions"][sl] @ np.linalg.inv(lat)))
            out.append({"trajectory": tr, "final_structure": fin, "momenta": d["momenta"][sl].copy(),
                        "status": STATUS_NAMES[d["status"][i]], "n_steps": int(d["n_steps"][i]),
                        "thermostat_state": run.thermostat_state(d, i)})
            if run.log_magmoms:
                out[-1]["magmoms"] = d["magmom"][sl].copy()
            if observed is not None:
                out[-1]["observables"] = observed[i]
        return out
