"""``MonteCarlo`` -- batched canonical Monte Carlo on the device: species swaps and single-atom displacements (not in the reference).

Molecular dynamics moves atoms continuously and never exchanges a Li with a Mn on a reachable time scale; configurational disorder
(cation ordering, site disorder, order-disorder temperatures, ground-state search by annealing) needs discrete moves.  Here the
sampler runs behind the C-ABI (``chg_mc_*``, include/chgnet_hip.h): every replica's float64 state stays in HBM, and one step kernel
(csrc/kernels_mc.h) decides the pending trial by the Metropolis rule and proposes the next one after each device graph build and
energy-only prediction.  ``run_batch`` runs replicas of different sizes, temperatures and seeds as one handle -- a temperature scan is
one batch -- and each gets the chain it would get alone.  DESIGN.md "Monte Carlo" states the semantics; tests/mc_ref.py restates them.

Atoms keep their species: a swap exchanges the *positions* of two atoms of different species (physically the species swap).
``atoms`` keeps the atom order with positions moved; ``species_on_sites()`` is the lattice-model view: the input site order with
the species permuted.  The random numbers are a pure function of (``seed``, trial number), so ``run(10); run(10)`` equals ``run(20)``.
A replica whose trial energy is non-finite even on the engine's wide-range sweep stops with status ``NONFINITE``, its configuration
and statistics untouched.

``ParallelTempering`` (and ``run_batch(..., ladders=..., exchange_interval=...)``) adds replica exchange: the replicas of a tempering
ladder exchange their configurations with their neighbours in temperature by a second kernel (csrc/kernels_mc_exchange.h), so the
cold rungs leave the basin they started in.  DESIGN.md "Replica exchange" states the rule; tests/mc_exchange_ref.py restates it.
"""

from __future__ import annotations

import ctypes
import pickle
import sys

import numpy as np

from chgnet_amd import _lib
from chgnet_amd.graph.structure import SYMBOL_TO_Z, Lattice, Structure

KB = 1.38064852e-23 / 1.6021766208e-19   # ase.units.kB (CODATA 2014), eV/K: the value of chgnet_amd.dynamics
STATUS_NAMES = ("RUNNING", "NONFINITE")
MOVE_KINDS = ("swap", "displacement")    # CHG_MC_SWAP, CHG_MC_DISPLACE
_U64 = (1 << 64) - 1


def _number(name: str, value, *, low=None, high=None, integer: bool = False):
    """``value`` as a finite float (or an int) within [low, high]: ``TypeError`` for another type, ``ValueError`` out of range."""
    if isinstance(value, (bool, str, bytes)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise TypeError(f"{name}={value!r} must be a number")
    if integer:
        if value != int(value):
            raise ValueError(f"{name}={value!r} must be an integer")
        value = int(value)
    else:
        value = float(value)
        if not np.isfinite(value):
            raise ValueError(f"{name}={value!r} must be finite")
    if (low is not None and value < low) or (high is not None and value > high):
        raise ValueError(f"{name}={value!r} must lie in [{low}, {'inf' if high is None else high}]")
    return value


def swap_numbers(swap_species) -> np.ndarray | None:
    """``swap_species`` (element symbols or atomic numbers; ``None``: every species) -> sorted unique atomic numbers."""
    if swap_species is None:
        return None
    if isinstance(swap_species, (str, bytes)) or not hasattr(swap_species, "__iter__"):
        raise TypeError(f"{swap_species=} must be a sequence of element symbols or atomic numbers")
    out = set()
    for s in swap_species:
        if isinstance(s, str):
            if s not in SYMBOL_TO_Z:
                raise ValueError(f"swap_species names the unknown element {s!r}")
            out.add(SYMBOL_TO_Z[s])
        elif isinstance(s, (int, np.integer)) and not isinstance(s, bool):
            if not 1 <= int(s) <= 94:
                raise ValueError(f"swap_species names the atomic number {int(s)}, outside 1..94")
            out.add(int(s))
        else:
            raise TypeError(f"swap_species entry {s!r} must be an element symbol or an atomic number")
    if len(out) < 2:
        raise ValueError(f"{swap_species=} must name at least two species: a swap exchanges atoms of different species")
    return np.array(sorted(out), np.int32)


def held_atoms(entry, n: int) -> np.ndarray:
    """One ``fixed_atoms`` entry -> mask [n] uint8 with 1 = held: ``None``, a sequence of atom indices or a bool [n] array."""
    mask = np.zeros(n, np.uint8)
    if entry is None:
        return mask
    a = np.asarray(entry)
    if a.dtype == bool:
        if a.shape != (n,):
            raise ValueError(f"a bool fixed_atoms mask must have shape ({n},), got {a.shape}: Monte Carlo moves hold whole atoms")
        mask[a] = 1
        return mask
    if a.size == 0:
        return mask
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise TypeError("fixed_atoms must be a sequence of atom indices or a bool [n] array")
    if a.min() < -n or a.max() >= n:
        raise ValueError(f"fixed_atoms index {int(a.max() if a.max() >= n else a.min())} is out of range for {n} atoms")
    mask[a] = 1
    return mask


def _as_structure(structure) -> Structure:
    if not (hasattr(structure, "frac_coords") and hasattr(structure, "lattice")):
        from chgnet_amd.calculator import atoms_to_structure

        structure = atoms_to_structure(structure)
    if len(structure) == 0:
        raise ValueError("the structure needs at least one site")
    return structure


class MCTrajectory:
    """Frames of one replica, after every ``loginterval``-th decision from the initial configuration (trial 0): the current energy
    (eV, total), the last move's record, cartesian positions and ``site[]`` (the input row every atom sits on)."""

    def __init__(self, atomic_numbers) -> None:
        self.atomic_numbers = np.asarray(atomic_numbers)
        self.trials: list[int] = []
        self.energies: list[float] = []          # E_cur after the decision
        self.trial_energies: list[float] = []    # E_trial of the last move (frame 0: the energy of the configuration as given)
        self.kinds: list[str | None] = []        # "swap", "displacement"; None for frame 0
        self.moves: list[tuple[int, int]] = []   # (i, j) atom indices; j = -1 for a displacement
        self.accepted: list[bool] = []
        self.u_acc: list[float] = []
        self.displacements: list[np.ndarray] = []
        self.atom_positions: list[np.ndarray] = []
        self.sites: list[np.ndarray] = []

    def __len__(self) -> int:
        return len(self.energies)

    @property
    def species_on_sites(self) -> list[np.ndarray]:
        """Per frame, the atomic numbers in input site order (the lattice-model view)."""
        out = []
        for site in self.sites:
            z = np.empty_like(self.atomic_numbers)
            z[site] = self.atomic_numbers
            out.append(z)
        return out

    def save(self, filename: str) -> None:
        with open(filename, "wb") as file:
            pickle.dump({"trial": self.trials, "energy": self.energies, "trial_energy": self.trial_energies, "kind": self.kinds,
                         "move": self.moves, "accepted": self.accepted, "u_acc": self.u_acc, "displacement": self.displacements,
                         "atom_positions": self.atom_positions, "site": self.sites, "species_on_sites": self.species_on_sites,
                         "atomic_number": self.atomic_numbers}, file)


class _DeviceMC:
    """One ``chg_mc`` handle over R replicas; ``run`` returns the final download and feeds every drained frame to a sink."""

    RING = 32

    def __init__(self, model, structures: list, temperatures, seeds, swap_z, fixed: list, cfg: dict, ladder=None,
                 exchange_interval: int = 0) -> None:
        self.eng, self.model = model.engine, model
        conv = model.graph_converter
        self.prep = prep = self.eng.prepare_structures(structures)
        self.B, self.N = prep.n_struct, int(prep.atom_off[-1])
        self.n_at = np.diff(prep.atom_off)
        self.loginterval = int(cfg["loginterval"])
        self.temperatures = np.ascontiguousarray(temperatures, np.float64)
        keys = np.array([int(k) & _U64 for k in seeds], np.uint64)
        if len(keys) != self.B or len(self.temperatures) != self.B:
            raise ValueError("one temperature and one seed per structure")
        held = np.ascontiguousarray(np.concatenate(fixed), np.uint8)
        swap_mask = np.ones(self.N, np.uint8) if swap_z is None else np.isin(prep.z, swap_z).astype(np.uint8)
        params = _lib.McParams(swap_probability=cfg["swap_probability"], max_displacement=cfg["max_displacement"], kB=KB,
                               loginterval=self.loginterval, ring_frames=self.RING, r_atom=conv.atom_graph_cutoff,
                               r_bond=conv.bond_graph_cutoff, numerical_tol=1e-8)
        host = prep.host()
        u8p = ctypes.POINTER(ctypes.c_uint8)
        self.handle = ctypes.c_void_p()
        self.eng._check(self.eng.lib.chg_mc_create(
            self.eng.handle, ctypes.byref(host), self.temperatures.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), swap_mask.ctypes.data_as(u8p), held.ctypes.data_as(u8p),
            ctypes.byref(params), ctypes.byref(self.handle)))
        self.trials = 0
        self.ladder = None if ladder is None else np.ascontiguousarray(ladder, np.int32)
        if self.ladder is not None:
            try:
                self.eng._check(self.eng.lib.chg_mc_set_exchange(self.eng.handle, self.handle, self.ladder.ctypes.data_as(_lib.c_int_p),
                                                                 int(exchange_interval)))
            except Exception:
                self.free()
                raise

    def free(self) -> None:
        if self.handle:
            self.eng.lib.chg_mc_free(self.eng.handle, self.handle)
            self.handle = ctypes.c_void_p()

    def set_temperatures(self, temperatures) -> None:
        t = np.ascontiguousarray(temperatures, np.float64)
        self.eng._check(self.eng.lib.chg_mc_set_temperatures(self.eng.handle, self.handle, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        self.temperatures = t

    def _download(self) -> dict:
        B, N, K = self.B, self.N, self.RING
        d = {"positions": np.empty((N, 3)), "site": np.empty(N, np.int32), "energy": np.empty(B), "temperatures": np.empty(B),
             "status": np.empty(B, np.int32), "n_trials": np.empty(B, np.int32), "counts": np.empty((B, _lib.MC_COUNTS), np.int64),
             "sums": np.empty((B, 2)), "best_energy": np.empty(B), "best_positions": np.empty((N, 3)), "best_site": np.empty(N, np.int32),
             "n_frames": np.zeros(1, np.int32), "frame_trial": np.empty(K, np.int32),
             "frame_scalars": np.empty((K, B, _lib.MC_FRAME_SCALARS)), "frame_moves": np.empty((K, B, _lib.MC_FRAME_MOVES), np.int32),
             "frame_positions": np.empty((K, N, 3)), "frame_site": np.empty((K, N), np.int32)}
        o = _lib.fill_out(_lib.McOutHost(), d)
        o.frame_capacity = K
        self.eng._check(self.eng.lib.chg_mc_download(self.eng.handle, self.handle, ctypes.byref(o)))
        d["xi"] = np.zeros((B, _lib.MC_EXCHANGE_INTS), np.int32)   # a handle without a ladder: nothing was ever exchanged
        if self.ladder is not None:
            self.eng._check(self.eng.lib.chg_mc_download_exchange(self.eng.handle, self.handle, d["xi"].ctypes.data_as(_lib.c_int_p)))
        return d

    def run(self, trials: int, sink) -> dict:
        """``trials`` more trials in chunks whose frames fit the ring; every drained frame goes to ``sink(d, k)``."""
        li = self.loginterval
        left = int(trials)
        while True:
            chunk = min(left, li * (self.RING - 1))
            self.eng._check(self.eng.lib.chg_mc_run(self.eng.handle, self.handle, chunk))
            self.trials += chunk
            left -= chunk
            d = self._download()
            for k in range(int(d["n_frames"][0])):
                sink(d, k)
            if left <= 0:
                return d

    def sink_into(self, trajs: list[MCTrajectory], rows: list | None = None):
        """The sink that appends replica i's part of every frame to ``trajs[i]`` (and replica 0's log row to ``rows``)."""
        off = self.prep.atom_off

        def sink(d, k):
            trial = int(d["frame_trial"][k])
            for i, tr in enumerate(trajs):
                if d["status"][i] != 0 and trial > d["n_trials"][i] - 1:
                    continue                     # NONFINITE replica: no frames from the trial that stopped it
                sl = slice(off[i], off[i + 1])
                sc, mv = d["frame_scalars"][k, i], d["frame_moves"][k, i]
                tr.trials.append(trial)
                tr.energies.append(float(sc[0]))
                tr.trial_energies.append(float(sc[1]))
                tr.u_acc.append(float(sc[2]))
                tr.displacements.append(sc[3:6].copy())
                tr.kinds.append(None if mv[1] < 0 else MOVE_KINDS[mv[1]])
                tr.moves.append((int(mv[2]), int(mv[3])))
                tr.accepted.append(bool(mv[4]))
                tr.atom_positions.append(d["frame_positions"][k, sl].copy())
                tr.sites.append(d["frame_site"][k, sl].copy())
                if i == 0 and rows is not None:
                    rows.append((trial, tr.energies[-1], tr.kinds[-1], tr.accepted[-1]))
        return sink

    def replica(self, d: dict, i: int, structure: Structure) -> dict:
        """Replica i's part of a download as plain values."""
        sl = slice(self.prep.atom_off[i], self.prep.atom_off[i + 1])
        z = np.asarray(structure.atomic_numbers)
        inv = np.linalg.inv(structure.lattice.matrix)
        on_sites = np.empty_like(z)
        on_sites[d["site"][sl]] = z
        return {"positions": d["positions"][sl].copy(), "site": d["site"][sl].copy(), "species_on_sites": on_sites,
                "final_structure": Structure(Lattice(structure.lattice.matrix.copy()), z.copy(), d["positions"][sl] @ inv),
                "energy": float(d["energy"][i]), "status": STATUS_NAMES[d["status"][i]], "n_trials": int(d["n_trials"][i]),
                "counts": d["counts"][i].copy(), "sums": d["sums"][i].copy(), "temperature": float(d["temperatures"][i]),
                "best": (float(d["best_energy"][i]), Structure(Lattice(structure.lattice.matrix.copy()), z.copy(), d["best_positions"][sl] @ inv)),
                "best_site": d["best_site"][sl].copy(),
                # replica exchange: the walker this rung holds, attempts and acceptances of the pair (this rung, the next one), and
                # the round trips of the walker that started on this rung
                "walker": int(d["xi"][i, 0]), "exchange_attempts": int(d["xi"][i, 1]), "exchange_accepts": int(d["xi"][i, 2]),
                "round_trips": int(d["xi"][i, 4])}


def _acceptance(counts) -> dict:
    return {name: (float(counts[2 * k + 1]) / float(counts[2 * k]) if counts[2 * k] > 0 else float("nan")) for k, name in enumerate(MOVE_KINDS)}


def _heat_capacity(counts, sums, temperature: float) -> float:
    if not temperature > 0:
        raise ValueError("the heat capacity needs a temperature > 0")
    if counts[4] <= 0:
        raise ValueError("no samples yet")
    mean, mean2 = sums[0] / counts[4], sums[1] / counts[4]
    return float((mean2 - mean * mean) / (KB * temperature * temperature))


class MonteCarlo:
    """Canonical Monte Carlo of one structure on the device: with probability ``swap_probability`` a trial swaps two atoms of different
    species out of ``swap_species`` (element symbols or atomic numbers; default: all), else it displaces one atom by up to
    ``max_displacement`` (A) per cartesian component; Metropolis at ``temperature`` (K; 0 is greedy descent).  ``fixed_atoms`` (atom indices
    or a bool [n] array) are never picked.  The cell is fixed."""

    def __init__(self, structure, *, model=None, temperature: float = 300.0, swap_species=None, swap_probability: float = 1.0,
                 max_displacement: float = 0.1, seed: int = 0, fixed_atoms=None, loginterval: int = 1, trajectory: str | None = None,
                 logfile: str | None = None) -> None:
        # everything is checked before a model is loaded or the device is touched
        self.temperature = _number("temperature", temperature, low=0.0)
        self.swap_z = swap_numbers(swap_species)
        self.cfg = {"swap_probability": _number("swap_probability", swap_probability, low=0.0, high=1.0),
                    "max_displacement": _number("max_displacement", max_displacement, low=0.0),
                    "loginterval": _number("loginterval", loginterval, low=1, integer=True)}
        self.seed = _number("seed", seed, integer=True) & _U64
        self._input = _as_structure(structure)
        self._held = held_atoms(fixed_atoms, len(self._input))
        z, free = np.asarray(self._input.atomic_numbers), self._held == 0
        if self.cfg["swap_probability"] < 1.0 and not free.any():
            raise ValueError("every atom is held: nothing is left to displace (swap_probability < 1)")
        if self.swap_z is not None and self.cfg["swap_probability"] > 0.0 and not np.isin(z[free], self.swap_z).any():
            raise ValueError(f"none of the free atoms belongs to {swap_species=}")
        self.trajectory, self.logfile = trajectory, logfile
        if model is None:
            from chgnet_amd.model import CHGNet

            model = CHGNet.load(verbose=False)
        self.model = getattr(model, "model", model)   # a CHGNetCalculator carries its model
        self.traj = MCTrajectory(z)
        self._run: _DeviceMC | None = None
        self._state: dict | None = None
        self._base_counts = np.zeros(_lib.MC_COUNTS, np.int64)
        self._base_sums = np.zeros(2)
        self._logged_header = False

    # ------------------------------------------------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_run", None) is not None:
            self._run.free()
            self._run = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001, S110
            pass

    def set_temperature(self, temperature: float) -> None:
        """The temperature (K) of the trials decided from now on: annealing schedules call this between runs."""
        self.temperature = _number("temperature", temperature, low=0.0)
        if self._run is not None:
            self._run.set_temperatures([self.temperature])

    def run(self, trials: int) -> MCTrajectory:
        """``trials`` more trials.  Frames every ``loginterval`` trials (the initial configuration on the first call) go to the in-memory
        trajectory, ``logfile`` and ``trajectory``; returns the trajectory."""
        trials = _number("trials", trials, low=0, integer=True)
        if self._run is None:
            from chgnet_amd.calculator import report_isolated_atoms

            report_isolated_atoms(self.model, [self._input])
            self._run = _DeviceMC(self.model, [self._input], [self.temperature], [self.seed], self.swap_z, [self._held], self.cfg)
        rows: list = []
        d = self._run.run(trials, self._run.sink_into([self.traj], rows))
        self._state = self._run.replica(d, 0, self._input)
        if self.logfile is not None and rows:
            self._log(rows)
        if self._state["status"] != "RUNNING":
            print(f"MonteCarlo: the run stopped at trial {self._state['n_trials']}: non-finite energy")
        if self.trajectory is not None:
            self.traj.save(self.trajectory)
        return self.traj

    def _log(self, rows: list) -> None:
        text = "" if self._logged_header else "%-10s %16s %-13s %s\n" % ("Trial", "E[eV]", "Move", "Accepted")
        self._logged_header = True
        text += "".join("%-10d %16.6f %-13s %d\n" % (t, e, kind or "-", acc) for t, e, kind, acc in rows)
        if self.logfile == "-":
            sys.stdout.write(text)
            return
        with open(self.logfile, "a") as fh:
            fh.write(text)

    # ------------------------------------------------------------------------------------------------------------------------
    def _need_state(self) -> dict:
        if self._state is None:
            raise ValueError("nothing has run yet")
        return self._state

    @property
    def atoms(self) -> Structure:
        """The current configuration: atom order kept, positions moved (the input structure before the first run)."""
        return self._input if self._state is None else self._state["final_structure"]

    def species_on_sites(self) -> np.ndarray:
        """Atomic numbers in input site order: the lattice-model view of the current configuration."""
        return np.asarray(self._input.atomic_numbers).copy() if self._state is None else self._state["species_on_sites"].copy()

    @property
    def site(self) -> np.ndarray:
        """``site[a]``: the input row atom ``a`` sits on."""
        return np.arange(len(self._input), dtype=np.int32) if self._state is None else self._state["site"].copy()

    @property
    def energy(self) -> float:
        return self._need_state()["energy"]

    @property
    def status(self) -> str:
        return self._need_state()["status"]

    @property
    def counts(self) -> np.ndarray:
        """Trials and acceptances per move kind and the number of samples since the last ``reset_statistics``."""
        return self._need_state()["counts"] - self._base_counts

    @property
    def sums(self) -> np.ndarray:
        return self._need_state()["sums"] - self._base_sums

    @property
    def acceptance(self) -> dict:
        """Accepted fraction per move kind (``nan`` for a kind that was never tried)."""
        return _acceptance(self.counts)

    @property
    def mean_energy(self) -> float:
        """Mean of E_cur over the samples (one after every decision, accepted or not), eV."""
        c = self.counts
        if c[4] <= 0:
            raise ValueError("no samples yet")
        return float(self.sums[0] / c[4])

    def heat_capacity(self) -> float:
        """``(<E^2> - <E>^2) / (kB T^2)`` in eV/K from the device sums, at the current temperature."""
        return _heat_capacity(self.counts, self.sums, self.temperature)

    def reset_statistics(self) -> None:
        """Start the counts and the sums afresh (equilibration): what has been downloaded so far is remembered and subtracted; the device
        is not touched."""
        if self._state is not None:
            self._base_counts = self._state["counts"].copy()
            self._base_sums = self._state["sums"].copy()

    @property
    def best(self) -> tuple[float, Structure]:
        """The lowest energy seen (eV) and its configuration."""
        return self._need_state()["best"]

    # ------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def run_batch(cls, structures, trials: int, *, temperatures=300.0, seeds=None, fixed_atoms=None, model=None, ladders=None,
                  exchange_interval: int = 0, **kwargs) -> list[dict]:
        """Run R independent replicas (possibly of different sizes) as one device handle: each gets the chain it would get alone with
        ``MonteCarlo(structures[i], temperature=temperatures[i], seed=seeds[i], **kwargs).run(trials)``.  ``temperatures``: one number
        for all or one per replica; ``seeds=None`` numbers the replicas 0, 1, ...  Returns, per replica, ``{"trajectory",
        "final_structure", "species_on_sites", "site", "energy", "best", "acceptance", "mean_energy", "heat_capacity", "counts",
        "status", "n_trials", "temperature", "walker", "exchange_attempts", "exchange_accepts", "round_trips"}``.  ``trajectory`` /
        ``logfile`` are not written here.

        ``ladders`` (one id per replica; consecutive replicas with the same id >= 0 form a tempering ladder, -1 is never exchanged) with
        ``exchange_interval`` K > 0 adds replica exchange: after every K-th trial neighbouring rungs of a ladder exchange their
        configurations by the Metropolis rule on their current energies (DESIGN.md "Replica exchange").  A result is then that of a
        *rung* -- a fixed temperature -- whatever configurations passed through it."""
        structures = list(structures)
        exchange_interval = _number("exchange_interval", exchange_interval, low=0, integer=True)
        if ladders is not None:
            ladders = [_number(f"ladders[{i}]", v, low=-1, integer=True) for i, v in enumerate(ladders)]
            if len(ladders) != len(structures):
                raise ValueError(f"ladders needs one id per structure ({len(structures)})")
        if not structures:
            return []
        R = len(structures)
        temperatures = [temperatures] * R if np.ndim(temperatures) == 0 else list(temperatures)
        seeds = list(range(R)) if seeds is None else list(seeds)
        fixed_atoms = [None] * R if fixed_atoms is None else list(fixed_atoms)
        if len(temperatures) != R or len(seeds) != R or len(fixed_atoms) != R:
            raise ValueError(f"temperatures, seeds and fixed_atoms need one entry per structure ({R})")
        for k in ("trajectory", "logfile"):
            if kwargs.get(k) is not None:
                raise ValueError(f"run_batch does not write {k}: save each returned trajectory instead")
        trials = _number("trials", trials, low=0, integer=True)
        mc = []
        for s, t, sd, fx in zip(structures, temperatures, seeds, fixed_atoms):   # one model for all replicas
            mc.append(cls(s, model=model, temperature=t, seed=sd, fixed_atoms=fx, **kwargs))
            model = mc[-1].model
        first = mc[0]
        from chgnet_amd.calculator import report_isolated_atoms

        report_isolated_atoms(first.model, [m._input for m in mc])
        run = _DeviceMC(first.model, [m._input for m in mc], [m.temperature for m in mc], [m.seed for m in mc], first.swap_z,
                        [m._held for m in mc], first.cfg, ladder=ladders, exchange_interval=exchange_interval)
        try:
            d = run.run(trials, run.sink_into([m.traj for m in mc]))
        finally:
            run.free()
        out = []
        for i, m in enumerate(mc):
            st = run.replica(d, i, m._input)
            c, s = st["counts"], st["sums"]
            st.update({"trajectory": m.traj, "acceptance": _acceptance(c), "mean_energy": float(s[0] / c[4]) if c[4] > 0 else float("nan"),
                       "heat_capacity": _heat_capacity(c, s, m.temperature) if c[4] > 0 and m.temperature > 0 else float("nan")})
            out.append(st)
        return out


def temperature_ladder(t_min: float, t_max: float, n: int) -> np.ndarray:
    """``n`` temperatures (K) from ``t_min`` to ``t_max`` in geometric progression: a constant ratio between neighbouring rungs gives
    about the same exchange acceptance along the ladder where the heat capacity is flat."""
    t_min = _number("t_min", t_min)
    t_max = _number("t_max", t_max)
    n = _number("n", n, low=2, integer=True)
    if not 0.0 < t_min < t_max:
        raise ValueError(f"a ladder needs 0 < t_min < t_max, got {t_min=} {t_max=}")
    t = t_min * (t_max / t_min) ** (np.arange(n) / (n - 1))
    t[0], t[-1] = t_min, t_max
    return t


class ParallelTempering:
    """Replica-exchange Monte Carlo of one structure on the device: one rung per temperature of ``temperatures`` (K, all > 0), all rungs
    one ``chg_mc`` handle that stays alive across ``run`` calls.  Every rung runs the canonical sampler of ``MonteCarlo``; after every
    ``exchange_interval``-th trial neighbouring rungs exchange their configurations by the Metropolis rule on their current energies
    (DESIGN.md "Replica exchange"), alternating between the pairs (0,1), (2,3), ... and (1,2), (3,4), ...  A rung keeps its temperature,
    seed, statistics and best record; configurations (walkers) travel.  ``structure``: one structure for all rungs, or one starting
    structure per rung with the same cell, species and atom order.  ``seeds=None`` numbers the rungs 0, 1, ...; the move parameters are
    those of ``MonteCarlo`` and hold for every rung."""

    def __init__(self, structure, temperatures, *, exchange_interval: int = 10, model=None, seeds=None, swap_species=None,
                 swap_probability: float = 1.0, max_displacement: float = 0.1, fixed_atoms=None, loginterval: int = 1) -> None:
        # everything is checked before a model is loaded or the device is touched
        if isinstance(temperatures, (str, bytes)) or not hasattr(temperatures, "__iter__"):
            raise TypeError(f"{temperatures=} must be a sequence of temperatures, one per rung")
        temps = [_number(f"temperatures[{i}]", t) for i, t in enumerate(temperatures)]
        if len(temps) < 2:
            raise ValueError(f"a ladder needs at least two temperatures, got {len(temps)}")
        for i, t in enumerate(temps):
            if not t > 0.0:
                raise ValueError(f"temperatures[{i}]={t!r} must be > 0: an exchange divides by it")
        L = len(temps)
        self.exchange_interval = _number("exchange_interval", exchange_interval, low=0, integer=True)
        starts = [_as_structure(s) for s in structure] if isinstance(structure, (list, tuple)) else [_as_structure(structure)] * L
        if len(starts) != L:
            raise ValueError(f"{len(starts)} starting structures for {L} temperatures: give one structure or one per rung")
        z0, cell0 = np.asarray(starts[0].atomic_numbers), np.asarray(starts[0].lattice.matrix)
        for i, s in enumerate(starts[1:], 1):
            if len(s) != len(starts[0]) or not np.array_equal(np.asarray(s.atomic_numbers), z0):
                raise ValueError(f"the structure of rung {i} has other species, or the same in another order, than that of rung 0")
            if not np.array_equal(np.asarray(s.lattice.matrix), cell0):
                raise ValueError(f"the structure of rung {i} has another cell than that of rung 0")
        seeds = list(range(L)) if seeds is None else list(seeds)
        if len(seeds) != L:
            raise ValueError(f"seeds needs one entry per rung ({L})")
        self.temperatures = np.array(temps)
        self._mc: list[MonteCarlo] = []
        for s, t, sd in zip(starts, temps, seeds):   # MonteCarlo checks the rest; the first one loads the model when none is given
            self._mc.append(MonteCarlo(s, model=model, temperature=t, seed=sd, swap_species=swap_species, swap_probability=swap_probability,
                                       max_displacement=max_displacement, fixed_atoms=fixed_atoms, loginterval=loginterval))
            model = self._mc[-1].model
        self.model = model
        self._run: _DeviceMC | None = None
        self._rungs: list[dict] | None = None
        self._base_counts = np.zeros((L, _lib.MC_COUNTS), np.int64)
        self._base_sums = np.zeros((L, 2))
        self._base_exchange = np.zeros((L, 3), np.int64)   # attempts, accepts, round trips

    def __len__(self) -> int:
        return len(self._mc)

    def close(self) -> None:
        if getattr(self, "_run", None) is not None:
            self._run.free()
            self._run = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001, S110
            pass

    def run(self, trials: int) -> list[MCTrajectory]:
        """``trials`` more trials of every rung, exchange events included; returns one trajectory per rung (frames show a rung before the
        event of their trial)."""
        trials = _number("trials", trials, low=0, integer=True)
        mc = self._mc
        if self._run is None:
            from chgnet_amd.calculator import report_isolated_atoms

            report_isolated_atoms(self.model, [m._input for m in mc])
            self._run = _DeviceMC(self.model, [m._input for m in mc], [m.temperature for m in mc], [m.seed for m in mc], mc[0].swap_z,
                                  [m._held for m in mc], mc[0].cfg, ladder=[0] * len(mc), exchange_interval=self.exchange_interval)
        d = self._run.run(trials, self._run.sink_into([m.traj for m in mc]))
        self._rungs = [self._run.replica(d, i, m._input) for i, m in enumerate(mc)]
        for i, st in enumerate(self._rungs):
            st["trajectory"] = mc[i].traj
            if st["status"] != "RUNNING":
                print(f"ParallelTempering: rung {i} stopped at trial {st['n_trials']}: non-finite energy")
        return [m.traj for m in mc]

    # ------------------------------------------------------------------------------------------------------------------------
    def _need(self) -> list[dict]:
        if self._rungs is None:
            raise ValueError("nothing has run yet")
        return self._rungs

    @property
    def rungs(self) -> list[dict]:
        """Per rung, the dict ``MonteCarlo.run_batch`` returns (cumulative counts: ``reset_statistics`` does not touch them)."""
        out = []
        for st, m in zip(self._need(), self._mc):
            c, s = st["counts"], st["sums"]
            out.append({**st, "acceptance": _acceptance(c), "mean_energy": float(s[0] / c[4]) if c[4] > 0 else float("nan"),
                        "heat_capacity": _heat_capacity(c, s, m.temperature) if c[4] > 0 else float("nan")})
        return out

    def _counts(self) -> np.ndarray:
        return np.array([st["counts"] for st in self._need()]) - self._base_counts

    def _sums(self) -> np.ndarray:
        return np.array([st["sums"] for st in self._need()]) - self._base_sums

    def _exchange(self) -> np.ndarray:
        return np.array([[st["exchange_attempts"], st["exchange_accepts"], st["round_trips"]] for st in self._need()], np.int64) - self._base_exchange

    @property
    def exchange_acceptance(self) -> np.ndarray:
        """Accepted fraction of the exchanges of every pair of neighbouring rungs, [L - 1]; ``nan`` where a pair was never tried."""
        x = self._exchange()[:-1]
        return np.array([a / n if n > 0 else np.nan for n, a in zip(x[:, 0].tolist(), x[:, 1].tolist())])

    @property
    def round_trips(self) -> np.ndarray:
        """Completed bottom -> top -> bottom journeys per walker (the configuration lineage that started on rung w), [L]."""
        return self._exchange()[:, 2].copy()

    @property
    def walkers(self) -> np.ndarray:
        """The walker every rung holds now, [L]."""
        return np.array([st["walker"] for st in self._need()])

    @property
    def mean_energies(self) -> np.ndarray:
        """Mean of E_cur over the samples of every rung (eV), [L]."""
        c, s = self._counts(), self._sums()
        if (c[:, 4] <= 0).any():
            raise ValueError("no samples yet")
        return s[:, 0] / c[:, 4]

    def heat_capacities(self) -> np.ndarray:
        """``(<E^2> - <E>^2) / (kB T^2)`` per rung in eV/K, [L]."""
        c, s = self._counts(), self._sums()
        return np.array([_heat_capacity(c[i], s[i], float(t)) for i, t in enumerate(self.temperatures)])

    @property
    def acceptance(self) -> list[dict]:
        """Accepted fraction per move kind and rung."""
        return [_acceptance(c) for c in self._counts()]

    @property
    def best(self) -> tuple[float, Structure]:
        """The lowest energy any rung has seen (eV) and its configuration."""
        return min((st["best"] for st in self._need()), key=lambda b: b[0])

    def reset_statistics(self) -> None:
        """Start the counts, the sums, the exchange counts and the round trips afresh (equilibration): what has been downloaded so far
        is remembered and subtracted; the device is not touched."""
        if self._rungs is not None:
            self._base_counts = np.array([st["counts"] for st in self._rungs])
            self._base_sums = np.array([st["sums"] for st in self._rungs])
            self._base_exchange = self._exchange() + self._base_exchange
