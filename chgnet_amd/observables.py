"""MD observables accumulated on the device while the run goes on (DESIGN.md "MD observables"; csrc/kernels_md_obs.h).

``MDObservers`` says what to accumulate; ``MolecularDynamics(..., observers=...)`` and ``MolecularDynamics.run_batch(...,
observers=...)`` hand it to the device handle (``chg_md_set_observers``), and ``MDObservables`` turns the downloaded sums into the
mean-squared displacement and velocity autocorrelation per species and lag, the radial distribution function per species pair, the
coordination number and the diffusion coefficient.  Not in the reference, which leaves all of this to post-processing of a trajectory.

Every ``sample_interval``-th completed step (step 0 included) is sampled.  With ``msd_lags = L`` the device keeps the last L samples
and adds, for every lag ``l < L`` that already has a partner, ``|dr_i|^2`` and ``v_i(k) . v_i(k - l)`` of every atom to the sums of
its species: every sample is a time origin.  Positions are the unwrapped ones of the integrator, so an atom that crosses the cell
keeps its displacement; with ``subtract_com`` they are taken relative to the replica's mass-weighted centre of mass.  With
``rdf_bins`` every sample adds all ordered pairs and lattice images closer than ``rdf_rmax`` to a histogram per species pair.

Transport (``collective``, ``non_gaussian``, ``vanhove_bins``; csrc/kernels_md_transport.h) rides on the same ring and needs
``msd_lags > 0``: for every lag the fourth moment of the displacement per species (the non-Gaussian parameter), the collective
displacement ``U_a = sum_{i in a} u_i`` and current ``J_a = sum_{i in a} v_i`` of every species correlated with every other (ionic
conductivity in its Einstein form with the Onsager cross terms, against the Nernst-Einstein estimate from the tracer MSD: the Haven
ratio), and the histogram of ``|u_i|`` per species at every ``vanhove_stride``-th lag (the self part of the van Hove function).

Charge states (``magmom_states``, ``magmom_bins``, ``state_rdf_bins``; csrc/kernels_md_magmom.h) follow the reference's
charge-informed MD on the device: every sample classifies each atom's site moment against the boundaries of its element and
accumulates the moment histogram, mean and spread per species, the populations of the states, the transitions between consecutive
samples, each site's occupancy of each state, the moment autocorrelation and state persistence over the lags of the ring, and the
radial distribution around one element resolved by the state of the centre atom.

``MDObservables`` is plain NumPy on the raw sums (which stay available as attributes), so its arithmetic runs without a device.
"""

from __future__ import annotations

import ctypes

import numpy as np

from chgnet_amd import _lib

# ase.units (CODATA 2014), as chgnet_amd.dynamics: one ASE time unit in fs
_E, _AMU, _KB_J = 1.6021766208e-19, 1.660539040e-27, 1.38064852e-23
_FS = 1e-15 * (1e10 * np.sqrt(_E / _AMU))
_KB = _KB_J / _E                       # eV/K, the value of chgnet_amd.dynamics
# 1 e^2 / (A fs eV) in S/cm: e / V is e coulomb per volt, an angstrom-femtosecond is 1e-25 m s, and 1 S/m is 0.01 S/cm
_E2_PER_A_FS_EV_IN_S_PER_CM = _E / (1e-10 * 1e-15) * 1e-2


def _atomic_number(key) -> int:
    """An element given as a symbol or as an atomic number."""
    from chgnet_amd.graph.structure import SYMBOL_TO_Z, Z_TO_SYMBOL

    if isinstance(key, str):
        if key not in SYMBOL_TO_Z:
            raise ValueError(f"unknown element symbol {key!r}")
        return SYMBOL_TO_Z[key]
    if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or int(key) not in Z_TO_SYMBOL:
        raise ValueError(f"{key!r} is neither an element symbol nor an atomic number")
    return int(key)


class MDObservers:
    """What a run accumulates.  ``msd_lags``: lags of the MSD / VACF (0: none, at most 4096), in units of ``sample_interval`` steps;
    ``rdf_rmax`` (A) and ``rdf_bins``: the pair histogram (``rdf_bins=0``: none); ``subtract_com``: displacements relative to the
    centre of mass.  ``n_species**2 * rdf_bins`` may not exceed 16384 and a batch may not hold more than 8 species: both are checked
    when the species are known (``species_map``).

    Transport, all off by default and each needing ``msd_lags > 0``: ``collective``: the species-by-species correlations of the summed
    displacements and currents (ionic conductivity); ``non_gaussian``: the fourth moment of the displacement; ``vanhove_bins`` bins
    up to ``vanhove_rmax`` (A) of ``|u_i|`` per species at lags 0, ``vanhove_stride``, ..., ``(vanhove_lags - 1) * vanhove_stride``
    (``vanhove_lags=None``: as many as fit ``msd_lags``).  ``n_species * vanhove_bins`` may not exceed 4096 (``transport_params``).

    Charge states, all off by default (csrc/kernels_md_magmom.h; the run then evaluates the site moments every step):
    ``magmom_states={"Mn": [3.4, 4.2]}``: up to 3 ascending boundaries (mu_B) per element, given by symbol or atomic number; an atom's
    state is the number of boundaries at or below its moment.  ``magmom_bins`` bins up to ``magmom_max`` of the moments per species;
    ``state_rdf_bins`` bins up to ``state_rdf_rmax`` (A) of the distances from atoms of ``state_rdf_center`` to every species,
    resolved by the state of the centre.  ``n_species * magmom_bins`` may not exceed 4096 and ``4 * n_species * state_rdf_bins``
    16384 (``charge_params``)."""

    def __init__(self, sample_interval: int = 1, msd_lags: int = 0, rdf_rmax: float | None = None, rdf_bins: int = 0,
                 subtract_com: bool = True, collective: bool = False, non_gaussian: bool = False, vanhove_bins: int = 0,
                 vanhove_rmax: float | None = None, vanhove_lags: int | None = None, vanhove_stride: int = 1,
                 magmom_states: dict | None = None, magmom_bins: int = 0, magmom_max: float | None = None, state_rdf_center=None,
                 state_rdf_bins: int = 0, state_rdf_rmax: float | None = None) -> None:
        for name, v in (("sample_interval", sample_interval), ("msd_lags", msd_lags), ("rdf_bins", rdf_bins), ("vanhove_bins", vanhove_bins),
                        ("vanhove_stride", vanhove_stride), ("magmom_bins", magmom_bins), ("state_rdf_bins", state_rdf_bins),
                        *((("vanhove_lags", vanhove_lags),) if vanhove_lags is not None else ())):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name}={v!r} must be an integer")
        if sample_interval < 1:
            raise ValueError(f"{sample_interval=} must be >= 1")
        if not 0 <= msd_lags <= _lib.MD_OBS_MAX_LAGS:
            raise ValueError(f"{msd_lags=} must be 0..{_lib.MD_OBS_MAX_LAGS}")
        if rdf_bins < 0:
            raise ValueError(f"{rdf_bins=} must be >= 0")
        if rdf_bins > _lib.MD_OBS_RDF_CELLS:
            raise ValueError(f"{rdf_bins=} exceeds the {_lib.MD_OBS_RDF_CELLS} histogram cells of the device")
        if rdf_bins > 0 and (rdf_rmax is None or not np.isfinite(rdf_rmax) or not rdf_rmax > 0):
            raise ValueError(f"{rdf_rmax=} must be > 0 and finite when rdf_bins > 0")
        if rdf_bins == 0 and rdf_rmax is not None:
            raise ValueError(f"{rdf_rmax=} needs rdf_bins > 0")
        if msd_lags == 0 and rdf_bins == 0:
            raise ValueError("nothing to observe: give msd_lags > 0 or rdf_bins > 0")
        self.sample_interval, self.msd_lags, self.rdf_bins = int(sample_interval), int(msd_lags), int(rdf_bins)
        self.rdf_rmax = float(rdf_rmax) if rdf_bins > 0 else 0.0
        self.subtract_com = bool(subtract_com)
        # transport
        if vanhove_bins < 0:
            raise ValueError(f"{vanhove_bins=} must be >= 0")
        for name, on in (("collective", collective), ("non_gaussian", non_gaussian), ("vanhove_bins", vanhove_bins)):
            if on and msd_lags == 0:
                raise ValueError(f"{name} needs msd_lags > 0: it is a correlation over the ring of samples")
        if vanhove_bins > _lib.MD_OBS_VH_CELLS:
            raise ValueError(f"{vanhove_bins=} exceeds the {_lib.MD_OBS_VH_CELLS} van Hove cells of the device")
        if vanhove_bins > 0 and (vanhove_rmax is None or not np.isfinite(vanhove_rmax) or not vanhove_rmax > 0):
            raise ValueError(f"{vanhove_rmax=} must be > 0 and finite when vanhove_bins > 0")
        if vanhove_bins == 0 and (vanhove_rmax is not None or vanhove_lags is not None or vanhove_stride != 1):
            raise ValueError("vanhove_rmax, vanhove_lags and vanhove_stride need vanhove_bins > 0")
        if vanhove_stride < 1:
            raise ValueError(f"{vanhove_stride=} must be >= 1")
        if vanhove_lags is not None and vanhove_lags < 1:
            raise ValueError(f"{vanhove_lags=} must be >= 1")
        if vanhove_bins > 0:
            if vanhove_lags is None:
                vanhove_lags = (msd_lags - 1) // vanhove_stride + 1
            if (vanhove_lags - 1) * vanhove_stride >= msd_lags:
                raise ValueError(f"lag (vanhove_lags - 1) * vanhove_stride = {(vanhove_lags - 1) * vanhove_stride} is not among the "
                                 f"{msd_lags=} lags of the ring")
        self.collective, self.non_gaussian, self.vanhove_bins = bool(collective), bool(non_gaussian), int(vanhove_bins)
        self.vanhove_rmax = float(vanhove_rmax) if vanhove_bins > 0 else 0.0
        self.vanhove_lags = int(vanhove_lags) if vanhove_bins > 0 else 0
        self.vanhove_stride = int(vanhove_stride)
        # charge states
        self.magmom_states = {}
        for key, bounds in (magmom_states or {}).items():
            z = _atomic_number(key)
            b = [float(v) for v in np.atleast_1d(np.asarray(bounds, np.float64))]
            if len(b) > _lib.MD_CHG_BOUNDS:
                raise ValueError(f"magmom_states[{key!r}] has {len(b)} boundaries: at most {_lib.MD_CHG_BOUNDS} ({_lib.MD_CHG_STATES} states)")
            if not all(np.isfinite(v) and v >= 0 for v in b):
                raise ValueError(f"magmom_states[{key!r}]={b} must be finite and >= 0 (the model's moments are magnitudes)")
            if any(hi <= lo for lo, hi in zip(b, b[1:])):
                raise ValueError(f"magmom_states[{key!r}]={b} must be ascending")
            if z in self.magmom_states:
                raise ValueError(f"magmom_states names element {z} twice")
            self.magmom_states[z] = b
        if magmom_bins < 0 or state_rdf_bins < 0:
            raise ValueError(f"{magmom_bins=} and {state_rdf_bins=} must be >= 0")
        if magmom_bins > _lib.MD_CHG_HIST_CELLS:
            raise ValueError(f"{magmom_bins=} exceeds the {_lib.MD_CHG_HIST_CELLS} moment-histogram cells of the device")
        if magmom_bins > 0 and (magmom_max is None or not np.isfinite(magmom_max) or not magmom_max > 0):
            raise ValueError(f"{magmom_max=} must be > 0 and finite when magmom_bins > 0")
        if magmom_bins == 0 and magmom_max is not None:
            raise ValueError(f"{magmom_max=} needs magmom_bins > 0")
        if state_rdf_bins > 0:
            if state_rdf_center is None:
                raise ValueError("state_rdf_bins > 0 needs state_rdf_center, the element whose states the distribution is resolved by")
            if state_rdf_rmax is None or not np.isfinite(state_rdf_rmax) or not state_rdf_rmax > 0:
                raise ValueError(f"{state_rdf_rmax=} must be > 0 and finite when state_rdf_bins > 0")
            if _lib.MD_CHG_STATES * state_rdf_bins > _lib.MD_CHG_SRDF_CELLS:
                raise ValueError(f"{state_rdf_bins=} exceeds the {_lib.MD_CHG_SRDF_CELLS} histogram cells of the device")
        elif state_rdf_center is not None or state_rdf_rmax is not None:
            raise ValueError("state_rdf_center and state_rdf_rmax need state_rdf_bins > 0")
        self.magmom_bins, self.state_rdf_bins = int(magmom_bins), int(state_rdf_bins)
        self.magmom_max = float(magmom_max) if magmom_bins > 0 else 0.0
        self.state_rdf_center = _atomic_number(state_rdf_center) if state_rdf_bins > 0 else None
        self.state_rdf_rmax = float(state_rdf_rmax) if state_rdf_bins > 0 else 0.0

    @property
    def charge_states(self) -> bool:
        """Whether any of the charge-state keywords was given (``chg_md_set_charge_states`` is called only then)."""
        return bool(self.magmom_states or self.magmom_bins or self.state_rdf_bins)

    def charge_params(self, species) -> "tuple[_lib.MdChargeParams, np.ndarray] | None":
        """What ``chg_md_set_charge_states`` is given for the batch's ``species`` (sorted atomic numbers): the params struct and the
        boundaries [S, 3]; ``None`` without charge-state keywords.  An element named in ``magmom_states`` or as ``state_rdf_center``
        that the batch does not hold is refused."""
        if not self.charge_states:
            return None
        species = [int(z) for z in species]
        S = len(species)
        for z in self.magmom_states:
            if z not in species:
                raise ValueError(f"magmom_states names element {z}, which is not among the species {species} of the run")
        if self.state_rdf_bins and self.state_rdf_center not in species:
            raise ValueError(f"state_rdf_center={self.state_rdf_center} is not among the species {species} of the run")
        if S * self.magmom_bins > _lib.MD_CHG_HIST_CELLS:
            raise ValueError(f"{S} species x magmom_bins={self.magmom_bins} exceeds the {_lib.MD_CHG_HIST_CELLS} moment-histogram cells "
                             "of the device: use fewer bins")
        if _lib.MD_CHG_STATES * S * self.state_rdf_bins > _lib.MD_CHG_SRDF_CELLS:
            raise ValueError(f"{_lib.MD_CHG_STATES} states x {S} species x state_rdf_bins={self.state_rdf_bins} exceeds the "
                             f"{_lib.MD_CHG_SRDF_CELLS} histogram cells of the device: use fewer bins")
        bounds = np.zeros((S, _lib.MD_CHG_BOUNDS))
        p = _lib.MdChargeParams(mag_bins=self.magmom_bins, center_species=species.index(self.state_rdf_center) if self.state_rdf_bins else -1,
                                srdf_bins=self.state_rdf_bins, reserved=0, mag_max=self.magmom_max, srdf_rmax=self.state_rdf_rmax)
        for s, z in enumerate(species):
            b = self.magmom_states.get(z, [])
            p.n_bounds[s] = len(b)
            bounds[s, :len(b)] = b
        return p, bounds

    def species_map(self, atomic_numbers) -> tuple[np.ndarray, np.ndarray]:
        """(species, index): the sorted unique atomic numbers of the batch and every atom's index into them."""
        species, index = np.unique(np.asarray(atomic_numbers, np.int64), return_inverse=True)
        if len(species) > _lib.MD_OBS_MAX_SPECIES:
            raise ValueError(f"{len(species)} species in the batch: the observers keep at most {_lib.MD_OBS_MAX_SPECIES}")
        if len(species) ** 2 * self.rdf_bins > _lib.MD_OBS_RDF_CELLS:
            raise ValueError(f"{len(species)} species x {len(species)} species x rdf_bins={self.rdf_bins} exceeds the "
                             f"{_lib.MD_OBS_RDF_CELLS} histogram cells of the device: use fewer bins")
        return species, np.ascontiguousarray(index.reshape(-1), np.int32)

    def params(self, n_species: int) -> _lib.MdObserveParams:
        return _lib.MdObserveParams(sample_interval=self.sample_interval, n_lags=self.msd_lags, subtract_com=int(self.subtract_com),
                                    n_species=int(n_species), rdf_bins=self.rdf_bins, reserved=0, rdf_rmax=self.rdf_rmax)

    def transport_params(self, n_species: int) -> _lib.MdTransportParams | None:
        """What ``chg_md_set_transport`` is given; ``None`` when no transport was asked for (and then it is never called)."""
        if not (self.collective or self.non_gaussian or self.vanhove_bins):
            return None
        if n_species * self.vanhove_bins > _lib.MD_OBS_VH_CELLS:
            raise ValueError(f"{n_species} species x vanhove_bins={self.vanhove_bins} exceeds the {_lib.MD_OBS_VH_CELLS} van Hove cells "
                             "of the device: use fewer bins")
        return _lib.MdTransportParams(collective=int(self.collective), non_gaussian=int(self.non_gaussian), vh_bins=self.vanhove_bins,
                                      vh_lags=self.vanhove_lags, vh_stride=self.vanhove_stride, reserved=0, vh_rmax=self.vanhove_rmax)


def empty_arrays(B: int, L: int, S: int, bins: int) -> dict:
    """Host arrays named like the fields of ``chg_md_observables_host``."""
    return {"msd": np.zeros((B, L, S)), "vacf": np.zeros((B, L, S)), "cnt": np.zeros((B, L), np.int64),
            "rdf": np.zeros((B, S, S, bins), np.uint64), "rdf_samples": np.zeros(B, np.int64), "vol_sum": np.zeros(B)}


def download(eng, handle, B: int, L: int, S: int, bins: int) -> dict:
    """``chg_md_download_observables`` of a device handle: the raw sums of all B replicas."""
    d = empty_arrays(B, L, S, bins)
    out = _lib.fill_out(_lib.MdObservablesHost(), d)
    eng._check(eng.lib.chg_md_download_observables(eng.handle, handle, ctypes.byref(out)))
    return d


def empty_transport_arrays(B: int, L: int, S: int, vh_lags: int, vh_bins: int) -> dict:
    """Host arrays named like the fields of ``chg_md_transport_host``."""
    return {"msd4": np.zeros((B, L, S)), "cmsd": np.zeros((B, L, S, S)), "jacf": np.zeros((B, L, S, S)),
            "vh": np.zeros((B, vh_lags, S, vh_bins), np.uint64), "samples": np.zeros(B, np.int64), "vol_sum": np.zeros(B)}


def download_transport(eng, handle, B: int, L: int, S: int, vh_lags: int, vh_bins: int) -> dict:
    """``chg_md_download_transport`` of a device handle: the raw transport sums of all B replicas (zeros where none were requested)."""
    d = empty_transport_arrays(B, L, S, vh_lags, vh_bins)
    out = _lib.fill_out(_lib.MdTransportHost(), d)
    eng._check(eng.lib.chg_md_download_transport(eng.handle, handle, ctypes.byref(out)))
    return d


def empty_charge_arrays(B: int, N: int, L: int, S: int, mag_bins: int, srdf_bins: int) -> dict:
    """Host arrays named like the fields of ``chg_md_charge_host``."""
    Q = _lib.MD_CHG_STATES
    return {"mhist": np.zeros((B, S, mag_bins), np.uint64), "msum": np.zeros((B, S)), "msq": np.zeros((B, S)),
            "pop": np.zeros((B, S, Q), np.int64), "trans": np.zeros((B, S, Q, Q), np.int64), "occ": np.zeros((N, Q), np.int64),
            "mcorr": np.zeros((B, L, S)), "same": np.zeros((B, L, S, Q), np.int64), "shist": np.zeros((B, Q, S, srdf_bins), np.uint64),
            "samples": np.zeros(B, np.int64), "skipped": np.zeros(B, np.int64), "vol_sum": np.zeros(B)}


def download_charge(eng, handle, B: int, N: int, L: int, S: int, mag_bins: int, srdf_bins: int) -> dict:
    """``chg_md_download_charge_states`` of a device handle: the raw charge-state sums of all B replicas."""
    d = empty_charge_arrays(B, N, L, S, mag_bins, srdf_bins)
    out = _lib.fill_out(_lib.MdChargeHost(), d)
    eng._check(eng.lib.chg_md_download_charge_states(eng.handle, handle, ctypes.byref(out)))
    return d


class ChargeStateSums:
    """The raw charge-state sums of ONE replica (include/chgnet_hip.h "Charge-informed MD"): ``mhist`` [S, bins], ``msum`` / ``msq``
    [S], ``pop`` [S, Q], ``trans`` [S, Q, Q] (from, to), ``occ`` [n, Q], ``mcorr`` [L, S], ``same`` [L, S, Q], ``shist`` [Q, S, bins],
    ``samples``, ``skipped``, ``vol_sum``, with ``n_bounds`` [S], ``bounds`` [S, 3], ``mag_max``, ``center`` (species index or -1)
    and ``srdf_rmax``."""

    def __init__(self, d: dict, i: int, atoms: slice, n_bounds, bounds, mag_max: float, center: int, srdf_rmax: float) -> None:
        for name in ("mhist", "msum", "msq", "pop", "trans", "mcorr", "same", "shist"):
            setattr(self, name, d[name][i].copy())
        self.occ = d["occ"][atoms].copy()
        self.samples, self.skipped, self.vol_sum = int(d["samples"][i]), int(d["skipped"][i]), float(d["vol_sum"][i])
        self.n_bounds, self.bounds = np.asarray(n_bounds, np.int64).copy(), np.asarray(bounds, np.float64).copy()
        self.mag_max, self.center, self.srdf_rmax = float(mag_max), int(center), float(srdf_rmax)


class MDObservables:
    """The observables of ONE replica from its raw sums.

    ``species``: atomic numbers [S]; ``n_per_species`` [S]: atoms of each in the replica; ``sample_dt_fs``: time between two samples;
    ``msd_sum`` / ``vacf_sum`` [L, S] and ``cnt`` [L]; ``rdf_hist`` [S, S, bins], ``rdf_samples``, ``vol_sum`` and ``rdf_rmax``.
    Species are addressed by atomic number.

    Transport (optional keywords): ``msd4_sum`` [L, S]; ``cmsd_sum`` / ``jacf_sum`` [L, S, S]; ``vanhove_hist`` [vanhove_lags, S, bins]
    with ``vanhove_rmax`` and ``vanhove_stride``; ``transport_samples`` and ``transport_vol_sum`` (the mean volume is their quotient).
    ``cnt`` normalises them as it does the MSD."""

    def __init__(self, species, n_per_species, sample_dt_fs: float, msd_sum=None, vacf_sum=None, cnt=None, rdf_hist=None,
                 rdf_samples: int = 0, vol_sum: float = 0.0, rdf_rmax: float = 0.0, msd4_sum=None, cmsd_sum=None, jacf_sum=None,
                 vanhove_hist=None, vanhove_rmax: float = 0.0, vanhove_stride: int = 1, transport_samples: int = 0,
                 transport_vol_sum: float = 0.0, charge: "ChargeStateSums | None" = None) -> None:
        self.charge = charge               # the raw charge-state sums, or None
        self.species = np.asarray(species, np.int64)
        self.n_per_species = np.asarray(n_per_species, np.int64)
        S = len(self.species)
        if self.n_per_species.shape != (S,):
            raise ValueError("one atom count per species")
        self.sample_dt_fs = float(sample_dt_fs)
        self.msd_sum = np.zeros((0, S)) if msd_sum is None else np.asarray(msd_sum, np.float64)
        self.vacf_sum = np.zeros((0, S)) if vacf_sum is None else np.asarray(vacf_sum, np.float64)
        self.cnt = np.zeros(len(self.msd_sum), np.int64) if cnt is None else np.asarray(cnt, np.int64)
        self.rdf_hist = np.zeros((S, S, 0), np.uint64) if rdf_hist is None else np.asarray(rdf_hist, np.uint64)
        if self.msd_sum.shape != self.vacf_sum.shape or self.msd_sum.shape != (len(self.cnt), S) or self.rdf_hist.shape[:2] != (S, S):
            raise ValueError("the raw arrays do not have the shapes [L, S], [L, S], [L] and [S, S, bins]")
        self.rdf_samples, self.vol_sum, self.rdf_rmax = int(rdf_samples), float(vol_sum), float(rdf_rmax)
        L = len(self.cnt)
        self.msd4_sum = None if msd4_sum is None else np.asarray(msd4_sum, np.float64)
        self.cmsd_sum = None if cmsd_sum is None else np.asarray(cmsd_sum, np.float64)
        self.jacf_sum = None if jacf_sum is None else np.asarray(jacf_sum, np.float64)
        self.vanhove_hist = None if vanhove_hist is None else np.asarray(vanhove_hist, np.uint64)
        if self.msd4_sum is not None and self.msd4_sum.shape != (L, S):
            raise ValueError("msd4_sum does not have the shape [L, S]")
        for name, x in (("cmsd_sum", self.cmsd_sum), ("jacf_sum", self.jacf_sum)):
            if x is not None and x.shape != (L, S, S):
                raise ValueError(f"{name} does not have the shape [L, S, S]")
        self.vanhove_rmax, self.vanhove_stride = float(vanhove_rmax), int(vanhove_stride)
        if self.vanhove_hist is not None:
            if self.vanhove_hist.ndim != 3 or self.vanhove_hist.shape[1] != S:
                raise ValueError("vanhove_hist does not have the shape [vanhove_lags, S, bins]")
            if self.vanhove_stride < 1 or (len(self.vanhove_hist) - 1) * self.vanhove_stride >= max(L, 1) or not self.vanhove_rmax > 0:
                raise ValueError("vanhove_hist needs vanhove_rmax > 0 and lags (vanhove_lags - 1) * vanhove_stride among those of cnt")
        self.transport_samples, self.transport_vol_sum = int(transport_samples), float(transport_vol_sum)

    @classmethod
    def from_download(cls, d: dict, i: int, species, index_i, sample_dt_fs: float, rdf_rmax: float, transport: dict | None = None,
                      observers: "MDObservers | None" = None, charge: "ChargeStateSums | None" = None) -> "MDObservables":
        """Replica ``i`` of a ``download`` (and of a ``download_transport`` made for ``observers``); ``index_i``: the species index of
        each of its atoms."""
        n_per = np.bincount(np.asarray(index_i), minlength=len(species))
        kw = {}
        if transport is not None:
            ob, t = observers, transport
            kw = {"msd4_sum": t["msd4"][i].copy() if ob.non_gaussian else None,
                  "cmsd_sum": t["cmsd"][i].copy() if ob.collective else None, "jacf_sum": t["jacf"][i].copy() if ob.collective else None,
                  "vanhove_hist": t["vh"][i].copy() if ob.vanhove_bins else None, "vanhove_rmax": ob.vanhove_rmax,
                  "vanhove_stride": ob.vanhove_stride, "transport_samples": int(t["samples"][i]),
                  "transport_vol_sum": float(t["vol_sum"][i])}
        return cls(species, n_per, sample_dt_fs, d["msd"][i].copy(), d["vacf"][i].copy(), d["cnt"][i].copy(), d["rdf"][i].copy(),
                   int(d["rdf_samples"][i]), float(d["vol_sum"][i]), rdf_rmax, charge=charge, **kw)

    def _s(self, z) -> int:
        hit = np.flatnonzero(self.species == int(z))
        if len(hit) != 1:
            raise ValueError(f"species {z!r} is not among {self.species.tolist()}")
        return int(hit[0])

    # ---- MSD / VACF -----------------------------------------------------------------------------------------------------------
    @property
    def lag_times_fs(self) -> np.ndarray:
        return np.arange(len(self.cnt)) * self.sample_dt_fs

    def _per_atom_and_origin(self, sums: np.ndarray, z) -> np.ndarray:
        s = self._s(z)
        norm = self.cnt * self.n_per_species[s]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(norm > 0, sums[:, s] / norm, np.nan)   # a lag no sample pair has reached yet: nan

    def msd(self, species) -> np.ndarray:
        """[L] A^2: the mean over the atoms of the species and over the time origins."""
        return self._per_atom_and_origin(self.msd_sum, species)

    def vacf(self, species, normalized: bool = False) -> np.ndarray:
        """[L] <v(0) . v(t)> per atom, in A^2/fs^2; ``normalized``: divided by its value at lag 0."""
        c = self._per_atom_and_origin(self.vacf_sum, species) * _FS ** 2   # ASE velocity units -> A/fs
        return c / c[0] if normalized else c

    def _slope(self, y: np.ndarray, fit: tuple[float, float]) -> float:
        """The least-squares slope of ``y`` over the lags with ``fit[0] <= t <= fit[1]`` (fs), per fs."""
        t = self.lag_times_fs
        pick = (t >= fit[0]) & (t <= fit[1]) & np.isfinite(y)
        if pick.sum() < 2:
            raise ValueError(f"fewer than two lags fall into the window {fit} fs")
        return float(np.polyfit(t[pick], y[pick], 1)[0])

    def diffusion_coefficient(self, species, fit: tuple[float, float]) -> float:
        """The least-squares slope of the MSD over the lags with ``fit[0] <= t <= fit[1]`` (fs), divided by 6, in cm^2/s."""
        return self._slope(self.msd(species), fit) / 6.0 * 0.1   # 1 A^2/fs = 1e-16 cm^2 / 1e-15 s = 0.1 cm^2/s

    # ---- transport -------------------------------------------------------------------------------------------------------------
    def _need(self, name: str, what: str) -> np.ndarray:
        x = getattr(self, name)
        if x is None:
            raise ValueError(f"no {name} was accumulated: pass {what} to MDObservers")
        return x

    def _per_origin(self, sums: np.ndarray) -> np.ndarray:
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.cnt > 0, sums / self.cnt, np.nan)   # a lag no sample pair has reached yet: nan

    def non_gaussian_parameter(self, species) -> np.ndarray:
        """[L] alpha_2 = 3 <r^4> / (5 <r^2>^2) - 1 of the displacements of the species: 0 for a Gaussian (diffusive) distribution,
        positive when a few atoms hop far while most rattle in place; nan where the MSD is 0 (lag 0) or the lag was not reached."""
        r4 = self._per_atom_and_origin(self._need("msd4_sum", "non_gaussian=True"), species)
        r2 = self.msd(species)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(r2 > 0, 3.0 * r4 / (5.0 * r2 * r2) - 1.0, np.nan)

    def collective_msd(self, a, b) -> np.ndarray:
        """[L] A^2: <U_a(t) . U_b(t)> per time origin, U_a the summed displacement of the atoms of species ``a``."""
        return self._per_origin(self._need("cmsd_sum", "collective=True")[:, self._s(a), self._s(b)])

    def current_correlation(self, a, b) -> np.ndarray:
        """[L] A^2/fs^2: <J_a(t) . J_b(0)> per time origin, J_a the summed velocity of the atoms of species ``a`` (not symmetric in a, b)."""
        return self._per_origin(self._need("jacf_sum", "collective=True")[:, self._s(a), self._s(b)]) * _FS ** 2

    @property
    def mean_volume(self) -> float:
        """A^3: the mean cell volume over the samples of the transport accumulators."""
        if self.transport_samples == 0:
            raise ValueError("no transport sample was accumulated")
        return self.transport_vol_sum / self.transport_samples

    def _charges(self, charges: dict) -> np.ndarray:
        for z in charges:
            self._s(z)
        return np.array([float(charges.get(int(z), 0.0)) for z in self.species])   # species without a charge count as 0

    def ionic_conductivity(self, charges: dict, temperature: float, fit: tuple[float, float]) -> float:
        """S/cm, Einstein form: the least-squares slope of ``sum_ab q_a q_b <U_a . U_b>`` over the lags with ``fit[0] <= t <= fit[1]``
        (fs), divided by ``6 <V> k_B T``.  ``charges``: ``{atomic number: charge in e}``; the cross terms between species and between
        atoms of one species are all in, so this is the real conductivity and not the Nernst-Einstein estimate."""
        q = self._charges(charges)
        y = self._per_origin(np.einsum("a,lab,b->l", q, self._need("cmsd_sum", "collective=True"), q))
        return self._slope(y, fit) / (6.0 * self.mean_volume * _KB * float(temperature)) * _E2_PER_A_FS_EV_IN_S_PER_CM

    def nernst_einstein_conductivity(self, charges: dict, temperature: float, fit: tuple[float, float]) -> float:
        """S/cm: ``sum_a q_a^2 n_a`` times the slope of the tracer MSD of ``a``, over ``6 <V> k_B T``: what the conductivity would be
        if no two atoms moved in a correlated way."""
        q = self._charges(charges)
        total = sum(q[s] ** 2 * self.n_per_species[s] * self._slope(self.msd(self.species[s]), fit)
                    for s in range(len(self.species)) if q[s] != 0.0 and self.n_per_species[s] > 0)
        return float(total) / (6.0 * self.mean_volume * _KB * float(temperature)) * _E2_PER_A_FS_EV_IN_S_PER_CM

    def haven_ratio(self, charges: dict, temperature: float, fit: tuple[float, float]) -> float:
        """``nernst_einstein_conductivity / ionic_conductivity``: 1 for independent carriers, below 1 for concerted motion."""
        return self.nernst_einstein_conductivity(charges, temperature, fit) / self.ionic_conductivity(charges, temperature, fit)

    @property
    def vanhove_r(self) -> np.ndarray:
        """The bin centres of the van Hove histogram (A)."""
        bins = self._need("vanhove_hist", "vanhove_bins").shape[2]
        return (np.arange(bins) + 0.5) * (self.vanhove_rmax / bins)

    @property
    def vanhove_lag_times_fs(self) -> np.ndarray:
        return np.arange(len(self._need("vanhove_hist", "vanhove_bins"))) * self.vanhove_stride * self.sample_dt_fs

    def van_hove_self(self, species) -> np.ndarray:
        """[vanhove_lags, bins] G_s(r, t) per A^3: the probability density of finding an atom of the species displaced by r after
        t, counts / (time origins x atoms x shell volume); lags not reached are nan.  Displacements at or beyond ``vanhove_rmax`` are
        not counted, so ``sum(G_s 4 pi r^2 dr)`` over the bins is the fraction that stayed inside, not 1."""
        hist = self._need("vanhove_hist", "vanhove_bins")
        s = self._s(species)
        lags, _, bins = hist.shape
        edges = np.arange(bins + 1) * (self.vanhove_rmax / bins)
        shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
        norm = (self.cnt[np.arange(lags) * self.vanhove_stride] * self.n_per_species[s]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(norm[:, None] > 0, hist[:, s].astype(np.float64) / (norm[:, None] * shell[None, :]), np.nan)

    # ---- RDF -----------------------------------------------------------------------------------------------------------------
    @property
    def r(self) -> np.ndarray:
        """The bin centres (A)."""
        bins = self.rdf_hist.shape[2]
        return (np.arange(bins) + 0.5) * (self.rdf_rmax / bins) if bins else np.zeros(0)

    def _pairs(self, a: int, b: int) -> int:
        return int(self.n_per_species[a] * (self.n_per_species[b] - (1 if a == b else 0)))   # ordered a-b pairs

    def rdf(self, a, b) -> np.ndarray:
        """g_ab(r) [bins]: the histogram over what an ideal gas of the same mean density puts into each shell."""
        sa, sb = self._s(a), self._s(b)
        bins = self.rdf_hist.shape[2]
        if bins == 0 or self.rdf_samples == 0:
            raise ValueError("no radial distribution was accumulated")
        edges = np.arange(bins + 1) * (self.rdf_rmax / bins)
        shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
        mean_v = self.vol_sum / self.rdf_samples
        pairs = self._pairs(sa, sb)
        if pairs == 0:
            raise ValueError(f"the replica has no {a}-{b} pair")
        return self.rdf_hist[sa, sb].astype(np.float64) / (self.rdf_samples * pairs / mean_v * shell)

    def coordination_number(self, a, b, r_cut: float) -> float:
        """The mean number of ``b`` atoms within ``r_cut`` of an ``a`` atom (whole bins below ``r_cut``)."""
        sa, sb = self._s(a), self._s(b)
        bins = self.rdf_hist.shape[2]
        if bins == 0 or self.rdf_samples == 0:
            raise ValueError("no radial distribution was accumulated")
        if not 0 < r_cut <= self.rdf_rmax * (1 + 1e-12):
            raise ValueError(f"{r_cut=} must be in (0, rdf_rmax={self.rdf_rmax}]")
        upper = np.arange(1, bins + 1) * (self.rdf_rmax / bins)
        inside = upper <= r_cut * (1 + 1e-12)
        return float(self.rdf_hist[sa, sb][inside].sum() / (self.rdf_samples * self.n_per_species[sa]))

    # ---- charge states --------------------------------------------------------------------------------------------------------
    def _charge(self) -> ChargeStateSums:
        if self.charge is None:
            raise ValueError("no charge states were accumulated: pass magmom_states, magmom_bins or state_rdf_bins to MDObservers")
        return self.charge

    def n_states(self, species) -> int:
        """The number of states of the species: its boundaries plus one."""
        return int(self._charge().n_bounds[self._s(species)]) + 1

    def _counted(self, s: int) -> int:
        return int(self._charge().pop[s].sum())          # atom-samples of the species with a finite moment

    @property
    def magmom_bin_centres(self) -> np.ndarray:
        c = self._charge()
        bins = c.mhist.shape[1]
        return (np.arange(bins) + 0.5) * (c.mag_max / bins) if bins else np.zeros(0)

    def magmom_histogram(self, species) -> np.ndarray:
        """[magmom_bins] per mu_B: the probability density of the moments of the species over atoms and samples; moments at or beyond
        ``magmom_max`` are not counted, so it integrates to the fraction below."""
        c, s = self._charge(), self._s(species)
        bins = c.mhist.shape[1]
        if bins == 0:
            raise ValueError("no moment histogram was accumulated: pass magmom_bins to MDObservers")
        n = self._counted(s)
        return c.mhist[s].astype(np.float64) / (n * c.mag_max / bins) if n else np.full(bins, np.nan)

    def mean_magmom(self, species) -> float:
        """mu_B: the mean moment of the species over atoms and samples."""
        s = self._s(species)
        n = self._counted(s)
        return float(self._charge().msum[s] / n) if n else float("nan")

    def magmom_std(self, species) -> float:
        """mu_B: the standard deviation of the moments of the species over atoms and samples."""
        s = self._s(species)
        n = self._counted(s)
        if not n:
            return float("nan")
        c = self._charge()
        return float(np.sqrt(max(c.msq[s] / n - (c.msum[s] / n) ** 2, 0.0)))

    def state_populations(self, species) -> np.ndarray:
        """[states] the fraction of atom-samples of the species in each state."""
        s = self._s(species)
        n = self._counted(s)
        pop = self._charge().pop[s, :self.n_states(species)].astype(np.float64)
        return pop / n if n else np.full(len(pop), np.nan)

    def transition_counts(self, species) -> np.ndarray:
        """[states, states] (from, to): atoms of the species seen in ``from`` at one sample and in ``to`` at the next; the diagonal
        counts those that stayed."""
        q = self.n_states(species)
        return self._charge().trans[self._s(species), :q, :q].copy()

    def transition_rate(self, species, q_from: int, q_to: int) -> float:
        """Per ps: transitions ``q_from -> q_to`` per atom-sample spent in ``q_from`` (with a following sample) and per sample spacing."""
        t = self.transition_counts(species)
        if not (0 <= q_from < len(t) and 0 <= q_to < len(t)):
            raise ValueError(f"states {q_from}, {q_to} are not among the {len(t)} states of species {species}")
        base = t[q_from].sum()
        return float(t[q_from, q_to] / base / (self.sample_dt_fs * 1e-3)) if base else float("nan")

    def state_persistence(self, species, q: int) -> np.ndarray:
        """[L] same[l] / same[0] per time origin: the fraction of atoms found in state ``q`` at both ends of lag l (not necessarily
        in between), relative to lag 0; nan where the lag was not reached."""
        if not 0 <= q < self.n_states(species):
            raise ValueError(f"state {q} is not among the {self.n_states(species)} states of species {species}")
        per = self._per_origin(self._charge().same[:, self._s(species), q].astype(np.float64))
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(per[:1] > 0, per / per[:1], np.nan) if len(per) else per

    def magmom_correlation(self, species) -> np.ndarray:
        """[L] mu_B^2: <m_i(t) m_i(0)> per atom of the species and time origin."""
        return self._per_atom_and_origin(self._charge().mcorr, species)

    def site_occupancy(self) -> np.ndarray:
        """[n, Q] the fraction of its counted samples every atom spent in each state (nan for an atom never counted)."""
        occ = self._charge().occ.astype(np.float64)
        tot = occ.sum(axis=1, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(tot > 0, occ / tot, np.nan)

    @property
    def state_rdf_r(self) -> np.ndarray:
        c = self._charge()
        bins = c.shist.shape[2]
        return (np.arange(bins) + 0.5) * (c.srdf_rmax / bins) if bins else np.zeros(0)

    def state_rdf(self, q: int, species_b) -> np.ndarray:
        """g(r) [state_rdf_bins] of ``species_b`` around the centre atoms that are in state ``q``: the histogram over what an ideal gas
        of the mean density of ``species_b`` puts into each shell around the ``pop[centre, q]`` centre atom-samples."""
        c, sb = self._charge(), self._s(species_b)
        bins = c.shist.shape[2]
        if bins == 0 or c.center < 0 or c.samples == 0:
            raise ValueError("no state-resolved radial distribution was accumulated: pass state_rdf_bins to MDObservers")
        if not 0 <= q < int(c.n_bounds[c.center]) + 1:
            raise ValueError(f"state {q} is not among the states of the centre species")
        centres = int(c.pop[c.center, q])
        if centres == 0 or self.n_per_species[sb] == 0:
            raise ValueError(f"no centre atom was ever in state {q}, or the replica has no atom of species {species_b}")
        edges = np.arange(bins + 1) * (c.srdf_rmax / bins)
        shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
        density = self.n_per_species[sb] / (c.vol_sum / c.samples)
        return c.shist[q, sb].astype(np.float64) / (centres * density * shell)
