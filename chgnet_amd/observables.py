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

``MDObservables`` is plain NumPy on the raw sums (which stay available as attributes), so its arithmetic runs without a device.
"""

from __future__ import annotations

import ctypes

import numpy as np

from chgnet_amd import _lib

# ase.units (CODATA 2014), as chgnet_amd.dynamics: one ASE time unit in fs
_E, _AMU = 1.6021766208e-19, 1.660539040e-27
_FS = 1e-15 * (1e10 * np.sqrt(_E / _AMU))


class MDObservers:
    """What a run accumulates.  ``msd_lags``: lags of the MSD / VACF (0: none, at most 4096), in units of ``sample_interval`` steps;
    ``rdf_rmax`` (A) and ``rdf_bins``: the pair histogram (``rdf_bins=0``: none); ``subtract_com``: displacements relative to the
    centre of mass.  ``n_species**2 * rdf_bins`` may not exceed 16384 and a batch may not hold more than 8 species: both are checked
    when the species are known (``species_map``)."""

    def __init__(self, sample_interval: int = 1, msd_lags: int = 0, rdf_rmax: float | None = None, rdf_bins: int = 0,
                 subtract_com: bool = True) -> None:
        for name, v in (("sample_interval", sample_interval), ("msd_lags", msd_lags), ("rdf_bins", rdf_bins)):
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


class MDObservables:
    """The observables of ONE replica from its raw sums.

    ``species``: atomic numbers [S]; ``n_per_species`` [S]: atoms of each in the replica; ``sample_dt_fs``: time between two samples;
    ``msd_sum`` / ``vacf_sum`` [L, S] and ``cnt`` [L]; ``rdf_hist`` [S, S, bins], ``rdf_samples``, ``vol_sum`` and ``rdf_rmax``.
    Species are addressed by atomic number."""

    def __init__(self, species, n_per_species, sample_dt_fs: float, msd_sum=None, vacf_sum=None, cnt=None, rdf_hist=None,
                 rdf_samples: int = 0, vol_sum: float = 0.0, rdf_rmax: float = 0.0) -> None:
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

    @classmethod
    def from_download(cls, d: dict, i: int, species, index_i, sample_dt_fs: float, rdf_rmax: float) -> "MDObservables":
        """Replica ``i`` of a ``download``; ``index_i``: the species index of each of its atoms."""
        n_per = np.bincount(np.asarray(index_i), minlength=len(species))
        return cls(species, n_per, sample_dt_fs, d["msd"][i].copy(), d["vacf"][i].copy(), d["cnt"][i].copy(), d["rdf"][i].copy(),
                   int(d["rdf_samples"][i]), float(d["vol_sum"][i]), rdf_rmax)

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

    def diffusion_coefficient(self, species, fit: tuple[float, float]) -> float:
        """The least-squares slope of the MSD over the lags with ``fit[0] <= t <= fit[1]`` (fs), divided by 6, in cm^2/s."""
        t = self.lag_times_fs
        y = self.msd(species)
        pick = (t >= fit[0]) & (t <= fit[1]) & np.isfinite(y)
        if pick.sum() < 2:
            raise ValueError(f"fewer than two lags fall into the window {fit} fs")
        slope = np.polyfit(t[pick], y[pick], 1)[0]      # A^2/fs
        return float(slope / 6.0 * 0.1)                 # 1 A^2/fs = 1e-16 cm^2 / 1e-15 s = 0.1 cm^2/s

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
