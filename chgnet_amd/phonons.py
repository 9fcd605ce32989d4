"""Vibrational modes at Gamma from a device Hessian (``CHGNet.predict_hessian``).

``gamma_frequencies`` mass-weights the Hessian of one structure and returns its mode frequencies in THz.  These are the modes
commensurate with the given (super)cell; q-point bands and symmetry reduction are out of scope.
"""

from __future__ import annotations

import numpy as np

from chgnet_amd.dynamics import _AMU, _E, ATOMIC_MASSES

# sqrt(eV / (A^2 amu)) in rad/s, then THz: the CODATA-2014 constants of dynamics.py (ase.units)
_THZ = np.sqrt(_E / (1e-20 * _AMU)) / (2.0 * np.pi * 1e12)


def _atomic_numbers(structure) -> np.ndarray:
    for attr in ("atomic_numbers", "atomic_number"):
        z = getattr(structure, attr, None)
        if z is not None:
            return np.asarray(z, np.int64).reshape(-1)
    raise TypeError(f"{type(structure)=}: expected a Structure or a CrystalGraph")


def gamma_frequencies(structure, hessian) -> np.ndarray:
    """Mode frequencies (THz, ascending) of ``hessian`` [3n,3n] (eV/A^2, indexed 3i+alpha) for the atoms of ``structure``.

    The Hessian is symmetrised and mass-weighted with the standard atomic masses of ``dynamics.ATOMIC_MASSES``:
    D = M^-1/2 H M^-1/2.  An eigenvalue lam < 0 (an unstable mode) is returned as -sqrt(|lam|), phonopy's convention."""
    z = _atomic_numbers(structure)
    n = len(z)
    h = np.asarray(hessian, np.float64)
    if h.shape != (3 * n, 3 * n):
        raise ValueError(f"hessian has shape {h.shape}; a structure of {n} atoms needs ({3 * n}, {3 * n})")
    inv_sqrt_m = np.repeat(1.0 / np.sqrt(ATOMIC_MASSES[z]), 3)
    dyn = 0.5 * (h + h.T) * inv_sqrt_m[:, None] * inv_sqrt_m[None, :]
    lam = np.linalg.eigvalsh(dyn)
    return np.sort(np.sign(lam) * np.sqrt(np.abs(lam)) * _THZ)


def _eigenvalues_off_translations(structure, hessian) -> np.ndarray:
    """Eigenvalues (ascending, eV/(A^2 amu)) of the mass-weighted Hessian on the complement of the three uniform translations, which
    in mass-weighted coordinates are the vectors sqrt(m_i) e_k: [3n - 3]."""
    z = _atomic_numbers(structure)
    n = len(z)
    h = np.asarray(hessian, np.float64)
    if h.shape != (3 * n, 3 * n):
        raise ValueError(f"hessian has shape {h.shape}; a structure of {n} atoms needs ({3 * n}, {3 * n})")
    if n < 2:
        raise ValueError("a structure of one atom has no mode off the translations")
    sqrt_m = np.sqrt(ATOMIC_MASSES[z])
    dyn = 0.5 * (h + h.T) / np.repeat(sqrt_m, 3)[:, None] / np.repeat(sqrt_m, 3)[None, :]
    t = np.zeros((3 * n, 3))
    for k in range(3):
        t[k::3, k] = sqrt_m
    q = np.linalg.qr(np.concatenate([t, np.eye(3 * n)], axis=1))[0][:, 3:3 * n]     # as elastic.translation_complement
    return np.linalg.eigvalsh(q.T @ dyn @ q)


def vineyard_prefactor(minimum, h_min, saddle, h_saddle) -> float:
    """Harmonic transition-state-theory attempt frequency (THz) of a hop, Vineyard (1957): the product of the 3n - 3 mode
    frequencies at the minimum over the product of the 3n - 4 real ones at the saddle, from two ``CHGNet.predict_hessian`` results
    (eV/A^2, [3n,3n]) for the two structures (same atoms in the same order).  The three uniform translations are projected out of
    both.  With the barrier E_s - E_min of the search, the hop rate is ``prefactor * exp(-barrier / kT)``.

    Raises ``ValueError`` unless the saddle has exactly one unstable mode off the translations and the minimum has none (a mode
    counts as unstable or stable only beyond 1e-8 of the largest eigenvalue): a dimer search or a climbing band that stopped
    somewhere else has not found a first-order saddle, and a rate from it would mean nothing."""
    if not np.array_equal(_atomic_numbers(minimum), _atomic_numbers(saddle)):
        raise ValueError("the minimum and the saddle differ in their atoms")
    lam_min, lam_sad = _eigenvalues_off_translations(minimum, h_min), _eigenvalues_off_translations(saddle, h_saddle)
    tol_min, tol_sad = 1e-8 * np.abs(lam_min).max(), 1e-8 * np.abs(lam_sad).max()
    if not np.all(lam_min > tol_min):
        raise ValueError(f"the minimum has {int((lam_min <= tol_min).sum())} mode(s) off the translations that are not stable: relax it first")
    n_neg, n_pos = int((lam_sad < -tol_sad).sum()), int((lam_sad > tol_sad).sum())
    if n_neg != 1 or n_pos != len(lam_sad) - 1:
        raise ValueError(f"the saddle has {n_neg} unstable and {len(lam_sad) - n_neg - n_pos} zero mode(s) off the translations; a "
                         "first-order saddle has exactly one unstable mode and no zero one")
    # prod(nu_min) / prod(nu_saddle) through logarithms: 3n - 3 factors of a few THz overflow nothing, but their ratio is what counts
    log_ratio = 0.5 * (np.log(lam_min).sum() - np.log(lam_sad[1:]).sum())
    return float(np.exp(log_ratio) * _THZ)
