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
