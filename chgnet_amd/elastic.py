"""Elastic constants from the strain blocks of the device Hessian (``CHGNet.predict_elastic_tensor``): the host algebra.

The energy is E(x, eps) with the lattice L (I + eps) and the atoms at fixed fractional coordinates.  With the Voigt unit strains
W_1..W_6 (xx, yy, zz, yz, xz, xy; W_4 = (e_yz + e_zy) / 2, so a Voigt shear strain is the engineering one):

    C_clamped[i][j] = (1/V) W_i : d2E/deps deps : W_j                        clamped-ion tensor
    Lambda[:, j]    = d2E/dx deps : W_j                    [3n, 6]           internal-strain tensor (eV/A)
    Phi             = d2E/dx dx                            [3n, 3n]          force constants (eV/A^2)
    C_relaxed       = C_clamped - (1/V) Lambda^T Phi^+ Lambda                 Phi^+ on the complement of the 3 translations

These are elastic constants only at a stress-free, force-free configuration: relax first (``StructOptimizer`` with a small
``fmax``).  ``elastic_moduli`` gives the Voigt / Reuss / Hill bulk and shear moduli of a 6x6 tensor.
"""

from __future__ import annotations

import numpy as np

EV_A3_TO_GPA = 160.21766208          # eV/A^3 -> GPa (model.py:532)
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def voigt_strains() -> np.ndarray:
    """[6,3,3] unit strains W_1..W_6 in Voigt order (xx, yy, zz, yz, xz, xy), the shear ones symmetric with entries 1/2."""
    w = np.zeros((6, 3, 3))
    for i, (a, b) in enumerate(VOIGT):
        w[i, a, b] += 0.5
        w[i, b, a] += 0.5
    return w


def to_voigt(t) -> np.ndarray:
    """A 3x3 stress (or any symmetric rank-2 tensor) -> its 6 Voigt components (xx, yy, zz, yz, xz, xy)."""
    t = np.asarray(t, np.float64).reshape(3, 3)
    return np.array([t[a, b] for a, b in VOIGT])


def translation_complement(n: int) -> np.ndarray:
    """[3n, 3n-3] orthonormal basis of the displacements of n atoms that are not uniform translations."""
    t = np.zeros((3 * n, 3))
    for k in range(3):
        t[k::3, k] = 1.0 / np.sqrt(n)
    q, _ = np.linalg.qr(np.concatenate([t, np.eye(3 * n)], axis=1))
    return q[:, 3:3 * n]


def relaxed_ion_tensor(clamped, internal_strain, force_constants, volume: float) -> np.ndarray:
    """C_clamped - (1/V) Lambda^T Phi^+ Lambda (GPa): ``clamped`` 6x6 (GPa), ``internal_strain`` [3n,6] (eV/A),
    ``force_constants`` [3n,3n] (eV/A^2, symmetrised here), ``volume`` (A^3).  Phi^+ is the pseudo-inverse on the complement of
    the uniform translations (which Lambda's columns are orthogonal to: the forces of any strained cell sum to zero)."""
    lam = np.asarray(internal_strain, np.float64)
    phi = np.asarray(force_constants, np.float64)
    n3 = phi.shape[0]
    if n3 <= 3:
        return np.array(clamped, np.float64)
    q = translation_complement(n3 // 3)
    pq = q.T @ (0.5 * (phi + phi.T)) @ q
    inv = np.linalg.pinv(pq, rcond=1e-10, hermitian=True)
    lq = q.T @ lam
    return np.asarray(clamped, np.float64) - (lq.T @ inv @ lq) * (EV_A3_TO_GPA / volume)


def min_phonon_eigenvalue(force_constants) -> float:
    """Lowest eigenvalue (eV/A^2) of the symmetrised force constants on the complement of the 3 translations (NaN for one atom).
    A negative value: the configuration is not a minimum, and its relaxed-ion tensor is not an elastic tensor."""
    phi = np.asarray(force_constants, np.float64)
    if phi.shape[0] <= 3:
        return float("nan")
    q = translation_complement(phi.shape[0] // 3)
    return float(np.linalg.eigvalsh(q.T @ (0.5 * (phi + phi.T)) @ q)[0])


def elastic_moduli(c) -> dict:
    """Voigt, Reuss and Hill bulk (K) and shear (G) moduli of a 6x6 Voigt elastic tensor, in its units."""
    c = np.asarray(c, np.float64)
    if c.shape != (6, 6):
        raise ValueError(f"elastic tensor has shape {c.shape}; expected (6, 6)")
    s = np.linalg.inv(c)
    a, b, d = c[0, 0] + c[1, 1] + c[2, 2], c[0, 1] + c[1, 2] + c[0, 2], c[3, 3] + c[4, 4] + c[5, 5]
    sa, sb, sd = s[0, 0] + s[1, 1] + s[2, 2], s[0, 1] + s[1, 2] + s[0, 2], s[3, 3] + s[4, 4] + s[5, 5]
    k_v, g_v = (a + 2 * b) / 9, (a - b + 3 * d) / 15
    k_r, g_r = 1 / (sa + 2 * sb), 15 / (4 * sa - 4 * sb + 3 * sd)
    return {"K_V": k_v, "K_R": k_r, "K_VRH": 0.5 * (k_v + k_r), "G_V": g_v, "G_R": g_r, "G_VRH": 0.5 * (g_v + g_r)}
