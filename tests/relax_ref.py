"""Float64 NumPy / SciPy restatement of the device relaxation (chgnet_amd/relax.py, csrc/kernels_relax.h): ASE's FIRE with its
defaults, through the Frechet cell filter.  Written from the semantics alone (DESIGN.md "Structure relaxation"); the tests
compare the step kernel and the whole driver against it.

Generalized coordinates of a structure with n atoms and initial cell L0 (rows a, b, c), deformation gradient F (cell = L0 F^T):
  atom rows u = r F^-T (so frac = u L0^-1), cell rows X = c log F (c = exp_cell_factor, default n)
Generalized forces g = -dE/d(u, X):
  atom rows f F, cell rows (1/c) L(A^T, W) with A = X / c, W = -V sigma F^-T, L the Frechet derivative of expm
Without cell relaxation the coordinates are the cartesian positions and g = f.
"""

from __future__ import annotations

import numpy as np
from scipy.linalg import expm, expm_frechet

RUNNING, CONVERGED, MAX_STEPS, NONFINITE = 0, 1, 2, 3
FIRE = {"dt": 0.1, "maxstep": 0.2, "dtmax": 1.0, "nmin": 5, "finc": 1.1, "fdec": 0.5, "astart": 0.1, "fa": 0.99}
GPA = 1.0 / 160.21766208


def fire_step(g, v, first, dt, a, nsteps, p=FIRE):
    """One ASE FIRE update on the flattened generalized force g and velocity v -> (dr, v, dt, a, nsteps)."""
    g = np.asarray(g, np.float64)
    if first:
        v = np.zeros_like(g)
    else:
        vf = float(np.vdot(g, v))
        if vf > 0.0:
            v = (1.0 - a) * v + a * g / np.sqrt(np.vdot(g, g)) * np.sqrt(np.vdot(v, v))
            if nsteps > p["nmin"]:
                dt = min(dt * p["finc"], p["dtmax"])
                a *= p["fa"]
            nsteps += 1
        else:
            v = v * 0.0
            a = p["astart"]
            dt *= p["fdec"]
            nsteps = 0
    v = v + dt * g
    dr = dt * v
    normdr = np.sqrt(np.vdot(dr, dr))
    if normdr > p["maxstep"]:
        dr = p["maxstep"] * dr / normdr
    return dr, v, dt, a, nsteps


class Relaxation:
    """State of one structure's optimizer."""

    def __init__(self, frac, lattice, *, relax_cell=True, exp_cell_factor=None, fmax=0.1, steps=500, p=FIRE):
        self.L0 = np.array(lattice, np.float64).reshape(3, 3)
        self.L0inv = np.linalg.inv(self.L0)
        frac = np.array(frac, np.float64).reshape(-1, 3)
        self.n = len(frac)
        self.relax_cell, self.fmax, self.max_steps, self.p = relax_cell, fmax, steps, dict(p)
        self.c = float(exp_cell_factor) if exp_cell_factor and exp_cell_factor > 0 else float(self.n)
        self.q = np.zeros((self.n + 3, 3))
        self.q[:self.n] = frac @ self.L0
        self.v = np.zeros_like(self.q)
        self.dt, self.a, self.nsteps, self.steps, self.status = p["dt"], p["astart"], 0, 0, RUNNING

    # ---- configuration
    def F(self) -> np.ndarray:
        return expm(self.q[self.n:] / self.c) if self.relax_cell else np.eye(3)

    def lattice(self) -> np.ndarray:
        return self.L0 @ self.F().T if self.relax_cell else self.L0.copy()

    def frac(self) -> np.ndarray:
        return self.q[:self.n] @ self.L0inv

    def positions(self) -> np.ndarray:
        return self.frac() @ self.lattice()

    # ---- generalized forces
    def generalized_forces(self, f, sigma) -> np.ndarray:
        """f [n,3] eV/A, sigma [3,3] eV/A^3 -> g [(n+3) or n, 3]."""
        f = np.asarray(f, np.float64).reshape(self.n, 3)
        if not self.relax_cell:
            return f.copy()
        A = self.q[self.n:] / self.c
        F = expm(A)
        vol = abs(np.linalg.det(self.L0 @ F.T))
        W = -vol * np.asarray(sigma, np.float64) @ np.linalg.inv(F).T
        gx = expm_frechet(A.T, W, compute_expm=False) / self.c
        return np.vstack([f @ F, gx])

    def advance(self, f, sigma, finite=True) -> int:
        """Decision + FIRE step on the evaluated configuration (forces f, stress sigma in eV/A^3)."""
        if self.status != RUNNING:
            return self.status
        g = self.generalized_forces(f, sigma) if finite else None
        if not finite or not np.all(np.isfinite(g)):
            self.status = NONFINITE
        elif (g ** 2).sum(1).max() < self.fmax ** 2:
            self.status = CONVERGED
        elif self.steps >= self.max_steps:
            self.status = MAX_STEPS
        else:
            rows = self.n + 3 if self.relax_cell else self.n
            dr, v, self.dt, self.a, self.nsteps = fire_step(g.ravel(), self.v[:rows].ravel(), self.steps == 0, self.dt, self.a, self.nsteps, self.p)
            self.v[:rows] = v.reshape(rows, 3)
            self.q[:rows] += dr.reshape(rows, 3)
            self.steps += 1
        return self.status


def relax_host(structure, predict, *, fmax=0.1, steps=500, relax_cell=True, stress_weight=GPA, max_evals=None):
    """The host loop: ``predict(frac, lattice) -> (f [n,3], s [3,3] GPa)`` every evaluation.  Returns the Relaxation and the frames
    [(frac, lattice)] of every evaluation."""
    r = Relaxation(structure.frac_coords, structure.lattice.matrix, relax_cell=relax_cell, fmax=fmax, steps=steps)
    frames, first = [], True
    while r.status == RUNNING and (max_evals is None or len(frames) < max_evals):
        frac, lat = (np.asarray(structure.frac_coords, np.float64), r.L0.copy()) if first else (r.frac(), r.lattice())
        first = False
        f, s = predict(frac, lat)
        frames.append((frac, lat))
        f = np.asarray(f, np.float64)
        sig = np.asarray(s, np.float64) * stress_weight
        r.advance(f, sig, bool(np.all(np.isfinite(f)) and np.all(np.isfinite(sig))))
    return r, frames


# ---- the flat state layout of chg_test_relax_step (include/chgnet_hip.h) ---------------------------------------------------
SD, SI = 24, 4


def pack_state(relaxations, atom_off):
    """List of Relaxation -> (q, v, sd, si) arrays in the layout of chg_test_relax_step."""
    B = len(relaxations)
    N = int(atom_off[-1])
    q, v = np.zeros((N + 3 * B, 3)), np.zeros((N + 3 * B, 3))
    sd, si = np.zeros((B, SD)), np.zeros((B, SI), np.int32)
    for o, r in enumerate(relaxations):
        r0 = atom_off[o] + 3 * o
        q[r0:r0 + r.n + 3], v[r0:r0 + r.n + 3] = r.q, r.v
        sd[o, :9], sd[o, 9:18], sd[o, 18], sd[o, 19], sd[o, 20] = r.L0.ravel(), r.L0inv.ravel(), r.c, r.dt, r.a
        si[o] = (r.nsteps, r.steps, r.status, 0)
    return q, v, sd, si


def unpack_state(relaxations, atom_off, q, v, sd, si) -> None:
    for o, r in enumerate(relaxations):
        r0 = atom_off[o] + 3 * o
        r.q, r.v = q[r0:r0 + r.n + 3].copy(), v[r0:r0 + r.n + 3].copy()
        r.dt, r.a = sd[o, 19], sd[o, 20]
        r.nsteps, r.steps, r.status = int(si[o, 0]), int(si[o, 1]), int(si[o, 2])
