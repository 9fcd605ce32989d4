"""Float64 NumPy restatement of the device L-BFGS relaxation (chgnet_amd/relax.py with optimizer_class="LBFGS",
csrc/kernels_lbfgs.h): ASE's LBFGS with its defaults and no line search, on the generalized coordinates and forces of
tests/relax_ref.py (same Frechet cell filter, same stop rules).  Written from the semantics alone (include/chgnet_hip.h, DESIGN.md
"L-BFGS"); the tests compare the step kernel and the whole driver against it.

One deviation from ASE: a triple whose curvature y . s is exactly 0 or non-finite is skipped (ASE would divide by zero).  A triple
with y . s < 0 is kept, as ASE keeps it.
"""

from __future__ import annotations

import numpy as np

from relax_ref import CONVERGED, GPA, MAX_STEPS, NONFINITE, RUNNING, Relaxation

LBFGS = {"maxstep": 0.2, "memory": 100, "damping": 1.0, "alpha": 70.0}


def two_loop(g, s, y, rho, alpha):
    """H g with H the L-BFGS inverse Hessian of the triples (oldest first) and H0 = 1 / alpha; g is the force (minus the gradient), so
    this is the direction p of the step."""
    t = -np.asarray(g, np.float64)
    m = len(s)
    a = np.empty(m)
    for i in range(m - 1, -1, -1):
        a[i] = rho[i] * np.dot(s[i], t)
        t = t - a[i] * y[i]
    z = t / alpha
    for i in range(m):
        b = rho[i] * np.dot(y[i], z)
        z = z + s[i] * (a[i] - b)
    return -z


def lbfgs_step(q, g, first, r0, g0, s, y, rho, p=LBFGS):
    """One ASE LBFGS update on the flattened coordinates q and generalized force g.  s, y, rho: the history (lists, oldest first),
    updated in place.  Returns (dr, whether a triple was appended); the caller then sets r0 = q, g0 = g, q += dr."""
    q, g = np.asarray(q, np.float64), np.asarray(g, np.float64)
    appended = False
    if not first:
        s0, y0 = q - r0, g0 - g
        ys = float(np.dot(y0, s0))
        if np.isfinite(ys) and ys != 0.0:
            appended = True
            s.append(s0)
            y.append(y0)
            rho.append(1.0 / ys)
            if len(s) > p["memory"]:
                s.pop(0)
                y.pop(0)
                rho.pop(0)
    d = two_loop(g, s, y, rho, p["alpha"]).reshape(-1, 3)
    longest = np.sqrt((d ** 2).sum(1).max())
    if longest >= p["maxstep"]:
        d = d * (p["maxstep"] / longest)
    return (p["damping"] * d).ravel(), appended


class LbfgsRelaxation(Relaxation):
    """State of one structure's L-BFGS optimizer: Relaxation's coordinates, cell filter and generalized forces; r0, g0, the history
    (oldest first) and the number of triples appended so far instead of FIRE's velocity."""

    def __init__(self, frac, lattice, *, relax_cell=True, exp_cell_factor=None, fmax=0.1, steps=500, p=LBFGS):
        super().__init__(frac, lattice, relax_cell=relax_cell, exp_cell_factor=exp_cell_factor, fmax=fmax, steps=steps)
        self.p = dict(p)
        self.r0, self.g0 = np.zeros_like(self.q), np.zeros_like(self.q)
        self.s, self.y, self.rho, self.appended = [], [], [], 0

    @property
    def rows(self) -> int:
        return self.n + 3 if self.relax_cell else self.n

    def advance(self, f, sigma, finite=True) -> int:
        """Decision + L-BFGS step on the evaluated configuration (forces f, stress sigma in eV/A^3)."""
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
            rows = self.rows
            q = self.q[:rows].ravel().copy()
            dr, appended = lbfgs_step(q, g.ravel(), self.steps == 0, self.r0[:rows].ravel(), self.g0[:rows].ravel(), self.s, self.y, self.rho,
                                      self.p)
            self.appended += int(appended)
            self.r0[:rows] = q.reshape(rows, 3)
            self.g0[:rows] = g
            self.q[:rows] += dr.reshape(rows, 3)
            self.steps += 1
        return self.status


def relax_host_lbfgs(structure, predict, *, fmax=0.1, steps=500, relax_cell=True, stress_weight=GPA, max_evals=None, p=LBFGS):
    """The host loop: ``predict(frac, lattice) -> (f [n,3], s [3,3] GPa)`` every evaluation.  Returns the LbfgsRelaxation and the
    frames [(frac, lattice)] of every evaluation."""
    r = LbfgsRelaxation(structure.frac_coords, structure.lattice.matrix, relax_cell=relax_cell, fmax=fmax, steps=steps, p=p)
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


# ---- the flat state layout of chg_test_lbfgs_step (include/chgnet_hip.h) ---------------------------------------------------
SD, SI = 24, 4


def ring_slots(memory: int, max_steps: int) -> int:
    return max(1, min(memory, max_steps))


def pack_state(relaxations, atom_off, slots):
    """List of LbfgsRelaxation -> (q, r0, g0, S, Y, rho, sd, si) in the layout of chg_test_lbfgs_step: the k-th triple appended
    (k from 0) sits in slot k % slots; a structure holds the last min(appended, slots) of them."""
    B, N = len(relaxations), int(atom_off[-1])
    R = N + 3 * B
    q, r0, g0 = np.zeros((R, 3)), np.zeros((R, 3)), np.zeros((R, 3))
    S, Y, rho = np.zeros((slots, R, 3)), np.zeros((slots, R, 3)), np.zeros((B, slots))
    sd, si = np.zeros((B, SD)), np.zeros((B, SI), np.int32)
    for o, r in enumerate(relaxations):
        a, m = atom_off[o] + 3 * o, len(r.rho)
        assert m == min(r.appended, slots), (m, r.appended, slots)
        q[a:a + r.n + 3], r0[a:a + r.n + 3], g0[a:a + r.n + 3] = r.q, r.r0, r.g0
        for i in range(m):
            k = (r.appended - m + i) % slots
            S[k, a:a + r.rows], Y[k, a:a + r.rows], rho[o, k] = r.s[i].reshape(-1, 3), r.y[i].reshape(-1, 3), r.rho[i]
        sd[o, :9], sd[o, 9:18], sd[o, 18] = r.L0.ravel(), r.L0inv.ravel(), r.c
        si[o] = (r.appended, r.steps, r.status, 0)
    return q, r0, g0, S, Y, rho, sd, si


def unpack_state(relaxations, atom_off, slots, q, r0, g0, S, Y, rho, sd, si) -> None:
    """The inverse of pack_state into objects that carry n and relax_cell."""
    for o, r in enumerate(relaxations):
        a = atom_off[o] + 3 * o
        r.q, r.r0, r.g0 = q[a:a + r.n + 3].copy(), r0[a:a + r.n + 3].copy(), g0[a:a + r.n + 3].copy()
        r.appended, r.steps, r.status = int(si[o, 0]), int(si[o, 1]), int(si[o, 2])
        m = min(r.appended, slots)
        ks = [(r.appended - m + i) % slots for i in range(m)]
        r.s = [S[k, a:a + r.rows].ravel().copy() for k in ks]
        r.y = [Y[k, a:a + r.rows].ravel().copy() for k in ks]
        r.rho = [float(rho[o, k]) for k in ks]
