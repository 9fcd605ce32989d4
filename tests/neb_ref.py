"""Float64 NumPy restatement of the device nudged elastic band (chgnet_amd/neb.py, csrc/kernels_neb.h): improved tangents
(Henkelman & Jonsson, J. Chem. Phys. 113, 9978 (2000)), spring forces, the climbing image (Henkelman, Uberuaga & Jonsson 2000) and
ONE FIRE optimizer (``relax_ref.fire_step``, ASE's rule with its defaults) over the interior images of a band.  Written from the
semantics alone (DESIGN.md "Nudged elastic band"); the tests compare the step kernel and the whole driver against it.

A band has M images with the same cell and species; ``R`` [M, n, 3] are UNWRAPPED cartesian positions and the step takes plain
differences between neighbouring images.  Images 0 and M - 1 never move.
"""

from __future__ import annotations

import numpy as np

from relax_ref import CONVERGED, FIRE, MAX_STEPS, NONFINITE, RUNNING, fire_step

SPRING = 0.1


def tangent(tp, tm, ep, e0, em):
    """Improved tangent of an image with energy e0 between neighbours of energy em (before) and ep (after); tp = R[i+1] - R[i],
    tm = R[i] - R[i-1].  Ties are exact and take the weighted branches.  A tangent of length 0 stays 0."""
    ep, e0, em = float(ep), float(e0), float(em)
    if ep > e0 > em:
        t = tp.copy()
    elif ep < e0 < em:
        t = tm.copy()
    else:
        dmax, dmin = max(abs(ep - e0), abs(em - e0)), min(abs(ep - e0), abs(em - e0))
        t = tp * dmax + tm * dmin if ep > em else tp * dmin + tm * dmax
    nrm = np.sqrt((t * t).sum())
    return t / nrm if nrm > 0.0 else t


def climbing_image(E, climb: bool) -> int:
    """Interior image of highest energy (first index on ties), -1 without climbing."""
    return 1 + int(np.argmax(np.asarray(E)[1:-1])) if climb else -1


def neb_forces(R, E, F, k=SPRING, climb=False, fixed=None):
    """R, F [M, n, 3], E [M] (the engine's f32 values, compared as they are), fixed [M, n, 3] bool or None -> (G [M, n, 3] with zero
    rows for the end points, climbing image)."""
    R, F = np.asarray(R, np.float64), np.array(F, np.float64)
    M = len(R)
    if fixed is not None:
        F[np.asarray(fixed, bool)] = 0.0
    G = np.zeros_like(R)
    ci = climbing_image(E, climb)
    for i in range(1, M - 1):
        tp, tm = R[i + 1] - R[i], R[i] - R[i - 1]
        tau = tangent(tp, tm, E[i + 1], E[i], E[i - 1])
        ft = (F[i] * tau).sum()
        if i == ci:
            G[i] = F[i] - 2.0 * ft * tau
        else:
            G[i] = F[i] - ft * tau + k * (np.sqrt((tp * tp).sum()) - np.sqrt((tm * tm).sum())) * tau
    if fixed is not None:
        G[np.asarray(fixed, bool)] = 0.0
    return G, ci


def neb_fmax(G) -> float:
    return float(np.sqrt((np.asarray(G)[1:-1] ** 2).sum(-1).max()))


class Band:
    """State of one band's optimizer."""

    def __init__(self, positions, lattice, *, k=SPRING, climb=False, fixed=None, fmax=0.05, steps=500, p=FIRE):
        self.R = np.array(positions, np.float64)
        self.M, self.n = self.R.shape[:2]
        self.L = np.array(lattice, np.float64).reshape(3, 3)
        self.Linv = np.linalg.inv(self.L)
        self.k, self.climb, self.fmax, self.max_steps, self.p = float(k), bool(climb), fmax, steps, dict(p)
        self.fixed = None if fixed is None else np.asarray(fixed, bool).reshape(self.R.shape)
        self.v = np.zeros((self.M - 2, self.n, 3))
        self.G = np.zeros_like(self.R)
        self.dt, self.a, self.nsteps, self.steps, self.status = p["dt"], p["astart"], 0, 0, RUNNING
        self.ci, self.neb_fmax = -1, 0.0

    def frac(self) -> np.ndarray:
        return self.R @ self.Linv

    def advance(self, E, F, finite=True) -> int:
        """Decision + FIRE step on the evaluated configuration: energies E [M], forces F [M, n, 3]."""
        if self.status != RUNNING:
            return self.status
        if not finite or not (np.all(np.isfinite(E)) and np.all(np.isfinite(F))):
            self.status = NONFINITE
            return self.status
        self.G, self.ci = neb_forces(self.R, E, F, self.k, self.climb, self.fixed)
        g = self.G[1:-1]
        gmax = (g ** 2).sum(-1).max()
        self.neb_fmax = float(np.sqrt(gmax))
        if gmax < self.fmax ** 2:
            self.status = CONVERGED
        elif self.steps >= self.max_steps:
            self.status = MAX_STEPS
        else:
            dr, v, self.dt, self.a, self.nsteps = fire_step(g.ravel(), self.v.ravel(), self.steps == 0, self.dt, self.a, self.nsteps, self.p)
            self.v = v.reshape(self.v.shape)
            self.R[1:-1] += dr.reshape(self.v.shape)
            self.steps += 1
        return self.status


def neb_host(band: Band, evaluate, max_evals=None):
    """The host loop: ``evaluate(R [M, n, 3]) -> (E [M], F [M, n, 3])`` every evaluation.  Returns the energies and forces of the
    last one."""
    E = F = None
    evals = 0
    while band.status == RUNNING and (max_evals is None or evals < max_evals):
        E, F = evaluate(band.R)
        evals += 1
        band.advance(np.asarray(E), np.asarray(F, np.float64))
    return E, F


# ---- the flat state layout of chg_test_neb_step (include/chgnet_hip.h) -----------------------------------------------------------
SD, SI = 24, 4


def pack_state(bands):
    """List of Band -> (band_off, atom_off, r, v, g, sd, si) in the layout of chg_test_neb_step."""
    band_off = np.concatenate([[0], np.cumsum([b.M for b in bands])]).astype(np.int32)
    atom_off = np.concatenate([[0], np.cumsum([b.n for b in bands for _ in range(b.M)])]).astype(np.int32)
    N = int(atom_off[-1])
    r, v, g = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((N, 3))
    sd, si = np.zeros((len(bands), SD)), np.zeros((len(bands), SI), np.int32)
    for k, b in enumerate(bands):
        a0 = atom_off[band_off[k]]
        r[a0:a0 + b.M * b.n] = b.R.reshape(-1, 3)
        v[a0 + b.n:a0 + (b.M - 1) * b.n] = b.v.reshape(-1, 3)
        g[a0:a0 + b.M * b.n] = b.G.reshape(-1, 3)
        sd[k, :9], sd[k, 9:18], sd[k, 18], sd[k, 19], sd[k, 20] = b.L.ravel(), b.Linv.ravel(), b.dt, b.a, b.neb_fmax
        si[k] = (b.nsteps, b.steps, b.status, b.ci)
    return band_off, atom_off, r, v, g, sd, si


def unpack_state(bands, band_off, atom_off, r, v, g, sd, si) -> None:
    for k, b in enumerate(bands):
        a0 = atom_off[band_off[k]]
        b.R = r[a0:a0 + b.M * b.n].reshape(b.M, b.n, 3).copy()
        b.v = v[a0 + b.n:a0 + (b.M - 1) * b.n].reshape(b.M - 2, b.n, 3).copy()
        b.G = g[a0:a0 + b.M * b.n].reshape(b.M, b.n, 3).copy()
        b.dt, b.a, b.neb_fmax = sd[k, 18], sd[k, 19], sd[k, 20]
        b.nsteps, b.steps, b.status, b.ci = (int(x) for x in si[k])
