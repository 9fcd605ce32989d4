"""Float64 NumPy restatement of the device dimer saddle search (chgnet_amd/dimer.py, csrc/kernels_dimer.h): the dimer method of
Henkelman & Jonsson (J. Chem. Phys. 111, 7010 (1999)) with the rotation of Heyden, Bell & Keil (2005) -- one trial rotation, a
Fourier fit of the curvature -- the force extrapolation of Kaestner & Sherwood (2008) and ONE FIRE optimizer
(``relax_ref.fire_step``, ASE's rule with its defaults) on the modified force.  Written from the semantics alone (DESIGN.md "Dimer
saddle search"); the tests compare the step kernel and the whole driver against it.

A search has a centre ``R`` [n, 3] (UNWRAPPED cartesian positions, fixed cell) and a unit axis ``N`` over all 3n components.  An
evaluation in phase PROBE predicts ``R`` and ``R + delta N``; one in phase TRIAL predicts ``R + delta N*`` alone, with
``N* = N cos(phi1) + Theta sin(phi1)``: the centre has not moved, F0 is kept.
"""

from __future__ import annotations

import numpy as np

from relax_ref import CONVERGED, FIRE, MAX_STEPS, NONFINITE, RUNNING, fire_step

PROBE, TRIAL = 0, 1
DELTA, MAX_ROTATIONS, ANGLE_TOL = 0.01, 4, 0.05


def normalise(x):
    return x / np.sqrt((x * x).sum())


def fit_rotation(C0, Ct, b1, phi1):
    """Curvature C0 at angle 0 with slope 2 b1 there and Ct at the trial angle phi1 -> (phim, a1, shift): the angle of the
    minimum of the fit C(phi) = (C0 - a1) + a1 cos 2 phi + b1 sin 2 phi and the pi/2 shift that was applied (0: none)."""
    a1 = (C0 - Ct + b1 * np.sin(2.0 * phi1)) / (1.0 - np.cos(2.0 * phi1))
    mean = C0 - a1
    phim = 0.5 * np.arctan2(b1, a1)
    shift = 0.0
    if mean + a1 * np.cos(2.0 * phim) + b1 * np.sin(2.0 * phim) > mean:      # a maximum of the fit
        shift = np.pi / 2 if phim <= 0.0 else -np.pi / 2
    return phim + shift, a1, shift


def extrapolate(F0, F1, F1t, phi1, phim):
    """Force at R + delta N(phim) from those at angle 0 (F1), at the trial angle phi1 (F1t) and at the centre (F0)."""
    return (np.sin(phi1 - phim) / np.sin(phi1) * F1 + np.sin(phim) / np.sin(phi1) * F1t
            + (1.0 - np.cos(phim) - np.sin(phim) * np.tan(0.5 * phi1)) * F0)


def modified_force(F0, N, C0):
    """What the translation follows: F0 with its part along N inverted where the curvature is negative, minus that part alone
    (a climb along the mode) where it is not."""
    fn = (F0 * N).sum()
    return F0 - 2.0 * fn * N if C0 < 0.0 else -fn * N


def check_params(delta=DELTA, max_rotations=MAX_ROTATIONS, angle_tol=ANGLE_TOL):
    if not 0.0 < delta <= 0.5:
        raise ValueError(f"{delta=} must lie in (0, 0.5]")
    if not 0 <= max_rotations <= 32:
        raise ValueError(f"{max_rotations=} must lie in 0..32")
    if not 1e-4 <= angle_tol < np.pi / 4:
        raise ValueError(f"{angle_tol=} must lie in [1e-4, pi/4)")


class Dimer:
    """State of one search."""

    def __init__(self, positions, mode, lattice, *, delta=DELTA, max_rotations=MAX_ROTATIONS, angle_tol=ANGLE_TOL, fixed=None, fmax=0.05,
                 steps=500, p=FIRE):
        check_params(delta, max_rotations, angle_tol)
        self.R = np.array(positions, np.float64).reshape(-1, 3)
        self.n = len(self.R)
        self.L = np.array(lattice, np.float64).reshape(3, 3)
        self.Linv = np.linalg.inv(self.L)
        self.fixed = None if fixed is None else np.asarray(fixed, bool).reshape(self.n, 3)
        N = np.array(mode, np.float64).reshape(self.n, 3)
        if self.fixed is not None:
            N[self.fixed] = 0.0
        if not (N * N).sum() > 0.0:
            raise ValueError("the mode has no free component")
        self.N = normalise(N)
        self.delta, self.max_rotations, self.angle_tol, self.fmax, self.max_steps, self.p = delta, max_rotations, angle_tol, fmax, steps, dict(p)
        z = np.zeros_like(self.R)
        self.v, self.F0, self.F1, self.Theta = z.copy(), z.copy(), z.copy(), z.copy()
        self.dt, self.a, self.C0, self.gn, self.phi1 = p["dt"], p["astart"], 0.0, 0.0, 0.0
        self.nsteps, self.steps, self.status, self.phase, self.rot, self.rot_total = 0, 0, RUNNING, PROBE, 0, 0
        self.curvature, self.fmax_now, self.energy = 0.0, 0.0, 0.0
        self.e_img, self.f_img = np.zeros(2, np.float32), np.zeros((2, self.n, 3), np.float32)      # the results as last evaluated, as they came

    # ---- what the next evaluation predicts
    def trial_axis(self):
        return self.N * np.cos(self.phi1) + self.Theta * np.sin(self.phi1)

    def staged(self):
        """Cartesian positions [1 or 2, n, 3] of the structures the next evaluation predicts."""
        if self.phase == PROBE:
            return np.array([self.R, self.R + self.delta * self.N])
        return np.array([self.R + self.delta * self.trial_axis()])

    def frac(self):
        return self.staged() @ self.Linv

    def _held(self, F):
        F = np.array(F, np.float64).reshape(self.n, 3)
        if self.fixed is not None:
            F[self.fixed] = 0.0
        return F

    # ---- the step after an evaluation
    def advance(self, E, F, finite=True) -> int:
        """E [1 or 2], F [1 or 2, n, 3]: the engine's results for ``staged()``."""
        t = self.trace = {}       # every quantity a branch was taken on, for tests that must stay clear of the thresholds
        if self.status != RUNNING:
            return self.status
        E, F = np.asarray(E), np.asarray(F, np.float64)
        if not finite or not (np.all(np.isfinite(E)) and np.all(np.isfinite(F))):
            self.status = NONFINITE
            return self.status
        d = self.delta
        if self.phase == PROBE:
            self.F0, self.F1 = self._held(F[0]), self._held(F[1])
            self.e_img[:], self.f_img[:] = E, F
            self.energy = float(E[0])
        else:
            F1t, Ns = self._held(F[0]), self.trial_axis()
            self.e_img[1], self.f_img[1] = E[0], F[0]
            Ct = ((self.F0 - F1t) * Ns).sum() / d
            phim, a1, t["shift"] = fit_rotation(self.C0, Ct, -self.gn, self.phi1)
            t["fit"] = (float(np.hypot(a1, self.gn)), abs(a1) + abs(self.gn))      # the fit at atan2(b1, a1) / 2 above its mean, and its scale
            self.F1 = extrapolate(self.F0, self.F1, F1t, self.phi1, phim)
            self.N = normalise(self.N * np.cos(phim) + self.Theta * np.sin(phim))
            self.rot += 1
            self.rot_total += 1
        df = self.F1 - self.F0
        dn = (df * self.N).sum()
        self.C0 = -dn / d
        g = (df - dn * self.N) / d
        self.gn = float(np.sqrt((g * g).sum()))
        self.phi1 = 0.5 * float(np.arctan2(self.gn, abs(self.C0)))
        self.fmax_now = float(np.sqrt((self.F0 ** 2).sum(1).max()))
        if self.rot < self.max_rotations:
            t["phi1"] = self.phi1
        if self.rot < self.max_rotations and self.phi1 >= self.angle_tol:
            self.Theta = g / self.gn
            self.phase = TRIAL
            return self.status
        # translate
        self.curvature = self.C0
        t["C0"] = (self.C0, float(np.sqrt((df * df).sum())) / d)                   # and its scale
        if self.C0 < 0.0:
            t["fmax"] = self.fmax_now
        if self.C0 < 0.0 and self.fmax_now < self.fmax:
            self.status = CONVERGED
        elif self.steps >= self.max_steps:
            self.status = MAX_STEPS
        else:
            G = modified_force(self.F0, self.N, self.C0)
            if self.steps > 0:
                t["Gv"] = (float((G * self.v).sum()), float(np.sqrt((G * G).sum() * (self.v * self.v).sum())))
            dr, v, self.dt, self.a, self.nsteps = fire_step(G.ravel(), self.v.ravel(), self.steps == 0, self.dt, self.a, self.nsteps, self.p)
            t["dr"] = self.dt * float(np.sqrt((v * v).sum()))                          # before the clamp
            self.v = v.reshape(self.n, 3)
            self.R = self.R + dr.reshape(self.n, 3)
            self.steps += 1
            self.phase, self.rot = PROBE, 0
        return self.status


def dimer_host(dm: Dimer, evaluate, max_evals=None, f32=False) -> int:
    """The host loop: ``evaluate(X [k, n, 3]) -> (E [k], F [k, n, 3])`` every evaluation (f32: results rounded as the engine's are).
    Returns the structures evaluated."""
    evals = structures = 0
    while dm.status == RUNNING and (max_evals is None or evals < max_evals):
        X = dm.staged()
        E, F = evaluate(X)
        if f32:
            E, F = np.asarray(E, np.float32), np.asarray(F, np.float32)
        evals += 1
        structures += len(X)
        dm.advance(np.asarray(E), np.asarray(F, np.float64))
    return structures


# ---- the flat state layout of chg_test_dimer_step (include/chgnet_hip.h) -------------------------------------------------------
SD, SI = 24, 8


def pack_state(dimers):
    """List of Dimer -> (atom_off, r, nvec, theta, v, f0, f1, sd, si, e_img, f_img) in the layout of chg_test_dimer_step."""
    atom_off = np.concatenate([[0], np.cumsum([d.n for d in dimers])]).astype(np.int32)
    r, nvec, theta, v, f0, f1 = (np.concatenate([getattr(d, name) for d in dimers]).astype(np.float64) for name in ("R", "N", "Theta", "v", "F0", "F1"))
    sd, si = np.zeros((len(dimers), SD)), np.zeros((len(dimers), SI), np.int32)
    e_img = np.array([d.e_img for d in dimers], np.float32)
    f_img = np.concatenate([d.f_img.reshape(-1, 3) for d in dimers]).astype(np.float32)
    for k, d in enumerate(dimers):
        sd[k, :9], sd[k, 9:18] = d.L.ravel(), d.Linv.ravel()
        sd[k, 18:24] = d.dt, d.a, d.C0, d.gn, d.phi1, d.fmax_now
        si[k, :6] = d.nsteps, d.steps, d.status, d.phase, d.rot, d.rot_total
    return atom_off, r, nvec, theta, v, f0, f1, sd, si, e_img, f_img


def unpack_state(dimers, atom_off, r, nvec, theta, v, f0, f1, sd, si, e_img, f_img) -> None:
    for k, d in enumerate(dimers):
        sl = slice(atom_off[k], atom_off[k + 1])
        d.R, d.N, d.Theta, d.v, d.F0, d.F1 = (a[sl].copy() for a in (r, nvec, theta, v, f0, f1))
        d.dt, d.a, d.C0, d.gn, d.phi1, d.fmax_now = sd[k, 18:24]
        d.nsteps, d.steps, d.status, d.phase, d.rot, d.rot_total = (int(x) for x in si[k, :6])
        d.e_img, d.f_img = e_img[k].copy(), f_img[2 * atom_off[k]:2 * atom_off[k + 1]].reshape(2, -1, 3).copy()
        d.energy = float(d.e_img[0])
