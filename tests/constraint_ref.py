"""Float64 NumPy restatement of the constrained relaxation and molecular dynamics (DESIGN.md "Constraints"), built on the
unconstrained restatements (relax_ref, lbfgs_ref, md_ref, langevin_ref, nhc_ref) and written from one rule alone: a constrained
step is the unconstrained step with the constraint projected after every update, as ASE's FixAtoms / FixCartesian do on every
get_forces, set_positions and set_momenta.

The mask is per cartesian component, bool [n, 3], True = held.

  relaxation  the force on a held component is 0 before it enters the generalized force (so its velocity, step and history stay 0
              and its coordinate never changes); the finiteness test still sees the raw forces; the stress is not masked.
  MD          forces are masked when they are evaluated; momenta are masked after every write (half kicks, Berendsen scaling,
              Langevin O step, the fixcm subtractions, chain scalings); sums are taken over the masked momenta (the Berendsen mean is
              still divided by n, the Langevin centre-of-mass velocity by the sum of all masses).
  dof         a replica that holds at least one component has dof = its free components: T = 2 Ekin / (dof kB), and N_f = dof in the
              Nose-Hoover chains (alpha, Q_1, W, the N_f kT eta_1 term).  A replica that holds nothing keeps 3 n and 3 (n - 1).
"""

from __future__ import annotations

import math

import numpy as np

import langevin_ref
import lbfgs_ref
import md_ref
import nhc_ref
import relax_ref
from md_ref import KB, kinetic_energy


def as_mask(mask, n) -> np.ndarray:
    m = np.zeros((n, 3), bool) if mask is None else np.array(mask, bool).reshape(n, 3)
    return m


def degrees_of_freedom(mask) -> int:
    """Free components of a replica that holds any, else 3 n."""
    mask = np.asarray(mask, bool)
    return int((~mask).sum()) if mask.any() else 3 * len(mask)


def temperature(p, masses, mask) -> float:
    """ase.Atoms.get_temperature (ASE >= 3.23): 2 Ekin / (dof kB); 0 when nothing is free."""
    dof = degrees_of_freedom(mask)
    return 2.0 * kinetic_energy(p, masses) / (dof * KB) if dof > 0 else 0.0


def project(x, mask):
    """The constraint applied to forces or momenta: held components are 0."""
    return np.where(mask, 0.0, x)


# ---- relaxation --------------------------------------------------------------------------------------------------------------------
class _FixedForces:
    """Mixin for Relaxation / LbfgsRelaxation: masked forces in, raw forces for the finiteness test."""

    def set_mask(self, mask):
        self.mask = as_mask(mask, self.n)
        if self.relax_cell:
            held = self.mask.sum(1)
            assert np.all((held == 0) | (held == 3)), "a partially held atom has no meaning while the cell moves"
        return self

    def generalized_forces(self, f, sigma):
        return super().generalized_forces(project(np.asarray(f, np.float64).reshape(self.n, 3), self.mask), sigma)

    def advance(self, f, sigma, finite=True):
        return super().advance(f, sigma, bool(finite) and bool(np.all(np.isfinite(np.asarray(f, np.float64)))))

    def reported_forces(self, f):
        return project(np.asarray(f, np.float64).reshape(self.n, 3), self.mask)


class FixedRelaxation(_FixedForces, relax_ref.Relaxation):
    def __init__(self, frac, lattice, mask=None, **kw):
        super().__init__(frac, lattice, **kw)
        self.set_mask(mask)


class FixedLbfgsRelaxation(_FixedForces, lbfgs_ref.LbfgsRelaxation):
    def __init__(self, frac, lattice, mask=None, **kw):
        super().__init__(frac, lattice, **kw)
        self.set_mask(mask)


def relax_host_fixed(structure, predict, mask, *, optimizer="FIRE", fmax=0.1, steps=500, relax_cell=True, stress_weight=relax_ref.GPA,
                     max_evals=None):
    """The host loop of relax_ref.relax_host / lbfgs_ref.relax_host_lbfgs with a mask: returns the relaxation, the frames
    [(frac, lattice)] of every evaluation and the raw forces of every evaluation."""
    cls = FixedLbfgsRelaxation if optimizer == "LBFGS" else FixedRelaxation
    r = cls(structure.frac_coords, structure.lattice.matrix, mask, relax_cell=relax_cell, fmax=fmax, steps=steps)
    frames, forces, first = [], [], True
    while r.status == relax_ref.RUNNING and (max_evals is None or len(frames) < max_evals):
        frac, lat = (np.asarray(structure.frac_coords, np.float64), r.L0.copy()) if first else (r.frac(), r.lattice())
        first = False
        f, s = predict(frac, lat)
        frames.append((frac, lat))
        f = np.asarray(f, np.float64)
        forces.append(f)
        sig = np.asarray(s, np.float64) * stress_weight
        r.advance(f, sig, bool(np.all(np.isfinite(f)) and np.all(np.isfinite(sig))))
    return r, frames, forces


# ---- molecular dynamics: NVE and Berendsen ----------------------------------------------------------------------------------------------
class FixedMDRef(md_ref.MDRef):
    def __init__(self, positions, cell, masses, momenta=None, mask=None, **kw):
        super().__init__(positions, cell, masses, momenta, **kw)
        self.mask = as_mask(mask, len(self.m))
        self.p = project(self.p, self.mask)                     # set_momenta

    def evaluate(self):
        e, f, s = super().evaluate()
        return e, project(f, self.mask), s                      # get_forces

    def temperature(self):
        return temperature(self.p, self.m, self.mask)

    def scale_velocities(self):
        self.p = project(md_ref.berendsen_lambda(self.temperature(), self.t0, self.dt, self.taut) * self.p, self.mask)

    def first_half(self, forces):
        p = project(self.p + 0.5 * self.dt * forces, self.mask)
        if self.fixcm:
            p = project(p - p.sum(axis=0) / float(len(p)), self.mask)
        self.r = self.r + self.dt * p / self.m[:, None]
        self.p = p
        self._moved()

    def second_half(self, forces):
        self.p = project(self.p + 0.5 * self.dt * forces, self.mask)

    def frame(self):
        fr = super().frame()
        fr["temperature"] = self.temperature()
        fr["forces"] = project(fr["forces"], self.mask)
        return fr


# ---- Langevin ------------------------------------------------------------------------------------------------------------------------
class FixedLangevinRef(langevin_ref.LangevinRef):
    def __init__(self, positions, cell, masses, momenta=None, mask=None, **kw):
        super().__init__(positions, cell, masses, momenta, **kw)
        self.mask = as_mask(mask, len(self.m))
        self.p = project(self.p, self.mask)

    def evaluate(self):
        e, f, s = super().evaluate()
        return e, project(f, self.mask), s

    def temperature(self):
        return temperature(self.p, self.m, self.mask)

    def first_half(self, forces):
        """B A O A: the noise is drawn for every atom (a free atom's noise does not depend on the mask) and dropped where held."""
        m = self.m[:, None]
        hdt = 0.5 * self.dt
        p = project(self.p + hdt * forces, self.mask)
        r = self.r + hdt * p / m
        c1 = math.exp(-self.friction * self.dt)
        sig = np.sqrt((1.0 - c1 * c1) * self.m * KB * self.t0)[:, None]
        p = project(c1 * p + (sig * self.noise() if np.any(sig > 0) else 0.0), self.mask)
        if self.fixcm:
            p = project(p - m * (p.sum(axis=0) / self.m.sum()), self.mask)
        self.r = r + hdt * p / m
        self.p = p
        self.results = None

    def second_half(self, forces):
        self.p = project(self.p + 0.5 * self.dt * forces, self.mask)
        self.nsteps += 1

    def frame(self):
        fr = super().frame()
        fr["temperature"] = self.temperature()
        fr["forces"] = project(fr["forces"], self.mask)
        return fr


# ---- Nose-Hoover chains ------------------------------------------------------------------------------------------------------------
class FixedNHCRef(nhc_ref.NHCRef):
    def __init__(self, positions, cell, masses, momenta=None, mask=None, **kw):
        super().__init__(positions, cell, masses, momenta, **kw)
        self.mask = as_mask(mask, len(self.m))
        self.p = project(self.p, self.mask)
        if self.mask.any():                                     # a pinned atom breaks momentum conservation: N_f = dof
            held = self.mask.sum(1)
            assert not self.npt or np.all((held == 0) | (held == 3))
            M = len(self.v)
            self.nf = degrees_of_freedom(self.mask)
            assert self.nf > 0
            self.alpha = 1.0 + 3.0 / self.nf
            self.Q = np.full(M, self.kt * self.taut ** 2)
            self.Q[0] *= self.nf
            self.W = (self.nf + 3) * self.kt * self.taup ** 2

    def evaluate(self):
        e, f, s = super().evaluate()
        return e, project(f, self.mask), s

    def temperature(self):
        return temperature(self.p, self.m, self.mask)

    def particle_kick(self, forces, tau):
        super().particle_kick(forces, tau)
        self.p = project(self.p, self.mask)

    def first_half(self, forces, stress):
        super().first_half(forces, stress)                       # chain scaling and kick keep a zero at zero; held atoms scale with the cell
        self.p = project(self.p, self.mask)

    def second_half(self, forces, stress):
        super().second_half(forces, stress)
        self.p = project(self.p, self.mask)

    def frame(self):
        fr = super().frame()
        fr["temperature"] = self.temperature()
        fr["forces"] = project(fr["forces"], self.mask)
        return fr
