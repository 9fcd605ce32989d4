"""Float64 NumPy restatement of the device molecular dynamics (chgnet_amd/dynamics.py, csrc/kernels_md.h): what the reference's
``MolecularDynamics`` (chgnet/model/dynamics.py:433-780) runs through ASE >= 3.23, written from the semantics alone (DESIGN.md
"Molecular dynamics").  The tests compare the step kernel and the whole driver against it.  Each block names the ASE function it
restates; units are ASE's (eV, A, amu, time in A sqrt(amu / eV)).

The force / stress callback takes (positions [n,3], cell [3,3]) and returns (energy eV, forces eV/A [n,3], stress eV/A^3 [3,3]
without the ideal-gas term, ASE sign convention).
"""

from __future__ import annotations

import numpy as np

# ---- ase.units (CODATA 2014, ase/units.py) -----------------------------------------------------------------------------------
_E = 1.6021766208e-19       # C
_AMU = 1.660539040e-27      # kg
_K = 1.38064852e-23         # J/K
FS = 1e-15 * (1e10 * np.sqrt(_E / _AMU))    # units.fs = 1e-15 * second, second = 1e10 sqrt(e / amu)
KB = _K / _E                                 # units.kB = 8.6173303e-5 eV/K
GPA = 1e9 * ((1 / _E) / 1e30)               # units.GPa = 1e9 Pascal, Pascal = (1 / e) / 1e30 eV/A^3 = 1 / 160.21766208

NVE, NVT, NPT_INHOM, NPT_ISO = "nve", "nvt", "npt_inhomogeneous", "npt_berendsen"


def berendsen_lambda(temperature, target, dt, taut):
    """ase.md.nvtberendsen.NVTBerendsen.scale_velocities: sqrt(1 + (T0 / T - 1) dt / taut) clamped to [0.9, 1.1].  T = 0 gives numpy's
    inf -> 1.1; T = T0 = 0 (0 / 0) is taken as 1 here (ASE would carry a NaN)."""
    if temperature > 0:
        ratio = target / temperature
    else:
        ratio = np.inf if target > 0 else 1.0
    lam = np.sqrt(1.0 + (ratio - 1.0) * (dt / taut))
    if lam > 1.1:
        lam = 1.1
    if lam < 0.9:
        lam = 0.9
    return float(lam)


def kinetic_energy(p, masses):
    """ase.Atoms.get_kinetic_energy: 0.5 vdot(p, p / m)."""
    return 0.5 * float(np.vdot(p, p / masses[:, None]))


def temperature(p, masses):
    """ase.Atoms.get_temperature without constraints: 2 Ekin / (3 N kB)."""
    return 2.0 * kinetic_energy(p, masses) / (3 * len(masses) * KB)


def ideal_gas_stress(p, masses, cell):
    """The term ase.Atoms.get_stress(include_ideal_gas=True) adds: -sum_k p_a p_b / m_k / V (3x3)."""
    vol = abs(np.linalg.det(cell))
    return -np.einsum("ka,kb,k->ab", p, p, 1.0 / masses) / vol


def maxwell_boltzmann(masses, temperature_k, rng):
    """ase.md.velocitydistribution.MaxwellBoltzmannDistribution(force_temp=True) then Stationary(preserve_temperature=True), with a
    seeded Generator instead of ASE's global RNG (same distribution, different draws).  A single atom keeps p = 0 (ASE: NaN)."""
    masses = np.asarray(masses, np.float64)
    kt = KB * temperature_k
    p = rng.standard_normal((len(masses), 3)) * np.sqrt(masses * kt)[:, None]

    def force_temperature(p, target_kt):
        cur = 2 * kinetic_energy(p, masses) / (3 * len(masses))
        return p * np.sqrt(target_kt / cur) if cur > 0 else p

    p = force_temperature(p, kt)
    t0 = temperature(p, masses)
    p = p - (p.sum(0) / masses.sum()) * masses[:, None]      # Stationary: mass-weighted
    return force_temperature(p, t0 * KB)


class MDRef:
    """One replica: positions, momenta, masses, cell, cached evaluation; ``step`` is the ASE integrator's step."""

    def __init__(self, positions, cell, masses, momenta=None, *, ensemble=NVT, dt=2.0 * FS, temperature_k=300.0, taut=None, taup=None,
                 pressure=1.01325e-4 * GPA, compressibility=None, fixcm=True, calc=None):
        self.r = np.array(positions, np.float64).reshape(-1, 3)
        self.cell = np.array(cell, np.float64).reshape(3, 3)
        self.m = np.array(masses, np.float64)
        self.p = np.zeros_like(self.r) if momenta is None else np.array(momenta, np.float64).reshape(-1, 3)
        self.ensemble, self.dt, self.t0 = ensemble, float(dt), float(temperature_k)
        self.taut = 100 * self.dt if taut is None else float(taut)
        self.taup = 1000 * self.dt if taup is None else float(taup)
        self.pressure, self.kappa = float(pressure), compressibility
        self.fixcm = bool(fixcm) and ensemble != NVE        # VelocityVerlet has no fixcm
        self.calc = calc
        self.results = None                                   # (energy, forces, stress) of the current (r, cell)
        self.nsteps = 0
        self.n_evals = 0

    # ---- evaluation with ASE's calculator cache: a change of positions or cell invalidates it -----------------------------
    def evaluate(self):
        if self.results is None:
            e, f, s = self.calc(self.r.copy(), self.cell.copy())
            self.results = (float(e), np.asarray(f, np.float64), np.asarray(s, np.float64))
            self.n_evals += 1
        return self.results

    def _moved(self):
        self.results = None

    # ---- pieces, in ASE's order -------------------------------------------------------------------------------------------
    def scale_velocities(self):
        """NVTBerendsen.scale_velocities."""
        self.p = berendsen_lambda(temperature(self.p, self.m), self.t0, self.dt, self.taut) * self.p

    def scale_positions_and_cell(self, stress):
        """Inhomogeneous_NPTBerendsen / NPTBerendsen.scale_positions_and_cell; ``stress`` = the model's (3x3, eV/A^3).  The ideal-gas
        term uses the momenta as they are now (after scale_velocities).  Mask (1, 1, 1), pbc assumed.  set_cell(scale_atoms=True):
        positions <- positions . solve(cell, new_cell)."""
        st = stress + ideal_gas_stress(self.p, self.m, self.cell)
        if self.ensemble == NPT_INHOM:
            taupscl = self.dt * self.kappa / self.taup / 3.0
            sig = -np.diag(st)
            scl = np.array([1.0 - taupscl * (self.pressure - sig[i]) for i in range(3)])
            new = scl[:, None] * self.cell
        else:
            taupscl = self.dt / self.taup
            old_pressure = -np.trace(st) / 3
            new = (1.0 - taupscl * self.kappa / 3.0 * (self.pressure - old_pressure)) * self.cell
        self.r = self.r @ np.linalg.solve(self.cell, new)
        self.cell = new
        self._moved()

    def first_half(self, forces):
        """First half kick, fixcm (mean momentum p.sum(0) / N, NOT mass-weighted), drift r += dt p / m."""
        p = self.p + 0.5 * self.dt * forces
        if self.fixcm:
            p = p - p.sum(axis=0) / float(len(p))
        self.r = self.r + self.dt * p / self.m[:, None]
        self.p = p
        self._moved()

    def second_half(self, forces):
        self.p = self.p + 0.5 * self.dt * forces

    def step(self):
        """VelocityVerlet.step (NVE), NVTBerendsen.step (NVT), NPTBerendsen.step (both NPT flavours; the inhomogeneous one only
        overrides scale_positions_and_cell)."""
        if self.ensemble != NVE:
            self.scale_velocities()
        if self.ensemble in (NPT_INHOM, NPT_ISO):
            self.scale_positions_and_cell(self.evaluate()[2])
        _, f, _ = self.evaluate()                 # NPT: the scaled configuration is evaluated again
        self.first_half(f)
        _, f, _ = self.evaluate()
        self.second_half(f)
        self.nsteps += 1

    def frame(self):
        e, f, s = self.evaluate()
        return {"step": self.nsteps, "epot": e, "ekin": kinetic_energy(self.p, self.m), "temperature": temperature(self.p, self.m),
                "positions": self.r.copy(), "momenta": self.p.copy(), "cell": self.cell.copy(), "forces": f.copy(), "stress": s.copy()}

    def run(self, steps, loginterval=1):
        """Dynamics.irun: evaluate, observers at step 0, then step() and observers every loginterval steps."""
        frames = []
        self.evaluate()
        if self.nsteps == 0:
            frames.append(self.frame())
        for _ in range(steps):
            self.step()
            if self.nsteps % loginterval == 0:
                frames.append(self.frame())
        return frames


def pair_potential(eps=0.05, rc=4.0):
    """Smooth soft-sphere pair potential phi(d) = eps (1 - d / rc)^4 (C3 at the cutoff) over the 27 nearest images (cells wider
    than rc): callback (positions, cell) -> (E, F, stress), for conservation tests."""

    def calc(r, cell):
        n = len(r)
        e, f, vir = 0.0, np.zeros_like(r), np.zeros((3, 3))
        shifts = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], np.float64) @ cell
        for i in range(n):
            d = r[None, :, :] - r[i][None, None, :] + shifts[:, None, :]          # [27, n, 3]
            dist = np.linalg.norm(d, axis=-1)
            mask = (dist > 1e-9) & (dist < rc)
            x = 1.0 - dist[mask] / rc
            phi = eps * x ** 4
            dphi = -4.0 * eps / rc * x ** 3                                         # d phi / d dist
            e += 0.5 * phi.sum()
            u = d[mask] / dist[mask][:, None]
            f[i] += (dphi[:, None] * u).sum(0)
            vir += 0.5 * np.einsum("k,ka,kb->ab", dphi * dist[mask], u, u)
        return e, f, vir / abs(np.linalg.det(cell))
    return calc
