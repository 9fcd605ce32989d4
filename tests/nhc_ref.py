"""Float64 NumPy restatement of the Nose-Hoover-chain integrators of the device molecular dynamics (chgnet_amd/dynamics.py
``thermostat="Nose-Hoover-Chain"``, csrc/kernels_md.h MD_NVT_NHC / MD_NPT_NHC), written from their specification alone: the
Martyna-Tobias-Klein equations of motion with Nose-Hoover chains on the particles and on the barostat, isotropic cell, in the
reversible factorisation of Tuckerman, Alejandre, Lopez-Rendon, Jochim and Martyna, J. Phys. A 39 (2006) 5629.

  kT = kB T,  N_f = 3 (n - 1),  alpha = 1 + 3 / N_f
  Q_1 = N_f kT taut^2,  Q_k = kT taut^2 (k > 1),  Q'_k = kT taup^2,  W = (N_f + 3) kT taup^2
  state: chain velocities v[M] and positions eta[M] (particles), vb[M] and xi[M] (barostat), strain rate veps; all start at 0

  chain(v, eta, Q, K2, dof, tau) -> s, with K2 twice the kinetic energy it thermostats:
    G(k) = (K2 - dof kT) / Q[0]             if k == 0
           (Q[k-1] v[k-1]^2 - kT) / Q[k]    otherwise
    for k = M-1 .. 0:  if k < M-1: v[k] *= exp(-tau/4 v[k+1]);  v[k] += tau/2 G(k);  if k < M-1: v[k] *= exp(-tau/4 v[k+1])
    s = exp(-tau v[0]);  K2 *= s^2;  eta += tau v
    for k = 0 .. M-1:  the same three operations, G from the updated K2 and v

  one step, tau = dt / 2, F and sigma cached ([npt] lines are skipped for NVT, where veps = 0):
    [npt] veps *= chain(vb, xi, Q', W veps^2, 1, tau)
          p    *= chain(v, eta, Q, sum p^2/m, N_f, tau)
    [npt] veps += tau (alpha sum p^2/m - V tr sigma - 3 Pext V) / W
          e = exp(-alpha veps tau/2);  p = (p e + tau F) e
          e = exp(veps dt/2);  r = (r e + dt p/m) e;  h *= exp(veps dt)
          evaluation of E, F, sigma at (r, h)
          e = exp(-alpha veps tau/2);  p = (p e + tau F) e
    [npt] veps += tau (alpha sum p^2/m - V tr sigma - 3 Pext V) / W
          p    *= chain(v, eta, Q, sum p^2/m, N_f, tau)
    [npt] veps *= chain(vb, xi, Q', W veps^2, 1, tau)

  conserved: H = E + 1/2 sum p^2/m + 1/2 sum Q_k v_k^2 + N_f kT eta_1 + kT sum_{k>1} eta_k
             [npt] + Pext V + 1/2 W veps^2 + 1/2 sum Q'_k vb_k^2 + kT sum xi_k

sigma is the potential's stress (eV/A^3, ASE's sign, no ideal-gas term), V = |det h|.  The centre-of-mass momentum is never touched
here: the caller removes it once.  Units are ASE's (md_ref: eV, A, amu, time in A sqrt(amu / eV)).
"""

from __future__ import annotations

import math

import numpy as np

from md_ref import FS, GPA, KB, kinetic_energy, pair_potential, temperature  # noqa: F401  (re-exported for the tests)


def remove_com_momentum(p, masses):
    """p_i -= m_i sum p / sum m (what MolecularDynamics does once, when the handle is created)."""
    masses = np.asarray(masses, np.float64)
    return p - masses[:, None] * (p.sum(axis=0) / masses.sum())


class NHCRef:
    """One replica, shaped like ``md_ref.MDRef``: ``calc(positions, cell) -> (energy, forces, stress)``."""

    def __init__(self, positions, cell, masses, momenta=None, *, npt=False, dt=2.0 * FS, temperature_k=300.0, taut=None, taup=None,
                 pressure=1.01325e-4 * GPA, chain_length=3, calc=None):
        self.r = np.array(positions, np.float64).reshape(-1, 3)
        self.cell = np.array(cell, np.float64).reshape(3, 3)
        self.m = np.array(masses, np.float64)
        self.p = np.zeros_like(self.r) if momenta is None else np.array(momenta, np.float64).reshape(-1, 3)
        self.npt, self.dt, self.t0 = bool(npt), float(dt), float(temperature_k)
        self.taut = 100 * self.dt if taut is None else float(taut)
        self.taup = 1000 * self.dt if taup is None else float(taup)
        self.pext = float(pressure)
        n, M = len(self.m), int(chain_length)
        self.kt = KB * self.t0
        self.nf = 3 * (n - 1)
        self.alpha = 1.0 + 3.0 / self.nf
        self.Q = np.full(M, self.kt * self.taut ** 2)
        self.Q[0] *= self.nf
        self.Qb = np.full(M, self.kt * self.taup ** 2)
        self.W = (self.nf + 3) * self.kt * self.taup ** 2
        self.v, self.eta, self.vb, self.xi = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M)
        self.veps = 0.0
        self.calc = calc
        self.results = None
        self.nsteps = 0
        self.n_evals = 0

    def evaluate(self):
        if self.results is None:
            e, f, s = self.calc(self.r.copy(), self.cell.copy())
            self.results = (float(e), np.asarray(f, np.float64), np.asarray(s, np.float64))
            self.n_evals += 1
        return self.results

    # ---- pieces ---------------------------------------------------------------------------------------------------------------
    def k2(self):
        return float(np.vdot(self.p, self.p / self.m[:, None]))

    def volume(self):
        return abs(float(np.linalg.det(self.cell)))

    def chain(self, v, eta, Q, K2, dof, tau):
        """Half a step of one chain, in place on v and eta; returns the factor for the momentum (or veps) it thermostats."""
        M, kt = len(v), self.kt

        def sweep(order, K2):
            for k in order:
                G = (K2 - dof * kt) / Q[0] if k == 0 else (Q[k - 1] * v[k - 1] ** 2 - kt) / Q[k]
                if k < M - 1:
                    v[k] *= math.exp(-0.25 * tau * v[k + 1])
                v[k] += 0.5 * tau * G
                if k < M - 1:
                    v[k] *= math.exp(-0.25 * tau * v[k + 1])

        sweep(range(M - 1, -1, -1), K2)
        s = math.exp(-tau * v[0])
        K2 = K2 * s * s
        eta += tau * v
        sweep(range(M), K2)
        return s

    def barostat_kick(self, stress, tau):
        vol = self.volume()
        self.veps += tau * (self.alpha * self.k2() - vol * float(np.trace(stress)) - 3.0 * self.pext * vol) / self.W

    def particle_kick(self, forces, tau):
        e = math.exp(-0.5 * self.alpha * self.veps * tau)
        self.p = (self.p * e + tau * forces) * e

    def first_half(self, forces, stress):
        """Everything of a step before its evaluation, with the cached forces and stress."""
        tau = 0.5 * self.dt
        if self.npt:
            self.veps *= self.chain(self.vb, self.xi, self.Qb, self.W * self.veps ** 2, 1, tau)
        self.p = self.p * self.chain(self.v, self.eta, self.Q, self.k2(), self.nf, tau)
        if self.npt:
            self.barostat_kick(stress, tau)
        self.particle_kick(forces, tau)
        e = math.exp(0.5 * self.veps * self.dt)
        self.r = (self.r * e + self.dt * self.p / self.m[:, None]) * e
        self.cell = self.cell * math.exp(self.veps * self.dt)
        self.results = None

    def second_half(self, forces, stress):
        tau = 0.5 * self.dt
        self.particle_kick(forces, tau)
        if self.npt:
            self.barostat_kick(stress, tau)
        self.p = self.p * self.chain(self.v, self.eta, self.Q, self.k2(), self.nf, tau)
        if self.npt:
            self.veps *= self.chain(self.vb, self.xi, self.Qb, self.W * self.veps ** 2, 1, tau)
        self.nsteps += 1

    def step(self):
        _, f, s = self.evaluate()
        self.first_half(f, s)
        _, f, s = self.evaluate()
        self.second_half(f, s)

    def reverse(self):
        """Negate every velocity-like variable: running on retraces the trajectory."""
        self.p, self.v, self.vb, self.veps = -self.p, -self.v, -self.vb, -self.veps

    def extended_energy(self):
        """H - E: everything of the conserved quantity but the potential energy."""
        h = 0.5 * self.k2() + 0.5 * float(np.dot(self.Q, self.v ** 2)) + self.nf * self.kt * self.eta[0] + self.kt * float(self.eta[1:].sum())
        if self.npt:
            h += self.pext * self.volume() + 0.5 * self.W * self.veps ** 2 + 0.5 * float(np.dot(self.Qb, self.vb ** 2))
            h += self.kt * float(self.xi.sum())
        return h

    def conserved(self):
        return self.evaluate()[0] + self.extended_energy()

    def frame(self):
        e, f, s = self.evaluate()
        return {"step": self.nsteps, "epot": e, "ekin": kinetic_energy(self.p, self.m), "temperature": temperature(self.p, self.m),
                "positions": self.r.copy(), "momenta": self.p.copy(), "cell": self.cell.copy(), "forces": f.copy(), "stress": s.copy(),
                "conserved": self.conserved(), "veps": self.veps}

    def run(self, steps, loginterval=1):
        """As ``MDRef.run``: the frame of step 0 on the first call, then a frame every ``loginterval`` steps."""
        frames = []
        self.evaluate()
        if self.nsteps == 0:
            frames.append(self.frame())
        for _ in range(steps):
            self.step()
            if self.nsteps % loginterval == 0:
                frames.append(self.frame())
        return frames
