"""Float64 NumPy restatement of the flexible-cell Nose-Hoover-chain NPT integrator of the device molecular dynamics (chgnet_amd/dynamics.py
``thermostat="Nose-Hoover-Chain", ensemble="npt", cell_dof="flexible" | "axes"``, csrc/kernels_md.h MD_NPT_NHC_FLEX / MD_NPT_NHC_AXES),
written from its specification alone: the Martyna-Tobias-Klein equations with a symmetric strain-rate matrix Vg in place of the scalar
veps of tests/nhc_ref.py, in the same reversible factorisation.  Conventions as there: rows of h are the lattice vectors, r, p, F are
row vectors, sigma is the potential's stress in ASE's sign, V = |det h|.

  kT = kB T,  N_f = 3 (n - 1) (with held atoms: the free components),  W = (N_f + 3) kT taup^2,  W_g = W / 3
  free components of Vg: all six symmetric ones ("flexible", d_b = 6) or the three diagonal ones ("axes", d_b = 3); the others stay 0
  Q'_1 = d_b kT taup^2,  Q'_k = kT taup^2 (k > 1);  the particle chain is that of nhc_ref
  state beyond nhc_ref: Vg [3, 3], zero at the start (veps is not used and stays 0)

  one step, tau = dt / 2, F and sigma cached, chain() of nhc_ref:
    Vg *= chain(vb, xi, Q', W_g sum_ab Vg_ab^2, d_b, tau)
    p  *= chain(v, eta, Q, sum p^2/m, N_f, tau)
    Vg_ab += tau G_ab / W_g on the free components,  G = sum p (x) p / m + (sum p^2/m / N_f - Pext V) I - V (sigma + sigma^T) / 2
    E = exp(-(Vg + tr Vg / N_f I) tau / 2);  p = (p E + tau F) E
    E = exp(Vg dt / 2);  r = (r E + dt p / m) E;  h = h exp(Vg dt)
    evaluation of E, F, sigma at (r, h)
    the first four lines in reverse order

  conserved: H = E + 1/2 sum p^2/m + 1/2 sum Q_k v_k^2 + N_f kT eta_1 + kT sum_{k>1} eta_k
                 + Pext V + 1/2 W_g sum_ab Vg_ab^2 + 1/2 sum Q'_k vb_k^2 + d_b kT xi_1 + kT sum_{k>1} xi_k

Held atoms (``mask`` [n, 3], True = held, whole atoms only): their forces and momenta are 0, so the drift leaves them the cell map
r <- r exp(Vg dt); every sum and N_f count the free components (the rules of constraint_ref.FixedNHCRef).
"""

from __future__ import annotations

import numpy as np

from nhc_ref import NHCRef

CELL_DOFS = ("flexible", "axes")


def expm_sym(a):
    """exp of a symmetric 3x3 matrix through its eigendecomposition, symmetrised to the bit."""
    w, v = np.linalg.eigh(np.asarray(a, np.float64))
    x = (v * np.exp(w)) @ v.T
    return 0.5 * (x + x.T)


def sym_outer_sum(p, m):
    """sum_i p_i (x) p_i / m_i, exactly symmetric: the upper triangle mirrored."""
    g = np.einsum("ka,kb,k->ab", p, p, 1.0 / m)
    return np.triu(g) + np.triu(g, 1).T


class NHCFlexRef(NHCRef):
    def __init__(self, positions, cell, masses, momenta=None, *, cell_dof="flexible", mask=None, **kw):
        assert cell_dof in CELL_DOFS
        kw["npt"] = True
        super().__init__(positions, cell, masses, momenta, **kw)
        n, M = len(self.m), len(self.v)
        self.cell_dof = cell_dof
        self.free = np.ones((3, 3), bool) if cell_dof == "flexible" else np.eye(3, dtype=bool)
        self.db = 6 if cell_dof == "flexible" else 3
        self.mask = np.zeros((n, 3), bool) if mask is None else np.array(mask, bool).reshape(n, 3)
        if self.mask.any():                                      # a pinned atom breaks momentum conservation: N_f = the free components
            held = self.mask.sum(1)
            assert np.all((held == 0) | (held == 3))             # the cell moves: whole atoms only
            self.nf = int((~self.mask).sum())
            assert self.nf > 0
            self.alpha = 1.0 + 3.0 / self.nf
            self.Q = np.full(M, self.kt * self.taut ** 2)
            self.Q[0] *= self.nf
            self.W = (self.nf + 3) * self.kt * self.taup ** 2
            self.p = np.where(self.mask, 0.0, self.p)
        self.Wg = self.W / 3.0
        self.Qb = np.full(M, self.kt * self.taup ** 2)
        self.Qb[0] *= self.db
        self.Vg = np.zeros((3, 3))

    def evaluate(self):
        e, f, s = super().evaluate()
        return e, np.where(self.mask, 0.0, f), s

    # ---- pieces ---------------------------------------------------------------------------------------------------------------
    def kb2(self):
        """Twice the kinetic energy of the cell: W_g sum_ab Vg_ab^2."""
        return self.Wg * float(np.sum(self.Vg * self.Vg))

    def barostat_chain(self, tau):
        self.Vg = self.Vg * self.chain(self.vb, self.xi, self.Qb, self.kb2(), self.db, tau)

    def particle_chain(self, tau):
        self.p = self.p * self.chain(self.v, self.eta, self.Q, self.k2(), self.nf, tau)

    def barostat_force(self, stress):
        vol = self.volume()
        stress = np.asarray(stress, np.float64).reshape(3, 3)
        return sym_outer_sum(self.p, self.m) + (self.k2() / self.nf - self.pext * vol) * np.eye(3) - vol * 0.5 * (stress + stress.T)

    def barostat_kick(self, stress, tau):
        self.Vg = self.Vg + np.where(self.free, tau * self.barostat_force(stress) / self.Wg, 0.0)

    def kick_factor(self, tau):
        return expm_sym(-(self.Vg + np.trace(self.Vg) / self.nf * np.eye(3)) * (0.5 * tau))

    def particle_kick(self, forces, tau):
        e = self.kick_factor(tau)
        self.p = np.where(self.mask, 0.0, (self.p @ e + tau * forces) @ e)

    def drift(self):
        e = expm_sym(self.Vg * (0.5 * self.dt))
        self.r = (self.r @ e + self.dt * self.p / self.m[:, None]) @ e
        self.cell = self.cell @ expm_sym(self.Vg * self.dt)
        self.results = None

    def first_half(self, forces, stress):
        tau = 0.5 * self.dt
        forces = np.where(self.mask, 0.0, forces)
        self.barostat_chain(tau)
        self.particle_chain(tau)
        self.barostat_kick(stress, tau)
        self.particle_kick(forces, tau)
        self.drift()

    def second_half(self, forces, stress):
        tau = 0.5 * self.dt
        forces = np.where(self.mask, 0.0, forces)
        self.particle_kick(forces, tau)
        self.barostat_kick(stress, tau)
        self.particle_chain(tau)
        self.barostat_chain(tau)
        self.nsteps += 1

    def reverse(self):
        super().reverse()
        self.Vg = -self.Vg

    def extended_energy(self):
        h = 0.5 * self.k2() + 0.5 * float(np.dot(self.Q, self.v ** 2)) + self.nf * self.kt * self.eta[0] + self.kt * float(self.eta[1:].sum())
        h += self.pext * self.volume() + 0.5 * self.kb2() + 0.5 * float(np.dot(self.Qb, self.vb ** 2))
        h += self.db * self.kt * self.xi[0] + self.kt * float(self.xi[1:].sum())
        return h

    def pressure_tensor(self):
        """Instantaneous pressure tensor of these equations of motion, G / V + Pext I (eV/A^3): sum p (x) p / (m V) - (sigma + sigma^T) / 2
        plus sum p^2/m / (N_f V) I, the 1 / N_f term that Martyna, Tobias and Klein add so that N_f momentum components -- not 3 n --
        give the ideal-gas pressure.  Its time average is Pext I on every free component of Vg, because Vg stays bounded."""
        _, _, s = self.evaluate()
        return (sym_outer_sum(self.p, self.m) + self.k2() / self.nf * np.eye(3)) / self.volume() - 0.5 * (s + s.T)

    def frame(self):
        fr = super().frame()
        fr["vg"] = self.Vg.copy()
        if self.mask.any():
            fr["temperature"] = 2.0 * fr["ekin"] / (self.nf * self.kt / self.t0)
        return fr
