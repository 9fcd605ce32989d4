"""Float64 NumPy restatement of the canonical Monte Carlo sampler of the device (chgnet_amd/montecarlo.py, csrc/kernels_mc.h),
written from its specification (DESIGN.md "Monte Carlo") alone:

  lists, fixed at creation:  movable = atoms not held, in atom order; swappable = movable atoms whose species is in the swap set
    (default: all), sorted by (species, atom index), in groups of equal species.
  random numbers:  block(k, b) = Philox4x32-10(counter (k, b, 0, 1), key (seed & 0xffffffff, seed >> 32)), k = trials proposed so far;
    each block gives the uniforms U(w0, w1), U(w2, w3) of langevin_ref._uniform.
  proposal k:  (u_kind, u_acc) = block(k, 0); swap iff u_kind < swap_probability.
    swap:  (u1, u2) = block(k, 1); t = min(floor(u1 n_s), n_s - 1), i = swappable[t], g = group of t with n_g members;
           t2 = min(floor(u2 (n_s - n_g)), n_s - n_g - 1), t2 += n_g if t2 >= start(g); j = swappable[t2]; positions of i and j exchange.
    displacement:  (u1, u2) = block(k, 1), (u3, u4) = block(k, 2); atom movable[min(floor(u1 n_m), n_m - 1)],
           delta = max_displacement (2 (u2, u3, u4) - 1).
  decision:  dE = E_trial - E_cur; accept iff dE <= 0 or (T > 0 and u_acc < exp(-dE / (kB T))).  An accepted move is committed to the
    positions, a swap also to site[] (site[a]: the input row atom a sits on).
  statistics:  trials and acceptances per kind; after every decision n_samples += 1, sumE += E_cur, sumE2 += E_cur^2; the lowest energy
    seen with its positions and site[].  The first evaluation sets E_cur and the best record; it is neither a trial nor a sample.

``calc(positions, cell) -> energy`` (total, eV) drives ``run``; ``propose`` / ``decide`` drive it from recorded energies.
"""

from __future__ import annotations

import math

import numpy as np

from langevin_ref import _uniform, philox4x32_10
from md_ref import KB

_MASK = 0xFFFFFFFF
SWAP, DISPLACE = 0, 1


def block(seed, k, b):
    """The two uniforms of block b of trial k."""
    seed = int(seed)
    w = philox4x32_10((k, b, 0, 1), (seed & _MASK, seed >> 32))
    return _uniform(w[0], w[1]), _uniform(w[2], w[3])


def atom_lists(species, swap_species=None, fixed=None):
    """(movable, swappable, group start per swappable entry, group size per swappable entry) of one replica."""
    species = [int(s) for s in species]
    held = np.zeros(len(species), bool) if fixed is None else np.asarray(fixed, bool)
    movable = [a for a in range(len(species)) if not held[a]]
    allowed = None if swap_species is None else {int(s) for s in swap_species}
    swappable = sorted((a for a in movable if allowed is None or species[a] in allowed), key=lambda a: (species[a], a))
    gstart, gsize = [], []
    for t, a in enumerate(swappable):
        members = [u for u, b in enumerate(swappable) if species[b] == species[a]]
        gstart.append(members[0])
        gsize.append(len(members))
    return movable, swappable, gstart, gsize


class McRef:
    """One replica.  ``k``: trials proposed so far (the stream is a function of (seed, k) alone)."""

    def __init__(self, positions, cell, species, *, temperature_k=300.0, seed=0, swap_probability=1.0, max_displacement=0.1,
                 swap_species=None, fixed=None, kB=KB, calc=None, k=0):
        self.r = np.array(positions, np.float64).reshape(-1, 3)
        self.cell = np.array(cell, np.float64).reshape(3, 3)
        self.species = np.array(species)
        self.t, self.seed, self.kB = float(temperature_k), int(seed), float(kB)
        self.swap_probability, self.max_displacement = float(swap_probability), float(max_displacement)
        self.movable, self.swappable, self.gstart, self.gsize = atom_lists(species, swap_species, fixed)
        self.calc = calc
        self.site = np.arange(len(self.r))
        self.k = int(k)
        self.started = False
        self.e_cur = self.e_best = None
        self.best_r, self.best_site = self.r.copy(), self.site.copy()
        self.counts = {SWAP: [0, 0], DISPLACE: [0, 0]}   # trials, acceptances
        self.n_samples, self.sum_e, self.sum_e2 = 0, 0.0, 0.0
        self.pending = None
        self.last = None

    # ---- the three phases
    def start(self, energy):
        """The first evaluation: E_cur and the best record."""
        self.e_cur = self.e_best = float(energy)
        self.best_r, self.best_site = self.r.copy(), self.site.copy()
        self.started = True

    def propose(self):
        """Draw trial k and keep it pending: {"kind", "i", "j", "delta", "u_acc"}."""
        k = self.k
        u_kind, u_acc = block(self.seed, k, 0)
        u1, u2 = block(self.seed, k, 1)
        if u_kind < self.swap_probability:
            ns = len(self.swappable)
            t = min(int(math.floor(u1 * ns)), ns - 1)
            ng = self.gsize[t]
            t2 = min(int(math.floor(u2 * (ns - ng))), ns - ng - 1)
            if t2 >= self.gstart[t]:
                t2 += ng
            move = {"kind": SWAP, "i": self.swappable[t], "j": self.swappable[t2], "delta": np.zeros(3)}
        else:
            u3, u4 = block(self.seed, k, 2)
            nm = len(self.movable)
            move = {"kind": DISPLACE, "i": self.movable[min(int(math.floor(u1 * nm)), nm - 1)], "j": -1,
                    "delta": self.max_displacement * (2.0 * np.array([u2, u3, u4]) - 1.0)}
        move["u_acc"] = u_acc
        self.k = k + 1
        self.pending = move
        return move

    def trial_positions(self):
        r = self.r.copy()
        m = self.pending
        if m["kind"] == SWAP:
            r[[m["i"], m["j"]]] = r[[m["j"], m["i"]]]
        else:
            r[m["i"]] = r[m["i"]] + m["delta"]
        return r

    def decide(self, e_trial):
        """The Metropolis decision on the pending trial; returns True when accepted."""
        m, e_trial = self.pending, float(e_trial)
        d_e = e_trial - self.e_cur
        acc = d_e <= 0.0 or (self.t > 0.0 and m["u_acc"] < math.exp(-d_e / (self.kB * self.t)))
        self.counts[m["kind"]][0] += 1
        self.counts[m["kind"]][1] += int(acc)
        if acc:
            self.r = self.trial_positions()
            if m["kind"] == SWAP:
                self.site[[m["i"], m["j"]]] = self.site[[m["j"], m["i"]]]
            self.e_cur = e_trial
        self.n_samples += 1
        self.sum_e += self.e_cur
        self.sum_e2 += self.e_cur * self.e_cur
        if acc and self.e_cur < self.e_best:
            self.e_best, self.best_r, self.best_site = self.e_cur, self.r.copy(), self.site.copy()
        self.last = dict(m, accepted=bool(acc), e_trial=e_trial)
        self.pending = None
        return bool(acc)

    # ---- driven by calc
    def frame(self):
        last = self.last or {"kind": -1, "i": -1, "j": -1, "delta": np.zeros(3), "u_acc": 0.0, "accepted": False, "e_trial": self.e_cur}
        return {"trial": self.k, "e_cur": self.e_cur, **{key: last[key] for key in ("kind", "i", "j", "accepted", "e_trial", "u_acc")},
                "delta": np.array(last["delta"]), "positions": self.r.copy(), "site": self.site.copy()}

    def run(self, trials, loginterval=1):
        """Frame 0 on the first call, then a frame after every decision with k % loginterval == 0."""
        frames = []
        if not self.started:
            self.start(self.calc(self.r.copy(), self.cell.copy()))
            frames.append(self.frame())
        for _ in range(trials):
            self.propose()
            self.decide(self.calc(self.trial_positions(), self.cell.copy()))
            if loginterval and self.k % loginterval == 0:
                frames.append(self.frame())
        return frames

    def species_on_sites(self):
        out = np.empty_like(self.species)
        out[self.site] = self.species
        return out
