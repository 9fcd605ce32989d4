"""Float64 NumPy restatement of the replica-exchange event of the device Monte Carlo (chg_mc_set_exchange, csrc/kernels_mc_exchange.h)
over a list of ``mc_ref.McRef`` replicas, written from its specification (DESIGN.md "Monte Carlo", part "Replica exchange") alone:

  ladders:  a run of >= 2 consecutive replicas with the same id >= 0; -1 is never exchanged.  The rung of replica o is p = o - first.
    A rung keeps its temperature, seed, stream, counters, sums and best record; the configuration (positions, site[], E_cur) moves.
  events:  with t trials decided and interval > 0, event m = t / interval follows the decisions of every trial with t % interval == 0.
  pairs of event m:  rungs (p, p + 1) with p % 2 == (m - 1) & 1 and p + 1 <= L - 1.
  decision for (a, b) = (lower, upper):  skipped uncounted unless both are RUNNING.  u = U(w0, w1) of Philox4x32-10(counter (m, 0, 0, 2),
    key (seed_a & 0xffffffff, seed_a >> 32)); D = (1/(kB T_a) - 1/(kB T_b)) (E_a - E_b); accept iff D >= 0 or u < exp(D);
    attempts[a] += 1, accepts[a] += accepted.
  on acceptance:  rows, site[], E_cur and walker exchange; then each of the two rungs whose new E_cur < E_best takes it as its best
    record.  Sums, samples, move counters, E_trial and the pending record stay.
  walkers:  walker[o] starts as the rung index; mark / trips of walker w live at row first + w; mark = 1 for walker 0 at the start.
    Accepted with p == 0, w = walker[a] (after the exchange): trips[w] += 1 if mark[w] == 2; mark[w] = 1.  Accepted with p + 1 == L - 1,
    w = walker[b]: mark[w] = 2 if mark[w] == 1.

``xi`` mirrors the device's exchange state [B, 6]: walker, attempts, accepts, mark, trips, spare.
"""

from __future__ import annotations

import math

import numpy as np

from langevin_ref import _uniform, philox4x32_10
from md_ref import KB

_MASK = 0xFFFFFFFF
WALKER, ATTEMPTS, ACCEPTS, MARK, TRIPS = 0, 1, 2, 3, 4


def exchange_uniform(seed, m):
    seed = int(seed)
    w = philox4x32_10((int(m), 0, 0, 2), (seed & _MASK, seed >> 32))
    return _uniform(w[0], w[1])


def exchange_delta(t_a, t_b, e_a, e_b, kB=KB):
    return (1.0 / (kB * t_a) - 1.0 / (kB * t_b)) * (e_a - e_b)


def ladders_of(ladder):
    """[(first, L)] of the ladder ids; ``ValueError`` for what no pair list can be built from."""
    ladder = [int(v) for v in ladder]
    out, closed, o = [], set(), 0
    while o < len(ladder):
        v = ladder[o]
        if v < -1:
            raise ValueError(f"replica {o}: ladder id {v}")
        if v == -1:
            o += 1
            continue
        if v in closed:
            raise ValueError(f"replica {o}: ladder {v} reappears after another id")
        end = o
        while end < len(ladder) and ladder[end] == v:
            end += 1
        if end - o < 2:
            raise ValueError(f"replica {o}: a ladder of one replica")
        out.append((o, end - o))
        closed.add(v)
        o = end
    return out


def pairs_of(ladder, m):
    """[(a, first, L)] of event m: the lower replica of every pair."""
    parity = (int(m) - 1) & 1
    return [(first + p, first, L) for first, L in ladders_of(ladder) for p in range(parity, L - 1, 2)]


def initial_xi(ladder):
    xi = np.zeros((len(ladder), 6), np.int32)
    for first, L in ladders_of(ladder):
        xi[first:first + L, WALKER] = np.arange(L)
        xi[first, MARK] = 1
    return xi


class ExchangeRef:
    """A batch of ``McRef`` replicas with ladder ids.  ``running[o]``: the replica's status is RUNNING."""

    def __init__(self, replicas, ladder, interval=0, kB=KB, xi=None, running=None):
        self.reps, self.ladder, self.interval, self.kB = list(replicas), [int(v) for v in ladder], int(interval), float(kB)
        if len(self.reps) != len(self.ladder):
            raise ValueError("one ladder id per replica")
        if self.interval < 0:
            raise ValueError("interval < 0")
        for first, L in ladders_of(self.ladder):
            for o in range(first, first + L):
                if not self.reps[o].t > 0.0:
                    raise ValueError(f"replica {o}: T <= 0")
                if len(self.reps[o].r) != len(self.reps[first].r):
                    raise ValueError(f"replica {o}: another atom count")
        self.xi = initial_xi(self.ladder) if xi is None else np.array(xi, np.int32).reshape(len(self.reps), 6)
        self.running = [True] * len(self.reps) if running is None else [bool(x) for x in running]
        self.log = []

    def event(self, m):
        """Exchange event m; returns one record per pair: {"a", "m", "u", "delta", "accepted"} (accepted None: skipped)."""
        out = []
        for a, first, L in pairs_of(self.ladder, m):
            b, p = a + 1, a - first
            ra, rb = self.reps[a], self.reps[b]
            if not (self.running[a] and self.running[b]):
                out.append({"a": a, "m": m, "u": None, "delta": None, "accepted": None})
                continue
            u = exchange_uniform(ra.seed, m)
            delta = exchange_delta(ra.t, rb.t, ra.e_cur, rb.e_cur, self.kB)
            acc = delta >= 0.0 or u < math.exp(delta)
            self.xi[a, ATTEMPTS] += 1
            self.xi[a, ACCEPTS] += int(acc)
            if acc:
                ra.r, rb.r = rb.r, ra.r
                ra.site, rb.site = rb.site, ra.site
                ra.e_cur, rb.e_cur = rb.e_cur, ra.e_cur
                self.xi[a, WALKER], self.xi[b, WALKER] = self.xi[b, WALKER], self.xi[a, WALKER]
                if p == 0:
                    w = first + self.xi[a, WALKER]
                    if self.xi[w, MARK] == 2:
                        self.xi[w, TRIPS] += 1
                    self.xi[w, MARK] = 1
                if p + 1 == L - 1:
                    w = first + self.xi[b, WALKER]
                    if self.xi[w, MARK] == 1:
                        self.xi[w, MARK] = 2
                for x in (ra, rb):
                    if x.e_cur < x.e_best:
                        x.e_best, x.best_r, x.best_site = x.e_cur, x.r.copy(), x.site.copy()
            out.append({"a": a, "m": m, "u": u, "delta": delta, "accepted": bool(acc)})
        self.log += out
        return out

    def after_trial(self, t):
        """What follows the decisions of trial t (t trials decided)."""
        if self.interval > 0 and t >= 1 and t % self.interval == 0:
            return self.event(t // self.interval)
        return []

    def run(self, trials, t0=0, visit=None):
        """``trials`` lockstep trials of every replica through its ``calc``, events included; ``visit(t)`` after each."""
        for t in range(t0 + 1, t0 + trials + 1):
            for x in self.reps:
                x.propose()
                x.decide(x.calc(x.trial_positions(), x.cell))
            self.after_trial(t)
            if visit is not None:
                visit(t)
