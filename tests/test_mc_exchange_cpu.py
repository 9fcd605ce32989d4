"""Replica exchange without a GPU: the NumPy restatement (tests/mc_exchange_ref.py) keeps every rung of a tempering ladder on its own
Boltzmann distribution, the pairing, skipping, acceptance and round-trip rules hold on a hand-driven table, the binding mirrors the
header, and bad arguments are refused before a model is loaded."""

from __future__ import annotations

import itertools
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO
from mc_exchange_ref import ACCEPTS, ATTEMPTS, MARK, TRIPS, WALKER, ExchangeRef, exchange_delta, exchange_uniform, initial_xi, ladders_of, pairs_of
from mc_ref import McRef
from md_ref import KB
from test_mc_cpu import CELL, RING_SPECIES, SEEDS, ring_calc, ring_energy_of


# ---- 1. every rung samples its own Boltzmann distribution -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_every_rung_samples_its_boltzmann_distribution(seed):
    temps, interval, trials = (300.0, 600.0, 1200.0), 5, 20000
    positions = np.stack([np.arange(5.0), np.zeros(5), np.zeros(5)], axis=1)
    reps = [McRef(positions, CELL, RING_SPECIES, temperature_k=t, seed=seed + 1000 * rung, swap_probability=1.0, calc=ring_calc(RING_SPECIES))
            for rung, t in enumerate(temps)]
    occupations = sorted(set(itertools.permutations(RING_SPECIES.tolist())))
    assert len(occupations) == 20
    visits = [dict.fromkeys(occupations, 0) for _ in temps]
    ex = ExchangeRef(reps, [0, 0, 0], interval)
    for x in reps:
        x.run(0)

    def visit(t):  # noqa: ARG001
        for v, x in zip(visits, reps):
            v[tuple(x.species_on_sites().tolist())] += 1

    ex.run(trials, visit=visit)
    for rung, (t, v) in enumerate(zip(temps, visits)):
        weights = np.array([math.exp(-ring_energy_of(o) / (KB * t)) for o in occupations])
        weights /= weights.sum()
        tv = 0.5 * np.abs(np.array([v[o] for o in occupations]) / trials - weights).sum()
        print(f"seed {seed} rung {rung} ({t:.0f} K): total variation {tv:.4f}")
        assert tv < 0.03
        assert reps[rung].n_samples == trials and reps[rung].t == t
    assert ex.xi[:2, ATTEMPTS].tolist() == [trials // interval // 2] * 2 and ex.xi[2, ATTEMPTS] == 0
    for pair in range(2):
        acceptance = ex.xi[pair, ACCEPTS] / ex.xi[pair, ATTEMPTS]
        print(f"seed {seed} pair ({pair}, {pair + 1}): exchange acceptance {acceptance:.3f}")
        assert 0.7 < acceptance < 0.97            # both branches of the decision occur
    assert sorted(ex.xi[:, WALKER].tolist()) == [0, 1, 2]
    print(f"seed {seed}: round trips {ex.xi[:, TRIPS].tolist()}")
    assert ex.xi[:, TRIPS].sum() > 0


# ---- 2. a hand-driven event table ---------------------------------------------------------------------------------------------------------
def _replica(t, seed, e, n=4, tag=0.0):
    x = McRef(np.arange(3.0 * n).reshape(n, 3) + tag, CELL, [1, 2, 3, 1][:n], temperature_k=t, seed=seed)
    x.start(e)
    x.site = np.roll(np.arange(n), int(tag))
    return x


def test_pairs_alternate_by_parity():
    assert pairs_of([0, 0], 1) == [(0, 0, 2)] and pairs_of([0, 0], 2) == []
    assert pairs_of([4, 4, 4], 1) == [(0, 0, 3)] and pairs_of([4, 4, 4], 2) == [(1, 0, 3)] and pairs_of([4, 4, 4], 3) == [(0, 0, 3)]
    five = [7] * 5
    assert pairs_of(five, 1) == [(0, 0, 5), (2, 0, 5)]            # the odd ladder leaves its top rung out on odd events
    assert pairs_of(five, 2) == [(1, 0, 5), (3, 0, 5)]
    assert pairs_of(five, 70001) == pairs_of(five, 1)
    mixed = [-1, 3, 3, -1, 1, 1, 1, 1, 1, -1]
    assert ladders_of(mixed) == [(1, 2), (4, 5)]
    assert pairs_of(mixed, 1) == [(1, 1, 2), (4, 4, 5), (6, 4, 5)] and pairs_of(mixed, 2) == [(5, 4, 5), (7, 4, 5)]
    for m in (1, 2):                                              # the pairs of one event are disjoint
        members = [o for a, _, _ in pairs_of(mixed, m) for o in (a, a + 1)]
        assert len(members) == len(set(members))
    assert initial_xi(mixed)[:, WALKER].tolist() == [0, 0, 1, 0, 0, 1, 2, 3, 4, 0]
    assert initial_xi(mixed)[:, MARK].tolist() == [0, 1, 0, 0, 1, 0, 0, 0, 0, 0]
    for bad in ([0, 1, 0], [0, 0, 1], [2], [0, 0, -2]):
        with pytest.raises(ValueError):
            ladders_of(bad)


def test_decision_exchanges_configurations_and_keeps_the_rungs():
    # D >= 0 always accepts: the colder rung holds the higher energy, whatever u is; equal energies give D == 0
    for m in range(1, 40, 2):
        for e_a, e_b in ((-3.0, -3.5), (-3.0, -3.0)):
            a, b = _replica(300.0, 5, e_a), _replica(900.0, 6, e_b, tag=1.0)
            a.e_best, b.e_best = -3.2, -9.0
            best_b = b.best_r.copy()
            ra, rb, sa, sb = a.r.copy(), b.r.copy(), a.site.copy(), b.site.copy()
            ex = ExchangeRef([a, b], [0, 0])
            rec, = ex.event(m)
            assert rec["delta"] == exchange_delta(300.0, 900.0, e_a, e_b) >= 0.0 and rec["accepted"] and rec["u"] == exchange_uniform(5, m)
            assert np.array_equal(a.r, rb) and np.array_equal(b.r, ra) and np.array_equal(a.site, sb) and np.array_equal(b.site, sa)
            assert (a.e_cur, b.e_cur) == (e_b, e_a) and (a.t, b.t, a.seed, b.seed) == (300.0, 900.0, 5, 6)
            # the incoming energy below the rung's best replaces it (strict <), the one above does not
            assert a.e_best == (e_b if e_b < -3.2 else -3.2) and b.e_best == -9.0 and np.array_equal(b.best_r, best_b)
            if e_b < -3.2:
                assert np.array_equal(a.best_r, rb) and np.array_equal(a.best_site, sb)
            assert ex.xi[:, WALKER].tolist() == [1, 0] and ex.xi[0, 1:3].tolist() == [1, 1] and ex.xi[1, 1:3].tolist() == [0, 0]
            assert a.n_samples == b.n_samples == 0 and a.sum_e == 0.0 and a.pending is None
    # D < 0: accepted iff u < exp(D); both outcomes occur over the events
    seen = set()
    for m in range(1, 60, 2):
        a, b = _replica(300.0, 5, -3.5), _replica(900.0, 6, -3.47, tag=1.0)
        ra = a.r.copy()
        rec, = ExchangeRef([a, b], [0, 0]).event(m)
        assert rec["delta"] < 0 and rec["accepted"] == (rec["u"] < math.exp(rec["delta"]))
        assert np.array_equal(b.r if rec["accepted"] else a.r, ra)
        seen.add(rec["accepted"])
    assert seen == {True, False}
    # an even event has no pair in a two-rung ladder; a -1 replica is never touched
    a, b, c = _replica(300.0, 5, -3.0), _replica(900.0, 6, -3.5, tag=1.0), _replica(900.0, 7, -9.0, tag=2.0)
    ex = ExchangeRef([a, b, c], [0, 0, -1])
    assert ex.event(2) == [] and a.e_cur == -3.0 and not ex.xi[:, 1:3].any()
    ex.event(1)
    assert c.e_cur == -9.0 and ex.xi[2].tolist() == [0] * 6


def test_a_member_that_is_not_running_skips_without_counting():
    reps = [_replica(300.0 * (o + 1), o, -3.0 - 0.5 * o, tag=float(o)) for o in range(5)]    # every pair would accept: D > 0
    ex = ExchangeRef(reps, [0] * 5, running=[True, True, True, False, True])
    recs = ex.event(1)                                               # pairs (0,1), (2,3): the second has a stopped member
    assert [r["accepted"] for r in recs] == [True, None]
    assert ex.xi[:, ATTEMPTS].tolist() == [1, 0, 0, 0, 0] and reps[2].e_cur == -4.0 and reps[3].e_cur == -4.5
    recs = ex.event(2)                                               # pairs (1,2), (3,4)
    assert [r["accepted"] for r in recs] == [True, None] and ex.xi[:, ATTEMPTS].tolist() == [1, 1, 0, 0, 0]
    assert ex.xi[:, WALKER].tolist() == [1, 2, 0, 3, 4]


def test_round_trips_count_bottom_top_bottom_journeys():
    def force(ex):                                                   # energies that rise with the rung: every pair accepts
        for o, x in enumerate(ex.reps):
            x.e_cur = -5.0 - o
    reps = [_replica(300.0 * (o + 1), o, 0.0, tag=float(o)) for o in range(3)]
    ex = ExchangeRef(reps, [0, 0, 0])
    table = [  # after event m: walkers per rung, marks per walker, trips per walker
        (1, [1, 0, 2], [1, 1, 0], [0, 0, 0]),     # (0,1): walker 1 reaches the bottom
        (2, [1, 2, 0], [2, 1, 0], [0, 0, 0]),     # (1,2): walker 0 reaches the top having seen the bottom
        (3, [2, 1, 0], [2, 1, 1], [0, 0, 0]),     # (0,1): walker 2 reaches the bottom; it never saw the top: no trip
        (4, [2, 0, 1], [2, 2, 1], [0, 0, 0]),     # (1,2): walker 1 reaches the top
        (5, [0, 2, 1], [1, 2, 1], [1, 0, 0]),     # (0,1): walker 0 is back at the bottom: one round trip
        (6, [0, 1, 2], [1, 2, 2], [1, 0, 0]),     # (1,2): walker 2 reaches the top
        (7, [1, 0, 2], [1, 1, 2], [1, 1, 0]),     # (0,1): walker 1 completes its journey
    ]
    for m, walkers, marks, trips in table:
        force(ex)
        assert all(r["accepted"] for r in ex.event(m))
        assert (ex.xi[:, WALKER].tolist(), ex.xi[:, MARK].tolist(), ex.xi[:, TRIPS].tolist()) == (walkers, marks, trips), m
    # two rungs: the bottom is one exchange away from the top
    two = ExchangeRef([_replica(300.0, 1, 0.0), _replica(600.0, 2, 0.0, tag=1.0)], [0, 0])
    for m, trips in ((1, [0, 0]), (3, [1, 0]), (5, [1, 1]), (7, [2, 1])):
        force(two)
        two.event(m)
        assert two.xi[:, TRIPS].tolist() == trips, m
    # the restatement refuses what the engine refuses
    with pytest.raises(ValueError, match="T <= 0"):
        ExchangeRef([_replica(0.0, 1, 0.0), _replica(600.0, 2, 0.0)], [0, 0])
    with pytest.raises(ValueError, match="atom count"):
        ExchangeRef([_replica(300.0, 1, 0.0, n=3), _replica(600.0, 2, 0.0)], [0, 0])
    with pytest.raises(ValueError, match="interval"):
        ExchangeRef([_replica(300.0, 1, 0.0), _replica(600.0, 2, 0.0)], [0, 0], interval=-1)


# ---- 3. binding and ABI -------------------------------------------------------------------------------------------------------------------
EXCHANGE_SYMBOLS = ("chg_mc_set_exchange", "chg_mc_download_exchange", "chg_test_mc_exchange")


def test_header_binding_and_library_carry_the_exchange_entry_points_without_a_bump():
    from chgnet_amd import _lib

    header = open(os.path.join(REPO, "include", "chgnet_hip.h")).read()
    assert int(re.search(r"#define\s+CHG_ABI_VERSION\s+(\d+)", header).group(1)) == 5 == _lib.ABI_VERSION
    lib = _lib.load()
    assert int(lib.chg_abi_version()) == 5
    for name in EXCHANGE_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(rf"\bint\s+{name}\s*\(", header), name
    assert int(re.search(r"#define\s+CHG_MC_EXCHANGE_INTS\s+(\d+)", header).group(1)) == 6 == _lib.MC_EXCHANGE_INTS
    assert len(lib.chg_mc_set_exchange.argtypes) == 4 and len(lib.chg_mc_download_exchange.argtypes) == 3
    assert len(lib.chg_test_mc_exchange.argtypes) == 15


# ---- 4. argument refusals without a device ------------------------------------------------------------------------------------------------
def _limn(scale=4.0, species=("Li", "Mn", "O", "O")):
    from chgnet_amd.graph.structure import Lattice, Structure

    return Structure(Lattice(np.eye(3) * scale), list(species), [[0, 0, 0], [0.5, 0.5, 0.5], [0.5, 0, 0], [0, 0.5, 0]])


@pytest.mark.parametrize(("structure", "temperatures", "kwargs", "error", "match"), [
    ("one", [300.0], {}, ValueError, "at least two"),
    ("one", [], {}, ValueError, "at least two"),
    ("one", 300.0, {}, TypeError, "sequence"),
    ("one", [300.0, 0.0], {}, ValueError, r"temperatures\[1\]"),
    ("one", [-5.0, 300.0], {}, ValueError, r"temperatures\[0\]"),
    ("one", [300.0, float("nan")], {}, ValueError, "finite"),
    ("one", [300.0, "hot"], {}, TypeError, "temperatures"),
    ("one", [300.0, 600.0], dict(exchange_interval=-1), ValueError, "exchange_interval"),
    ("one", [300.0, 600.0], dict(exchange_interval=2.5), ValueError, "exchange_interval"),
    ("one", [300.0, 600.0], dict(exchange_interval="3"), TypeError, "exchange_interval"),
    ("one", [300.0, 600.0], dict(seeds=[1]), ValueError, "seeds"),
    ("one", [300.0, 600.0], dict(swap_probability=1.5), ValueError, "swap_probability"),
    ("three", [300.0, 600.0], {}, ValueError, "starting structures"),
    ("order", [300.0, 600.0], {}, ValueError, "rung 1 has other species"),
    ("cell", [300.0, 600.0], {}, ValueError, "rung 1 has another cell"),
])
def test_parallel_tempering_checks_arguments_before_a_model_is_loaded(structure, temperatures, kwargs, error, match):
    from chgnet_amd.montecarlo import ParallelTempering

    s = {"one": _limn(), "three": [_limn()] * 3, "order": [_limn(), _limn(species=("Mn", "Li", "O", "O"))],
         "cell": [_limn(), _limn(scale=4.0 + 1e-12)]}[structure]
    with pytest.raises(error, match=match):
        ParallelTempering(s, temperatures, model=object(), **kwargs)


def test_ladder_arguments_are_normalised_and_the_package_exports_them():
    import chgnet_amd
    from chgnet_amd.montecarlo import MonteCarlo, ParallelTempering, temperature_ladder

    assert chgnet_amd.ParallelTempering is ParallelTempering and chgnet_amd.temperature_ladder is temperature_ladder
    t = temperature_ladder(300.0, 2400.0, 4)
    np.testing.assert_allclose(t, [300.0, 600.0, 1200.0, 2400.0], rtol=1e-14)
    assert t[0] == 300.0 and t[-1] == 2400.0
    for args, error in (((300.0, 300.0, 3), ValueError), ((0.0, 300.0, 3), ValueError), ((300.0, 600.0, 1), ValueError), ((300.0, 600.0, 2.5), ValueError),
                        (("a", 600.0, 3), TypeError)):
        with pytest.raises(error):
            temperature_ladder(*args)
    pt = ParallelTempering([_limn(), _limn()], t[:2], model=object(), exchange_interval=3, swap_species=("Li", "Mn"))
    assert len(pt) == 2 and pt.exchange_interval == 3 and pt.temperatures.tolist() == [300.0, 600.0]
    assert [m.seed for m in pt._mc] == [0, 1] and pt._mc[1].swap_z.tolist() == [3, 25]
    with pytest.raises(ValueError, match="nothing has run yet"):
        pt.exchange_acceptance
    for kwargs, error, match in ((dict(ladders=[0]), ValueError, "one id per structure"), (dict(ladders=[0, -2]), ValueError, "ladders"),
                                 (dict(ladders=[0, 0.5]), ValueError, "ladders"), (dict(ladders=[0, "0"]), TypeError, "ladders"),
                                 (dict(ladders=[0, 0], exchange_interval=-3), ValueError, "exchange_interval"),
                                 (dict(ladders=[0, 0], exchange_interval=1.5), ValueError, "exchange_interval")):
        with pytest.raises(error, match=match):
            MonteCarlo.run_batch([_limn(), _limn()], 5, temperatures=[300.0, 600.0], model=object(), **kwargs)
