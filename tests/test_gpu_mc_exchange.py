"""Replica exchange on the MI355X: the exchange kernel against the float64 restatement (tests/mc_exchange_ref.py) bit for bit, a
four-rung ParallelTempering run replayed by the restatement from the logged trial energies, run_batch with ladders beside a lone
replica, and the engine's refusals."""

from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import mc_exchange_ref as xr
import mc_ref
from md_ref import KB
from test_gpu_mc import DELTA, E_BEST, E_CUR, E_TRIAL, SUM_E, SUM_E2, U_ACC, _replay, _structure

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(trained_like_weights):
    from chgnet_amd import CHGNet

    return CHGNet(state_dict=trained_like_weights)


# ---- 1. the exchange kernel on its own ------------------------------------------------------------------------------------------------
#          ladder 0: 2 x 2 atoms | lone: 5 atoms | ladder 1: 3 x 17 atoms | ladder 2: 5 x 300 atoms (rows beyond one pass of the workgroup)
SIZES = [2, 2, 5, 17, 17, 17, 300, 300, 300, 300, 300]
LADDER = [0, 0, -1, 1, 1, 1, 2, 2, 2, 2, 2]
TEMPS = [300.0, 900.0, 0.0, 400.0, 700.0, 1500.0, 300.0, 420.0, 600.0, 850.0, 1200.0]     # the lone replica may be greedy
SEEDS = [7, 99, 5, (1 << 32) + 12345, 3, (1 << 64) - 1, 0, 11, (1 << 40) + 1, 13, 14]
NONFINITE = 9                                                                             # rung 3 of ladder 2 has stopped
EVENTS = (1, 2, 70001)                                                                    # both parities; one above 2^16
# what the running pairs of every event are made to be (lower replica -> class)
PLAN = {1: {0: "positive", 3: "zero", 6: "accept"}, 2: {4: "reject", 7: "positive"}, 70001: {0: "reject", 3: "accept", 6: "zero"}}


def _kernel_case(m):
    """The batch on entry to event m: the restatement's replicas, the raw state arrays, and the class of every running pair."""
    rng = np.random.default_rng(1000 + m % 997)
    B = len(SIZES)
    cells = {}
    reps, sd, si = [], np.zeros((B, 32)), np.zeros((B, 8), np.int32)
    for o, (n, lad) in enumerate(zip(SIZES, LADDER)):
        cell = cells.setdefault((lad, n) if lad >= 0 else ("lone", o), np.diag(rng.uniform(5, 9, 3)) + rng.normal(0, 0.5, (3, 3)))
        z = np.resize([3, 25, 8], n)
        ref = mc_ref.McRef(rng.random((n, 3)) @ cell, cell, z, temperature_k=TEMPS[o], seed=SEEDS[o], k=int(rng.integers(1, 90)))
        ref.site = rng.permutation(n)
        ref.start(-40.0 - 0.37 * o)
        ref.best_r, ref.best_site = rng.random((n, 3)), rng.permutation(n)
        reps.append(ref)
    # energies by class: the Metropolis branch is steered through the event's own uniform, which depends on (seed_a, m) alone
    for a, kind in PLAN[m].items():
        ra, rb = reps[a], reps[a + 1]
        dbeta = 1.0 / (KB * ra.t) - 1.0 / (KB * rb.t)
        u = xr.exchange_uniform(ra.seed, m)
        want = {"positive": 1.3, "zero": 0.0, "accept": 0.5 * math.log(u), "reject": 2.0 * math.log(u) - 0.5}[kind]
        rb.e_cur = ra.e_cur if kind == "zero" else ra.e_cur - want / dbeta
    for o, ref in enumerate(reps):
        ref.e_best = ref.e_cur - (0.01 if o % 3 == 0 else 0.0)            # some rungs hold their best configuration, others do not
        sd[o, :9], sd[o, 9:18] = ref.cell.ravel(), np.linalg.inv(ref.cell).ravel()
        sd[o, [E_CUR, E_BEST]] = ref.e_cur, ref.e_best
        sd[o, [SUM_E, SUM_E2, E_TRIAL, U_ACC]] = rng.normal(size=4)      # none of the exchange's business: must come back untouched
        sd[o, DELTA:DELTA + 3] = rng.normal(size=3)
        si[o] = [ref.k, 1 if o == NONFINITE else 0, 1, -1, 0, 0, int(rng.integers(0, 2)), 0]
    # walkers mid-run: a permutation per ladder, marks and counts of any history
    xi = np.zeros((B, 6), np.int32)
    for first, L in xr.ladders_of(LADDER):
        xi[first:first + L, xr.WALKER] = np.roll(np.arange(L), 1)        # walker 0 sits on rung 1: at the top of a two-rung ladder
        xi[first:first + L, xr.MARK] = [2, 1, 0, 2, 1][:L]               # walker 0 has seen the top, walker 1 the bottom
        xi[first:first + L, 1:3] = np.sort(rng.integers(0, 50, (L, 2)), axis=1)[:, ::-1]   # attempts >= accepts
        xi[first:first + L, xr.TRIPS] = rng.integers(0, 9, L)
    ex = xr.ExchangeRef(reps, LADDER, xi=xi, running=[o != NONFINITE for o in range(B)])
    return ex, sd, si


def _launch_exchange(hip_engine, ex, sd, si, m):
    from chgnet_amd import _lib

    reps = ex.reps
    aoff = np.concatenate([[0], np.cumsum([len(x.r) for x in reps])]).astype(np.int32)
    state = {"r": np.concatenate([x.r for x in reps]), "site": np.concatenate([x.site for x in reps]).astype(np.int32), "sd": sd.copy(),
             "si": si.copy(), "best_pos": np.concatenate([x.best_r for x in reps]),
             "best_site": np.concatenate([x.best_site for x in reps]).astype(np.int32), "xi": ex.xi.copy()}
    state = {k: np.ascontiguousarray(v) for k, v in state.items()}
    before = {k: v.copy() for k, v in state.items()}
    ladder, temps, seeds = np.array(LADDER, np.int32), np.array(TEMPS), np.array(SEEDS, np.uint64)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(_lib.c_int_p)  # noqa: E731
    hip_engine._check(hip_engine.lib.chg_test_mc_exchange(
        hip_engine.handle, len(reps), ip(aoff), ip(ladder), dp(temps), seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), KB, m,
        dp(state["r"]), ip(state["site"]), dp(state["sd"]), ip(state["si"]), dp(state["best_pos"]), ip(state["best_site"]), ip(state["xi"])))
    return aoff, before, state


@pytest.mark.parametrize("m", EVENTS)
def test_exchange_kernel_matches_restatement_bit_for_bit(hip_engine, m):
    ex, sd, si = _kernel_case(m)
    aoff, before, got = _launch_exchange(hip_engine, ex, sd, si, m)
    best_before = [x.e_best for x in ex.reps]
    recs = ex.event(m)
    # the fixture: the planned classes occur and no decision sits on a rounding edge
    running = {r["a"]: r for r in recs if r["accepted"] is not None}
    assert sorted(running) == sorted(PLAN[m]) and [r["a"] for r in recs if r["accepted"] is None] == ([8] if m % 2 else [9])
    for a, kind in PLAN[m].items():
        r = running[a]
        assert abs(r["u"] - math.exp(r["delta"])) > 1e-9, r
        assert {"positive": r["delta"] > 0, "zero": r["delta"] == 0.0, "accept": r["delta"] < 0 and r["accepted"],
                "reject": r["delta"] < 0 and not r["accepted"]}[kind], (kind, r)
        assert r["accepted"] == (kind != "reject")
    # expected arrays from the restatement
    want_sd = sd.copy()
    for o, x in enumerate(ex.reps):
        want_sd[o, [E_CUR, E_BEST]] = x.e_cur, x.e_best
    want = {"r": np.concatenate([x.r for x in ex.reps]), "site": np.concatenate([x.site for x in ex.reps]), "sd": want_sd, "si": si,
            "best_pos": np.concatenate([x.best_r for x in ex.reps]), "best_site": np.concatenate([x.best_site for x in ex.reps]), "xi": ex.xi}
    for key, w in want.items():
        assert np.array_equal(got[key], w), key
    # replicas outside an accepted pair come back byte for byte (all but attempts of a rejected pair's lower rung)
    moved = {o for a, r in running.items() if r["accepted"] for o in (a, a + 1)}
    for o in range(len(SIZES)):
        if o in moved:
            continue
        sl = slice(aoff[o], aoff[o + 1])
        for key in ("r", "site", "best_pos", "best_site"):
            assert got[key][sl].tobytes() == before[key][sl].tobytes(), (o, key)
        assert got["sd"][o].tobytes() == before["sd"][o].tobytes() and got["si"][o].tobytes() == before["si"][o].tobytes()
        if o not in running:
            assert got["xi"][o, :3].tobytes() == before["xi"][o, :3].tobytes()
    assert np.array_equal(got["si"], before["si"])
    # accepted rows are copies of the partner's rows, and both sides of the best-record rule were met
    kept = [o for o in moved if ex.reps[o].e_best < best_before[o]]
    if m == 1:
        assert kept and set(moved) - set(kept)                               # an incoming energy below the rung's best, and one above
        for o in kept:
            sl = slice(aoff[o], aoff[o + 1])
            assert got["best_pos"][sl].tobytes() == got["r"][sl].tobytes() and np.array_equal(got["best_site"][sl], got["site"][sl])
        # ladder 0: walker 0 came back to the bottom having seen the top -- a round trip; walker 1 reached the top
        assert got["xi"][0, xr.TRIPS] == before["xi"][0, xr.TRIPS] + 1 and got["xi"][:2, xr.WALKER].tolist() == [0, 1]
        assert got["xi"][:2, xr.MARK].tolist() == [1, 2]
    for a, r in running.items():
        assert got["xi"][a, 1] == before["xi"][a, 1] + 1 and got["xi"][a, 2] == before["xi"][a, 2] + int(r["accepted"])
        if r["accepted"]:
            sa, sb = slice(aoff[a], aoff[a + 1]), slice(aoff[a + 1], aoff[a + 2])
            assert got["r"][sa].tobytes() == before["r"][sb].tobytes() and got["r"][sb].tobytes() == before["r"][sa].tobytes()


# ---- 2. end to end: a four-rung ladder replayed from the logged trial energies ---------------------------------------------------------
PT_TEMPS = (300.0, 2000.0, 2200.0, 5000.0)
PT_SEEDS = (0, 1, 2, 3)          # give accepted and rejected exchanges in 40 trials (asserted below)
PT_KW = dict(exchange_interval=3, swap_species=("Li", "Mn"), swap_probability=0.5, max_displacement=0.1, loginterval=1)


def _replay_ladder(trajs, s, seeds, temps, interval):
    """The restatement over the logged frames of every rung, deciding on the logged E_trial, with the events between the trials."""
    z, cell = np.asarray(s.atomic_numbers), s.lattice.matrix
    reps = []
    for tr, seed, t in zip(trajs, seeds, temps):
        ref = mc_ref.McRef(s.frac_coords @ cell, cell, z, temperature_k=t, seed=seed, swap_probability=0.5, max_displacement=0.1,
                           swap_species=(3, 25))
        assert tr.trials[0] == 0 and tr.kinds[0] is None and np.array_equal(tr.sites[0], np.arange(len(z)))
        np.testing.assert_allclose(tr.atom_positions[0], ref.r, rtol=0, atol=1e-12 * np.abs(ref.r).max())
        ref.r = tr.atom_positions[0].copy()                                 # from here on every row is compared bit for bit
        ref.start(tr.energies[0])
        reps.append(ref)
    ex = xr.ExchangeRef(reps, [0] * len(reps), interval)
    for f in range(1, len(trajs[0])):
        for rung, (tr, ref) in enumerate(zip(trajs, reps)):
            assert tr.trials[f] == f == ref.k + 1
            mv = ref.propose()
            assert (tr.kinds[f], tr.moves[f]) == (("swap", "displacement")[mv["kind"]], (mv["i"], mv["j"])), (rung, f, mv)
            assert tr.u_acc[f] == mv["u_acc"] and np.array_equal(tr.displacements[f], mv["delta"]), (rung, f)
            acc = ref.decide(tr.trial_energies[f])
            assert tr.accepted[f] == acc and tr.energies[f] == ref.e_cur, (rung, f)
            assert np.array_equal(tr.atom_positions[f], ref.r) and np.array_equal(tr.sites[f], ref.site), (rung, f)   # before the event
        ex.after_trial(f)
    return ex


def _assert_state(pt, ex):
    for rung, (st, ref) in enumerate(zip(pt.rungs, ex.reps)):
        assert st["energy"] == ref.e_cur and st["best"][0] == ref.e_best, rung
        assert np.array_equal(st["positions"], ref.r) and np.array_equal(st["site"], ref.site), rung   # after the last event
        assert np.array_equal(st["best_site"], ref.best_site), rung
        c = st["counts"]
        assert c[:5].tolist() == [*ref.counts[mc_ref.SWAP], *ref.counts[mc_ref.DISPLACE], ref.n_samples], rung
        np.testing.assert_allclose(st["sums"], [ref.sum_e, ref.sum_e2], rtol=1e-12)
        assert [st["walker"], st["exchange_attempts"], st["exchange_accepts"], st["round_trips"]] == ex.xi[rung, [0, 1, 2, 4]].tolist(), rung
        assert st["status"] == "RUNNING" and st["n_trials"] == ref.k and st["temperature"] == ref.t


ENERGY_ULPS = 16   # float32 ulps two evaluations of one configuration may differ by (below)


def _same_chain(xs, ys):
    """Two device runs of one batch (one trajectory per replica each), frame by frame; returns the number of frames over which they are the
    same chain.

    The sampler is a pure function of the seeds and of the energies the engine returns, and every run is checked against the
    restatement bit for bit from its own logged energies.  Two runs can be compared bit for bit only as far as the engine returns the
    same energies, and it does not: its float32 sums are accumulated by atomics in hardware order (DESIGN.md "Reproducibility": not
    bit-reproducible run to run, fp32 reassociation, about 1e-7 relative).  Measured here on one MI355X, 11 runs of this ladder and of
    the same batch without any ladder (MonteCarlo.run_batch as it was before replica exchange): every pair of runs differed in a logged
    E_trial of every replica within the first 0-35 frames, each time by exactly one float32 ulp of the per-atom energy (7.6e-6 eV of
    -93 eV), frame 0 -- the configuration as given -- included.  So: the draws (kind, atoms, u_acc, displacement) depend on (seed, trial)
    alone and must be equal in every frame; decisions, positions and site[] must be equal, and energies within ENERGY_ULPS float32
    ulps of the per-atom energy (the number format's precision with a margin of 16 for the depth of the sums), for as long as the two
    chains coincide; they may part -- a decision or an exchange that sits within an ulp of its threshold -- only at or after a frame
    whose logged energies differ.  Where the energies never differ the two runs are equal bit for bit."""
    differed = False
    for f in range(len(xs[0])):
        assert all(len(x) == len(xs[0]) == len(y) for x, y in zip(xs, ys))
        for x, y in zip(xs, ys):
            assert (x.trials[f], x.kinds[f], x.moves[f], x.u_acc[f]) == (y.trials[f], y.kinds[f], y.moves[f], y.u_acc[f]), f
            assert np.array_equal(x.displacements[f], y.displacements[f]), f
            differed |= x.trial_energies[f] != y.trial_energies[f]
        if not all(x.accepted[f] == y.accepted[f] and np.array_equal(x.atom_positions[f], y.atom_positions[f]) and
                   np.array_equal(x.sites[f], y.sites[f]) for x, y in zip(xs, ys)):
            assert differed, f"the chains part at frame {f} although the engine returned the same energies"
            return f
        for x, y in zip(xs, ys):
            n = len(x.atomic_numbers)
            ulp = n * float(np.spacing(np.float32(abs(x.trial_energies[f]) / n)))
            assert abs(x.trial_energies[f] - y.trial_energies[f]) <= ENERGY_ULPS * ulp, (f, x.trial_energies[f], y.trial_energies[f])
            assert abs(x.energies[f] - y.energies[f]) <= ENERGY_ULPS * ulp, (f, x.energies[f], y.energies[f])
            if not differed:
                assert x.energies[f] == y.energies[f]
    return len(xs[0])


def test_ladder_run_is_replayed_by_the_restatement_and_splits_do_not_matter(model):
    """The issue asks that the split run equal a fresh run of 40 trials bit for bit.  Both are replayed bit for bit by the restatement as
    one stream with the events between the trials, which is what makes the split immaterial; run against run they are compared by
    ``_same_chain``, because the engine's energies are not reproducible to the last float32 bit (figures there)."""
    from chgnet_amd.montecarlo import ParallelTempering

    s = _structure("limno2", (2, 1, 1), rattle=0.05, seed=3)
    assert len(s) == 16
    pt = ParallelTempering(s, PT_TEMPS, model=model, seeds=PT_SEEDS, **PT_KW)
    pt.run(17)
    trajs = pt.run(23)
    assert all(len(tr) == 41 and tr.trials == list(range(41)) for tr in trajs)
    ex = _replay_ladder(trajs, s, PT_SEEDS, PT_TEMPS, 3)
    outcomes = [(r["a"], r["m"], r["accepted"]) for r in ex.log]
    print("exchanges (lower rung, event, accepted):", outcomes)
    print("exchange acceptance", pt.exchange_acceptance, "walkers", pt.walkers, "round trips", pt.round_trips)
    assert len(ex.log) == 7 * 2 + 6 and max(r["m"] for r in ex.log) == 13            # the event of trial 39; none after trial 40
    assert any(r["accepted"] for r in ex.log) and any(r["accepted"] is False for r in ex.log)
    _assert_state(pt, ex)
    x = ex.xi
    np.testing.assert_array_equal(pt.exchange_acceptance, x[:3, 2] / x[:3, 1])
    assert pt.walkers.tolist() == x[:, 0].tolist() and pt.round_trips.tolist() == x[:, 4].tolist() and sorted(pt.walkers.tolist()) == [0, 1, 2, 3]
    np.testing.assert_allclose(pt.mean_energies, [r.sum_e / 40 for r in ex.reps], rtol=1e-12)
    assert pt.heat_capacities().shape == (4,) and pt.best[0] == min(r.e_best for r in ex.reps)
    # an exchange shows between two frames: the rung's next frame starts from the partner's configuration
    r = next(r for r in ex.log if r["accepted"])
    a, f = r["a"], 3 * r["m"]
    if f + 1 < 41 and not trajs[a].accepted[f + 1]:
        assert np.array_equal(trajs[a].atom_positions[f + 1], trajs[a + 1].atom_positions[f])
    # one run of 40 trials: replayed by the same single stream, events included, and the same chain as the split run
    whole = ParallelTempering(s, PT_TEMPS, model=model, seeds=PT_SEEDS, **PT_KW)
    trajs_whole = whole.run(40)
    _assert_state(whole, _replay_ladder(trajs_whole, s, PT_SEEDS, PT_TEMPS, 3))
    frames = _same_chain(trajs, trajs_whole)
    print("split and whole run: the same chain over", frames, "of 41 frames")
    if frames == 41:
        for sa, sb in zip(pt.rungs, whole.rungs):
            for key in ("positions", "site", "counts", "best_site"):
                assert np.array_equal(sa[key], sb[key]), key
            for key in ("walker", "exchange_attempts", "exchange_accepts", "round_trips"):
                assert sa[key] == sb[key], key
    # statistics start afresh on request; a ladder member cannot be set to 0 K
    pt.reset_statistics()
    assert not pt.round_trips.any() and np.isnan(pt.exchange_acceptance).all()
    with pytest.raises(RuntimeError, match=r"chg_mc_set_temperatures: replica 2 of ladder 0 needs a temperature > 0"):
        pt._run.set_temperatures([300.0, 2000.0, 0.0, 5000.0])
    pt.close()
    whole.close()


# ---- 3. run_batch: ladders beside a lone replica -------------------------------------------------------------------------------------------
def test_run_batch_ladders_leave_the_other_replicas_alone(model):
    """The issue asks for trajectories equal bit for bit between runs.  A replica that is never exchanged is replayed bit for bit, from
    its own logged energies, by the restatement of the sampler as it was before replica exchange (tests/mc_ref.py through
    test_gpu_mc._replay), and so is every replica under ``exchange_interval=0``; run against run they are compared by ``_same_chain``
    (the engine's energies are not reproducible to the last float32 bit: figures there)."""
    from chgnet_amd.montecarlo import MonteCarlo

    big, small = _structure("limno2", (2, 1, 1), rattle=0.05, seed=3), _structure("limno2", rattle=0.05, seed=4)
    structures = [big, big, big, big, small, small]
    ladders = [4, 4, 4, -1, 0, 0]                                          # three rungs of 16 atoms, a lone replica, two rungs of 8 atoms
    temps, seeds, trials = [1500.0, 2000.0, 2600.0, 2000.0, 1800.0, 2400.0], [21, 22, 23, (1 << 32) + 5, 25, 26], 12
    kw = dict(temperatures=temps, seeds=seeds, model=model, swap_species=("Li", "Mn"), swap_probability=0.5, max_displacement=0.1)
    res = MonteCarlo.run_batch(structures, trials, ladders=ladders, exchange_interval=2, **kw)
    plain = MonteCarlo.run_batch(structures, trials, **kw)
    off = MonteCarlo.run_batch(structures, trials, ladders=ladders, exchange_interval=0, **kw)
    alone = MonteCarlo.run_batch([big], trials, **{**kw, "temperatures": [temps[3]], "seeds": [seeds[3]]})
    replay_kw = dict(swap_species=(3, 25), swap_probability=0.5)

    def replayed(out, o):                                                  # the chain of the sampler without exchanges, bit for bit
        ref, _ = _replay(out["trajectory"], structures[o], seeds[o], temps[o], **replay_kw)
        assert out["energy"] == ref.e_cur and out["best"][0] == ref.e_best and np.array_equal(out["site"], ref.site)
        assert out["counts"][:5].tolist() == [*ref.counts[mc_ref.SWAP], *ref.counts[mc_ref.DISPLACE], trials]
        np.testing.assert_allclose(out["sums"], [ref.sum_e, ref.sum_e2], rtol=1e-12)

    # the lone replica: the chain it gets with no ladder in the batch, and alone
    replayed(res[3], 3)
    for other in (plain[3], alone[0]):
        frames = _same_chain([res[3]["trajectory"]], [other["trajectory"]])
        if frames == trials + 1:
            assert np.array_equal(res[3]["positions"], other["positions"]) and np.array_equal(res[3]["counts"], other["counts"])
    assert [res[3][k] for k in ("walker", "exchange_attempts", "exchange_accepts", "round_trips")] == [0, 0, 0, 0]
    # interval 0 with ladders: today's result for every replica, nothing attempted
    for o, (a, b) in enumerate(zip(off, plain)):
        replayed(a, o)
        frames = _same_chain([a["trajectory"]], [b["trajectory"]])
        if frames == trials + 1:
            for key in ("positions", "site", "counts"):
                assert np.array_equal(a[key], b[key]), key
        assert a["exchange_attempts"] == a["exchange_accepts"] == a["round_trips"] == 0
    assert [o["walker"] for o in off] == [0, 1, 2, 0, 0, 1] and [o["walker"] for o in plain] == [0] * 6
    # the ladders: six events; pairs (0,1) and (4,5) on the odd ones, (1,2) on the even ones; rungs keep their temperatures
    assert [o["exchange_attempts"] for o in res] == [3, 3, 0, 0, 3, 0]
    assert sorted(o["walker"] for o in res[:3]) == [0, 1, 2] and sorted(o["walker"] for o in res[4:]) == [0, 1]
    assert [o["temperature"] for o in res] == temps and all(o["n_trials"] == trials and o["status"] == "RUNNING" for o in res)
    assert sum(o["exchange_accepts"] for o in res) > 0
    # the rungs of every ladder are replayed by the restatement with the events between the trials
    for first, L in ((0, 3), (4, 2)):
        sl = slice(first, first + L)
        ex = _replay_ladder([o["trajectory"] for o in res[sl]], structures[first], seeds[sl], temps[sl], 2)
        for o, ref, x in zip(res[sl], ex.reps, ex.xi):
            assert o["energy"] == ref.e_cur and np.array_equal(o["positions"], ref.r) and np.array_equal(o["site"], ref.site)
            assert [o["walker"], o["exchange_attempts"], o["exchange_accepts"], o["round_trips"]] == x[[0, 1, 2, 4]].tolist()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_engine_refuses_ladders_it_cannot_exchange(model):
    from chgnet_amd import _lib
    from chgnet_amd.graph.structure import Structure
    from chgnet_amd.montecarlo import MonteCarlo

    s = _structure("limno2", (2, 1, 1), rattle=0.05, seed=3)
    z = np.asarray(s.atomic_numbers)
    perm = np.concatenate([[1, 0], np.arange(2, 16)]) if z[0] != z[1] else np.argsort(-z, kind="stable")
    assert not np.array_equal(z[perm], z)
    reordered = Structure(s.lattice, z[perm], s.frac_coords[perm])
    kw = dict(model=model, swap_species=("Li", "Mn"), swap_probability=0.5, exchange_interval=2)
    cases = [
        (dict(structures=[s, reordered], ladders=[0, 0]), r"chg_mc_set_exchange: replica 1 has species in another order than replica 0 of ladder 0"),
        (dict(structures=[s, s], ladders=[0, 0], fixed_atoms=[None, [0]]), r"chg_mc_set_exchange: replica 1 has other held atoms \(fixed\) than replica 0"),
        (dict(structures=[s, s], ladders=[0, 0], temperatures=[300.0, 0.0]), r"chg_mc_set_exchange: replica 1 of ladder 0 needs a temperature > 0"),
        (dict(structures=[s, s, s, s], ladders=[0, 0, -1, 0]), r"chg_mc_set_exchange: replica 3 takes up ladder 0 again after another id"),
        (dict(structures=[s, s, s], ladders=[0, 0, 1]), r"chg_mc_set_exchange: replica 2 is the only member of ladder 1"),
        (dict(structures=[s, _structure("limno2", rattle=0.05, seed=4)], ladders=[0, 0]), r"chg_mc_set_exchange: replica 1 has 8 atoms"),
    ]
    for case, match in cases:
        args = {"temperatures": 1000.0, **case}
        with pytest.raises(RuntimeError, match=match):
            MonteCarlo.run_batch(args.pop("structures"), 2, **args, **kw)
    # a ladder set after the first run
    mc = MonteCarlo(s, model=model, temperature=1000.0, swap_species=("Li", "Mn"), swap_probability=0.5)
    mc.run(1)
    eng, ladder = mc._run.eng, np.array([-1], np.int32)
    with pytest.raises(RuntimeError, match=r"chg_mc_set_exchange: the ladders must be set before the handle's first chg_mc_run"):
        eng._check(eng.lib.chg_mc_set_exchange(eng.handle, mc._run.handle, ladder.ctypes.data_as(_lib.c_int_p), 2))
    xi = np.zeros((1, 6), np.int32)
    with pytest.raises(RuntimeError, match=r"chg_mc_download_exchange: the handle has no ladder"):
        eng._check(eng.lib.chg_mc_download_exchange(eng.handle, mc._run.handle, xi.ctypes.data_as(_lib.c_int_p)))
    assert len(mc.run(2)) == 4                                             # the refused calls changed nothing
    mc.close()
