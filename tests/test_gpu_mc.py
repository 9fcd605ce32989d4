"""Canonical Monte Carlo on the MI355X: the step kernel against the float64 restatement (tests/mc_ref.py) on every flag set,
MonteCarlo replayed by the restatement from the logged trial energies, run_batch per replica, swap-only runs, the statistics, and the
engine's refusals."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import mc_ref
from conftest import load_case
from md_ref import KB

pytestmark = pytest.mark.gpu

ABSORB, PROPOSE = 1, 2
NONE, SWAP, DISPLACE = -1, 0, 1
E_CUR, E_BEST, SUM_E, SUM_E2, E_TRIAL, U_ACC, DELTA = 18, 19, 20, 21, 22, 23, 24    # csrc/kernels_mc.h: doubles of a replica


@pytest.fixture(scope="module")
def model(trained_like_weights):
    from chgnet_amd import CHGNet

    return CHGNet(state_dict=trained_like_weights)


def _structure(name, supercell=(1, 1, 1), rattle=0.0, seed=0):
    from chgnet_amd.graph.structure import Lattice, Structure

    _, d = load_case(name)
    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]).make_supercell(supercell)
    rng = np.random.default_rng(seed)
    cart = s.frac_coords @ s.lattice.matrix + rattle * rng.normal(size=(len(s), 3))
    return Structure(s.lattice, s.atomic_numbers, cart @ np.linalg.inv(s.lattice.matrix))


# ---- 1. the step kernel on its own ---------------------------------------------------------------------------------------------
SIZES = [2, 5, 17, 300, 40]                # 300: rows beyond one pass of the workgroup; 2: one atom per species
SEEDS = [7, (1 << 32) + 12345, 0, (1 << 64) - 1, 99]
TRIALS0 = [0, 70000, 3, 49, 11]            # trials proposed on entry (one above 2^16); 0 with ABSORB: the first evaluation
TEMPS = [700.0, 0.0, 300.0, 2000.0, 300.0]                       # replica 1 is greedy
D_E = [None, 0.03, -0.02, 0.01, 0.0]                             # E_trial - E_cur: 0 K rejects, a new best, a coin toss, exactly 0
HELD = {2: [0, 5, 16]}                                           # replica 2 holds three atoms
SWAP_SET = {3: (3, 25)}                                          # replica 3 swaps Li and Mn only
FLAGSETS = {"absorb_only": ABSORB, "propose_only": PROPOSE, "absorb_propose": ABSORB | PROPOSE}


def _make_replicas(flags, swap_probability, intensive, max_displacement=0.1):
    """Five replicas as dicts: the state arrays on entry, the engine's energy, and the restatement in the same state."""
    rng = np.random.default_rng(100 * flags + int(10 * swap_probability) + intensive)
    reps = []
    for o, (n, seed, k0) in enumerate(zip(SIZES, SEEDS, TRIALS0)):
        cell = np.diag(rng.uniform(5, 9, 3)) + rng.normal(0, 0.5, (3, 3))
        z = np.array([3, 25], np.int32) if n == 2 else np.concatenate([[3, 25, 8], rng.choice([3, 25, 8], n - 3)]).astype(np.int32)
        fixed = np.zeros(n, np.uint8)
        fixed[HELD.get(o, [])] = 1
        swap_set = SWAP_SET.get(o)
        swap_mask = np.ones(n, np.uint8) if swap_set is None else np.isin(z, swap_set).astype(np.uint8)
        first = bool(flags & ABSORB) and k0 == 0
        ref = mc_ref.McRef(rng.random((n, 3)) @ cell, cell, z, temperature_k=TEMPS[o], seed=seed, swap_probability=swap_probability,
                           max_displacement=max_displacement, swap_species=swap_set, fixed=fixed.astype(bool), k=max(k0 - 1, 0))
        ref.site = rng.permutation(n)
        scale = float(n) if intensive else 1.0
        e32 = np.float32((-40.0 - o + (D_E[o] or 0.0)) / scale)
        e_trial = float(e32) * scale                                     # what the kernel forms from the engine's float32
        if not first:
            ref.started = True
            ref.e_cur = e_trial if D_E[o] == 0.0 else -40.0 - o
            ref.e_best = ref.e_cur - (0.02 if o % 2 else 0.0)
            ref.best_r, ref.best_site = rng.random((n, 3)), rng.permutation(n)
            ref.counts = {mc_ref.SWAP: [int(rng.integers(5, 90)), 3], mc_ref.DISPLACE: [int(rng.integers(5, 90)), 4]}
            ref.n_samples = int(rng.integers(100, 200))
            ref.sum_e, ref.sum_e2 = ref.n_samples * -40.3, ref.n_samples * 1625.7
            if flags & ABSORB:
                ref.propose()                                            # the pending trial: k0 - 1, so k0 trials have been proposed
            else:
                ref.k = k0
        sd = np.zeros(32)
        sd[:9], sd[9:18] = cell.ravel(), np.linalg.inv(cell).ravel()
        si = np.array([k0, 0, 0 if first else 1, NONE, 0, 0, 0, 0], np.int32)
        counts = np.zeros(8, np.int64)
        if not first:
            sd[[E_CUR, E_BEST, SUM_E, SUM_E2]] = ref.e_cur, ref.e_best, ref.sum_e, ref.sum_e2
            counts[:5] = [*ref.counts[mc_ref.SWAP], *ref.counts[mc_ref.DISPLACE], ref.n_samples]
            if ref.pending is not None:
                p = ref.pending
                si[3:6] = p["kind"], p["i"], max(p["j"], 0) if p["kind"] == SWAP else -1
                sd[U_ACC], sd[DELTA:DELTA + 3] = p["u_acc"], p["delta"]
        reps.append({"n": n, "z": z, "fixed": fixed, "swap_mask": swap_mask, "seed": seed, "temp": TEMPS[o], "ref": ref, "first": first,
                     "r": ref.r.copy(), "site": ref.site.astype(np.int32), "sd": sd, "si": si, "counts": counts,
                     "best_pos": ref.best_r.copy(), "best_site": ref.best_site.astype(np.int32), "energy": e32, "e_trial": e_trial})
    return reps


def _launch(hip_engine, reps, flags, swap_probability, intensive, final_try=1, max_displacement=0.1):
    """One launch on the replicas in the given order; returns one dict of outputs per replica."""
    from chgnet_amd import _lib

    cat = lambda key, dtype: np.ascontiguousarray(np.concatenate([np.atleast_1d(x[key]) for x in reps]), dtype)  # noqa: E731
    B = len(reps)
    aoff = np.concatenate([[0], np.cumsum([x["n"] for x in reps])]).astype(np.int32)
    N = int(aoff[-1])
    r, site, best_pos, best_site = cat("r", np.float64), cat("site", np.int32), cat("best_pos", np.float64), cat("best_site", np.int32)
    sd, si, counts = cat("sd", np.float64), cat("si", np.int32), cat("counts", np.int64)
    z, fixed, swap_mask = cat("z", np.int32), cat("fixed", np.uint8), cat("swap_mask", np.uint8)
    temps, seeds, energy = cat("temp", np.float64), np.array([x["seed"] for x in reps], np.uint64), cat("energy", np.float32)
    frac_next, retry = np.full((N, 3), -7.0), np.full(B, -1, np.int32)
    f_scal, f_moves, f_pos, f_site = np.full((B, 6), -7.0), np.full((B, 6), -7, np.int32), np.full((N, 3), -7.0), np.full(N, -7, np.int32)
    prm = _lib.McParams(swap_probability=swap_probability, max_displacement=max_displacement, kB=KB, loginterval=1, ring_frames=1, r_atom=6.0,
                        r_bond=3.0, numerical_tol=1e-8)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(_lib.c_int_p)  # noqa: E731
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    hip_engine._check(hip_engine.lib.chg_test_mc_step(
        hip_engine.handle, ctypes.byref(prm), B, ip(aoff), ip(z), u8(swap_mask), u8(fixed), dp(temps),
        seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), flags, final_try, intensive, dp(r), ip(site), dp(sd), ip(si),
        counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), dp(best_pos), ip(best_site), energy.ctypes.data_as(_lib.c_float_p),
        dp(frac_next), ip(retry), dp(f_scal), ip(f_moves), dp(f_pos), ip(f_site)))
    out = []
    for o in range(B):
        sl = slice(aoff[o], aoff[o + 1])
        out.append({"r": r[sl], "site": site[sl], "sd": sd[32 * o:32 * o + 32], "si": si[8 * o:8 * o + 8], "counts": counts[8 * o:8 * o + 8],
                    "best_pos": best_pos[sl], "best_site": best_site[sl], "frac_next": frac_next[sl], "retry": int(retry[o]),
                    "f_scal": f_scal[o], "f_moves": f_moves[o], "f_pos": f_pos[sl], "f_site": f_site[sl]})
    return out


def _close(got, want, what, worst):
    scale = np.abs(want).max() + 1e-300
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max() / scale)
    worst[what] = max(worst.get(what, 0.0), err)
    assert err <= 1e-12, (what, err)


def _check_replica(flags, rep, got, worst):
    """Advance the restatement through what the launch did and compare."""
    ref, k0 = rep["ref"], int(rep["si"][0])
    decided = None
    if flags & ABSORB:
        if rep["first"]:
            ref.start(rep["e_trial"])
        else:
            decided = dict(ref.pending)
            decided["accepted"] = ref.decide(rep["e_trial"])
        assert got["retry"] == 0
        assert got["sd"][E_CUR] == ref.e_cur and got["sd"][E_BEST] == ref.e_best and got["sd"][E_TRIAL] == rep["e_trial"]
        _close(got["sd"][[SUM_E, SUM_E2]], np.array([ref.sum_e, ref.sum_e2]), "sums", worst)
        assert got["counts"][:5].tolist() == [*ref.counts[mc_ref.SWAP], *ref.counts[mc_ref.DISPLACE], ref.n_samples]
        assert np.array_equal(got["site"], ref.site)
        if decided is not None and decided["kind"] == SWAP:
            assert np.array_equal(got["r"], ref.r)                      # swapped rows are copies: bit for bit
        else:
            _close(got["r"], ref.r, "r", worst)
        assert np.array_equal(got["best_site"], ref.best_site)
        _close(got["best_pos"], ref.best_r, "best_pos", worst)
        # the frame: the decision just taken
        assert got["f_scal"][0] == ref.e_cur and got["f_scal"][1] == rep["e_trial"]
        if decided is None:
            assert got["f_moves"][:5].tolist() == [0, NONE, -1, -1, 0] and not got["f_scal"][2:].any()
            assert got["si"][2] == 1
        else:
            assert got["f_moves"][:5].tolist() == [k0, decided["kind"], decided["i"], decided["j"], int(decided["accepted"])]
            assert got["f_scal"][2] == decided["u_acc"] and np.array_equal(got["f_scal"][3:6], decided["delta"])
            assert got["si"][6] == int(decided["accepted"])
        assert np.array_equal(got["f_pos"], got["r"]) and np.array_equal(got["f_site"], got["site"])
    else:
        for key in ("r", "site", "counts", "best_pos", "best_site"):
            assert np.array_equal(got[key], rep[key]), key
        assert np.array_equal(got["sd"][:U_ACC], rep["sd"][:U_ACC])
        assert (got["f_scal"] == -7.0).all() and (got["f_moves"] == -7).all() and (got["f_pos"] == -7.0).all()
    assert got["si"][1] == 0
    if flags & PROPOSE:
        m = ref.propose()
        assert got["si"][[0, 3, 4, 5]].tolist() == [k0 + 1, m["kind"], m["i"], m["j"]], (got["si"], m)
        assert got["sd"][U_ACC] == m["u_acc"] and np.array_equal(got["sd"][DELTA:DELTA + 3], m["delta"])
        _close(got["frac_next"], ref.trial_positions() @ np.linalg.inv(ref.cell), "frac_next", worst)
        if m["kind"] == SWAP:
            assert ref.species[m["i"]] != ref.species[m["j"]]
        held = np.flatnonzero(rep["fixed"])
        assert m["i"] not in held and m["j"] not in held
    else:
        assert got["si"][0] == k0 and got["si"][3] == NONE and (got["frac_next"] == -7.0).all()
    return decided


@pytest.mark.parametrize("intensive", [0, 1])
@pytest.mark.parametrize("swap_probability", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("mode", list(FLAGSETS))
def test_step_kernel_matches_restatement(hip_engine, mode, swap_probability, intensive):
    flags = FLAGSETS[mode]
    reps = _make_replicas(flags, swap_probability, intensive)
    out = _launch(hip_engine, reps, flags, swap_probability, intensive)
    back = _launch(hip_engine, reps[::-1], flags, swap_probability, intensive)[::-1]        # the same replicas in reversed slot order
    worst, seen = {}, []
    for rep, got, rev in zip(reps, out, back):
        for key in got:
            assert np.array_equal(got[key], rev[key]), ("slot order", key)
        seen.append(_check_replica(flags, rep, got, worst))
    print(mode, "swap_probability", swap_probability, "intensive", intensive, "worst relative errors", worst)
    if flags & ABSORB:
        assert seen[0] is None                                             # the first evaluation
        assert not seen[1]["accepted"] and seen[2]["accepted"] and seen[4]["accepted"]   # 0 K rejects dE > 0; dE < 0; dE == 0
        assert out[2]["sd"][E_BEST] == out[2]["sd"][E_CUR]                   # replica 2 found a new best
        kinds = {d["kind"] for d in seen[1:]}
        assert kinds == ({SWAP} if swap_probability == 1.0 else {DISPLACE} if swap_probability == 0.0 else kinds)
    if flags & PROPOSE:
        kinds = {int(o["si"][3]) for o in out}
        assert kinds <= {SWAP, DISPLACE} and (swap_probability != 1.0 or kinds == {SWAP}) and (swap_probability != 0.0 or kinds == {DISPLACE})


@pytest.mark.parametrize("final_try", [0, 1])
def test_step_kernel_nonfinite_replica_is_left_untouched(hip_engine, final_try):
    flags, bad = ABSORB | PROPOSE, 3
    reps = _make_replicas(flags, 0.5, 1)
    reps[bad]["energy"] = np.float32(np.nan)
    out = _launch(hip_engine, reps, flags, 0.5, 1, final_try=final_try)
    got, rep = out[bad], reps[bad]
    assert got["retry"] == (0 if final_try else 1)
    want_si = rep["si"].copy()
    want_si[1] = 1 if final_try else 0                                     # CHG_MC_NONFINITE only on the final try
    assert np.array_equal(got["si"], want_si)
    for key in ("r", "site", "sd", "counts", "best_pos", "best_site"):
        assert np.array_equal(got[key], rep[key]), key
    assert (got["frac_next"] == -7.0).all() and (got["f_scal"] == -7.0).all() and (got["f_pos"] == -7.0).all()
    worst = {}
    for o, (rep, got) in enumerate(zip(reps, out)):                        # its neighbours step as usual
        if o != bad:
            _check_replica(flags, rep, got, worst)


# ---- 2. end to end, replayed from the logged trial energies -------------------------------------------------------------------------
def _replay(traj, structure, seed, temperature, *, swap_species, swap_probability, max_displacement=0.1, fixed=None, model=None,
            ref=None, first_frame=0):
    """The restatement as one stream over the logged frames (loginterval 1), deciding on the logged E_trial.  ``temperature``: K, or a
    function of the trial number.  Returns the restatement and the largest |predict_structure - E_trial| (eV) when ``model`` is given."""
    from chgnet_amd.graph.structure import Lattice, Structure

    z = np.asarray(structure.atomic_numbers)
    cell = structure.lattice.matrix
    t_of = temperature if callable(temperature) else (lambda k: temperature)
    worst_e = 0.0

    def predicted(r):
        pred = model.predict_structure(Structure(Lattice(cell), z, r @ np.linalg.inv(cell)), task="e")
        return float(pred["e"]) * (len(z) if model.is_intensive else 1)

    if ref is None:
        ref = mc_ref.McRef(structure.frac_coords @ cell, cell, z, temperature_k=t_of(0), seed=seed, swap_probability=swap_probability,
                           max_displacement=max_displacement, swap_species=swap_species, fixed=fixed)
        assert traj.trials[0] == 0 and traj.kinds[0] is None and traj.energies[0] == traj.trial_energies[0]
        np.testing.assert_allclose(traj.atom_positions[0], ref.r, rtol=0, atol=1e-12 * np.abs(ref.r).max())
        assert np.array_equal(traj.sites[0], np.arange(len(z)))
        ref.start(traj.energies[0])
        if model is not None:
            worst_e = abs(predicted(ref.r) - traj.trial_energies[0])
        first_frame = 1
    for f in range(first_frame, len(traj)):
        assert traj.trials[f] == ref.k + 1
        ref.t = float(t_of(traj.trials[f]))
        m = ref.propose()
        assert (traj.kinds[f], traj.moves[f]) == (("swap", "displacement")[m["kind"]], (m["i"], m["j"])), (f, m)
        assert traj.u_acc[f] == m["u_acc"] and np.array_equal(traj.displacements[f], m["delta"]), (f, m)
        if model is not None:
            worst_e = max(worst_e, abs(predicted(ref.trial_positions()) - traj.trial_energies[f]))
        e_before = ref.e_cur
        acc = ref.decide(traj.trial_energies[f])
        d_e = traj.trial_energies[f] - e_before
        assert acc == (d_e <= 0 or (ref.t > 0 and traj.u_acc[f] < np.exp(-d_e / (KB * ref.t))))
        assert traj.accepted[f] == acc and traj.energies[f] == ref.e_cur, (f, d_e)
        np.testing.assert_allclose(traj.atom_positions[f], ref.r, rtol=0, atol=1e-12 * np.abs(ref.r).max())
        assert np.array_equal(traj.sites[f], ref.site)
    return ref, worst_e


def _outcomes(traj):
    return {(k, a) for k, a in zip(traj.kinds[1:], traj.accepted[1:])}


REPLAY_SEED = 0    # gives accepted and rejected trials of both kinds in 40 trials (asserted below)


def test_run_is_replayed_by_the_restatement(model):
    from chgnet_amd.montecarlo import MonteCarlo

    s = _structure("limno2", (2, 1, 1), rattle=0.05, seed=3)
    assert len(s) == 16 and sorted(np.unique(s.atomic_numbers, return_counts=True)[1]) == [4, 4, 8]
    mc = MonteCarlo(s, model=model, temperature=2000.0, swap_species=("Li", "Mn"), swap_probability=0.5, max_displacement=0.1,
                    seed=REPLAY_SEED, loginterval=1)
    mc.run(17)
    traj = mc.run(23)
    assert len(traj) == 41 and traj.trials == list(range(41))
    ref, worst_e = _replay(traj, s, REPLAY_SEED, 2000.0, swap_species=(3, 25), swap_probability=0.5, model=model)
    print("outcomes", sorted(_outcomes(traj)), "acceptance", mc.acceptance, "max |predict_structure - E_trial|", worst_e, "eV")
    assert worst_e < 1e-4
    assert _outcomes(traj) == {("swap", True), ("swap", False), ("displacement", True), ("displacement", False)}
    c = mc.counts
    assert c[0] + c[2] == 40 == c[4] and c[1] == ref.counts[mc_ref.SWAP][1] and c[3] == ref.counts[mc_ref.DISPLACE][1]
    np.testing.assert_allclose(mc.atoms.frac_coords @ s.lattice.matrix, ref.r, rtol=0, atol=1e-12 * np.abs(ref.r).max())
    assert np.array_equal(mc.species_on_sites(), ref.species_on_sites()) and mc.energy == ref.e_cur
    mc.close()


# ---- 3. a batch of replicas at their own temperatures ---------------------------------------------------------------------------------
def test_run_batch_replicas_follow_their_own_streams(model):
    from chgnet_amd.montecarlo import MonteCarlo

    big, small = _structure("limno2", (2, 1, 1), rattle=0.05, seed=3), _structure("limno2", rattle=0.05, seed=4)
    structures = [big, big, big, big, small]
    temps, seeds, trials = [0.0, 300.0, 2000.0, 1e7, 2000.0], [11, (1 << 32) + 5, 13, 14, 15], 36     # 37 frames: two drains of the ring
    res = MonteCarlo.run_batch(structures, trials, temperatures=temps, seeds=seeds, model=model, swap_species=("Li", "Mn"),
                               swap_probability=0.5, max_displacement=0.1)
    for s, t, seed, out in zip(structures, temps, seeds, res):
        traj = out["trajectory"]
        assert len(traj) == trials + 1 and out["status"] == "RUNNING" and out["n_trials"] == trials and out["temperature"] == t
        ref, _ = _replay(traj, s, seed, t, swap_species=(3, 25), swap_probability=0.5)
        c = out["counts"]
        assert c[:5].tolist() == [*ref.counts[mc_ref.SWAP], *ref.counts[mc_ref.DISPLACE], trials]
        assert c[0] + c[2] == trials and 0 <= c[1] <= c[0] and 0 <= c[3] <= c[2]
        for kind, k in (("swap", 0), ("displacement", 2)):
            n_acc = sum(1 for x, a in zip(traj.kinds[1:], traj.accepted[1:]) if x == kind and a)
            n_rej = sum(1 for x, a in zip(traj.kinds[1:], traj.accepted[1:]) if x == kind and not a)
            assert (n_acc, n_acc + n_rej) == (c[k + 1], c[k])
        assert out["energy"] == ref.e_cur and out["best"][0] == ref.e_best
        assert np.array_equal(out["species_on_sites"], ref.species_on_sites())
    e0 = res[0]["trajectory"].energies
    assert all(b <= a for a, b in zip(e0, e0[1:]))                         # 0 K: E_cur never rises
    assert all(res[3]["trajectory"].accepted[1:])                          # 1e7 K: every trial is accepted
    assert res[0]["trajectory"].u_acc != res[1]["trajectory"].u_acc


# ---- 4. swaps only --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", [False, True])
def test_swap_only_run_permutes_the_input_rows(model, hold):
    from chgnet_amd.montecarlo import MonteCarlo

    s = _structure("limno2", (2, 1, 1), rattle=0.05, seed=3)
    z = np.asarray(s.atomic_numbers)
    held = np.flatnonzero(z == 3)[:2] if hold else np.array([], int)
    mc = MonteCarlo(s, model=model, temperature=5000.0, swap_species=("Li", "Mn"), swap_probability=1.0, seed=21,
                    fixed_atoms=held.tolist() if hold else None)
    traj = mc.run(30)
    rows, final = traj.atom_positions[0], traj.atom_positions[-1]
    site = mc.site
    assert sorted(site.tolist()) == list(range(16)) and any(traj.accepted) and (site != np.arange(16)).any()
    assert np.array_equal(final, rows[site])                               # a permutation of the input rows, bit for bit
    np.testing.assert_allclose(mc.atoms.frac_coords @ s.lattice.matrix, final, rtol=0, atol=1e-12 * np.abs(final).max())
    on_sites = mc.species_on_sites()
    assert np.array_equal(on_sites[site], z) and sorted(on_sites.tolist()) == sorted(z.tolist())
    assert np.array_equal(on_sites, traj.species_on_sites[-1])
    assert set(traj.kinds[1:]) == {"swap"} and mc.counts[2] == 0 and mc.counts[0] == 30
    for i, j in traj.moves[1:]:
        assert {z[i], z[j]} == {3, 25}                                     # O is outside the swap set
        assert i not in held and j not in held
    for f in range(len(traj)):
        assert np.array_equal(traj.atom_positions[f][held], rows[held]) and np.array_equal(traj.sites[f][held], held)
    _replay(traj, s, 21, 5000.0, swap_species=(3, 25), swap_probability=1.0, fixed=np.isin(np.arange(16), held))
    mc.close()


# ---- 5. statistics ----------------------------------------------------------------------------------------------------------------------
def test_statistics_follow_the_frames(model):
    from chgnet_amd.montecarlo import MonteCarlo

    s = _structure("limno2", (2, 1, 1), rattle=0.05, seed=3)
    mc = MonteCarlo(s, model=model, temperature=2000.0, swap_species=("Li", "Mn"), swap_probability=0.5, seed=5)
    traj = mc.run(20)
    e = np.array(traj.energies)
    assert mc.counts[4] == 20
    np.testing.assert_allclose(mc.sums, [e[1:].sum(), (e[1:] ** 2).sum()], rtol=1e-12)
    np.testing.assert_allclose(mc.mean_energy, e[1:].mean(), rtol=1e-12)
    np.testing.assert_allclose(mc.heat_capacity(), (mc.sums[1] / 20 - (mc.sums[0] / 20) ** 2) / (KB * 2000.0 ** 2), rtol=1e-9)
    best_e, best_s = mc.best
    f = int(np.argmin(e))                                                  # the first frame at the minimum: later ties do not replace it
    assert best_e == e[f] == e.min()
    np.testing.assert_allclose(best_s.frac_coords @ s.lattice.matrix, traj.atom_positions[f], rtol=0, atol=1e-12 * np.abs(traj.atom_positions[f]).max())
    acc = mc.acceptance
    assert acc["swap"] == mc.counts[1] / mc.counts[0] and acc["displacement"] == mc.counts[3] / mc.counts[2]
    # after reset_statistics the means cover the last 10 trials only
    mc.reset_statistics()
    assert mc.counts.tolist() == [0] * 8
    traj = mc.run(10)
    e = np.array(traj.energies)
    assert len(e) == 31 and mc.counts[4] == 10 and mc.counts[0] + mc.counts[2] == 10
    np.testing.assert_allclose(mc.mean_energy, e[21:].mean(), rtol=1e-12)   # a difference of two sums 30 samples long
    np.testing.assert_allclose(mc.sums[1], (e[21:] ** 2).sum(), rtol=1e-12)
    # 0 K between two runs: the second run is greedy
    mc.set_temperature(0)
    traj = mc.run(15)
    e = np.array(traj.energies)
    assert len(e) == 46 and all(b <= a for a, b in zip(e[30:], e[31:]))
    for f in range(31, 46):
        assert traj.accepted[f] == (traj.trial_energies[f] <= e[f - 1])
    _replay(traj, s, 5, lambda k: 2000.0 if k <= 30 else 0.0, swap_species=(3, 25), swap_probability=0.5)
    assert mc.best[0] == e.min()
    with pytest.raises(ValueError, match="temperature > 0"):
        mc.heat_capacity()
    mc.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_engine_refuses_a_replica_that_cannot_swap(model):
    from chgnet_amd.montecarlo import MonteCarlo

    s = _structure("limno2", (2, 1, 1))
    z = np.asarray(s.atomic_numbers)
    ok = MonteCarlo(s, model=model, swap_species=("Li", "Mn"), swap_probability=0.5)
    bad = MonteCarlo(s, model=model, swap_species=("Li", "Mn"), swap_probability=0.5, fixed_atoms=np.flatnonzero(z == 25).tolist())
    with pytest.raises(RuntimeError, match=r"chg_mc_create: structure 0 has 1 swappable species"):
        bad.run(1)                                                         # every Mn is held: Li alone cannot swap
    with pytest.raises(RuntimeError, match=r"chg_mc_create: structure 1 has 1 swappable species"):
        MonteCarlo.run_batch([s, s], 1, fixed_atoms=[None, z == 25], model=model, swap_species=("Li", "Mn"), swap_probability=0.5)
    with pytest.raises(RuntimeError, match=r"frames do not fit the ring"):
        ok.run(0)
        ok._run.eng._check(ok._run.eng.lib.chg_mc_run(ok._run.eng.handle, ok._run.handle, 40))
    assert len(ok.run(3)) == 4                                             # the refused call ran nothing
    ok.close()
