"""L-BFGS relaxation on the MI355X: the step kernel against the float64 restatement (tests/lbfgs_ref.py), the driver replayed
teacher-forced through the restatement (with and without compaction), StructOptimizer(optimizer_class="LBFGS") end to end and a
1024-structure batch."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
from scipy.linalg import logm

from conftest import load_case
from lbfgs_ref import LBFGS, LbfgsRelaxation, pack_state, ring_slots, unpack_state
from relax_ref import FIRE, GPA, Relaxation

pytestmark = pytest.mark.gpu


def _params(relax_cell=1, fmax=0.1, max_steps=500):
    """chg_relax_params: the FIRE numbers are ignored by chg_relax_create_lbfgs; the binding passes the defaults."""
    from chgnet_amd import _lib

    return _lib.RelaxParams(fmax=fmax, max_steps=max_steps, relax_cell=relax_cell, dt=FIRE["dt"], maxstep=FIRE["maxstep"], dtmax=FIRE["dtmax"],
                            finc=FIRE["finc"], fdec=FIRE["fdec"], astart=FIRE["astart"], fa=FIRE["fa"], nmin=FIRE["nmin"], exp_cell_factor=0.0,
                            r_atom=6.0, r_bond=3.0, numerical_tol=1e-8, stress_weight=GPA)


def _lbfgs(memory=LBFGS["memory"]):
    from chgnet_amd import _lib

    return _lib.LbfgsParams(maxstep=LBFGS["maxstep"], damping=LBFGS["damping"], alpha=LBFGS["alpha"], memory=memory)


@pytest.fixture(scope="module")
def model(trained_like_weights):
    from chgnet_amd import CHGNet

    return CHGNet(state_dict=trained_like_weights)


def _structure(name, supercell=(1, 1, 1), rattle=0.0, strain=0.0, seed=0):
    from chgnet_amd.graph.structure import Lattice, Structure

    _, d = load_case(name)
    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]).make_supercell(supercell)
    rng = np.random.default_rng(seed)
    lat = s.lattice.matrix @ (np.eye(3) + strain * rng.normal(size=(3, 3)))
    cart = s.frac_coords @ s.lattice.matrix + rattle * rng.normal(size=(len(s), 3))
    return Structure(Lattice(lat), s.atomic_numbers, cart @ np.linalg.inv(lat))


# ---- 1. the step kernel on its own ---------------------------------------------------------------------------------------------
# One workgroup of 256 threads per structure, thread t owning rows t, t + 256, ...: no size switch, but the row loop takes a second
# trip beyond 256 rows and the reductions change shape at the wave (64 rows).  With the cell a structure has n + 3 rows.
SIZES = [1, 2, 5, 40, 300, 17, 11, 8, 61, 62, 64, 65, 253, 254, 256, 257]
STEP_FMAX, STEP_MAX_STEPS = 1e-3, 50
# kind -> steps of history built before the launch.  "clamp": forces x 40 on the first step (g / alpha); forces x 40 on top of a
# history do not clamp (the triple they append makes the model stiff), so "clamp_history" moves the well 1 A away instead, which
# keeps the curvature and asks for a step of about that length
GROUPS = {4: {"first": 0, "partial": 3, "wrapped": 9, "clamp": 0, "clamp_history": 3, "converged": 3, "max_steps": 3, "nonfinite": 3, "skipped": 3},
          100: {"first": 0, "partial": 3, "memory100": 12}}
WANT_STATUS = {"converged": 1, "max_steps": 2, "nonfinite": 3}


def _build_case(rng, n, kind, k, relax_cell, memory):
    """A state after k restatement steps on synthetic smooth forces f = -K (q - q*) (q* drifting a little every step, so that small
    structures do not converge while the history is built) with a random f32 stress, and the results of the evaluation to step on."""
    L0 = np.diag(rng.uniform(4, 9, 3)) + rng.normal(0, 0.6, (3, 3))
    r = LbfgsRelaxation(rng.random((n, 3)), L0, relax_cell=bool(relax_cell), fmax=STEP_FMAX, steps=STEP_MAX_STEPS, p={**LBFGS, "memory": memory})
    flat = kind == "skipped"          # no stress and X = 0: F = I exactly on both sides, so g == g0 can hold to the bit
    if relax_cell and not flat:
        r.q[n:] = r.c * rng.normal(0, 0.1, (3, 3))
    K = rng.uniform(2.0, 30.0, (n, 3))
    target = r.q[:n] + rng.normal(0, 0.15, (n, 3))
    s0 = rng.normal(0, 2.0, (3, 3))
    s0 = (s0 + s0.T) / 2

    def results():
        f = (-K * (r.q[:n] - target)).astype(np.float32)
        A = r.q[n:] / r.c
        s = np.zeros((3, 3), np.float32) if flat else (s0 - 40.0 * (A + A.T)).astype(np.float32)
        return f, s

    f, s = results()
    for i in range(k):
        assert r.advance(f.astype(np.float64), s.astype(np.float64) * GPA) == 0
        target = target + rng.normal(0, 1.0 if kind == "clamp_history" and i == k - 1 else 0.04, (n, 3))
        f_prev, (f, s) = f, results()
    assert r.steps == k and r.status == 0
    if kind == "clamp":
        f = f * np.float32(40)
    if kind == "converged":
        f, s = f * np.float32(1e-5), s * np.float32(1e-6)
    if kind == "max_steps":
        r.steps = STEP_MAX_STEPS
    if kind == "nonfinite":
        f[n // 2, 1] = np.nan
    if kind == "skipped":
        f = f_prev                    # the forces of the previous evaluation once more
    return r, f, s


def _launch(eng, relax_cell, memory, state, atom_off, energy, force, stress, magmom, final_try=1):
    from chgnet_amd import _lib

    q, r0, g0, S, Y, rho, sd, si = (a.copy() for a in state)
    B, N = len(atom_off) - 1, int(atom_off[-1])
    frac_next, lat_next, retry = np.zeros((N, 3)), np.zeros((B, 3, 3)), np.zeros(B, np.int32)
    p, lp = _params(relax_cell, STEP_FMAX, STEP_MAX_STEPS), _lbfgs(memory)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(_lib.c_int_p)  # noqa: E731
    eng._check(eng.lib.chg_test_lbfgs_step(eng.handle, ctypes.byref(p), ctypes.byref(lp), B, ip(atom_off), dp(q), dp(r0), dp(g0), dp(S), dp(Y),
                                           dp(rho), dp(sd), ip(si), fp(energy), fp(force), fp(stress), fp(magmom), final_try, dp(frac_next),
                                           dp(lat_next), ip(retry)))
    return (q, r0, g0, S, Y, rho, sd, si), frac_next, lat_next, retry


def _segment(state, atom_off, o):
    """Everything the state holds of structure o (status apart), for bitwise comparison."""
    q, r0, g0, S, Y, rho, sd, si = state
    a, b = atom_off[o] + 3 * o, atom_off[o + 1] + 3 * (o + 1)
    return [q[a:b], r0[a:b], g0[a:b], S[:, a:b], Y[:, a:b], rho[o], sd[o], si[o, :2]]


@pytest.mark.parametrize("memory", [4, 100])
@pytest.mark.parametrize("relax_cell", [1, 0])
def test_step_kernel_matches_restatement(hip_engine, relax_cell, memory):
    rng = np.random.default_rng(100 * memory + relax_cell)
    slots = ring_slots(memory, STEP_MAX_STEPS)
    cases = [(n, kind, k) for kind, k in GROUPS[memory].items() for n in SIZES]
    rel, forces, stresses = [], [], []
    for n, kind, k in cases:
        r, f, s = _build_case(rng, n, kind, k, relax_cell, memory)
        rel.append(r)
        forces.append(f)
        stresses.append(s)
    atom_off = np.concatenate([[0], np.cumsum([n for n, _, _ in cases])]).astype(np.int32)
    state = pack_state(rel, atom_off, slots)
    energy = rng.normal(-5, 1, len(cases)).astype(np.float32)
    force = np.ascontiguousarray(np.concatenate(forces), np.float32)
    stress = np.ascontiguousarray(np.stack(stresses), np.float32)
    magmom = rng.random(atom_off[-1]).astype(np.float32)
    out, frac_next, lat_next, retry = _launch(hip_engine, relax_cell, memory, state, atom_off, energy, force, stress, magmom)
    assert not retry.any()

    got = [LbfgsRelaxation.__new__(LbfgsRelaxation) for _ in rel]
    for gr, r in zip(got, rel):
        gr.n, gr.relax_cell = r.n, r.relax_cell
    unpack_state(got, atom_off, slots, *out)
    tol = lambda ref: 2e-12 * (np.abs(ref).max() + 1.0)  # noqa: E731
    for o, (r, (n, kind, k)) in enumerate(zip(rel, cases)):
        tag = (kind, n)
        q0, appended0 = r.q.copy(), r.appended
        r.advance(forces[o].astype(np.float64), stresses[o].astype(np.float64) * GPA, True)
        gr = got[o]
        assert r.status == WANT_STATUS.get(kind, 0) == gr.status, (tag, r.status, gr.status)
        assert (r.steps, r.appended) == (gr.steps, gr.appended), tag
        if r.status != 0:                       # stopped: bit-identical to the input, history included
            assert all(np.array_equal(a, b) for a, b in zip(_segment(out, atom_off, o), _segment(state, atom_off, o))), tag
            continue
        assert r.appended == (appended0 if k == 0 or kind == "skipped" else appended0 + 1), tag      # no triple on a first step
        assert len(gr.rho) == len(r.rho) == min(r.appended, slots), tag
        if kind == "wrapped":
            assert r.appended == 9 and len(r.rho) == 4
        if kind == "memory100":
            assert len(r.rho) == 12
        for name in ("q", "r0", "g0"):
            ref = getattr(r, name)
            assert np.abs(getattr(gr, name) - ref).max() <= tol(ref), (tag, name)
        for i in range(len(r.rho)):
            assert np.abs(gr.s[i] - r.s[i]).max() <= tol(r.s[i]) and np.abs(gr.y[i] - r.y[i]).max() <= tol(r.y[i]), (tag, i)
            assert abs(gr.rho[i] - r.rho[i]) <= 1e-10 * abs(r.rho[i]), (tag, i, gr.rho[i], r.rho[i])
        rows = r.rows
        if kind in ("clamp", "clamp_history"):
            for moved in (r.q[:rows] - q0[:rows], gr.q[:rows] - q0[:rows]):
                assert np.sqrt((moved ** 2).sum(1).max()) == pytest.approx(LBFGS["maxstep"], rel=1e-12), tag
        sl = slice(atom_off[o], atom_off[o + 1])
        assert np.abs(frac_next[sl] - r.frac()).max() <= tol(r.frac()), tag
        lat = r.lattice()
        assert np.abs(lat_next[o] - lat).max() <= tol(lat), tag
        if not relax_cell:
            assert np.array_equal(lat_next[o], r.L0), tag

    # the same input once more: the same bits
    again, frac2, lat2, _ = _launch(hip_engine, relax_cell, memory, state, atom_off, energy, force, stress, magmom)
    assert all(np.array_equal(a, b) for a, b in zip(again, out))
    assert np.array_equal(frac2, frac_next) and np.array_equal(lat2, lat_next)

    # not the final try: a structure with non-finite results is held back untouched (still running, flag set); the others step as before
    if memory == 4:
        held, frac3, _, retry = _launch(hip_engine, relax_cell, memory, state, atom_off, energy, force, stress, magmom, final_try=0)
        for o, (n, kind, k) in enumerate(cases):
            assert retry[o] == (kind == "nonfinite"), (kind, n)
            want = state if kind == "nonfinite" else out
            assert all(np.array_equal(a, b) for a, b in zip(_segment(held, atom_off, o), _segment(want, atom_off, o))), (kind, n)
            assert held[7][o, 2] == (0 if kind == "nonfinite" else out[7][o, 2])


# ---- 2. / 3. the driver, teacher-forced -----------------------------------------------------------------------------------------
# The engine's fp32 forces are not bit-reproducible run to run and L-BFGS amplifies the difference through y, so the restatement is
# fed the forces and stress the device downloaded for every evaluation; its next configuration must then be the device's.
def _download(eng, handle, B, N):
    from chgnet_amd import _lib

    out = {"frac": np.empty((N, 3)), "lattice": np.empty((B, 3, 3)), "energy": np.empty(B, np.float32), "force": np.empty((N, 3), np.float32),
           "stress": np.empty((B, 3, 3), np.float32), "magmom": np.empty(N, np.float32), "n_steps": np.empty(B, np.int32),
           "status": np.empty(B, np.int32)}
    eng._check(eng.lib.chg_relax_download(eng.handle, handle, ctypes.byref(_lib.fill_out(_lib.RelaxOutHost(), out))))
    return out


def _replay(model, structs, relax_cell, fmax, max_steps, memory, evaluations):
    """Run the handle one evaluation at a time; returns the restatements and the active counts.  Every structure that was running
    before an evaluation must sit where its restatement sits (1e-10 A, and 1e-10 in fractional coordinates x cell)."""
    eng = model.engine
    prep = eng.prepare_structures(structs)
    host = prep.host()
    B, N = len(structs), int(prep.atom_off[-1])
    p, lp = _params(int(relax_cell), fmax, max_steps), _lbfgs(memory)
    rel = [LbfgsRelaxation(s.frac_coords, s.lattice.matrix, relax_cell=relax_cell, fmax=fmax, steps=max_steps, p={**LBFGS, "memory": memory})
           for s in structs]
    h = ctypes.c_void_p()
    eng._check(eng.lib.chg_relax_create_lbfgs(eng.handle, ctypes.byref(host), ctypes.byref(p), ctypes.byref(lp), ctypes.byref(h)))
    counts = []
    try:
        n_active = ctypes.c_int32()
        for k in range(evaluations):
            running = [r.status == 0 for r in rel]
            eng._check(eng.lib.chg_relax_run(eng.handle, h, 1, ctypes.byref(n_active)))
            counts.append(n_active.value)
            d = _download(eng, h, B, N)
            for i, r in enumerate(rel):
                if not running[i]:
                    continue
                sl = slice(prep.atom_off[i], prep.atom_off[i + 1])
                lat = r.lattice()
                assert np.abs(d["lattice"][i] - lat).max() < 1e-10, (k, i)
                assert np.abs(d["frac"][sl] @ d["lattice"][i] - r.frac() @ lat).max() < 1e-10, (k, i)
                if not relax_cell:
                    assert np.array_equal(d["lattice"][i], r.L0), (k, i)
                f, sig = d["force"][sl].astype(np.float64), d["stress"][i].astype(np.float64) * GPA
                r.advance(f, sig, bool(np.all(np.isfinite(f)) and np.all(np.isfinite(sig))))
                assert (d["n_steps"][i], d["status"][i]) == (r.steps, r.status), (k, i)
            assert n_active.value == sum(r.status == 0 for r in rel), k
            if n_active.value == 0:
                break
    finally:
        eng.lib.chg_relax_free(eng.handle, h)
    return rel, counts


@pytest.mark.parametrize("relax_cell", [True, False])
def test_driver_teacher_forced(model, relax_cell):
    structs = [_structure("limno2", rattle=0.08, strain=0.03, seed=11), _structure("li9co7o16", rattle=0.08, strain=0.03, seed=12)]
    rel, counts = _replay(model, structs, relax_cell, fmax=1e-6, max_steps=500, memory=4, evaluations=12)
    assert counts == [2] * 12
    for r in rel:
        assert r.steps == 12 and r.appended == 11 and len(r.rho) == 4      # the ring wrapped on the way


def test_compaction_keeps_history_with_its_structure(model):
    from chgnet_amd.graph.structure import Lattice, Structure

    lone = Structure(Lattice(np.eye(3) * 4.0), [3], [[0.0, 0.0, 0.0]])      # no force on it: converged at evaluation 0
    structs = [lone, _structure("limno2", rattle=0.08, seed=21), _structure("li9co7o16", rattle=0.08, seed=22)]
    rel, counts = _replay(model, structs, False, fmax=0.05, max_steps=8, memory=4, evaluations=12)
    assert counts[0] == 2 and all(a >= b for a, b in zip(counts, counts[1:])) and counts[-1] == 0
    assert (rel[0].status, rel[0].steps) == (1, 0)
    for r in rel[1:]:
        assert r.status in (1, 2) and r.steps >= 3
        assert r.steps == 8 if r.status == 2 else r.steps <= 8


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
def test_struct_optimizer_lbfgs_end_to_end(model, capsys):
    from chgnet_amd.relax import StructOptimizer

    s = _structure("limno2", rattle=0.06, strain=0.02, seed=5)
    opt = StructOptimizer(model=model, optimizer_class="LBFGS")
    res = opt.relax_batch([s], fmax=0.05, steps=200)[0]
    assert res["status"] == "CONVERGED" and res["converged"] and 0 < res["n_steps"] < 200
    fin = res["final_structure"]
    p0, p1 = model.predict_structure(s), model.predict_structure(fin)
    # the generalized force of the final configuration in the coordinates of the run: F = (L0^-1 L)^T, X = c log F
    r = Relaxation(s.frac_coords, s.lattice.matrix)
    F = (np.linalg.inv(r.L0) @ fin.lattice.matrix).T
    r.q[r.n:] = r.c * np.real(logm(F))
    r.q[:r.n] = fin.frac_coords @ r.L0
    g = r.generalized_forces(np.asarray(p1["f"], np.float64), np.asarray(p1["s"], np.float64) * GPA)
    assert np.sqrt((g ** 2).sum(1).max()) < 0.05 + 1e-4
    assert float(p1["e"]) < float(p0["e"])
    res3 = opt.relax_batch([s], fmax=1e-6, steps=3)[0]
    assert res3["status"] == "MAX_STEPS" and res3["n_steps"] == 3
    capsys.readouterr()
    one = opt.relax(s, fmax=0.05, steps=200, verbose=True)
    printed = capsys.readouterr().out
    assert printed.count("LBFGS[0]:") == len(one["trajectory"]) - 1 and "FIRE[" not in printed and "CONVERGED" in printed
    assert len(one["trajectory"]) - 2 == res["n_steps"]      # frames: one per evaluation (n_steps + 1) and the final one once more
    # keywords reach the engine: without the cell no atom moves further than maxstep in a step, and the first step (g / alpha with
    # forces above fmax = 0.05 > alpha maxstep) is clamped to exactly that
    short = opt.relax_batch([s], fmax=1e-6, steps=5, relax_cell=False, maxstep=5e-4, memory=2, trajectory=True)[0]
    pos = short["trajectory"].atom_positions
    moved = [np.sqrt(((b - a) ** 2).sum(1).max()) for a, b in zip(pos[:5], pos[1:6])]
    assert short["n_steps"] == 5 and max(moved) <= 5e-4 * (1 + 1e-6) and moved[0] == pytest.approx(5e-4, rel=1e-6)


# ---- 5. a large batch -----------------------------------------------------------------------------------------------------------
def test_large_batch_five_steps(model):
    structs = [_structure("limno2", (5, 1, 1), rattle=0.05, strain=0.02, seed=100 + i) for i in range(1024)]
    eng = model.engine
    prep = eng.prepare_structures(structs)
    host = prep.host()
    p, lp = _params(1, 0.1, 5), _lbfgs(100)           # memory 100, capped to min(memory, max_steps) = 5 slots
    h = ctypes.c_void_p()
    eng._check(eng.lib.chg_relax_create_lbfgs(eng.handle, ctypes.byref(host), ctypes.byref(p), ctypes.byref(lp), ctypes.byref(h)))
    assert h.value
    try:
        n_active, history = ctypes.c_int32(), []
        for _ in range(8):
            eng._check(eng.lib.chg_relax_run(eng.handle, h, 1, ctypes.byref(n_active)))
            history.append(n_active.value)
            if n_active.value == 0:
                break
        out = _download(eng, h, 1024, int(prep.atom_off[-1]))
    finally:
        eng.lib.chg_relax_free(eng.handle, h)
    assert history[-1] == 0 and len(history) == 6 and all(a >= b for a, b in zip(history, history[1:]))
    for k in ("frac", "lattice", "energy", "force", "stress", "magmom"):
        assert np.all(np.isfinite(out[k])), k
    assert set(np.unique(out["status"])) <= {1, 2}
    assert np.all(out["n_steps"][out["status"] == 2] == 5) and np.all(out["n_steps"] <= 5)
