"""Dimer saddle search on the MI355X: the step kernel against the float64 restatement (tests/dimer_ref.py), the refusals of the
entry points, the driver replayed teacher-forced through the restatement (phases that diverge, compaction) and ``DimerSearch`` end to
end on the vacancy hop of tests/test_gpu_neb.py, against the restatement and against a climbing band of the same hop."""

from __future__ import annotations

import copy
import ctypes

import numpy as np
import pytest

from conftest import load_case
from dimer_ref import PROBE, TRIAL, Dimer, modified_force, pack_state, unpack_state
from relax_ref import FIRE

pytestmark = pytest.mark.gpu

DELTA, ANGLE_TOL = 0.01, 0.05


def _params(fmax=0.05, max_steps=500, max_rotations=4, delta=DELTA, angle_tol=ANGLE_TOL):
    from chgnet_amd import _lib

    return _lib.DimerParams(fmax=fmax, max_steps=max_steps, max_rotations=max_rotations, dt=FIRE["dt"], maxstep=FIRE["maxstep"],
                            dtmax=FIRE["dtmax"], finc=FIRE["finc"], fdec=FIRE["fdec"], astart=FIRE["astart"], fa=FIRE["fa"], nmin=FIRE["nmin"],
                            reserved=0, delta=delta, angle_tol=angle_tol, r_atom=6.0, r_bond=3.0, numerical_tol=1e-8)


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
    return Structure(Lattice(s.lattice.matrix), s.atomic_numbers, cart @ np.linalg.inv(s.lattice.matrix))


# ---- 1. the step kernel on its own ---------------------------------------------------------------------------------------------
# One workgroup of 256 threads per search; every pass strides over the 3 n components or the n rows (a second trip beyond 85 atoms
# and beyond 256, reductions change shape at the wave).  Every case lives on a quadratic surface of its own,
#   F(X) = Fc - H (X - R),   H = mu + l1 u1 u1^T + l2 u2 u2^T,   u1 = N cos a1 + T sin a1,   u2 = N cos a2 + W sin a2
# with N, T, W orthonormal over the free components: the torque on the given axis is l1 cos a1 sin a1 T + l2 cos a2 sin a2 W, so a1 and
# a2 decide whether a rotation is wanted, l2 whether one rotation is enough, mu and l1 the sign of the curvature.  The forces reach the
# kernel and the restatement rounded to f32, with garbage on the held components.
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 600]
STEP_FMAX, STEP_MAX_STEPS, STEP_MAX_ROTATIONS = 1e-3, 50, 4
ROTATING = dict(mu=1.0, l1=-4.0, a1=0.5, l2=3.0, a2=1.0)        # phi1 = 0.53 on the given axis, 0.15 after one rotation
ONE_ROTATION = dict(mu=1.0, l1=-4.0, a1=0.5, l2=0.0, a2=0.0)    # the softest mode lies in the plane of the first rotation
ALIGNED = dict(mu=1.0, l1=-4.0, a1=0.004, l2=0.0, a2=0.0)       # phi1 = 0.0027 < angle_tol, C0 = -3
CONVEX = dict(mu=5.0, l1=-1.0, a1=0.004, l2=0.0, a2=0.0)        # C0 = +4
# input phase PROBE
PROBE_KINDS = {"rotate": ROTATING, "aligned": ALIGNED, "convex": CONVEX, "first": ALIGNED, "first_convex": CONVEX, "uphill_old": ALIGNED,
               "downhill": ALIGNED, "downhill_convex": CONVEX, "clamp": ALIGNED, "converged": ALIGNED, "convex_no_force": CONVEX,
               "max_steps": ALIGNED, "nonfinite_f": ALIGNED, "nonfinite_e": ROTATING, "stopped": ALIGNED}
# input phase TRIAL: the restatement's own state after a PROBE on the surface
TRIAL_KINDS = {"trial_again": ROTATING, "trial_enough": ONE_ROTATION, "trial_cap": ROTATING, "trial_other_shift": ROTATING,
               "trial_clamp": ONE_ROTATION, "trial_nonfinite_f": ROTATING, "trial_nonfinite_e": ROTATING, "trial_stopped": ROTATING}
KINDS = {**PROBE_KINDS, **TRIAL_KINDS}
WANT_STATUS = {"converged": 1, "max_steps": 2, "nonfinite_f": 3, "nonfinite_e": 3, "stopped": 1, "trial_nonfinite_f": 3, "trial_nonfinite_e": 3,
               "trial_stopped": 1}
WANT_PHASE = {"rotate": TRIAL, "trial_again": TRIAL}             # of the searches that go on; every other one translates: PROBE
SENTINEL = 777.0


def _build_case(rng, n, kind, mask):
    """-> (Dimer as the kernel gets it, E, F of the evaluation to step on)."""
    spec = KINDS[kind]
    L = np.diag(rng.uniform(4, 9, 3)) + rng.normal(0, 0.6, (3, 3))
    R = rng.uniform(0, 5, (n, 3))
    fixed = None
    if mask:
        fixed = rng.random((n, 3)) < 0.3
        fixed[0] = False                                   # three free components at least ...
        if n == 1:                                         # ... but for one atom: z is held wherever a rotation in one plane will do
            fixed[0, 2] = spec["l2"] == 0.0
    free = np.ones((n, 3), bool) if fixed is None else ~fixed
    basis = []
    for _ in range(3 if free.sum() >= 3 else 2):           # N, T, W: orthonormal, 0 on the held components
        x = rng.normal(size=(n, 3)) * free
        for b in basis:
            x -= (x * b).sum() * b
        basis.append(x / np.sqrt((x * x).sum()))
    N, T = basis[:2]
    W = basis[2] if len(basis) == 3 else np.zeros((n, 3))
    u1 = N * np.cos(spec["a1"]) + T * np.sin(spec["a1"])
    u2 = N * np.cos(spec["a2"]) + W * np.sin(spec["a2"])
    target = {"clamp": 50.0, "trial_clamp": 50.0, "converged": 1e-5, "convex_no_force": 1e-5}.get(kind, 1.0)
    Fc = rng.normal(0, 1, (n, 3)) * target / np.sqrt(3 * n)

    def evaluate(X):
        F = np.array([Fc - (spec["mu"] * (x - R) + spec["l1"] * u1 * (u1 * (x - R)).sum() + spec["l2"] * u2 * (u2 * (x - R)).sum()) for x in X])
        if fixed is not None:
            F[:, fixed] = rng.normal(0, 3, (len(X), int(fixed.sum())))
        return rng.normal(-5, 1, len(X)).astype(np.float32), F.astype(np.float32)

    dm = Dimer(R, N, L, delta=DELTA, max_rotations=STEP_MAX_ROTATIONS, angle_tol=ANGLE_TOL, fixed=fixed, fmax=STEP_FMAX, steps=STEP_MAX_STEPS)
    dm.steps, dm.nsteps = 3, 2
    dm.dt, dm.a = 0.1 * rng.uniform(0.8, 1.2), 0.1 * rng.uniform(0.8, 1.0)
    dm.v = 0.1 * rng.normal(size=(n, 3)) * free
    dm.Theta = T.copy()
    if kind in TRIAL_KINDS:
        dm.advance(*evaluate(dm.staged()))
        assert dm.phase == TRIAL and dm.status == 0 and dm.rot == 0, kind
        if kind == "trial_cap":
            dm.rot = dm.rot_total = STEP_MAX_ROTATIONS - 1
        if kind == "trial_other_shift":                    # no search gets here by itself: the torque it remembers has the wrong sign
            dm.gn = -dm.gn
    E, F = evaluate(dm.staged())
    # the velocity relative to the modified force of the translation this step takes (none: the noise above stays)
    dry = copy.deepcopy(dm)
    dry.advance(E, F)
    if "C0" in dry.trace:
        G = modified_force(dry.F0, dry.N, dry.C0)
        noise = 0.05 * np.sqrt((G ** 2).mean()) * rng.normal(size=G.shape) * free
        dm.v = (-0.5 if kind.startswith("downhill") else 0.5) * G + noise      # G.v = -+ |G|^2 / 2, far from 0
    if kind.startswith("first"):
        dm.steps = dm.nsteps = 0                           # the velocity is ignored: the first step starts from v = 0
    if kind == "uphill_old":
        dm.nsteps = FIRE["nmin"] + 2
    if kind == "max_steps":
        dm.steps = STEP_MAX_STEPS
    if kind in ("nonfinite_f", "trial_nonfinite_f"):
        F[len(F) - 1 if n % 2 else 0, n // 2, 1] = np.nan
    if kind in ("nonfinite_e", "trial_nonfinite_e"):
        E[-1] = np.inf
    if kind in ("stopped", "trial_stopped"):
        dm.status = 1
    return dm, E, F


def _clear_of_thresholds(dm, tag, rel=1e-6):
    """Every quantity the restatement branched on in its last step is at least ``rel`` (relative) away from its threshold."""
    t = dm.trace
    if "phi1" in t:
        assert abs(t["phi1"] - dm.angle_tol) >= rel * dm.angle_tol, (tag, t)
    if "fit" in t:
        assert t["fit"][0] >= rel * t["fit"][1] > 0.0, (tag, t)
    if "C0" in t:
        assert abs(t["C0"][0]) >= rel * t["C0"][1] > 0.0, (tag, t)
    if "fmax" in t:
        assert abs(t["fmax"] - dm.fmax) >= rel * dm.fmax, (tag, t)
    if "Gv" in t:
        assert abs(t["Gv"][0]) >= rel * t["Gv"][1] > 0.0, (tag, t)
    if "dr" in t:
        assert abs(t["dr"] - dm.p["maxstep"]) >= rel * dm.p["maxstep"], (tag, t)


def _launch(eng, state, energy, force, fixed, final_try=1):
    from chgnet_amd import _lib

    atom_off = state[0]
    arrays = [a.copy() for a in state[1:]]
    S, N = len(atom_off) - 1, int(atom_off[-1])
    frac_next = np.full((2 * N, 3), SENTINEL)
    phase_next, status_next, retry = np.full(S, -7, np.int32), np.full(S, -7, np.int32), np.zeros(S, np.int32)
    p = _params(STEP_FMAX, STEP_MAX_STEPS, STEP_MAX_ROTATIONS)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(_lib.c_int_p)  # noqa: E731
    fx = fixed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if fixed is not None else None
    r, nvec, theta, v, f0, f1, sd, si, e_img, f_img = arrays
    eng._check(eng.lib.chg_test_dimer_step(eng.handle, ctypes.byref(p), S, ip(atom_off), dp(r), dp(nvec), dp(theta), dp(v), dp(f0), dp(f1), dp(sd),
                                           ip(si), fp(e_img), fp(f_img), fp(energy), fp(force), final_try, fx, dp(frac_next), ip(phase_next),
                                           ip(status_next), ip(retry)))
    return arrays, frac_next, phase_next, status_next, retry


def _same_bits(a, b, atom_off, k):
    """The rows of search k in every state array (r .. f1 by atoms, sd, si, e_img by search, f_img by two images)."""
    sl, sl2 = slice(atom_off[k], atom_off[k + 1]), slice(2 * atom_off[k], 2 * atom_off[k + 1])
    return (all(np.array_equal(x[sl], y[sl], equal_nan=True) for x, y in zip(a[:6], b[:6])) and np.array_equal(a[6][k], b[6][k])
            and np.array_equal(a[7][k], b[7][k]) and np.array_equal(a[8][k], b[8][k]) and np.array_equal(a[9][sl2], b[9][sl2]))


@pytest.mark.parametrize("mask", [False, True])
def test_step_kernel_matches_restatement(hip_engine, mask):
    rng = np.random.default_rng(2000 + mask)
    cases = [(n, kind) for kind in KINDS for n in SIZES]
    built = [_build_case(rng, n, kind, mask) for n, kind in cases]
    dimers = [d for d, _, _ in built]
    state = pack_state(dimers)
    atom_off, inp = state[0], state[1:]
    energy = np.ascontiguousarray(np.concatenate([E for _, E, _ in built]), np.float32)
    force = np.ascontiguousarray(np.concatenate([F.reshape(-1, 3) for _, _, F in built]), np.float32)
    assert len(energy) == sum(2 if d.phase == PROBE else 1 for d in dimers)
    fixed = np.ascontiguousarray(np.concatenate([d.fixed for d in dimers]).astype(np.uint8)) if mask else None

    # the restatement first: every case takes the branch it was built for, clear of every threshold
    before = [copy.deepcopy(d) for d in dimers]
    for d, (n, kind), (_, E, F) in zip(dimers, cases, built):
        d.advance(E, F.astype(np.float64))
        _clear_of_thresholds(d, (kind, n))
        assert d.status == WANT_STATUS.get(kind, 0), (kind, n, d.status)
        if d.status == 0 and kind != "trial_other_shift":      # (that one goes where its made-up torque sends it)
            assert d.phase == WANT_PHASE.get(kind, PROBE), (kind, n, d.trace)
        if kind in TRIAL_KINDS and d.status != 3 and kind != "trial_stopped":
            assert d.trace["shift"] == (-np.pi / 2 if kind == "trial_other_shift" else np.pi / 2), (kind, n)
        if kind == "trial_cap":
            assert d.phi1 >= ANGLE_TOL and d.rot_total == STEP_MAX_ROTATIONS and "phi1" not in d.trace, (kind, n)
        if kind == "trial_enough":
            assert d.trace["phi1"] < ANGLE_TOL and d.rot_total == 1, (kind, n)
        if kind in ("convex", "first_convex", "downhill_convex", "convex_no_force"):
            assert d.C0 > 0 and d.status == 0, (kind, n)
        if kind == "convex_no_force":
            assert d.fmax_now < STEP_FMAX, (kind, n)

    out, frac_next, phase_next, status_next, retry = _launch(hip_engine, state, energy, force, fixed)
    assert not retry.any()
    got = [Dimer.__new__(Dimer) for _ in dimers]
    unpack_state(got, atom_off, *out)
    tol = lambda ref: 2e-12 * (np.abs(ref).max() + 1.0)  # noqa: E731
    seen = set()
    for k, (b, b0, g, (n, kind), (_, E, F)) in enumerate(zip(dimers, before, got, cases, built)):
        tag = (kind, n)
        rows = frac_next[2 * atom_off[k]:2 * atom_off[k + 1]]
        assert (status_next[k], g.status) == (b.status, b.status) and phase_next[k] == b.phase == g.phase, (tag, status_next[k], phase_next[k])
        if kind in ("stopped", "trial_stopped") or b.status == 3:        # nothing evaluated: every array of the search is what it was
            want = [a.copy() for a in inp]
            want[7][k, 2] = b.status
            assert _same_bits(out, want, atom_off, k) and np.all(rows == SENTINEL), tag
            continue
        # what was evaluated, as it came
        if b0.phase == PROBE:
            assert np.array_equal(g.e_img, E) and np.array_equal(g.f_img, F), tag
        else:
            assert g.e_img[1] == E[0] and np.array_equal(g.f_img[1], F[0]) and g.e_img[0] == b0.e_img[0] and np.array_equal(g.f_img[0], b0.f_img[0]), tag
        for name in ("N", "Theta", "F0", "F1", "v", "R"):
            assert np.abs(getattr(g, name) - getattr(b, name)).max() <= tol(getattr(b, name)), (tag, name)
        for name in ("C0", "gn", "phi1", "fmax_now"):
            assert abs(getattr(g, name) - getattr(b, name)) <= tol(getattr(b, name)), (tag, name, getattr(g, name), getattr(b, name))
        assert (g.nsteps, g.steps, g.rot, g.rot_total) == (b.nsteps, b.steps, b.rot, b.rot_total), tag
        assert abs(g.dt - b.dt) <= 1e-15 and abs(g.a - b.a) <= 1e-15, tag
        assert abs((g.N * g.N).sum() - 1.0) <= 1e-14, tag
        if b.fixed is not None:
            assert np.all(g.N[b.fixed] == 0.0) and np.all(g.F0[b.fixed] == 0.0) and np.all(g.F1[b.fixed] == 0.0), tag
            assert np.array_equal(g.R[b.fixed], b0.R[b.fixed]) and np.all(g.v[b.fixed] == 0.0) and np.all(g.Theta[b.fixed] == 0.0), tag
        moved = b.status == 0 and b.phase == PROBE
        if not moved:                                           # a rotation decision or a stop: centre and optimizer bit-identical
            assert np.array_equal(g.R, b0.R) and np.array_equal(g.v, b0.v) and (g.dt, g.a, g.nsteps, g.steps) == (b0.dt, b0.a, b0.nsteps, b0.steps), tag
        if b.status != 0:
            assert np.all(rows == SENTINEL), tag
            continue
        want = b.frac().reshape(-1, 3)                          # the rows of the next evaluation, exact in count
        assert len(want) == (2 * n if moved else n), tag
        assert np.abs(rows[:len(want)] - want).max() <= tol(want) and np.all(rows[len(want):] == SENTINEL), tag
        if not moved:
            assert np.array_equal(g.Theta, b.Theta) or np.abs(g.Theta - b.Theta).max() <= tol(b.Theta), tag
            seen.add(kind)
            continue
        assert np.array_equal(g.Theta, b0.Theta), tag           # no rotation asked for: the direction of the last one stays
        step = np.sqrt(((b.R - b0.R) ** 2).sum())
        if kind in ("clamp", "trial_clamp"):
            assert step == pytest.approx(FIRE["maxstep"], rel=1e-12) and np.sqrt(((g.R - b0.R) ** 2).sum()) == pytest.approx(FIRE["maxstep"], rel=1e-12), tag
        else:
            assert step < 0.9 * FIRE["maxstep"], tag
        if kind.startswith("first"):
            assert b0.steps == 0 and b.nsteps == 0 and "Gv" not in b.trace, tag
        elif kind.startswith("downhill"):
            assert b.trace["Gv"][0] < 0 and b.nsteps == 0 and b.dt == b0.dt * FIRE["fdec"] and b.a == FIRE["astart"], tag
        else:
            assert b.trace["Gv"][0] > 0 and b.nsteps == b0.nsteps + 1 and (b.dt > b0.dt) == (kind == "uphill_old"), tag
        seen.add(kind)
    assert seen == set(KINDS) - set(WANT_STATUS)

    # the same input once more: the same bits
    again = _launch(hip_engine, state, energy, force, fixed)
    assert all(np.array_equal(a, c, equal_nan=True) for a, c in zip(again[0], out))
    assert all(np.array_equal(a, c) for a, c in zip(again[1:], (frac_next, phase_next, status_next, retry)))

    # not the final try: a search with a non-finite image is held back untouched (still running, flag set); the others step as before
    held, frac3, phase3, status3, retry3 = _launch(hip_engine, state, energy, force, fixed, final_try=0)
    for k, (n, kind) in enumerate(cases):
        nonfinite = "nonfinite" in kind
        assert retry3[k] == nonfinite, (kind, n)
        assert _same_bits(held, inp if nonfinite else out, atom_off, k), (kind, n)
        rows = slice(2 * atom_off[k], 2 * atom_off[k + 1])
        if nonfinite:
            assert status3[k] == 0 and phase3[k] == before[k].phase and np.all(frac3[rows] == SENTINEL), (kind, n)
        else:
            assert status3[k] == status_next[k] and phase3[k] == phase_next[k] and np.array_equal(frac3[rows], frac_next[rows]), (kind, n)


# ---- 2. creation ----------------------------------------------------------------------------------------------------------------
def test_create_and_set_fixed_refusals(hip_engine):
    from chgnet_amd.graph.structure import Lattice, Structure

    eng = hip_engine
    s = Structure(Lattice(np.eye(3) * 5.0), [3, 8], [[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]])
    prep = eng.prepare_structures([s, s])
    host = prep.host()
    good = np.tile([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0]], (2, 1))

    def create(mode, fixed=None, **kw):
        h = ctypes.c_void_p()
        mode = np.ascontiguousarray(mode, np.float64)
        rc = eng.lib.chg_dimer_create(eng.handle, ctypes.byref(host), mode.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(_params(**kw)),
                                      ctypes.byref(h))
        msg = eng.lib.chg_last_error(eng.handle).decode()
        if rc == 0 and fixed is not None:
            fixed = np.ascontiguousarray(fixed, np.uint8)
            rc = eng.lib.chg_dimer_set_fixed(eng.handle, h, fixed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
            msg = eng.lib.chg_last_error(eng.handle).decode()
        if h.value:
            eng.lib.chg_dimer_free(eng.handle, h)
        return rc, msg

    assert create(good)[0] == 0
    assert create(good, delta=0.5, max_rotations=0, angle_tol=1e-4)[0] == 0 and create(good, max_rotations=32, angle_tol=0.78)[0] == 0
    for kw, word in ((dict(delta=0.0), "delta"), (dict(delta=-0.01), "delta"), (dict(delta=0.51), "delta"), (dict(delta=float("nan")), "delta"),
                     (dict(max_rotations=-1), "max_rotations"), (dict(max_rotations=33), "max_rotations"), (dict(angle_tol=9e-5), "angle_tol"),
                     (dict(angle_tol=np.pi / 4), "angle_tol"), (dict(angle_tol=float("nan")), "angle_tol")):
        rc, msg = create(good, **kw)
        assert rc == -1 and word in msg, (kw, msg)
    zero = good.copy()
    zero[2:] = 0.0
    rc, msg = create(zero)
    assert rc == -1 and "mode of search 1 is zero" in msg, msg
    bad = good.copy()
    bad[0, 1] = np.inf
    rc, msg = create(bad)
    assert rc == -1 and "search 0" in msg and "finite" in msg, msg
    mask = np.zeros((4, 3), np.uint8)
    mask[0, 0] = mask[1, 1] = 1                               # everything the mode of search 0 moves
    rc, msg = create(good, fixed=mask)
    assert rc == -1 and "mode of search 0 has no free component" in msg, msg
    mask[1, 1] = 0
    assert create(good, fixed=mask)[0] == 0


# ---- 3. the driver, teacher-forced ---------------------------------------------------------------------------------------------
# The engine's fp32 forces are not bit-reproducible run to run, so the restatement is fed the energies and forces the device
# downloaded for every evaluation (image_energy, image_force); its next centre and axis must then be the device's.
def _download(eng, handle, S, N):
    from chgnet_amd import _lib

    out = {"frac": np.empty((N, 3)), "mode": np.empty((N, 3)), "force": np.empty((N, 3)), "image_energy": np.empty((S, 2), np.float32),
           "image_force": np.empty((2 * N, 3), np.float32), "curvature": np.empty(S), "fmax": np.empty(S), "n_steps": np.empty(S, np.int32),
           "n_rotations": np.empty(S, np.int32), "n_evaluated": np.empty(S, np.int32), "status": np.empty(S, np.int32),
           "phase": np.empty(S, np.int32)}
    eng._check(eng.lib.chg_dimer_download(eng.handle, handle, ctypes.byref(_lib.fill_out(_lib.DimerOutHost(), out))))
    return out


def _replay(model, structs, modes, fmax, max_steps, evaluations, fixed=None):
    """Run the handle one evaluation at a time -> (restatements, active counts, structures evaluated by every call, phases before every
    call).  Every search that was running before an evaluation must have staged what its restatement stages (exact in count) and sit
    where its restatement sits afterwards (1e-10 in the centre, A, and in the axis)."""
    eng = model.engine
    prep = eng.prepare_structures(structs)
    host = prep.host()
    S, N = len(structs), int(prep.atom_off[-1])
    off = prep.atom_off
    ref = [Dimer(s.frac_coords @ s.lattice.matrix, m, s.lattice.matrix, fixed=None if fixed is None else fixed[off[k]:off[k + 1]], fmax=fmax,
                 steps=max_steps) for k, (s, m) in enumerate(zip(structs, modes))]
    h = ctypes.c_void_p()
    mode = np.ascontiguousarray(np.concatenate(modes), np.float64)
    eng._check(eng.lib.chg_dimer_create(eng.handle, ctypes.byref(host), mode.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                        ctypes.byref(_params(fmax, max_steps)), ctypes.byref(h)))
    counts, evaluated, phases = [], [], []
    try:
        if fixed is not None:
            fx = np.ascontiguousarray(fixed, np.uint8)
            eng._check(eng.lib.chg_dimer_set_fixed(eng.handle, h, fx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        d = _download(eng, h, S, N)
        for k, r in enumerate(ref):
            assert np.abs(d["mode"][off[k]:off[k + 1]] - r.N).max() < 1e-15 and np.abs(d["frac"][off[k]:off[k + 1]] @ r.L - r.R).max() < 1e-12
        n_active, total = ctypes.c_int32(), np.zeros(S, np.int64)
        for it in range(evaluations):
            running = [r.status == 0 for r in ref]
            phases.append([r.phase if run else None for r, run in zip(ref, running)])
            eng._check(eng.lib.chg_dimer_run(eng.handle, h, 1, ctypes.byref(n_active)))
            counts.append(n_active.value)
            d = _download(eng, h, S, N)
            evaluated.append(int(d["n_evaluated"].sum() - total.sum()))
            for k, r in enumerate(ref):
                staged = (2 if r.phase == PROBE else 1) if running[k] else 0
                assert d["n_evaluated"][k] - total[k] == staged, (it, k)
                if not running[k]:
                    continue
                img = d["image_force"][2 * off[k]:2 * off[k + 1]].astype(np.float64).reshape(2, r.n, 3)
                E, F = (d["image_energy"][k], img) if r.phase == PROBE else (d["image_energy"][k, 1:], img[1:])
                r.advance(E, F)
                sl = slice(off[k], off[k + 1])
                assert np.abs(d["frac"][sl] @ r.L - r.R).max() < 1e-10 and np.abs(d["mode"][sl] - r.N).max() < 1e-10, (it, k)
                assert (d["n_steps"][k], d["status"][k], d["phase"][k], d["n_rotations"][k]) == (r.steps, r.status, r.phase, r.rot_total), (it, k)
                assert abs(d["curvature"][k] - r.C0) <= 1e-8 * (1 + abs(r.C0)) and abs(d["fmax"][k] - r.fmax_now) <= 1e-12, (it, k)
                assert np.array_equal(d["force"][sl], r.F0), (it, k)
            total = d["n_evaluated"].astype(np.int64)
            assert n_active.value == sum(r.status == 0 for r in ref), it
            if n_active.value == 0:
                break
    finally:
        eng.lib.chg_dimer_free(eng.handle, h)
    return ref, counts, evaluated, phases


def _modes(structs, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(len(s), 3)) for s in structs]


def test_driver_teacher_forced(model):
    structs = [_structure("s16tri", rattle=0.05, seed=60), _structure("limno2", rattle=0.05, seed=61)]
    ref, counts, evaluated, phases = _replay(model, structs, _modes(structs, 62), fmax=1e-6, max_steps=500, evaluations=12)
    assert counts == [2] * 12 and phases[0] == [PROBE, PROBE] and evaluated[0] == 4
    assert evaluated == [sum(2 if p == PROBE else 1 for p in ph) for ph in phases]
    print("phases", phases, "structures", evaluated)
    assert any(p[0] != p[1] for p in phases), "the two searches never diverged in phase"
    assert all(r.status == 0 and r.steps >= 1 and r.rot_total >= 1 for r in ref)


def _one_free_component(structs, seed):
    """A mask that holds 30% of the components of the first structure and all but one of the second: with a single free component the
    torque on the axis is exactly 0, so that search never rotates -- every evaluation of it is a PROBE, whatever the forces are."""
    n0, n1 = len(structs[0]), len(structs[1])
    fixed = np.ones((n0 + n1, 3), bool)
    fixed[:n0] = np.random.default_rng(seed).random((n0, 3)) < 0.3
    fixed[n0 + 3, 1] = False
    return fixed


def test_driver_with_a_mask_and_phases_that_must_diverge(model):
    structs = [_structure("s16tri", rattle=0.05, seed=63), _structure("limno2", rattle=0.05, seed=64)]
    fixed = _one_free_component(structs, 65)
    ref, counts, evaluated, phases = _replay(model, structs, _modes(structs, 66), fmax=1e-6, max_steps=500, evaluations=8, fixed=fixed)
    assert counts == [2] * 8
    assert all(p[1] == PROBE for p in phases) and phases[1][0] == TRIAL        # the free search rotates at once, the other one never
    assert evaluated == [4] + [3 if p[0] == TRIAL else 4 for p in phases[1:]]
    assert ref[1].rot_total == 0 and ref[1].steps == 8 and ref[0].rot_total >= 1
    for k, r in enumerate(ref):
        s = structs[k]
        assert np.all(r.N[r.fixed] == 0.0) and np.array_equal(r.R[r.fixed], (s.frac_coords @ s.lattice.matrix)[r.fixed])


def test_compaction_drops_a_search_that_stops_at_its_first_translation(model):
    """fmax far above every force and no translation allowed: a search stops at its first translation decision, CONVERGED where the
    curvature is negative and MAX_STEPS where it is not.  The search with one free component decides at the first evaluation, the
    other one rotates first: the batch shrinks to its trial image."""
    structs = [_structure("s16tri", rattle=0.05, seed=63), _structure("limno2", rattle=0.05, seed=64)]
    fixed = _one_free_component(structs, 65)
    fixed[:16] = False
    ref, counts, evaluated, phases = _replay(model, structs, _modes(structs, 66), fmax=1e3, max_steps=0, evaluations=10, fixed=fixed)
    print("active", counts, "structures", evaluated, [(r.status, r.steps, r.rot_total, r.C0) for r in ref])
    k = len(counts)
    assert 2 <= k <= 6 and counts == [1] * (k - 1) + [0] and evaluated == [4] + [1] * (k - 1)
    assert (ref[1].steps, ref[1].rot_total) == (0, 0) and ref[1].status == (1 if ref[1].C0 < 0 else 2)
    assert (ref[0].steps, ref[0].rot_total) == (0, k - 1) and ref[0].status == (1 if ref[0].C0 < 0 else 2)


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------
# The vacancy hop of tests/test_gpu_neb.py, built again here in the same well-posed way: a 3x2x2 LiMnO2 supercell with one Li removed
# (95 atoms), three cells along the hop, a seeded 0.01 A displacement before relaxing, the final end made from the relaxed initial
# one by the crystal's own translation, and the smooth random-initialisation weights.
@pytest.fixture(scope="module")
def smooth_model(golden_weights):
    from chgnet_amd import CHGNet

    return CHGNet(state_dict=golden_weights)


def _vacancy_hop(model):
    """-> (the two relaxed end points, their relaxation results, index of the hopping Li)."""
    from chgnet_amd.graph.structure import Lattice, Structure
    from chgnet_amd.relax import StructOptimizer

    s = _structure("limno2", (3, 2, 2))
    z, frac, lat = s.atomic_numbers, s.frac_coords, s.lattice.matrix
    vac = int(np.flatnonzero(z == 3)[0])
    keep = np.arange(len(z)) != vac
    z1, sites = z[keep], frac[keep]
    d = sites - frac[vac]
    d -= np.round(d)
    dist = np.sqrt(((d @ lat) ** 2).sum(1))
    dist[z1 != 3] = np.inf
    hop = int(np.argmin(dist))
    h = d[hop]
    opt = StructOptimizer(model=model)
    start = sites + 0.01 * np.random.default_rng(7).normal(size=sites.shape) @ np.linalg.inv(lat)
    a = opt.relax_batch([Structure(Lattice(lat), z1, start)], fmax=0.02, steps=500, relax_cell=False)[0]["final_structure"]
    fa, fb, used = a.frac_coords, np.empty_like(a.frac_coords), np.zeros(len(z1), bool)
    for j in range(len(z1)):
        t = sites - (sites[j] - h)
        t -= np.round(t)
        k = int(np.argmin((t ** 2).sum(1)))
        if (t[k] ** 2).sum() < 1e-10:
            assert z1[k] == z1[j]
            fb[j], used[k] = fa[k] + h, True
        else:
            assert j == hop
    (left,) = np.flatnonzero(~used)
    assert z1[left] == 3
    fb[hop] = fa[left] + h
    out = opt.relax_batch([a, Structure(Lattice(lat), z1, fb)], fmax=0.02, steps=500, relax_cell=False)
    return [r["final_structure"] for r in out], out, hop


@pytest.fixture(scope="module")
def hop(smooth_model):
    """(relaxed end points, index of the hopping Li, the start 0.35 along the interpolated path, the hop direction [n, 3] in A)."""
    from chgnet_amd.graph.structure import Lattice, Structure

    (a, b), out, i = _vacancy_hop(smooth_model)
    assert all(r["converged"] for r in out) and abs(out[0]["energy"] - out[1]["energy"]) <= 1e-3
    d = b.frac_coords - a.frac_coords
    d -= np.round(d)
    start = Structure(Lattice(a.lattice.matrix), a.atomic_numbers, a.frac_coords + 0.35 * d)
    return a, b, i, start, d @ a.lattice.matrix


def _recompute(model, structure, mode, fixed=None, delta=DELTA):
    """(curvature, fmax, energy) of the restatement from two fresh predictions at the centre and at the centre + delta mode."""
    from chgnet_amd.graph.structure import Lattice, Structure

    lat = structure.lattice.matrix
    other = Structure(Lattice(lat), structure.atomic_numbers, structure.frac_coords + delta * mode @ np.linalg.inv(lat))
    pred = model.predict_structure([structure, other], task="ef")
    F = np.array([p["f"] for p in pred], np.float64)
    if fixed is not None:
        F[:, fixed] = 0.0
    return -((F[1] - F[0]) * mode).sum() / delta, float(np.sqrt((F[0] ** 2).sum(1).max())), float(pred[0]["e"]) * (len(structure) if model.is_intensive else 1)


FORCE_NOISE = 2e-5       # eV/A: the bound smoke() puts on a force component of the engine against the float64 oracle


def _curvature_tol(n, delta=DELTA):
    """Reported and recomputed curvature are both -(F1 - F0).N / delta from f32 engine forces at the same two configurations.  If
    every force component is within e = FORCE_NOISE of the exact one, |(dF1 - dF0).N| <= |dF1 - dF0|_2 |N|_2 <= 2 sqrt(3n) e for the
    unit axis N, so either curvature is within 2 sqrt(3n) e / delta of the exact finite difference and the two are within
    4 sqrt(3n) e / delta of each other: 0.135 eV/A^2 for the 95 atoms and delta = 0.01 A here.  (Where the reported one rests on an
    extrapolated F1, its second-order error, delta |d3E| sin(phi) / 2, is a few 1e-3 on this smooth surface and sits inside.)"""
    return 4.0 * np.sqrt(3.0 * n) * FORCE_NOISE / delta


# |E(dimer saddle) - E(climbing image)| measured on the MI355X, eV (DESIGN.md "Dimer saddle search"): the dimer stopped at
# E - E(a) = 0.0591 eV with curvature -0.577 eV/A^2 after 13 translations and 28 rotations, the climbing image of the 5-image band
# 0.0222 eV above it.  On this weak surface fmax = 0.05 eV/A is a loose criterion (the largest force at the start is 0.0548), so both
# searches stop early and the difference is what that criterion leaves open along the soft modes across the path, ten times the
# floor along the mode itself.  The test allows three times the measured value, and no less than what the band's own convergence
# leaves open along the mode, fmax^2 / (2 |curvature|) = 2.2e-3 eV
SADDLE_ENERGY_DIFFERENCE_MEASURED = 2.22e-2


def test_search_end_to_end_against_restatement_and_band(smooth_model, hop):
    """Curvature tolerance: see ``_curvature_tol``."""
    from chgnet_amd import DimerSearch, NudgedElasticBand

    a, b, _, start, direction = hop
    c_start, f_start, _ = _recompute(smooth_model, start, direction / np.sqrt((direction ** 2).sum()))
    search = DimerSearch(start, direction, model=smooth_model)
    res = search.run(fmax=0.05, steps=150)
    assert search.structure is res["final_structure"] and search.mode is res["mode"]
    assert res["status"] in ("CONVERGED", "MAX_STEPS") and res["converged"] == (res["status"] == "CONVERGED")
    assert abs((res["mode"] ** 2).sum() - 1.0) < 1e-12 and res["forces"].shape == (len(a), 3) and "trajectory" not in res
    assert 2 * res["n_steps"] + res["n_rotations"] <= res["n_evaluated"] <= 2 * (res["n_steps"] + 1) + res["n_rotations"]
    c, f, e = _recompute(smooth_model, res["final_structure"], res["mode"])
    e_a = float(smooth_model.predict_structure([a, b], task="ef")[0]["e"]) * (len(a) if smooth_model.is_intensive else 1)
    print(f"dimer: {res['status']} after {res['n_steps']} translations, {res['n_rotations']} rotations, {res['n_evaluated']} structures; "
          f"curvature {res['curvature']:.5f} reported, {c:.5f} recomputed ({c_start:.5f} at the start); fmax {res['fmax']:.6f} reported, "
          f"{f:.6f} recomputed ({f_start:.6f} at the start); E - E(a) = {e - e_a:.6f} eV")
    assert abs(f - res["fmax"]) <= 1e-3 and abs(c - res["curvature"]) <= _curvature_tol(len(a))
    assert abs(e - res["energy"]) <= 1e-3
    assert res["fmax"] < f_start
    if res["converged"]:
        assert res["curvature"] < 0 and res["fmax"] < 0.05
    # the same saddle from both ends: a climbing band of the same hop
    band = NudgedElasticBand(NudgedElasticBand.interpolate(a, b, 5), model=smooth_model).run(fmax=0.05, steps=200, climb=True)
    if not (res["converged"] and band["converged"]):
        print(f"no comparison: dimer {res['status']}, band {band['status']}")
        return
    diff = abs(res["energy"] - band["energies"][band["climbing_image"]])
    floor = 0.05 ** 2 / (2.0 * abs(res["curvature"]))
    print(f"saddle energy: dimer {res['energy']:.6f}, climbing image {band['energies'][band['climbing_image']]:.6f}, difference {diff:.3e} eV; "
          f"band floor fmax^2 / (2 |curvature|) = {floor:.3e} eV")
    assert diff <= max(3.0 * SADDLE_ENERGY_DIFFERENCE_MEASURED, floor)


def test_max_steps_log_fixed_atoms_and_run_batch(smooth_model, hop, capsys):
    from chgnet_amd import DimerSearch

    model = smooth_model
    a, b, moving, start, direction = hop
    short = DimerSearch(start, direction, model=model).run(fmax=1e-6, steps=3)
    assert short["status"] == "MAX_STEPS" and short["n_steps"] == 3 and not short["converged"] and "trajectory" not in short
    capsys.readouterr()
    logged = DimerSearch(start, direction, model=model).run(fmax=1e-6, steps=3, verbose=True, trajectory=True)
    printed = capsys.readouterr().out
    assert printed.count("Dimer[0]:") == 4 == len(logged["trajectory"])          # translation decisions 0..3, the last one the stop
    assert logged["n_steps"] == 3 and "MAX_STEPS" in printed.splitlines()[-1]
    first, last = logged["trajectory"][0], logged["trajectory"][-1]
    assert np.abs(first["positions"] - start.frac_coords @ start.lattice.matrix).max() < 1e-12
    assert np.abs(last["positions"] - logged["final_structure"].frac_coords @ a.lattice.matrix).max() < 1e-12 and last["fmax"] == logged["fmax"]

    held = sorted({0, 5, (moving + 1) % len(a)})
    fixed = DimerSearch(start, direction, model=model, fixed_atoms=held).run(fmax=1e-6, steps=5)
    got, free = fixed["final_structure"], np.setdiff1d(np.arange(len(a)), held)
    assert fixed["n_steps"] == 5 and np.all(fixed["mode"][held] == 0.0) and np.all(fixed["forces"][held] == 0.0)
    assert np.abs((got.frac_coords[held] - start.frac_coords[held]) @ a.lattice.matrix).max() < 1e-12
    assert got.site_properties["selective_dynamics"][held[0]] == [False, False, False]
    assert np.abs((got.frac_coords[free] - start.frac_coords[free]) @ a.lattice.matrix).max() > 1e-4      # A: the free atoms did move
    mask = np.zeros((len(a), 3), bool)
    mask[held] = True
    c, f, _ = _recompute(model, got, fixed["mode"], mask)
    assert abs(f - fixed["fmax"]) <= 1e-3 and abs(c - fixed["curvature"]) <= _curvature_tol(len(a))

    # two searches from the same minimum, pushed in two directions
    (s0, m0), (s1, m1) = (DimerSearch.displace(a, [moving], radius=3.0, stdev=0.1, seed=seed) for seed in (0, 1))
    two = DimerSearch.run_batch([s0, s1], [m0, m1], model=model, fmax=1e-6, steps=4)
    assert all(r["status"] == "MAX_STEPS" and r["n_steps"] == 4 for r in two)
    assert not np.allclose(two[0]["final_structure"].frac_coords, two[1]["final_structure"].frac_coords, atol=1e-3)
    for r in two:
        assert 2 * 5 + r["n_rotations"] == r["n_evaluated"]                 # five PROBE evaluations, one structure per rotation
        c, f, e = _recompute(model, r["final_structure"], r["mode"])
        assert abs(f - r["fmax"]) <= 1e-3 and abs(c - r["curvature"]) <= _curvature_tol(len(a)) and abs(e - r["energy"]) <= 1e-3
    # a batch gives every search what it gets alone (up to the engine's f32 forces, which differ in their last bits from run to run:
    # the centres are compared where both runs took the same rotation decisions)
    alone = DimerSearch(s1, m1, model=model).run(fmax=1e-6, steps=4)
    print("alone", alone["n_evaluated"], "in the batch", two[1]["n_evaluated"])
    if alone["n_evaluated"] == two[1]["n_evaluated"]:
        assert np.abs((alone["final_structure"].frac_coords - two[1]["final_structure"].frac_coords) @ a.lattice.matrix).max() < 1e-3
