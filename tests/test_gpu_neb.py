"""Nudged elastic band on the MI355X: the step kernel against the float64 restatement (tests/neb_ref.py), the driver replayed
teacher-forced through the restatement (with and without compaction) and ``NudgedElasticBand`` end to end."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from conftest import load_case
from neb_ref import Band, neb_fmax, neb_forces, pack_state, unpack_state
from relax_ref import FIRE

pytestmark = pytest.mark.gpu

SPRING = 0.1


def _params(fmax=0.05, max_steps=500, climb=0, spring=SPRING):
    from chgnet_amd import _lib

    return _lib.NebParams(fmax=fmax, max_steps=max_steps, climb=int(climb), dt=FIRE["dt"], maxstep=FIRE["maxstep"], dtmax=FIRE["dtmax"],
                          finc=FIRE["finc"], fdec=FIRE["fdec"], astart=FIRE["astart"], fa=FIRE["fa"], nmin=FIRE["nmin"], reserved=0,
                          spring=spring, r_atom=6.0, r_bond=3.0, numerical_tol=1e-8)


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
# One workgroup of 256 threads per band.  The per-image sums take one wave per image (lanes stride over the atoms: a second trip
# beyond 64 atoms, images beyond the fourth share a wave); the band passes stride over the (M - 2) n interior rows (a second trip
# beyond 256 rows, reductions change shape at the wave).
SIZES = [1, 2, 40, 63, 64, 65, 255, 256, 257]
IMAGES = [3, 4, 5, 9]
STEP_FMAX, STEP_MAX_STEPS = 1e-3, 50
# energy patterns (each with an ordinary uphill step) and optimizer situations (each on an interior maximum)
PATTERNS = ["rising", "falling", "intmax", "intmin", "tie_next", "tie_prev", "peak_first", "peak_last", "flat_top"]
SITUATIONS = ["first", "uphill_old", "downhill", "clamp", "converged", "max_steps", "nonfinite_f", "nonfinite_e", "stopped"]
WANT_STATUS = {"converged": 1, "max_steps": 2, "nonfinite_f": 3, "nonfinite_e": 3, "stopped": 1}
# (mask, all_images, climb) of a launch: MASK and climb are per launch
CONFIGS = [(False, 1, 0), (False, 1, 1), (True, 0, 1), (True, 1, 0), (False, 0, 0)]


def _energies(pattern, M):
    i = np.arange(M, dtype=np.float64)
    c = (M - 1) / 2 + 0.25
    if pattern == "rising":
        e = 0.37 * i - 5
    elif pattern == "falling":
        e = -0.37 * i - 5
    elif pattern == "intmax":
        e = -np.abs(i - c) - 5
    elif pattern == "intmin":
        e = np.abs(i - c) - 5
    elif pattern == "tie_next":          # E[2] == E[1] exactly (M = 3: the last image)
        e = 0.37 * i - 5
        e[2] = e[1]
    elif pattern == "tie_prev":          # E[1] == E[0] exactly
        e = 0.37 * i - 5
        e[1] = e[0]
    elif pattern == "peak_first":        # the highest interior image is the first one
        e = -0.3 * i - 5
        e[0] = -9
    elif pattern == "peak_last":         # ... the last one
        e = 0.3 * i - 5
        e[-1] = -9
    else:                                # flat_top: every interior image ties; the first one climbs
        e = np.full(M, -4.0)
        e[0], e[-1] = -5.0, -6.0
    return e.astype(np.float32)


def _build_case(rng, n, M, kind, mask, climb):
    """A band state and the results of the evaluation to step on: images along a straight line plus noise, random f32 forces
    scaled so that the whole band's |G| is about 1 (the step is then 0.06 A, below maxstep) or about 50 (kind "clamp")."""
    situation = kind if kind in SITUATIONS else "uphill_young"
    L = np.diag(rng.uniform(4, 9, 3)) + rng.normal(0, 0.6, (3, 3))
    A = rng.uniform(0, 5, (n, 3))
    Bp = A + rng.normal(0, 0.5, (n, 3))
    R = np.array([A + (Bp - A) * i / (M - 1) for i in range(M)])
    if situation != "converged":
        R[1:-1] += rng.normal(0, 0.05, R[1:-1].shape)
    fixed = None
    if mask:
        fixed = np.broadcast_to(rng.random((1, n, 3)) < 0.3, (M, n, 3)).copy()
        fixed[:, 0, 0] = False           # something is left to move
    band = Band(R, L, k=SPRING, climb=bool(climb), fixed=fixed, fmax=STEP_FMAX, steps=STEP_MAX_STEPS)
    E = _energies(kind if kind in PATTERNS else "intmax", M)
    target = {"clamp": 50.0, "converged": 1e-6}.get(situation, 1.0)
    F = (rng.normal(0, 1, (M, n, 3)) * target / np.sqrt(3 * (M - 2) * n)).astype(np.float32)
    free = np.ones((M - 2, n, 3), bool) if fixed is None else ~fixed[1:-1]
    G = neb_forces(R, E, F, SPRING, bool(climb), fixed)[0][1:-1]
    noise = 0.05 * np.sqrt((G ** 2).mean()) * rng.normal(size=G.shape) * free
    if situation == "first":
        band.v = 0.1 * rng.normal(size=G.shape) * free           # ignored: the first step starts from v = 0
    else:
        band.steps, band.nsteps = 3, 2
        band.v = (-0.5 if situation == "downhill" else 0.5) * G + noise       # G.v = -+ |G|^2 / 2, far from 0
        band.dt, band.a = 0.1 * rng.uniform(0.8, 1.2), 0.1 * rng.uniform(0.8, 1.0)
    if situation == "uphill_old":
        band.nsteps = FIRE["nmin"] + 2
    if situation == "max_steps":
        band.steps = STEP_MAX_STEPS
    if situation == "nonfinite_f":
        F[1 + (M - 2) // 2, n // 2, 1] = np.nan
    if situation == "nonfinite_e":
        E[M - 2] = np.inf
    if situation == "stopped":
        band.status = 1
    return band, E, F


def _launch(eng, state, e_img, energy, force, all_images, climb, fixed, final_try=1):
    from chgnet_amd import _lib

    band_off, atom_off = state[0], state[1]
    r, v, g, sd, si = (a.copy() for a in state[2:])
    e_img = e_img.copy()
    nb, N = len(band_off) - 1, int(atom_off[-1])
    frac_next, retry = np.zeros((N, 3)), np.zeros(nb, np.int32)
    p = _params(STEP_FMAX, STEP_MAX_STEPS, climb)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(_lib.c_int_p)  # noqa: E731
    fx = fixed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if fixed is not None else None
    eng._check(eng.lib.chg_test_neb_step(eng.handle, ctypes.byref(p), nb, ip(band_off), ip(atom_off), dp(r), dp(v), dp(g), dp(sd), ip(si),
                                         fp(e_img), fp(energy), fp(force), all_images, final_try, fx, dp(frac_next), ip(retry)))
    return (r, v, g, sd, si), e_img, frac_next, retry


def _rows(state, k):
    band_off, atom_off = state[0], state[1]
    return slice(atom_off[band_off[k]], atom_off[band_off[k + 1]])


@pytest.mark.parametrize(("mask", "all_images", "climb"), CONFIGS)
def test_step_kernel_matches_restatement(hip_engine, mask, all_images, climb):
    rng = np.random.default_rng(1000 + 100 * mask + 10 * all_images + climb)
    cases = [(n, M, kind) for kind in PATTERNS + SITUATIONS for n in SIZES for M in IMAGES]
    built = [_build_case(rng, n, M, kind, mask, climb) for n, M, kind in cases]
    bands = [b for b, _, _ in built]
    state = pack_state(bands)
    band_off, atom_off = state[0], state[1]
    # what the state knows of the energies: with all_images everything comes from the batch, otherwise the end points from the state
    e_all = np.concatenate([E for _, E, _ in built]).astype(np.float32)
    e_img = np.full_like(e_all, 77.0)
    if not all_images:
        e_img[band_off[:-1]], e_img[band_off[1:] - 1] = e_all[band_off[:-1]], e_all[band_off[1:] - 1]
    take = (lambda a: a) if all_images else (lambda a: a[1:-1])
    energy = np.ascontiguousarray(np.concatenate([take(E) for _, E, _ in built]), np.float32)
    force = np.ascontiguousarray(np.concatenate([take(F).reshape(-1, 3) for _, _, F in built]), np.float32)
    fixed = np.ascontiguousarray(np.concatenate([b.fixed.reshape(-1, 3) for b in bands]).astype(np.uint8)) if mask else None
    inp = state[2:]
    out, e_out, frac_next, retry = _launch(hip_engine, state, e_img, energy, force, all_images, climb, fixed)
    assert not retry.any()

    got = [Band.__new__(Band) for _ in bands]
    for gb, b in zip(got, bands):
        gb.M, gb.n = b.M, b.n
    unpack_state(got, band_off, atom_off, *out)
    tol = lambda ref: 2e-12 * (np.abs(ref).max() + 1.0)  # noqa: E731
    next_off = np.concatenate([[0], np.cumsum([(b.M - 2) * b.n for b in bands])])
    seen = set()
    for k, (b, (n, M, kind), (_, E, F)) in enumerate(zip(bands, cases, built)):
        tag, gb, sl = (kind, n, M), got[k], _rows(state, k)
        R0, v0 = b.R.copy(), b.v.copy()
        optimizer0 = (b.dt, b.a, b.nsteps, b.steps)
        first = b.steps == 0
        gv = float((neb_forces(R0, np.nan_to_num(E, posinf=0.0), np.nan_to_num(F), SPRING, bool(climb), b.fixed)[0][1:-1] * v0).sum())
        b.advance(E, F.astype(np.float64))
        assert b.status == WANT_STATUS.get(kind, 0) == gb.status, (tag, b.status, gb.status)
        stopped_before, nonfinite = kind == "stopped", kind in ("nonfinite_f", "nonfinite_e")
        if b.status != 0:                                   # stopped: positions, velocities and optimizer bit-identical to the input
            assert np.array_equal(gb.R, R0) and np.array_equal(gb.v, v0) and (gb.dt, gb.a, gb.nsteps, gb.steps) == optimizer0, tag
            if stopped_before or nonfinite:                 # nothing evaluated: every array of the band is what it was
                assert all(np.array_equal(a[sl], c[sl]) for a, c in zip(out[:3], inp[:3])), tag
                assert np.array_equal(out[3][k], inp[3][k]) and np.array_equal(out[4][k, [0, 1, 3]], inp[4][k, [0, 1, 3]]), tag
                assert np.array_equal(e_out[band_off[k]:band_off[k + 1]], e_img[band_off[k]:band_off[k + 1]]), tag
                continue
        assert np.array_equal(e_out[band_off[k]:band_off[k + 1]], E), tag
        assert gb.ci == b.ci and (b.ci >= 1) == bool(climb), (tag, gb.ci, b.ci)
        if climb and kind in ("peak_first", "flat_top"):
            assert b.ci == 1, tag
        if climb and kind == "peak_last":
            assert b.ci == M - 2, tag
        assert np.abs(gb.G[1:-1] - b.G[1:-1]).max() <= tol(b.G), tag
        assert abs(gb.neb_fmax - b.neb_fmax) <= np.sqrt(3.0) * tol(b.G), tag       # a row norm of G: three components within tol each
        if b.fixed is not None:
            assert np.all(gb.G[b.fixed] == 0.0), tag
        if b.status != 0:
            continue
        assert (gb.nsteps, gb.steps) == (b.nsteps, b.steps), tag
        assert abs(gb.dt - b.dt) <= 1e-15 and abs(gb.a - b.a) <= 1e-15, tag
        assert np.abs(gb.R - b.R).max() <= tol(b.R) and np.abs(gb.v - b.v).max() <= tol(b.v), tag
        assert np.array_equal(gb.R[[0, -1]], R0[[0, -1]]), tag                      # the end points never move
        if b.fixed is not None:
            assert np.array_equal(gb.R[b.fixed], R0[b.fixed]) and np.all(gb.v[b.fixed[1:-1]] == 0.0), tag
        fn = frac_next[next_off[k]:next_off[k + 1]].reshape(M - 2, n, 3)
        assert np.abs(fn - b.frac()[1:-1]).max() <= tol(b.frac()), tag
        # the situation the case was built for is the one the restatement took
        moved = np.sqrt(((b.R - R0) ** 2).sum())
        if kind == "clamp":
            assert moved == pytest.approx(FIRE["maxstep"], rel=1e-12) and np.sqrt(((gb.R - R0) ** 2).sum()) == pytest.approx(FIRE["maxstep"], rel=1e-12), tag
        else:
            assert moved < 0.9 * FIRE["maxstep"], tag
        if first:
            assert kind == "first" and b.nsteps == 0, tag
        elif kind == "downhill":
            assert gv < 0 and b.nsteps == 0 and b.dt == optimizer0[0] * FIRE["fdec"] and b.a == FIRE["astart"], tag
        else:
            assert gv > 0 and b.nsteps == optimizer0[2] + 1, tag
            assert (b.dt > optimizer0[0]) == (kind == "uphill_old"), tag
        seen.add(kind)
    assert seen == set(PATTERNS + SITUATIONS) - set(WANT_STATUS)

    # the same input once more: the same bits
    again, e2, frac2, _ = _launch(hip_engine, state, e_img, energy, force, all_images, climb, fixed)
    assert all(np.array_equal(a, c) for a, c in zip(again, out))
    assert np.array_equal(e2, e_out) and np.array_equal(frac2, frac_next)

    # not the final try: a band with a non-finite image is held back untouched (still running, flag set); the others step as before
    held, e3, frac3, retry = _launch(hip_engine, state, e_img, energy, force, all_images, climb, fixed, final_try=0)
    for k, (n, M, kind) in enumerate(cases):
        nonfinite, sl = kind in ("nonfinite_f", "nonfinite_e"), _rows(state, k)
        assert retry[k] == nonfinite, (kind, n, M)
        want, want_e = (inp, e_img) if nonfinite else (out, e_out)
        assert all(np.array_equal(a[sl], c[sl]) for a, c in zip(held[:3], want[:3])), (kind, n, M)
        assert np.array_equal(held[3][k], want[3][k]) and np.array_equal(held[4][k], want[4][k]), (kind, n, M)
        assert np.array_equal(e3[band_off[k]:band_off[k + 1]], want_e[band_off[k]:band_off[k + 1]]), (kind, n, M)
        if not nonfinite:
            assert np.array_equal(frac3[next_off[k]:next_off[k + 1]], frac_next[next_off[k]:next_off[k + 1]]), (kind, n, M)


def test_create_refuses_bad_bands(hip_engine):
    from chgnet_amd.graph.structure import Lattice, Structure

    eng = hip_engine
    lat = Lattice(np.eye(3) * 5.0)
    s = Structure(lat, [3, 8], [[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]])

    def create(structs, band_off):
        prep = eng.prepare_structures(structs)
        host, h = prep.host(), ctypes.c_void_p()
        off = np.asarray(band_off, np.int32)
        rc = eng.lib.chg_neb_create(eng.handle, ctypes.byref(host), off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(off) - 1,
                                    ctypes.byref(_params()), ctypes.byref(h))
        if rc == 0:
            eng.lib.chg_neb_free(eng.handle, h)
        return rc, eng.lib.chg_last_error(eng.handle).decode()

    assert create([s] * 3, [0, 3])[0] == 0
    for structs, off, word in (([s] * 2, [0, 2], "images"), ([s] * 67, [0, 67], "images"), ([s] * 5, [0, 3, 5], "images"),
                               ([s, Structure(lat, [3], [[0.0, 0.0, 0.0]]), s], [0, 3], "atom count"),
                               ([s, Structure(lat, [8, 3], s.frac_coords), s], [0, 3], "species"),
                               ([s, s, Structure(Lattice(np.eye(3) * 5.5), [3, 8], s.frac_coords)], [0, 3], "cell")):
        rc, msg = create(structs, off)
        assert rc == -1 and word in msg, (off, msg)


# ---- 2. / 3. the driver, teacher-forced -----------------------------------------------------------------------------------------
# The engine's fp32 forces are not bit-reproducible run to run, so the restatement is fed the energies and forces the device
# downloaded for every evaluation; its next configuration must then be the device's.
def _download(eng, handle, nb, B, N):
    from chgnet_amd import _lib

    out = {"frac": np.empty((N, 3)), "energy": np.empty(B, np.float32), "force": np.empty((N, 3), np.float32), "neb_fmax": np.empty(nb),
           "climbing_image": np.empty(nb, np.int32), "n_steps": np.empty(nb, np.int32), "status": np.empty(nb, np.int32),
           "n_evaluated": np.empty(nb, np.int32)}
    eng._check(eng.lib.chg_neb_download(eng.handle, handle, ctypes.byref(_lib.fill_out(_lib.NebOutHost(), out))))
    return out


def _replay(model, bands_of_structs, fmax, max_steps, climb, evaluations):
    """Run the handle one evaluation at a time; returns the restatements, the active counts and the structures evaluated by every call.
    Every band that was running before an evaluation must sit where its restatement sits (1e-10 A), its end points bit for bit
    where they were given."""
    eng = model.engine
    structs = [s for band in bands_of_structs for s in band]
    prep = eng.prepare_structures(structs)
    host = prep.host()
    nb, B, N = len(bands_of_structs), len(structs), int(prep.atom_off[-1])
    band_off = np.concatenate([[0], np.cumsum([len(b) for b in bands_of_structs])]).astype(np.int32)
    ref = [Band(np.array([s.frac_coords @ s.lattice.matrix for s in band]), band[0].lattice.matrix, k=SPRING, climb=climb, fmax=fmax, steps=max_steps)
           for band in bands_of_structs]
    h = ctypes.c_void_p()
    p = _params(fmax, max_steps, climb)
    eng._check(eng.lib.chg_neb_create(eng.handle, ctypes.byref(host), band_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), nb, ctypes.byref(p),
                                      ctypes.byref(h)))
    counts, evaluated, total = [], [], 0
    try:
        n_active = ctypes.c_int32()
        for it in range(evaluations):
            running = [r.status == 0 for r in ref]
            eng._check(eng.lib.chg_neb_run(eng.handle, h, 1, ctypes.byref(n_active)))
            counts.append(n_active.value)
            d = _download(eng, h, nb, B, N)
            evaluated.append(int(d["n_evaluated"].sum()) - total)
            total = int(d["n_evaluated"].sum())
            for k, r in enumerate(ref):
                i0, i1 = band_off[k], band_off[k + 1]
                sl = slice(prep.atom_off[i0], prep.atom_off[i1])
                frac = d["frac"][sl].reshape(r.M, r.n, 3)
                assert np.array_equal(frac[[0, -1]], prep.frac[sl].reshape(r.M, r.n, 3)[[0, -1]]), (it, k)
                if not running[k]:
                    continue
                assert np.abs(frac @ r.L - r.R).max() < 1e-10, (it, k)
                E, F = d["energy"][i0:i1], d["force"][sl].astype(np.float64).reshape(r.M, r.n, 3)
                r.advance(E, F)
                assert (d["n_steps"][k], d["status"][k], d["climbing_image"][k]) == (r.steps, r.status, r.ci), (it, k)
                assert abs(d["neb_fmax"][k] - r.neb_fmax) <= 1e-9 * (1 + r.neb_fmax), (it, k)
            assert n_active.value == sum(r.status == 0 for r in ref), it
            if n_active.value == 0:
                break
    finally:
        eng.lib.chg_neb_free(eng.handle, h)
    return ref, counts, evaluated


@pytest.mark.parametrize("climb", [False, True])
def test_driver_teacher_forced(model, climb):
    bands = [[_structure("limno2", rattle=0.08, seed=30 + i) for i in range(5)], [_structure("li9co7o16", rattle=0.08, seed=40 + i) for i in range(4)]]
    ref, counts, evaluated = _replay(model, bands, fmax=1e-6, max_steps=500, climb=climb, evaluations=12)
    assert counts == [2] * 12
    assert evaluated == [9] + [5] * 11          # every image once, then the interior ones
    for r in ref:
        assert r.steps == 12 and r.status == 0 and (r.ci >= 1) == climb


def test_compaction_drops_a_converged_band(model):
    from chgnet_amd.graph.structure import Lattice, Structure

    lone = Structure(Lattice(np.eye(3) * 4.0), [3], [[0.0, 0.0, 0.0]])      # no force on it and no distance between the images: G = 0
    bands = [[lone] * 3, [_structure("limno2", rattle=0.08, seed=50 + i) for i in range(4)]]
    ref, counts, evaluated = _replay(model, bands, fmax=0.01, max_steps=500, climb=False, evaluations=6)
    assert counts == [1] * 6
    assert evaluated == [7] + [2] * 5
    assert (ref[0].status, ref[0].steps) == (1, 0)
    assert (ref[1].status, ref[1].steps) == (0, 6)


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
# The scenario is a Li vacancy hop in a 3x2x2 LiMnO2 supercell (95 atoms), built so that it is well-posed:
#   * three cells along the hop direction (a): with two, the Li that hops is the vacancy's neighbour on BOTH sides through the periodic
#     boundary and the minimum image of its displacement is decided by rounding;
#   * the ideal lattice with one Li removed is a symmetric stationary point that a relaxation leaves in a direction decided by rounding,
#     so the atoms are displaced by a seeded 0.01 A first;
#   * the final end is the relaxed initial end translated by the hop vector and renumbered (the hop maps the crystal with its vacancy
#     onto itself), so both ends are the SAME minimum: relax_batch leaves both where they are and their energies agree;
#   * the weights are the random-initialisation golden set (the set of smoke() and of the kernel parity tests): its surface is smooth
#     and weak, the straight path crosses a barrier of about 0.1 eV.  The trained-like set is no potential for this: the straight path
#     squeezes the Li between two O at 1.5 A through a wall of 6-17 eV, and a climbing image, whose force along the tangent is
#     inverted, is driven up that wall instead of towards a saddle.
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
    h = d[hop]                               # site of the hopping Li - site of the vacancy: a lattice vector of the primitive cell
    opt = StructOptimizer(model=model)
    start = sites + 0.01 * np.random.default_rng(7).normal(size=sites.shape) @ np.linalg.inv(lat)
    a = opt.relax_batch([Structure(Lattice(lat), z1, start)], fmax=0.02, steps=500, relax_cell=False)[0]["final_structure"]
    # the initial end translated by h: the atom that sat on site s - h now sits on site s; the vacancy moves onto the hopping Li's site
    # and the Li that lands on the old vacancy is the one the hopping Li's index takes (left unwrapped)
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


def _neb_fmax_of(model, images, climb, fixed=None):
    pred = model.predict_structure(list(images), task="ef")
    R = np.array([s.frac_coords @ s.lattice.matrix for s in images])
    E = np.array([p["e"] for p in pred], np.float32)
    F = np.array([p["f"] for p in pred], np.float64)
    return neb_fmax(neb_forces(R, E, F, SPRING, climb, fixed)[0]), E


@pytest.fixture(scope="module")
def hop(smooth_model):
    """(relaxed end points, index of the hopping Li, 5 interpolated images) of the vacancy hop, shared by the tests below."""
    from chgnet_amd import NudgedElasticBand

    (a, b), out, i = _vacancy_hop(smooth_model)
    assert all(r["converged"] for r in out) and abs(out[0]["energy"] - out[1]["energy"]) <= 1e-3      # one minimum, twice
    return a, b, i, NudgedElasticBand.interpolate(a, b, 5)


def _check_result(model, images, res, climb):
    """What holds for every result: end points, barrier, reaction coordinate, the reported neb_fmax against the restatement."""
    a = images[0]
    assert len(res["images"]) == 5 and res["status"] in ("CONVERGED", "MAX_STEPS") and res["converged"] == (res["status"] == "CONVERGED")
    for got, want in ((res["images"][0], images[0]), (res["images"][-1], images[-1])):
        assert np.array_equal(got.frac_coords, want.frac_coords) and np.array_equal(got.lattice.matrix, want.lattice.matrix)
    assert res["barrier"] == res["energies"].max() - res["energies"][0] >= 0
    assert res["reverse_barrier"] == res["energies"].max() - res["energies"][-1] >= 0
    assert res["reaction_coordinate"][0] == 0 and np.all(np.diff(res["reaction_coordinate"]) > 0)
    assert res["climbing_image"] == (1 + int(np.argmax(res["energies"][1:-1])) if climb else None)
    start, _ = _neb_fmax_of(model, images, climb)
    again, E = _neb_fmax_of(model, res["images"], climb)
    print(f"climb {climb}: {res['status']} after {res['n_steps']} steps: neb_fmax {res['neb_fmax']:.6f} reported, {again:.6f} recomputed, "
          f"{start:.6f} at the start; barrier {res['barrier']:.6f} eV")
    assert abs(again - res["neb_fmax"]) <= 1e-3
    assert np.allclose(E * (len(a) if model.is_intensive else 1), res["energies"], atol=1e-3)
    return start, again


def test_climbing_band_end_to_end(smooth_model, hop):
    """``interpolate`` to 5 images, then ``run(fmax=0.05, steps=200, climb=True)``: the end points are unchanged, the barrier is
    max(E) - E[0], the reported neb_fmax is the restatement's on the returned images, below fmax when converged and in any case
    below its value at step 0."""
    from chgnet_amd import NudgedElasticBand

    a, b, _, images = hop
    neb = NudgedElasticBand(images, model=smooth_model)
    res = neb.run(fmax=0.05, steps=200, climb=True)
    assert neb.images is res["images"]
    start, again = _check_result(smooth_model, images, res, True)
    if res["converged"]:
        assert again < 0.05 + 1e-3
    assert again < start


def test_plain_band_end_to_end(smooth_model, hop):
    """The same band without climbing, the first stage of a two-stage search, and the second stage from its images.  A band that is
    below fmax where it starts stops there, so the force does not have to fall."""
    from chgnet_amd import NudgedElasticBand

    a, b, _, images = hop
    neb = NudgedElasticBand(images, model=smooth_model)
    res = neb.run(fmax=0.05, steps=200)
    start, again = _check_result(smooth_model, images, res, False)
    assert again <= start + 1e-3
    if res["converged"]:
        assert again < 0.05 + 1e-3
    second = neb.run(fmax=0.05, steps=200, climb=True)
    _check_result(smooth_model, res["images"], second, True)


def test_max_steps_fixed_atoms_and_run_batch(smooth_model, hop, capsys):
    from chgnet_amd import NudgedElasticBand

    model = smooth_model
    a, b, moving, images = hop
    short = NudgedElasticBand(images, model=model).run(fmax=1e-6, steps=3)
    assert short["status"] == "MAX_STEPS" and short["n_steps"] == 3 and short["climbing_image"] is None and not short["converged"]
    assert "trajectory" not in short
    capsys.readouterr()
    logged = NudgedElasticBand(images, model=model).run(fmax=1e-6, steps=3, verbose=True, loginterval=2, trajectory=True)
    printed = capsys.readouterr().out
    assert printed.count("NEB[0]:") == 2 == len(logged["trajectory"])       # evaluations 0 and 2 of 0..3

    held = sorted({0, 5, moving})
    fixed = NudgedElasticBand(images, model=model, fixed_atoms=held).run(fmax=1e-6, steps=5, climb=True)
    assert fixed["n_steps"] == 5
    for got, want in zip(fixed["images"], images):
        assert np.abs((got.frac_coords[held] - want.frac_coords[held]) @ a.lattice.matrix).max() < 1e-12
        assert got.site_properties["selective_dynamics"][moving] == [False, False, False]
    free = np.setdiff1d(np.arange(len(a)), held)
    assert max(np.abs((got.frac_coords[free] - want.frac_coords[free]) @ a.lattice.matrix).max()
               for got, want in zip(fixed["images"][1:-1], images[1:-1])) > 1e-4      # A: the free atoms did move

    two = NudgedElasticBand.run_batch([NudgedElasticBand(images, model=model), NudgedElasticBand(NudgedElasticBand.interpolate(a, b, 4), model=model)],
                                      fmax=1e-6, steps=3, climb=True)
    assert [len(r["images"]) for r in two] == [5, 4] and all(r["status"] == "MAX_STEPS" and r["n_steps"] == 3 for r in two)
    assert two[0]["n_evaluated"] == 5 + 3 * 3 and two[1]["n_evaluated"] == 4 + 2 * 3
