"""Fixed atoms on the MI355X: the three *_fixed single-launch entry points against the float64 restatement (tests/constraint_ref.py)
with the bounds of the unconstrained step tests, bit identity of a null mask, an all-zero mask and the entry points they extend,
StructOptimizer and MolecularDynamics on a rattled LiMnO2 cell with a third of the atoms held against the restatement's host loops,
mixed batches, and the refusals of the C entry points."""

from __future__ import annotations

import copy
import ctypes
import zlib

import numpy as np
import pytest

import constraint_ref as cref
import lbfgs_ref
import md_ref
import relax_ref
from conftest import load_case
from relax_ref import FIRE, GPA

pytestmark = pytest.mark.gpu

ABSORB, KICK2, START = 1, 2, 4
SW = 1.0 / 160.21766208
NHC_STATE = 20
SIZES = [1, 2, 5, 17, 300]                 # 300: rows beyond one pass of the 256-thread workgroup; 1 and 2: the smallest
MASK_KINDS = ("free", "held_all", "atoms", "components")


def _mask(kind, n, rng, keep_free=False):
    """Mask [n, 3] bool of one structure.  "atoms": whole atoms, among them 0, 255, 256 and 299 of the 300-atom structure (the
    seams of the row loop); keep_free: at least one atom stays free (a thermostat needs something to act on)."""
    m = np.zeros((n, 3), bool)
    if kind == "held_all":
        m[:] = True
    elif kind == "atoms":
        rows = {1: [0], 2: [1], 5: [0, 3], 17: [0, 5, 16], 300: [0, 255, 256, 299, 7, 64, 128, 191]}.get(n, list(range(0, n, 3)))
        if keep_free and len(rows) == n:
            rows = []
        m[rows] = True
    elif kind == "components":
        m = rng.random((n, 3)) < 0.35
        if n == 300:
            m[[0, 255, 256, 299], :] = [[True, False, False], [False, True, True], [True, True, True], [False, False, True]]
        if keep_free and m.all():
            m[0, 0] = False
    return m


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def _ptr(a, t=ctypes.c_double):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def _u8(mask):
    return None if mask is None else np.ascontiguousarray(mask, np.uint8)


@pytest.fixture(scope="module")
def model(trained_like_weights):
    from chgnet_amd import CHGNet

    return CHGNet(state_dict=trained_like_weights)


@pytest.fixture(scope="module")
def calc(model):
    from chgnet_amd.calculator import CHGNetCalculator

    return CHGNetCalculator(model=model)


# ---- 1. FIRE: one launch against the restatement -----------------------------------------------------------------------------------
def _relax_params(relax_cell=1, fmax=0.1, max_steps=500):
    from chgnet_amd import _lib

    return _lib.RelaxParams(fmax=fmax, max_steps=max_steps, relax_cell=relax_cell, dt=FIRE["dt"], maxstep=FIRE["maxstep"], dtmax=FIRE["dtmax"],
                            finc=FIRE["finc"], fdec=FIRE["fdec"], astart=FIRE["astart"], fa=FIRE["fa"], nmin=FIRE["nmin"], exp_cell_factor=0.0,
                            r_atom=6.0, r_bond=3.0, numerical_tol=1e-8, stress_weight=GPA)


# a per-component mask has no meaning while the cell moves: refused (test_c_entry_points_refuse), so it runs at fixed cell only
RELAX_MASKS = [(cell, kind) for cell in (1, 0) for kind in MASK_KINDS if not (cell and kind == "components")]
FIRE_CASES = list(zip(SIZES + [8, 3], ["first", "downhill", "uphill", "clamp", "downhill", "held_only", "nan_on_held"]))


def _fire_inputs(relax_cell, kind, max_steps=50):
    rng = np.random.default_rng(_seed("fire", relax_cell, kind))
    rel, forces, stresses, masks = [], [], [], []
    for n, what in FIRE_CASES:
        mask = _mask(kind, n, rng)
        if what in ("held_only", "nan_on_held") and kind != "free":
            mask = np.zeros((n, 3), bool)
            mask[: n // 2 + 1] = True                                    # whole atoms: valid with and without the cell
        L0 = np.diag(rng.uniform(4, 9, 3)) + rng.normal(0, 0.6, (3, 3))
        r = cref.FixedRelaxation(rng.random((n, 3)), L0, mask, relax_cell=bool(relax_cell), fmax=0.1, steps=max_steps)
        if relax_cell:
            r.q[n:] = r.c * rng.normal(0, 0.25, (3, 3))
        r.q[:n] += rng.normal(0, 0.3, (n, 3))
        r.steps, r.nsteps = int(rng.integers(1, 30)), int(rng.integers(0, 12))
        r.dt, r.a = rng.uniform(0.05, 0.5), rng.uniform(0.02, 0.1)
        f = rng.normal(0, 0.6, (n, 3)).astype(np.float32)
        s = rng.normal(0, 2.0, (3, 3))
        s = ((s + s.T) / 2).astype(np.float32)
        if what == "clamp":
            f *= 40
        if what == "first":
            r.steps, r.nsteps = 0, 0
        if what == "held_only":                                          # the only forces above fmax sit on held atoms
            f = np.where(mask, f * 20, f * 1e-3).astype(np.float32)
            s = (s * 1e-4).astype(np.float32)
        if what == "nan_on_held":
            f[0, 1] = np.nan                                             # the finiteness test sees the raw forces
        rows = n + 3 if relax_cell else n
        g = r.generalized_forces(np.nan_to_num(f.astype(np.float64)), s.astype(np.float64) * GPA)
        r.v[:rows] = (-1.0 if what == "uphill" else 1.0) * g * rng.uniform(0.2, 2.0) + rng.normal(0, 0.01, (rows, 3))
        r.v[:n] = cref.project(r.v[:n], mask)                            # a held component never had a velocity
        rel.append(r)
        forces.append(f)
        stresses.append(s)
        masks.append(mask)
    atom_off = np.concatenate([[0], np.cumsum([n for n, _ in FIRE_CASES])]).astype(np.int32)
    B = len(FIRE_CASES)
    data = dict(atom_off=atom_off, energy=rng.normal(-5, 1, B).astype(np.float32), force=np.ascontiguousarray(np.concatenate(forces), np.float32),
                stress=np.ascontiguousarray(np.stack(stresses), np.float32), magmom=rng.random(atom_off[-1]).astype(np.float32),
                fixed=_u8(np.concatenate(masks)))
    return rel, forces, stresses, masks, data


def _fire_launch(eng, relax_cell, state, d, fixed, entry="fixed", max_steps=50, handed=None):
    """handed: a list that receives the arrays handed to the entry point (in place), for a look at them after a refused call."""
    q, v, sd, si = (a.copy() for a in state)
    N, B = int(d["atom_off"][-1]), len(d["atom_off"]) - 1
    frac_next, lat_next = np.zeros((N, 3)), np.zeros((B, 3, 3))
    if handed is not None:
        handed.extend([q, v, sd, si, frac_next, lat_next])
    p = _relax_params(relax_cell, 0.1, max_steps)
    args = [eng.handle, ctypes.byref(p), B, _ptr(d["atom_off"], ctypes.c_int32), _ptr(q), _ptr(v), _ptr(sd), _ptr(si, ctypes.c_int32),
            _ptr(d["energy"], ctypes.c_float), _ptr(d["force"], ctypes.c_float), _ptr(d["stress"], ctypes.c_float),
            _ptr(d["magmom"], ctypes.c_float), _ptr(frac_next), _ptr(lat_next)]
    if entry == "fixed":
        eng._check(eng.lib.chg_test_relax_step_fixed(*args, _ptr(fixed, ctypes.c_uint8)))
    else:
        eng._check(eng.lib.chg_test_relax_step(*args))
    return (q, v, sd, si), frac_next, lat_next


@pytest.mark.parametrize(("relax_cell", "kind"), RELAX_MASKS)
def test_fire_step_matches_restatement(hip_engine, relax_cell, kind):
    rel, forces, stresses, masks, d = _fire_inputs(relax_cell, kind)
    atom_off = d["atom_off"]
    state = relax_ref.pack_state(rel, atom_off)
    (q, v, sd, si), frac_next, lat_next = _fire_launch(hip_engine, relax_cell, state, d, d["fixed"])
    got = [relax_ref.Relaxation.__new__(relax_ref.Relaxation) for _ in rel]
    for gr, r in zip(got, rel):
        gr.n = r.n
    relax_ref.unpack_state(got, atom_off, q, v, sd, si)
    tol = lambda ref: 2e-12 * (np.abs(ref).max() + 1.0)  # noqa: E731
    for o, (r, (n, what)) in enumerate(zip(rel, FIRE_CASES)):
        q0, v0 = r.q.copy(), r.v.copy()
        r.advance(forces[o].astype(np.float64), stresses[o].astype(np.float64) * GPA, True)
        gr, tag = got[o], (what, n, kind)
        assert r.status == gr.status and (r.steps, r.nsteps) == (gr.steps, gr.nsteps), (tag, r.status, gr.status)
        if what == "nan_on_held":
            assert r.status == 3, tag
        if what == "held_only" and kind != "free":
            assert r.status == 1, tag                                     # CONVERGED: only the masked forces are tested
        if kind == "held_all" and not relax_cell:
            assert r.status in (1, 3), tag
        assert np.abs(gr.q - r.q).max() <= tol(r.q) and np.abs(gr.v - r.v).max() <= tol(r.v), tag
        assert abs(gr.dt - r.dt) <= 1e-15 * r.dt and abs(gr.a - r.a) <= 1e-15 * r.a, tag
        assert np.array_equal(gr.q[:n][masks[o]], q0[:n][masks[o]]) and not gr.v[:n][masks[o]].any(), tag      # held: exactly where they were
        if r.status != 0:
            assert np.array_equal(gr.q, q0) and np.array_equal(gr.v, v0), tag
            continue
        sl = slice(atom_off[o], atom_off[o + 1])
        assert np.abs(frac_next[sl] - r.frac()).max() <= 2e-12 * (np.abs(r.frac()).max() + 1), tag
        assert np.abs(lat_next[o] - r.lattice()).max() <= 2e-12 * np.abs(r.lattice()).max(), tag
        if what == "clamp":
            assert np.sqrt(((r.q - q0) ** 2).sum()) == pytest.approx(FIRE["maxstep"], rel=1e-12)


@pytest.mark.parametrize("relax_cell", [1, 0])
def test_fire_null_mask_zero_mask_and_plain_entry_point_agree_bitwise(hip_engine, relax_cell):
    rel, _, _, _, d = _fire_inputs(relax_cell, "free")
    state = relax_ref.pack_state(rel, d["atom_off"])
    plain = _fire_launch(hip_engine, relax_cell, state, d, None, entry="plain")
    null = _fire_launch(hip_engine, relax_cell, state, d, None)
    zero = _fire_launch(hip_engine, relax_cell, state, d, np.zeros_like(d["fixed"]))
    for other in (null, zero):
        assert all(np.array_equal(a, b) for a, b in zip(plain[0], other[0]))
        assert np.array_equal(plain[1], other[1]) and np.array_equal(plain[2], other[2])
    assert not np.array_equal(plain[0][0], state[0])                       # and something did step


# ---- 2. L-BFGS: one launch against the restatement --------------------------------------------------------------------------------------
LBFGS_FMAX, LBFGS_MAX_STEPS, MEMORY = 1e-3, 50, 4
LBFGS_CASES = list(zip(SIZES + [8, 3], ["first", "partial", "wrapped", "partial", "wrapped", "held_only", "nan_on_held"]))
HISTORY = {"first": 0, "partial": 3, "wrapped": 9, "held_only": 3, "nan_on_held": 3}


def _lbfgs_params():
    from chgnet_amd import _lib

    p = lbfgs_ref.LBFGS
    return _lib.LbfgsParams(maxstep=p["maxstep"], damping=p["damping"], alpha=p["alpha"], memory=MEMORY)


def _lbfgs_inputs(relax_cell, kind):
    """States after some restatement steps on smooth synthetic forces f = -K (q - q*), as tests/test_gpu_lbfgs.py builds them.  A
    structure that converges on the way (everything held, no cell) is handed over stopped: both sides must leave it alone."""
    rng = np.random.default_rng(_seed("lbfgs", relax_cell, kind))
    rel, forces, stresses, masks = [], [], [], []
    for n, what in LBFGS_CASES:
        mask = _mask(kind, n, rng)
        if what in ("held_only", "nan_on_held") and kind != "free":
            mask = np.zeros((n, 3), bool)
            mask[: n // 2 + 1] = True
        L0 = np.diag(rng.uniform(4, 9, 3)) + rng.normal(0, 0.6, (3, 3))
        r = cref.FixedLbfgsRelaxation(rng.random((n, 3)), L0, mask, relax_cell=bool(relax_cell), fmax=LBFGS_FMAX, steps=LBFGS_MAX_STEPS,
                                      p={**lbfgs_ref.LBFGS, "memory": MEMORY})
        if relax_cell:
            r.q[n:] = r.c * rng.normal(0, 0.1, (3, 3))
        K = rng.uniform(2.0, 30.0, (n, 3))
        target = r.q[:n] + rng.normal(0, 0.15, (n, 3))
        s0 = rng.normal(0, 2.0, (3, 3))
        s0 = (s0 + s0.T) / 2

        def results():
            A = r.q[n:] / r.c
            return (-K * (r.q[:n] - target)).astype(np.float32), (s0 - 40.0 * (A + A.T)).astype(np.float32)

        f, s = results()
        for _ in range(HISTORY[what]):
            if r.advance(f.astype(np.float64), s.astype(np.float64) * GPA) != 0:
                break
            target = target + rng.normal(0, 0.04, (n, 3))
            f, s = results()
        if what == "held_only":
            f = np.where(mask, f * 50 + 1, f * 1e-6).astype(np.float32)
            s = (s * 1e-7).astype(np.float32)
        if what == "nan_on_held":
            f[0, 1] = np.nan
        rel.append(r)
        forces.append(f)
        stresses.append(s)
        masks.append(mask)
    atom_off = np.concatenate([[0], np.cumsum([n for n, _ in LBFGS_CASES])]).astype(np.int32)
    B = len(LBFGS_CASES)
    data = dict(atom_off=atom_off, energy=rng.normal(-5, 1, B).astype(np.float32), force=np.ascontiguousarray(np.concatenate(forces), np.float32),
                stress=np.ascontiguousarray(np.stack(stresses), np.float32), magmom=rng.random(atom_off[-1]).astype(np.float32),
                fixed=_u8(np.concatenate(masks)))
    return rel, forces, stresses, masks, data


def _lbfgs_launch(eng, relax_cell, state, d, fixed, entry="fixed", handed=None):
    q, r0, g0, S, Y, rho, sd, si = (a.copy() for a in state)
    N, B = int(d["atom_off"][-1]), len(d["atom_off"]) - 1
    frac_next, lat_next, retry = np.zeros((N, 3)), np.zeros((B, 3, 3)), np.zeros(B, np.int32)
    if handed is not None:
        handed.extend([q, r0, g0, S, Y, rho, sd, si, frac_next, lat_next])
    p, lp = _relax_params(relax_cell, LBFGS_FMAX, LBFGS_MAX_STEPS), _lbfgs_params()
    i32, f32 = ctypes.c_int32, ctypes.c_float
    args = [eng.handle, ctypes.byref(p), ctypes.byref(lp), B, _ptr(d["atom_off"], i32), _ptr(q), _ptr(r0), _ptr(g0), _ptr(S), _ptr(Y), _ptr(rho),
            _ptr(sd), _ptr(si, i32), _ptr(d["energy"], f32), _ptr(d["force"], f32), _ptr(d["stress"], f32), _ptr(d["magmom"], f32), 1,
            _ptr(frac_next), _ptr(lat_next), _ptr(retry, i32)]
    if entry == "fixed":
        eng._check(eng.lib.chg_test_lbfgs_step_fixed(*args, _ptr(fixed, ctypes.c_uint8)))
    else:
        eng._check(eng.lib.chg_test_lbfgs_step(*args))
    return (q, r0, g0, S, Y, rho, sd, si), frac_next, lat_next


@pytest.mark.parametrize(("relax_cell", "kind"), RELAX_MASKS)
def test_lbfgs_step_matches_restatement(hip_engine, relax_cell, kind):
    rel, forces, stresses, masks, d = _lbfgs_inputs(relax_cell, kind)
    atom_off = d["atom_off"]
    slots = lbfgs_ref.ring_slots(MEMORY, LBFGS_MAX_STEPS)
    state = lbfgs_ref.pack_state(rel, atom_off, slots)
    out, frac_next, lat_next = _lbfgs_launch(hip_engine, relax_cell, state, d, d["fixed"])
    got = [lbfgs_ref.LbfgsRelaxation.__new__(lbfgs_ref.LbfgsRelaxation) for _ in rel]
    for gr, r in zip(got, rel):
        gr.n, gr.relax_cell = r.n, r.relax_cell
    lbfgs_ref.unpack_state(got, atom_off, slots, *out)
    tol = lambda ref: 2e-12 * (np.abs(ref).max() + 1.0)  # noqa: E731
    stepped = 0
    for o, (r, (n, what)) in enumerate(zip(rel, LBFGS_CASES)):
        tag = (what, n, kind)
        q0, was = r.q.copy(), r.status
        r.advance(forces[o].astype(np.float64), stresses[o].astype(np.float64) * GPA, True)
        gr = got[o]
        assert r.status == gr.status and (r.steps, r.appended) == (gr.steps, gr.appended), (tag, r.status, gr.status)
        if was == 0 and what == "nan_on_held":
            assert r.status == 3, tag
        if was == 0 and what == "held_only" and kind != "free":
            assert r.status == 1, tag
        a, b = atom_off[o] + 3 * o, atom_off[o + 1] + 3 * (o + 1)
        if r.status != 0:                       # stopped: bit-identical to the input, history included
            for x, y in zip(out[:5], state[:5]):
                assert np.array_equal(x[..., a:b, :], y[..., a:b, :]), tag
            continue
        stepped += 1
        for name in ("q", "r0", "g0"):
            ref = getattr(r, name)
            assert np.abs(getattr(gr, name) - ref).max() <= tol(ref), (tag, name)
        assert len(gr.rho) == len(r.rho) == min(r.appended, slots), tag
        for i in range(len(r.rho)):
            assert np.abs(gr.s[i] - r.s[i]).max() <= tol(r.s[i]) and np.abs(gr.y[i] - r.y[i]).max() <= tol(r.y[i]), (tag, i)
            assert abs(gr.rho[i] - r.rho[i]) <= 1e-10 * abs(r.rho[i]), (tag, i)
            hm = np.zeros((r.rows, 3), bool)
            hm[:n] = masks[o]
            assert not gr.s[i].reshape(-1, 3)[hm].any() and not gr.y[i].reshape(-1, 3)[hm].any(), tag      # the history of a held component is 0
        assert np.array_equal(gr.q[:n][masks[o]], q0[:n][masks[o]]), tag
        sl = slice(atom_off[o], atom_off[o + 1])
        assert np.abs(frac_next[sl] - r.frac()).max() <= tol(r.frac()), tag
        assert np.abs(lat_next[o] - r.lattice()).max() <= tol(r.lattice()), tag
    assert stepped >= (3 if kind != "held_all" or relax_cell else 0)


@pytest.mark.parametrize("relax_cell", [1, 0])
def test_lbfgs_null_mask_zero_mask_and_plain_entry_point_agree_bitwise(hip_engine, relax_cell):
    rel, _, _, _, d = _lbfgs_inputs(relax_cell, "free")
    state = lbfgs_ref.pack_state(rel, d["atom_off"], lbfgs_ref.ring_slots(MEMORY, LBFGS_MAX_STEPS))
    plain = _lbfgs_launch(hip_engine, relax_cell, state, d, None, entry="plain")
    null = _lbfgs_launch(hip_engine, relax_cell, state, d, None)
    zero = _lbfgs_launch(hip_engine, relax_cell, state, d, np.zeros_like(d["fixed"]))
    for other in (null, zero):
        assert all(np.array_equal(a, b) for a, b in zip(plain[0], other[0]))
        assert np.array_equal(plain[1], other[1]) and np.array_equal(plain[2], other[2])
    assert not np.array_equal(plain[0][0], state[0])


# ---- 3. molecular dynamics: one launch against the restatement, every ensemble code ------------------------------------------------------
NVE, NVT, NPT_INHOM, NPT_ISO, LANGEVIN, NVT_NHC, NPT_NHC = range(7)
REF_KIND = {NVE: md_ref.NVE, NVT: md_ref.NVT, NPT_INHOM: md_ref.NPT_INHOM, NPT_ISO: md_ref.NPT_ISO}
MOVING_CELL = (NPT_INHOM, NPT_ISO, NPT_NHC)
FLAGSETS = {"start_only": START, "finish_only": ABSORB | KICK2, "finish_start": ABSORB | KICK2 | START, "npt_mid": ABSORB}
DT, T0, KAPPA, PRESSURE, FRICTION, CHAIN = 2.0 * md_ref.FS, 300.0, 1.0 / (80.0 / 160.2176), 2.0 * md_ref.GPA, 0.01 / md_ref.FS, 3
MD_SEEDS = [7, (1 << 32) + 12345, 0, (1 << 64) - 1, 99]
MD_STEPS0 = [0, 70000, 3, 49, 11]


def _md_sizes(code):
    return [2, 2, 5, 17, 300] if code in (NVT_NHC, NPT_NHC) else SIZES      # the chains refuse a one-atom replica


def _md_params(code):
    from chgnet_amd import _lib

    nhc = code in (NVT_NHC, NPT_NHC)
    return _lib.MdParams(ensemble=code, fixcm=0 if nhc else 1, dt=DT, temperature=T0, taut=100 * DT, taup=50 * DT if nhc else 1000 * DT,
                         pressure=0.5 * md_ref.GPA if nhc else PRESSURE, compressibility=0.0 if nhc else KAPPA, kB=md_ref.KB, stress_weight=SW,
                         loginterval=1, ring_frames=1, log_stress=1, log_crystal_fea=0, r_atom=6.0, r_bond=3.0, numerical_tol=1e-8)


def _md_inputs(code, mode, kind):
    rng = np.random.default_rng(_seed("md", code, mode, kind))
    refs, cached, new_f, new_s, masks = [], [], [], [], []
    for o, n in enumerate(_md_sizes(code)):
        mask = _mask(kind, n, rng, keep_free=code != NVE)
        cell = np.diag(rng.uniform(5, 9, 3)) + rng.normal(0, 0.5, (3, 3))
        m = rng.uniform(1.0, 200.0, n)
        pos, mom = rng.random((n, 3)) @ cell, rng.normal(0, 0.3, (n, 3)) * np.sqrt(m)[:, None]
        if code in REF_KIND:
            ref = cref.FixedMDRef(pos, cell, m, mom, mask, ensemble=REF_KIND[code], dt=DT, temperature_k=T0, pressure=PRESSURE, compressibility=KAPPA)
            if o == 2:
                ref.p[:] = 0.0                                            # T = 0: lambda clamps to 1.1
            ref.phase = 1 if mode == "npt_mid" else 0
        elif code == LANGEVIN:
            ref = cref.FixedLangevinRef(pos, cell, m, mom, mask, dt=DT, temperature_k=T0, friction=FRICTION, seed=MD_SEEDS[o], fixcm=True)
        else:
            ref = cref.FixedNHCRef(pos, cell, m, mom, mask, npt=code == NPT_NHC, dt=DT, temperature_k=T0, taut=100 * DT, taup=50 * DT,
                                   pressure=0.5 * md_ref.GPA, chain_length=CHAIN)
            ref.v, ref.eta = rng.normal(0, 0.03, CHAIN), rng.normal(0, 0.5, CHAIN)
            if ref.npt:
                ref.vb, ref.xi, ref.veps = rng.normal(0, 0.05, CHAIN), rng.normal(0, 0.5, CHAIN), float(rng.normal(0, 0.02))
        ref.nsteps = MD_STEPS0[o]
        s = rng.normal(0, 0.02, (3, 3))
        ref.stress_cached = (s + s.T) / 2
        refs.append(ref)
        cached.append(cref.project(rng.normal(0, 0.5, (n, 3)), mask))       # the cache holds masked forces
        new_f.append(rng.normal(0, 0.5, (n, 3)).astype(np.float32))
        s2 = rng.normal(0, 3.0, (3, 3))
        new_s.append(((s2 + s2.T) / 2).astype(np.float32))
        masks.append(mask)
    return refs, cached, new_f, new_s, masks


def _md_pack(code, refs, cached, new_f, new_s, masks):
    B = len(refs)
    aoff = np.concatenate([[0], np.cumsum([len(x.m) for x in refs])]).astype(np.int32)
    st = dict(r=np.ascontiguousarray(np.concatenate([x.r for x in refs])), p=np.ascontiguousarray(np.concatenate([x.p for x in refs])),
              f=np.ascontiguousarray(np.concatenate(cached)), sd=np.zeros((B, 40)), si=np.zeros((B, 4), np.int32), nhc=np.zeros((B, NHC_STATE)))
    for o, x in enumerate(refs):
        st["sd"][o, :9], st["sd"][o, 9:18] = x.cell.ravel(), np.linalg.inv(x.cell).ravel()
        st["sd"][o, 18] = -50.0 - o
        st["sd"][o, 19], st["sd"][o, 20] = md_ref.kinetic_energy(x.p, x.m), cref.temperature(x.p, x.m, masks[o])
        st["sd"][o, 21:30] = x.stress_cached.ravel()
        st["sd"][o, 30:39] = np.einsum("ka,kb,k->ab", x.p, x.p, 1.0 / x.m).ravel()
        st["si"][o] = [x.nsteps, 0, getattr(x, "phase", 0), 0]
        if code in (NVT_NHC, NPT_NHC):
            M = CHAIN
            st["nhc"][o, 0:M], st["nhc"][o, 4:4 + M], st["nhc"][o, 8:8 + M], st["nhc"][o, 12:12 + M], st["nhc"][o, 16] = x.v, x.eta, x.vb, x.xi, x.veps
            st["nhc"][o, 17] = 123.0
    const = dict(aoff=aoff, m=np.ascontiguousarray(np.concatenate([x.m for x in refs])), energy=np.linspace(-120, -80, B).astype(np.float32),
                 force=np.ascontiguousarray(np.concatenate(new_f), np.float32), stress=np.ascontiguousarray(np.stack(new_s), np.float32),
                 seeds=np.array(MD_SEEDS[:B], np.uint64), fixed=_u8(np.concatenate(masks)))
    return st, const


def _md_launch(eng, code, flags, st, c, fixed, entry="fixed", handed=None):
    st = {k: v.copy() for k, v in st.items()}
    st["frac_next"], st["lat_next"] = np.zeros_like(st["r"]), np.zeros((len(c["aoff"]) - 1, 3, 3))
    if handed is not None:
        handed.append(st)
    prm = _md_params(code)
    i32, f32 = ctypes.c_int32, ctypes.c_float
    args = [eng.handle, ctypes.byref(prm), len(c["aoff"]) - 1, _ptr(c["aoff"], i32), flags, _ptr(st["r"]), _ptr(st["p"]), _ptr(st["f"]), _ptr(c["m"]),
            _ptr(st["sd"]), _ptr(st["si"], i32), _ptr(c["energy"], f32), _ptr(c["force"], f32), _ptr(c["stress"], f32), _ptr(st["frac_next"]),
            _ptr(st["lat_next"])]
    lan, nhc = code == LANGEVIN, code in (NVT_NHC, NPT_NHC)
    if entry == "fixed":
        eng._check(eng.lib.chg_test_md_step_fixed(*args, FRICTION if lan else 0.0, _ptr(c["seeds"], ctypes.c_uint64) if lan else None,
                                                  CHAIN if nhc else 0, _ptr(st["nhc"]) if nhc else None, _ptr(fixed, ctypes.c_uint8)))
    elif lan:
        eng._check(eng.lib.chg_test_md_step_langevin(*args, FRICTION, _ptr(c["seeds"], ctypes.c_uint64)))
    elif nhc:
        eng._check(eng.lib.chg_test_md_step_nhc(*args, CHAIN, _ptr(st["nhc"])))
    else:
        eng._check(eng.lib.chg_test_md_step(*args))
    return st


MD_CASES = [(code, mode) for code in range(7) for mode in ("start_only", "finish_only", "finish_start")]
MD_CASES += [(NPT_INHOM, "npt_mid"), (NPT_ISO, "npt_mid")]                   # phase 1 exists only for the Berendsen barostats
# everything held: NVE only (refused elsewhere); per-component masks: fixed cell only (refused under a moving cell)
MD_MASKED_CASES = [(code, mode, kind) for code, mode in MD_CASES for kind in MASK_KINDS
                   if not (kind == "held_all" and code != NVE) and not (kind == "components" and code in MOVING_CELL)]


def _md_expect(code, flags, ref, cached, new_f, new_s, mask):
    """Advance the restatement replica through what one launch does; returns what the launch must leave behind."""
    want = {"fcache": cached, "steps": ref.nsteps, "phase": getattr(ref, "phase", 0), "next": False, "done": None, "pscale": None}
    sigma = ref.stress_cached
    fnew = cref.project(new_f.astype(np.float64), mask)
    if code in REF_KIND:
        if flags & ABSORB:
            want["fcache"], sigma = fnew, new_s.astype(np.float64) * SW
            if ref.phase == 1:
                ref.first_half(fnew)
                want["next"], want["phase"] = True, 0
            else:
                ref.second_half(fnew)
                want["steps"] += 1
                want["done"] = copy.deepcopy(ref)
        if flags & START and not (flags & ABSORB and getattr(ref, "phase", 0) == 1):
            if code != NVE:
                ref.scale_velocities()
            if code in (NPT_INHOM, NPT_ISO):
                ref.scale_positions_and_cell(sigma)
                want["phase"] = 1
            else:
                ref.first_half(want["fcache"])
            want["next"] = True
    elif code == LANGEVIN:
        if flags & ABSORB:
            want["fcache"], sigma = fnew, new_s.astype(np.float64) * SW
            ref.second_half(fnew)
            want["steps"] += 1
            want["done"] = copy.deepcopy(ref)
        if flags & START:
            loose = copy.deepcopy(ref)           # the momenta before the centre-of-mass removal set the rounding scale of p
            loose.fixcm = False
            loose.first_half(want["fcache"])
            ref.first_half(want["fcache"])
            want["pscale"] = max(np.abs(loose.p).max(), np.abs(ref.p).max())
            want["next"] = True
    else:
        terms = [abs(ref.veps)]                  # the strain rate is a sum of terms of either sign: its rounding scale is the largest

        def kick_size(sig):
            vol = ref.volume()
            return 0.5 * ref.dt * max(ref.alpha * ref.k2(), abs(vol * np.trace(sig)), abs(3 * ref.pext * vol)) / ref.W

        if flags & ABSORB:
            want["fcache"], sigma = fnew, new_s.astype(np.float64) * SW
            terms.append(kick_size(sigma))
            ref.second_half(fnew, sigma)         # counts the step
            want["steps"] += 1
            want["done"] = copy.deepcopy(ref)
        if flags & START:
            terms.append(kick_size(sigma))
            ref.first_half(want["fcache"], sigma)
            want["next"] = True
        want["veps_scale"] = max(terms)
    want["sigma"] = sigma
    return want


@pytest.mark.parametrize(("code", "mode", "kind"), MD_MASKED_CASES)
def test_md_step_matches_restatement(hip_engine, code, mode, kind):
    flags = FLAGSETS[mode]
    refs, cached, new_f, new_s, masks = _md_inputs(code, mode, kind)
    st, c = _md_pack(code, refs, cached, new_f, new_s, masks)
    out = _md_launch(hip_engine, code, flags, st, c, c["fixed"])
    aoff = c["aoff"]
    worst = {}

    def close(got, want, what, scale=None):
        scale = (np.abs(want).max() if scale is None else scale) + 1e-300
        err = np.abs(got - want).max() / scale
        worst[what] = max(worst.get(what, 0.0), err)
        assert err <= 1e-12, (what, o, err)

    for o, ref0 in enumerate(refs):
        ref, mask = copy.deepcopy(ref0), masks[o]
        sl = slice(aoff[o], aoff[o + 1])
        w = _md_expect(code, flags, ref, cached[o], new_f[o], new_s[o], mask)
        close(out["r"][sl], ref.r, "r")
        close(out["p"][sl], ref.p, "p", w["pscale"])
        close(out["f"][sl], w["fcache"], "f")
        close(out["sd"][o, :9].reshape(3, 3), ref.cell, "cell")
        close(out["sd"][o, 9:18].reshape(3, 3), np.linalg.inv(ref.cell), "cell^-1")
        assert list(out["si"][o, :3]) == [w["steps"], 0, w["phase"]], (o, out["si"][o])
        assert not out["p"][sl][mask].any() and not out["f"][sl][mask].any(), o               # held: no momentum, no cached force
        if code not in MOVING_CELL:
            assert np.array_equal(out["r"][sl][mask], st["r"][sl][mask]), o                     # and no drift, to the bit
        else:
            held = mask.all(1)
            if held.any():                                                                      # held atoms scale with the cell
                close(out["r"][sl][held] @ out["sd"][o, 9:18].reshape(3, 3), st["r"][sl][held] @ st["sd"][o, 9:18].reshape(3, 3), "held frac", 1.0)
        if w["done"] is not None:
            done = w["done"]
            close(out["sd"][o, 18], float(c["energy"][o]), "epot")
            close(out["sd"][o, 19], md_ref.kinetic_energy(done.p, done.m), "ekin")
            close(out["sd"][o, 20], cref.temperature(done.p, done.m, mask), "T")
            close(out["sd"][o, 30:39].reshape(3, 3), np.einsum("ka,kb,k->ab", done.p, done.p, 1.0 / done.m), "sum p p / m")
        if flags & ABSORB:
            close(out["sd"][o, 21:30].reshape(3, 3), w["sigma"], "stress")
        if w["next"]:
            close(out["frac_next"][sl], ref.r @ np.linalg.inv(ref.cell), "frac_next")
            close(out["lat_next"][o], ref.cell, "lat_next")
        if code in (NVT_NHC, NPT_NHC):
            x, M = out["nhc"][o], CHAIN
            close(x[0:M], ref.v, "v")
            close(x[4:4 + M], ref.eta, "eta")
            if ref.npt:
                close(x[8:8 + M], ref.vb, "vb")
                close(x[12:12 + M], ref.xi, "xi")
                close(x[16], ref.veps, "veps", w["veps_scale"])
            if w["done"] is not None:
                h = w["done"].extended_energy()
                close(x[17], h, "H - Epot", max(abs(h), 0.5 * w["done"].k2(), abs(ref.nf * ref.kt * w["done"].eta[0])))
            else:
                assert x[17] == 123.0
    print(code, mode, kind, "worst relative errors", worst)


@pytest.mark.parametrize(("code", "mode"), MD_CASES)
def test_md_null_mask_zero_mask_and_plain_entry_point_agree_bitwise(hip_engine, code, mode):
    flags = FLAGSETS[mode]
    refs, cached, new_f, new_s, masks = _md_inputs(code, mode, "free")
    st, c = _md_pack(code, refs, cached, new_f, new_s, masks)
    st["sd"][:, 20] = [md_ref.temperature(x.p, x.m) for x in refs]
    plain = _md_launch(hip_engine, code, flags, st, c, None, entry="plain")
    null = _md_launch(hip_engine, code, flags, st, c, None)
    zero = _md_launch(hip_engine, code, flags, st, c, np.zeros_like(c["fixed"]))
    for other in (null, zero):
        for k in plain:
            assert np.array_equal(plain[k], other[k]), (k, code, mode)
    assert not np.array_equal(plain["p"], st["p"]) or not np.array_equal(plain["r"], st["r"])


# ---- 3b. one launch, constrained and unconstrained structures side by side ----------------------------------------------------------------
def _free_every_other(masks, fixed, atom_off):
    """Clear the mask of structures 1, 3, ...: returns their indices."""
    free = list(range(1, len(masks), 2))
    for o in free:
        fixed[atom_off[o]:atom_off[o + 1]] = 0
    return free


@pytest.mark.parametrize("optimizer", ["FIRE", "LBFGS"])
@pytest.mark.parametrize("relax_cell", [1, 0])
def test_unconstrained_members_of_a_mixed_launch_step_to_the_same_bits(hip_engine, optimizer, relax_cell):
    """What the end-to-end mixed batches cannot show through the engine's run-to-run noise: given the same evaluation, a structure
    without held components steps to exactly the bits of the entry point without a mask while its neighbours are constrained."""
    if optimizer == "FIRE":
        rel, _, _, masks, d = _fire_inputs(relax_cell, "atoms")
        state = relax_ref.pack_state(rel, d["atom_off"])
        launch = _fire_launch
    else:
        rel, _, _, masks, d = _lbfgs_inputs(relax_cell, "atoms")
        state = lbfgs_ref.pack_state(rel, d["atom_off"], lbfgs_ref.ring_slots(MEMORY, LBFGS_MAX_STEPS))
        launch = _lbfgs_launch
    atom_off, fixed = d["atom_off"], d["fixed"].copy()
    free = _free_every_other(masks, fixed, atom_off)
    mixed = launch(hip_engine, relax_cell, state, d, fixed)
    plain = launch(hip_engine, relax_cell, state, d, None, entry="plain")
    differs = 0
    for o in range(len(masks)):
        a, b, sl = atom_off[o] + 3 * o, atom_off[o + 1] + 3 * (o + 1), slice(atom_off[o], atom_off[o + 1])
        same = all(np.array_equal(x[..., a:b, :], y[..., a:b, :]) for x, y in zip(mixed[0], plain[0]) if x.ndim >= 2 and x.shape[-2] == state[0].shape[0])
        same = same and np.array_equal(mixed[0][-2][o], plain[0][-2][o]) and np.array_equal(mixed[0][-1][o], plain[0][-1][o])      # sd, si
        same = same and np.array_equal(mixed[1][sl], plain[1][sl]) and np.array_equal(mixed[2][o], plain[2][o])
        if optimizer == "LBFGS":
            same = same and np.array_equal(mixed[0][5][o], plain[0][5][o])                                                        # rho
        if o in free:
            assert same, o
        else:
            differs += not same
    assert differs >= 2                                                    # and the constrained ones did step differently


@pytest.mark.parametrize(("code", "mode"), MD_CASES)
def test_unconstrained_replicas_of_a_mixed_launch_step_to_the_same_bits(hip_engine, code, mode):
    flags = FLAGSETS[mode]
    refs, cached, new_f, new_s, masks = _md_inputs(code, mode, "atoms")
    st, c = _md_pack(code, refs, cached, new_f, new_s, masks)
    fixed = c["fixed"].copy()
    free = _free_every_other(masks, fixed, c["aoff"])
    for o in free:                                                         # their state as an unconstrained replica holds it: T over 3 n
        st["sd"][o, 20] = md_ref.temperature(refs[o].p, refs[o].m)
    mixed = _md_launch(hip_engine, code, flags, st, c, fixed)
    plain = _md_launch(hip_engine, code, flags, st, c, None, entry="plain")
    for o in free:
        sl = slice(c["aoff"][o], c["aoff"][o + 1])
        for k in ("r", "p", "f", "frac_next"):
            assert np.array_equal(mixed[k][sl], plain[k][sl]), (k, o)
        for k in ("sd", "si", "nhc", "lat_next"):
            assert np.array_equal(mixed[k][o], plain[k][o]), (k, o)
    if not (mode == "start_only" and code in (NVE, NPT_INHOM, NPT_ISO)):   # (masked p and cached f in, no fixcm yet: nothing to mask there)
        assert not np.array_equal(mixed["p"], plain["p"]) or not np.array_equal(mixed["f"], plain["f"])


# ---- 4. the refusals of the C entry points ------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse(hip_engine, model):
    eng = hip_engine
    # single launches: a per-component mask with a moving cell, nothing free outside NVE (no launch: the state comes back untouched)
    rel, _, _, _, d = _fire_inputs(1, "free")
    state = relax_ref.pack_state(rel, d["atom_off"])
    partial = np.zeros_like(d["fixed"])
    partial[5, 1] = 1
    handed = []
    with pytest.raises(Exception, match="only some components"):
        _fire_launch(eng, 1, state, d, partial, handed=handed)
    assert all(np.array_equal(a, b) for a, b in zip(handed[:4], state)) and not handed[4].any() and not handed[5].any()      # nothing ran
    rel, _, _, _, d2 = _lbfgs_inputs(1, "free")
    lstate, handed = lbfgs_ref.pack_state(rel, d2["atom_off"], lbfgs_ref.ring_slots(MEMORY, LBFGS_MAX_STEPS)), []
    with pytest.raises(Exception, match="only some components"):
        _lbfgs_launch(eng, 1, lstate, d2, partial, handed=handed)
    assert all(np.array_equal(a, b) for a, b in zip(handed[:8], lstate)) and not handed[8].any() and not handed[9].any()
    def untouched(handed, st):
        got = handed[0]
        return all(np.array_equal(got[k], st[k]) for k in st) and not got["frac_next"].any() and not got["lat_next"].any()

    for code in range(7):
        refs, cached, new_f, new_s, masks = _md_inputs(code, "start_only", "free")
        st, c = _md_pack(code, refs, cached, new_f, new_s, masks)
        frozen = np.zeros_like(c["fixed"])
        frozen[c["aoff"][1]:c["aoff"][2]] = 1                                # replica 1: nothing free
        if code == NVE:
            _md_launch(eng, code, START, st, c, frozen)
        else:
            handed = []
            with pytest.raises(Exception, match="no free component"):
                _md_launch(eng, code, START, st, c, frozen, handed=handed)
            assert untouched(handed, st), code
        some = np.zeros_like(c["fixed"])
        some[c["aoff"][4] + 3, 2] = 1
        if code in MOVING_CELL:
            handed = []
            with pytest.raises(Exception, match="only some components"):
                _md_launch(eng, code, START, st, c, some, handed=handed)
            assert untouched(handed, st), code
        else:
            _md_launch(eng, code, START, st, c, some)
    # handles: the same refusals, and no mask after the first run
    from chgnet_amd import _lib

    s = _limno2()
    meng = model.engine
    prep = meng.prepare_structures([s])
    host = prep.host()
    n = len(s)
    u8 = lambda a: _ptr(np.ascontiguousarray(a, np.uint8), ctypes.c_uint8)  # noqa: E731
    whole, part, everything = np.zeros((n, 3)), np.zeros((n, 3)), np.ones((n, 3))
    whole[[0, 3]] = 1
    part[2, 0] = 1
    for cell in (1, 0):
        h = ctypes.c_void_p()
        p = _relax_params(cell, 0.05, 3)
        meng._check(meng.lib.chg_relax_create(meng.handle, ctypes.byref(host), ctypes.byref(p), ctypes.byref(h)))
        try:
            assert (meng.lib.chg_relax_set_fixed(meng.handle, h, u8(part)) != 0) == bool(cell)
            assert meng.lib.chg_relax_set_fixed(meng.handle, h, u8(whole)) == 0
            assert meng.lib.chg_relax_set_fixed(meng.handle, h, None) == 0                      # null clears it
            assert meng.lib.chg_relax_set_fixed(meng.handle, h, u8(everything)) == 0
            n_active = ctypes.c_int32()
            meng._check(meng.lib.chg_relax_run(meng.handle, h, 1, ctypes.byref(n_active)))
            assert meng.lib.chg_relax_set_fixed(meng.handle, h, u8(whole)) != 0                 # after the first run
            assert "already run" in meng.lib.chg_last_error(meng.handle).decode()
        finally:
            meng.lib.chg_relax_free(meng.handle, h)
    from chgnet_amd.dynamics import ATOMIC_MASSES

    masses = np.ascontiguousarray(ATOMIC_MASSES[s.atomic_numbers])
    mom = np.ascontiguousarray(np.random.default_rng(0).normal(0, 1.0, (n, 3)))
    for code in range(7):
        prm = _md_params(code)
        prm.loginterval, prm.ring_frames = 1, 4
        h = ctypes.c_void_p()
        if code == LANGEVIN:
            seeds = np.array([5], np.uint64)
            rc = meng.lib.chg_md_create_langevin(meng.handle, ctypes.byref(host), _ptr(masses), _ptr(mom), ctypes.byref(prm), FRICTION,
                                                 _ptr(seeds, ctypes.c_uint64), ctypes.byref(h))
        elif code in (NVT_NHC, NPT_NHC):
            rc = meng.lib.chg_md_create_nhc(meng.handle, ctypes.byref(host), _ptr(masses), _ptr(mom), ctypes.byref(prm), CHAIN, ctypes.byref(h))
        else:
            rc = meng.lib.chg_md_create(meng.handle, ctypes.byref(host), _ptr(masses), _ptr(mom), ctypes.byref(prm), ctypes.byref(h))
        meng._check(rc)
        try:
            assert (meng.lib.chg_md_set_fixed(meng.handle, h, u8(part)) != 0) == (code in MOVING_CELL), code
            if code != NVE:                                                 # NVE takes it (and zeroes every momentum): below
                assert meng.lib.chg_md_set_fixed(meng.handle, h, u8(everything)) != 0, code
            assert meng.lib.chg_md_set_fixed(meng.handle, h, u8(whole)) == 0
            out = {"momenta": np.empty((n, 3))}
            o = _lib.fill_out(_lib.MdOutHost(), out)
            meng._check(meng.lib.chg_md_download(meng.handle, h, ctypes.byref(o)))
            free_rows = [i for i in range(n) if i not in (0, 3)]              # every call starts from the created momenta: `part` left no trace
            assert not out["momenta"][[0, 3]].any() and np.array_equal(out["momenta"][free_rows], mom[free_rows])     # the held momenta are zeroed
            assert meng.lib.chg_md_set_fixed(meng.handle, h, None) == 0        # null clears the mask and gives the created momenta back
            meng._check(meng.lib.chg_md_download(meng.handle, h, ctypes.byref(o)))
            assert np.array_equal(out["momenta"], mom)
            assert meng.lib.chg_md_set_fixed(meng.handle, h, u8(whole)) == 0
            if code == NVE:
                assert meng.lib.chg_md_set_fixed(meng.handle, h, u8(everything)) == 0
                meng._check(meng.lib.chg_md_download(meng.handle, h, ctypes.byref(o)))
                assert not out["momenta"].any()
            meng._check(meng.lib.chg_md_run(meng.handle, h, 0))
            assert meng.lib.chg_md_set_fixed(meng.handle, h, u8(whole)) != 0                    # after the first run
        finally:
            meng.lib.chg_md_free(meng.handle, h)


# ---- 5. end to end on the golden LiMnO2 cell ------------------------------------------------------------------------------------------------
def _limno2(rattle=0.08, strain=0.0, seed=11):
    from chgnet_amd.graph.structure import Lattice, Structure

    _, d = load_case("limno2")
    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"])
    rng = np.random.default_rng(seed)
    lat = s.lattice.matrix @ (np.eye(3) + strain * rng.normal(size=(3, 3)))
    cart = s.frac_coords @ s.lattice.matrix + rattle * rng.normal(size=(len(s), 3))
    return Structure(Lattice(lat), s.atomic_numbers, cart @ np.linalg.inv(lat))


def _third(n):
    return list(range(0, n, 3))                                            # about a third of the atoms


def _host_predict(model, z):
    from chgnet_amd.graph.structure import Lattice, Structure

    def f(frac, lat):
        pred = model.predict_structure(Structure(Lattice(lat), z, frac), task="efsm")
        return pred["f"], pred["s"]
    return f


@pytest.mark.parametrize("relax_cell", [True, False])
@pytest.mark.parametrize("optimizer", ["FIRE", "LBFGS"])
def test_relax_with_held_atoms_matches_host_loop(model, optimizer, relax_cell):
    """The pattern and tolerances of test_gpu_relax.test_relax_matches_host_loop, 15 evaluations."""
    from chgnet_amd.relax import StructOptimizer

    s = _limno2(rattle=0.08, strain=0.03)
    held = _third(len(s))
    mask = np.zeros((len(s), 3), bool)
    mask[held] = True
    steps = 14
    res = StructOptimizer(model=model, optimizer_class=optimizer).relax(s, fmax=1e-4, steps=steps, relax_cell=relax_cell, loginterval=1,
                                                                        verbose=False, fixed_atoms=held)
    traj, fin = res["trajectory"], res["final_structure"]
    r, frames, raw = cref.relax_host_fixed(s, _host_predict(model, s.atomic_numbers), mask, optimizer=optimizer, fmax=1e-4, steps=steps,
                                           relax_cell=relax_cell)
    assert len(frames) == steps + 1 and len(traj) == steps + 2
    worst = 0.0
    for k, (frac, lat) in enumerate(frames):
        worst = max(worst, np.abs(traj.cells[k] - lat).max(), np.abs(traj.atom_positions[k] - frac @ lat).max())
        assert not traj.forces[k][held].any(), k                           # the reported forces are the masked ones
        assert np.abs(traj.forces[k] - r.reported_forces(raw[k])).max() < 1e-3, k
        if not relax_cell:
            assert np.array_equal(traj.cells[k], s.lattice.matrix)
    print(optimizer, "relax_cell", relax_cell, "worst |device - host loop|", worst)
    assert worst < 1e-5
    assert np.abs(fin.lattice.matrix - r.lattice()).max() < 1e-5
    assert np.array_equal(fin.frac_coords[held], s.frac_coords[held])      # held atoms keep their fractional coordinates, to the bit
    free = [i for i in range(len(s)) if i not in held]
    assert np.abs(fin.frac_coords[free] - s.frac_coords[free]).max() > 1e-4
    assert fin.site_properties["selective_dynamics"][0] == [False] * 3 and fin.site_properties["selective_dynamics"][1] == [True] * 3
    if relax_cell:
        assert np.abs(fin.lattice.matrix - s.lattice.matrix).max() > 1e-4  # the cell did move, and the held atoms went with it


@pytest.mark.parametrize("optimizer", ["FIRE", "LBFGS"])
def test_relax_converges_on_the_free_atoms(model, optimizer):
    from chgnet_amd.graph.structure import Lattice, Structure
    from chgnet_amd.relax import StructOptimizer

    s = _limno2(rattle=0.05)
    held = _third(len(s))
    fmax = 0.3
    res = StructOptimizer(model=model, optimizer_class=optimizer).relax_batch([s], fmax=fmax, steps=30, relax_cell=False, fixed_atoms=[held])[0]
    fin = res["final_structure"]
    assert not res["forces"][held].any() and np.array_equal(fin.frac_coords[held], s.frac_coords[held])
    assert res["status"] in ("CONVERGED", "MAX_STEPS")
    if optimizer == "LBFGS":                  # measured: L-BFGS converges here in 20 steps; FIRE needs more than the 30 it gets
        assert res["converged"], res["n_steps"]
    if res["converged"]:
        f = np.asarray(model.predict_structure(Structure(Lattice(fin.lattice.matrix), fin.atomic_numbers, fin.frac_coords))["f"], np.float64)
        free = [i for i in range(len(s)) if i not in held]
        assert np.sqrt((f[free] ** 2).sum(1).max()) < fmax + 1e-4
        assert np.sqrt((res["forces"] ** 2).sum(1).max()) < fmax
    print(optimizer, res["status"], res["n_steps"])


def _host_calc(model, z):
    from chgnet_amd.graph.structure import Lattice, Structure

    def calc(r, cell):
        pred = model.predict_structure(Structure(Lattice(cell), z, r @ np.linalg.inv(cell)), task="efs")
        e = float(pred["e"]) * (len(z) if model.is_intensive else 1)
        return e, np.asarray(pred["f"], np.float64), np.asarray(pred["s"], np.float64) * SW
    return calc


MD_E2E = {"nve": dict(ensemble="nve", starting_temperature=300.0),
          "nvt_berendsen": dict(ensemble="nvt", temperature=600.0, starting_temperature=200.0, taut=20.0),
          "langevin": dict(ensemble="nvt", thermostat="Langevin", temperature=600.0, starting_temperature=200.0, friction=0.02),
          "nvt_nhc": dict(ensemble="nvt", thermostat="Nose-Hoover-Chain", temperature=600.0, starting_temperature=200.0, taut=50.0),
          "npt_nhc": dict(ensemble="npt", thermostat="Nose-Hoover-Chain", temperature=600.0, starting_temperature=200.0, taut=50.0, taup=500.0,
                          pressure=0.5)}


@pytest.mark.parametrize("case", list(MD_E2E))
def test_md_with_held_atoms_matches_host_loop(model, calc, case):
    """The tolerances of the unconstrained counterparts (test_gpu_md / test_gpu_langevin / test_gpu_nhc test_run_matches_host_loop)."""
    from chgnet_amd.dynamics import ATOMIC_MASSES, MolecularDynamics

    s = _limno2(rattle=0.05, seed=3)
    n = len(s)
    held = _third(n)
    mask = np.zeros((n, 3), bool)
    mask[held] = True
    kw, steps, dt = dict(MD_E2E[case]), 20, 1.0 * md_ref.FS
    md = MolecularDynamics(s, model=calc, timestep=1.0, loginterval=1, seed=7, fixed_atoms=held, **kw)
    traj = md.run(steps)
    p0, m = md.traj.momenta[0], ATOMIC_MASSES[s.atomic_numbers]
    host, pos0 = _host_calc(model, s.atomic_numbers), s.frac_coords @ s.lattice.matrix
    if case in ("nve", "nvt_berendsen"):
        ref = cref.FixedMDRef(pos0, s.lattice.matrix, m, p0, mask, ensemble=md_ref.NVE if case == "nve" else md_ref.NVT, dt=dt,
                              temperature_k=kw.get("temperature", 300.0), taut=kw["taut"] * md_ref.FS if "taut" in kw else None, calc=host)
    elif case == "langevin":
        ref = cref.FixedLangevinRef(pos0, s.lattice.matrix, m, p0, mask, dt=dt, temperature_k=600.0, friction=0.02 / md_ref.FS,
                                    seed=md.thermostat_seed, fixcm=True, calc=host)
    else:
        ref = cref.FixedNHCRef(pos0, s.lattice.matrix, m, p0, mask, npt=case == "npt_nhc", dt=dt, temperature_k=600.0, taut=50.0 * md_ref.FS,
                               taup=500.0 * md_ref.FS, pressure=0.5 * md_ref.GPA, chain_length=3, calc=host)
    frames = ref.run(steps)
    assert len(traj) == len(frames) == steps + 1
    assert not p0[held].any() and p0[[i for i in range(n) if i not in held]].all()
    assert np.array_equal(traj.momenta[0], frames[0]["momenta"])
    errs = {"pos": 0.0, "mom": 0.0, "cell": 0.0, "e": 0.0, "T": 0.0, "H": 0.0}
    pscale = max(np.abs(fr["momenta"]).max() for fr in frames)
    dof = 3 * (n - len(held))
    frac0 = s.frac_coords[held]
    for k, fr in enumerate(frames):
        errs["pos"] = max(errs["pos"], np.abs(traj.atom_positions[k] - fr["positions"]).max())
        errs["mom"] = max(errs["mom"], np.abs(traj.momenta[k] - fr["momenta"]).max() / pscale)
        errs["cell"] = max(errs["cell"], np.abs(traj.cells[k] - fr["cell"]).max())
        errs["e"] = max(errs["e"], abs(traj.energies[k] - fr["epot"]) / n)
        errs["T"] = max(errs["T"], abs(traj.temperatures[k] - fr["temperature"]))
        if traj.conserved:
            errs["H"] = max(errs["H"], abs(traj.conserved[k] - fr["conserved"]) / n)
        assert not traj.momenta[k][held].any() and not traj.forces[k][held].any(), k                      # exactly 0 in every frame
        assert traj.temperatures[k] == pytest.approx(2.0 * traj.kinetic_energies[k] / (dof * md_ref.KB), rel=1e-12), k
        if case == "npt_nhc":
            assert np.abs(traj.atom_positions[k][held] @ np.linalg.inv(traj.cells[k]) - frac0).max() < 1e-12, k
        else:
            assert np.array_equal(traj.atom_positions[k][held], traj.atom_positions[0][held]), k
    print(case, errs, "T first / last", traj.temperatures[0], traj.temperatures[-1])
    assert errs["pos"] < 2e-5 and errs["cell"] < 2e-5, errs
    assert errs["mom"] < 1e-4 and errs["e"] < 1e-4 and errs["T"] < 0.05 and errs["H"] < 1e-4, errs
    assert md.atoms.site_properties["selective_dynamics"][0] == [False] * 3 and not md.momenta[held].any()
    if case == "npt_nhc":
        assert np.abs(traj.cells[-1] - traj.cells[0]).max() > 1e-4


# ---- 6. mixed batches ---------------------------------------------------------------------------------------------------------------------
def _relax_download(eng, handle, B, N):
    from chgnet_amd import _lib

    out = {"frac": np.empty((N, 3)), "lattice": np.empty((B, 3, 3)), "energy": np.empty(B, np.float32), "force": np.empty((N, 3), np.float32),
           "stress": np.empty((B, 3, 3), np.float32), "magmom": np.empty(N, np.float32), "n_steps": np.empty(B, np.int32),
           "status": np.empty(B, np.int32)}
    eng._check(eng.lib.chg_relax_download(eng.handle, handle, ctypes.byref(_lib.fill_out(_lib.RelaxOutHost(), out))))
    return out


@pytest.mark.parametrize("relax_cell", [True, False])
@pytest.mark.parametrize("optimizer", ["FIRE", "LBFGS"])
def test_mixed_batch_follows_each_structures_own_restatement(model, optimizer, relax_cell):
    """The driver one evaluation at a time, teacher-forced as tests/test_gpu_lbfgs.py does it (L-BFGS amplifies the engine's run-to-run
    force noise through y, so two runs cannot be compared closely): every structure of a batch that mixes constrained and unconstrained
    ones, fed the forces the device reports, must sit where its own single-structure restatement sits (1e-10 A)."""
    structs = [_limno2(0.06, 0.02, seed=1), _limno2(0.05, 0.02, seed=2), _limno2(0.07, 0.01, seed=3), _limno2(0.04, 0.03, seed=4)]
    fixed = [None, _third(len(structs[1])), None, [0, 1, 5]]
    masks = [cref.as_mask(None, len(s)) for s in structs]
    for m, fx in zip(masks, fixed):
        if fx is not None:
            m[fx] = True
    eng = model.engine
    prep = eng.prepare_structures(structs)
    host = prep.host()
    B, N = len(structs), int(prep.atom_off[-1])
    p = _relax_params(int(relax_cell), 1e-6, 500)
    h = ctypes.c_void_p()
    if optimizer == "LBFGS":
        lp = _lbfgs_params()
        eng._check(eng.lib.chg_relax_create_lbfgs(eng.handle, ctypes.byref(host), ctypes.byref(p), ctypes.byref(lp), ctypes.byref(h)))
        rel = [cref.FixedLbfgsRelaxation(s.frac_coords, s.lattice.matrix, m, relax_cell=relax_cell, fmax=1e-6, steps=500,
                                         p={**lbfgs_ref.LBFGS, "memory": MEMORY}) for s, m in zip(structs, masks)]
    else:
        eng._check(eng.lib.chg_relax_create(eng.handle, ctypes.byref(host), ctypes.byref(p), ctypes.byref(h)))
        rel = [cref.FixedRelaxation(s.frac_coords, s.lattice.matrix, m, relax_cell=relax_cell, fmax=1e-6, steps=500) for s, m in zip(structs, masks)]
    try:
        eng._check(eng.lib.chg_relax_set_fixed(eng.handle, h, _ptr(_u8(np.concatenate(masks)), ctypes.c_uint8)))
        n_active = ctypes.c_int32()
        for k in range(10):
            eng._check(eng.lib.chg_relax_run(eng.handle, h, 1, ctypes.byref(n_active)))
            d = _relax_download(eng, h, B, N)
            for i, r in enumerate(rel):
                sl = slice(prep.atom_off[i], prep.atom_off[i + 1])
                lat = r.lattice()
                assert np.abs(d["lattice"][i] - lat).max() < 1e-10, (k, i)
                assert np.abs(d["frac"][sl] @ d["lattice"][i] - r.frac() @ lat).max() < 1e-10, (k, i)
                assert np.array_equal(d["frac"][sl][masks[i].all(1)], structs[i].frac_coords[masks[i].all(1)]), (k, i)
                f, sig = d["force"][sl].astype(np.float64), d["stress"][i].astype(np.float64) * GPA
                assert not f[masks[i]].any() and f[~masks[i]].all(), (k, i)      # the reported forces are the masked ones
                r.advance(f, sig, True)
                assert (d["n_steps"][i], d["status"][i]) == (r.steps, r.status) == (k + 1, 0), (k, i)
    finally:
        eng.lib.chg_relax_free(eng.handle, h)


def test_relax_batch_mixes_constrained_and_free_structures(model, optimizer="FIRE"):
    """FIRE only: two L-BFGS runs of the same structure drift apart by more than any useful bound within a few steps (measured: 3.5e-5 A
    after 6 steps between an unconstrained structure in a batch and alone), which is why tests/test_gpu_lbfgs.py and the test above
    compare L-BFGS teacher-forced."""
    from chgnet_amd.relax import StructOptimizer

    structs = [_limno2(0.06, 0.02, seed=1), _limno2(0.05, 0.02, seed=2), _limno2(0.07, 0.01, seed=3), _limno2(0.04, 0.03, seed=4)]
    fixed = [None, _third(len(structs[1])), None, [0, 1, 5]]
    opt = StructOptimizer(model=model, optimizer_class=optimizer)
    kw = dict(fmax=0.05, steps=6, trajectory=True)
    mixed = opt.relax_batch(structs, fixed_atoms=fixed, **kw)
    plain, again = opt.relax_batch(structs, **kw), opt.relax_batch(structs, **kw)
    frames = lambda r: r["trajectory"].atom_positions + r["trajectory"].cells + r["trajectory"].forces  # noqa: E731
    # "bit-identical to a batch run with no mask at all" has a meaning only where that batch is bit-identical to itself: the engine's fp32
    # forces are not reproducible run to run (atomic accumulation order; measured here: two identical no-mask batches differ from the first
    # step on, |dT| / T = 5e-8 after one MD step).  Two no-mask runs are the control: where they agree to the bit the mixed batch must
    # too; where they do not, what is not evaluated (the first frame's configuration) is still compared to the bit and the rest within
    # the run-to-run bound of test_gpu_relax.test_batch_equals_single.  That an unconstrained structure steps to the same bits beside
    # constrained ones, given the same forces, is test_unconstrained_members_of_a_mixed_launch_step_to_the_same_bits.
    reproducible = all(np.array_equal(x, y) for a, b in zip(plain, again) for x, y in zip(frames(a), frames(b)))
    print(optimizer, "two no-mask batches bit-identical:", reproducible, "-> unconstrained structures compared",
          "to the bit" if reproducible else "at frame 0 to the bit, then within 2e-5 A")
    for i, (s, fx) in enumerate(zip(structs, fixed)):
        alone = opt.relax_batch([s], fixed_atoms=[fx], **kw)[0]
        a, b = mixed[i], alone
        assert (a["n_steps"], a["status"]) == (b["n_steps"], b["status"]), i
        pa = a["final_structure"].frac_coords @ a["final_structure"].lattice.matrix
        pb = b["final_structure"].frac_coords @ b["final_structure"].lattice.matrix
        assert np.abs(pa - pb).max() < 2e-5 and np.abs(a["final_structure"].lattice.matrix - b["final_structure"].lattice.matrix).max() < 2e-5, i
        if fx is None:
            c = plain[i]
            assert (a["n_steps"], a["status"]) == (c["n_steps"], c["status"]), i
            assert "selective_dynamics" not in a["final_structure"].site_properties
            assert np.array_equal(a["trajectory"].atom_positions[0], c["trajectory"].atom_positions[0]), i
            assert np.array_equal(a["trajectory"].cells[0], c["trajectory"].cells[0]), i
            if reproducible:
                assert all(np.array_equal(x, y) for x, y in zip(frames(a), frames(c))), i
            else:
                pc = c["final_structure"].frac_coords @ c["final_structure"].lattice.matrix
                assert np.abs(pa - pc).max() < 2e-5 and np.abs(a["final_structure"].lattice.matrix - c["final_structure"].lattice.matrix).max() < 2e-5, i
        else:
            assert np.array_equal(a["final_structure"].frac_coords[fx], s.frac_coords[fx]) and not a["forces"][fx].any(), i


@pytest.mark.parametrize("case", ["nvt_berendsen", "langevin", "nvt_nhc"])
def test_run_batch_mixes_constrained_and_free_replicas(calc, case):
    from chgnet_amd.dynamics import MolecularDynamics

    structs = [_limno2(0.05, seed=1), _limno2(0.04, seed=2), _limno2(0.03, seed=3)]
    fixed = [None, _third(len(structs[1])), [2]]
    seeds = [11, 12, 13]
    kw = dict(MD_E2E[case], timestep=2.0, loginterval=2)
    mixed = MolecularDynamics.run_batch(structs, 10, seeds=seeds, model=calc, fixed_atoms=fixed, **kw)
    plain = MolecularDynamics.run_batch(structs, 10, seeds=seeds, model=calc, **kw)
    again = MolecularDynamics.run_batch(structs, 10, seeds=seeds, model=calc, **kw)
    frames = lambda r: r["trajectory"].atom_positions + r["trajectory"].momenta + [np.array(r["trajectory"].temperatures)]  # noqa: E731
    # the control of test_relax_batch_mixes_constrained_and_free_structures: bit identity with a no-mask batch where two no-mask batches
    # agree to the bit, else frame 0 (nothing evaluated yet) to the bit and the rest within the bound of test_gpu_md.test_batch_equals_single
    reproducible = all(np.array_equal(x, y) for a, b in zip(plain, again) for x, y in zip(frames(a), frames(b)))
    print(case, "two no-mask batches bit-identical:", reproducible, "-> unconstrained replicas compared",
          "to the bit" if reproducible else "at frame 0 to the bit, then within 2e-5 A and 0.5 K")
    for i, (s, sd, fx) in enumerate(zip(structs, seeds, fixed)):
        t1 = MolecularDynamics(s, model=calc, seed=sd, fixed_atoms=fx, **kw).run(10)
        tb = mixed[i]["trajectory"]
        assert tb.steps == t1.steps == [0, 2, 4, 6, 8, 10] and np.array_equal(tb.momenta[0], t1.momenta[0]), i
        for k in range(len(t1)):
            assert np.abs(tb.atom_positions[k] - t1.atom_positions[k]).max() < 2e-5 and abs(tb.temperatures[k] - t1.temperatures[k]) < 0.5, (i, k)
        if fx is None:
            tp = plain[i]["trajectory"]
            assert np.array_equal(tb.atom_positions[0], tp.atom_positions[0]) and np.array_equal(tb.momenta[0], tp.momenta[0])
            assert tb.temperatures[0] == tp.temperatures[0]                # 3 n in the denominator, exactly as without a mask
            if reproducible:
                assert all(np.array_equal(x, y) for x, y in zip(frames(mixed[i]), frames(plain[i]))), i
            else:
                for k in range(len(tp)):
                    assert np.abs(tb.atom_positions[k] - tp.atom_positions[k]).max() < 2e-5 and abs(tb.temperatures[k] - tp.temperatures[k]) < 0.5, (i, k)
        else:
            assert all(not p[fx].any() for p in tb.momenta) and not mixed[i]["momenta"][fx].any()
            assert all(np.array_equal(x[fx], tb.atom_positions[0][fx]) for x in tb.atom_positions)
            assert mixed[i]["final_structure"].site_properties["selective_dynamics"][fx[0]] == [False] * 3
