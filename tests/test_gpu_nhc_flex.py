"""Flexible-cell Nose-Hoover-chain NPT molecular dynamics on the MI355X (``cell_dof="flexible"`` / ``"axes"``): the step kernel against
the float64 restatement (tests/nhc_flex_ref.py) on every flag set the driver uses, with and without held atoms, a non-finite replica,
the refusals of the entry points, MolecularDynamics against the restatement driven by predict_structure, run_batch == run per
replica, split runs, and the drift of the conserved energy against the isotropic barostat's."""

from __future__ import annotations

import copy
import ctypes
import json
import os

import numpy as np
import pytest

import md_ref
import nhc_flex_ref
from conftest import load_case

pytestmark = pytest.mark.gpu

NPT_NHC, FLEX, AXES = 6, 7, 8
CODES = {"flexible": FLEX, "axes": AXES}
CELL_MODES = {"flexible": 1, "axes": 2}
ABSORB, KICK2, START = 1, 2, 4
SW = 1.0 / 160.21766208
NHC_STATE = 20
MODES = ("flexible", "axes")


@pytest.fixture(scope="module")
def model(trained_like_weights):
    from chgnet_amd import CHGNet

    return CHGNet(state_dict=trained_like_weights)


@pytest.fixture(scope="module")
def calc(model):
    from chgnet_amd.calculator import CHGNetCalculator

    return CHGNetCalculator(model=model)


def _structure(name, supercell=(1, 1, 1), rattle=0.0, seed=0):
    from chgnet_amd.graph.structure import Lattice, Structure

    _, d = load_case(name)
    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]).make_supercell(supercell)
    rng = np.random.default_rng(seed)
    cart = s.frac_coords @ s.lattice.matrix + rattle * rng.normal(size=(len(s), 3))
    return Structure(s.lattice, s.atomic_numbers, cart @ np.linalg.inv(s.lattice.matrix))


def _host_calc(model, z):
    from chgnet_amd.graph.structure import Lattice, Structure

    def calc(r, cell):
        pred = model.predict_structure(Structure(Lattice(cell), z, r @ np.linalg.inv(cell)), task="efs")
        e = float(pred["e"]) * (len(z) if model.is_intensive else 1)
        return e, np.asarray(pred["f"], np.float64), np.asarray(pred["s"], np.float64) * SW
    return calc


# ---- 1. the step kernel on its own ---------------------------------------------------------------------------------------------
SIZES = [2, 5, 300]                        # the smallest N_f, a partial wave, more than one 256-row pass with a ragged tail
STEPS0 = [0, 70000, 3]
REPEATED, ZERO = 0, 1                      # Vg with two equal eigenvalues; Vg = 0 (and a left-handed cell)
FLAGSETS = {"start_only": START, "finish_only": ABSORB | KICK2, "finish_start": ABSORB | KICK2 | START}


def _masks(kind):
    """Whole atoms held: atom 0 of every replica with more than two atoms, atom 2 of the 5-atom one, the last one of the 300-atom one."""
    if kind is None:
        return [None] * len(SIZES)
    masks = [np.zeros((n, 3), bool) for n in SIZES]
    if kind == "held":
        masks[0][1] = True
        masks[1][[0, 2]] = True
        masks[2][[0, 17, 255, 256, 299]] = True
    return masks


def _run_step_kernel(hip_engine, flags, mode, chain_length, nan_replica=None, mask_kind=None, masks=None):
    """One launch of the step kernel on three replicas with non-zero chain state and strain rate; returns inputs, outputs and the
    restatement replicas before the launch.  taut = 100 dt; taup = 50 dt, so that the barostat moves the cell by about a percent."""
    from chgnet_amd import _lib

    rng = np.random.default_rng(1000 * flags + 10 * chain_length + (mode == "axes"))
    dt, t0, M = 2.0 * md_ref.FS, 300.0, chain_length
    masks = _masks(mask_kind) if masks is None else masks
    refs, cached, new_f = [], [], []
    for o, (n, k) in enumerate(zip(SIZES, STEPS0)):
        cell = np.diag(rng.uniform(5, 9, 3)) + rng.normal(0, 0.5, (3, 3))                       # sheared, neither triangular form
        if o == ZERO:
            cell[2] = -cell[2]                                                                      # left-handed
        m = rng.uniform(1.0, 200.0, n)
        ref = nhc_flex_ref.NHCFlexRef(rng.random((n, 3)) @ cell, cell, m, rng.normal(0, 0.3, (n, 3)) * np.sqrt(m)[:, None], cell_dof=mode,
                                      mask=masks[o], dt=dt, temperature_k=t0, taut=100 * dt, taup=50 * dt, pressure=0.5 * md_ref.GPA,
                                      chain_length=M)
        ref.v, ref.eta = rng.normal(0, 0.03, M), rng.normal(0, 0.5, M)
        ref.vb, ref.xi = rng.normal(0, 0.05, M), rng.normal(0, 0.5, M)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if mode == "axes":
            q = np.eye(3)
        if o == REPEATED:
            a, b = rng.normal(0, 0.02, 2)
            vg = q @ np.diag([a, a, b]) @ q.T
        elif o == ZERO:
            vg = np.zeros((3, 3))
        else:
            vg = q @ np.diag(rng.normal(0, 0.02, 3)) @ q.T
        ref.Vg = np.triu(vg) + np.triu(vg, 1).T
        ref.nsteps = k
        refs.append(ref)
        cached.append(rng.normal(0, 0.5, (n, 3)))
        new_f.append(rng.normal(0, 0.5, (n, 3)).astype(np.float32))
    assert np.linalg.det(refs[ZERO].cell) < 0 < np.linalg.det(refs[0].cell)
    w = np.linalg.eigvalsh(refs[REPEATED].Vg)
    assert min(w[1] - w[0], w[2] - w[1]) <= 1e-15 < w[2] - w[0]
    B = len(SIZES)
    aoff = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    r = np.ascontiguousarray(np.concatenate([x.r for x in refs]))
    p = np.ascontiguousarray(np.concatenate([x.p for x in refs]))
    f = np.ascontiguousarray(np.concatenate([np.where(x.mask, 0.0, c) for x, c in zip(refs, cached)]))
    m = np.ascontiguousarray(np.concatenate([x.m for x in refs]))
    sd = np.zeros((B, 40))
    si = np.zeros((B, 4), np.int32)
    nhc = np.zeros((B, NHC_STATE))
    vg = np.zeros((B, 3, 3))
    old_stress = rng.normal(0, 3.0, (B, 3, 3)) * SW                       # the cached stress MD_START reads: not symmetric
    for o, x in enumerate(refs):
        sd[o, :9] = x.cell.ravel()
        sd[o, 9:18] = np.linalg.inv(x.cell).ravel()
        sd[o, 18] = -50.0 - o
        sd[o, 19] = md_ref.kinetic_energy(x.p, x.m)
        sd[o, 20] = md_ref.temperature(x.p, x.m)
        sd[o, 21:30] = old_stress[o].ravel()
        sd[o, 30:39] = nhc_flex_ref.sym_outer_sum(x.p, x.m).ravel()
        si[o] = [x.nsteps, 0, 0, 0]
        nhc[o, 0:M], nhc[o, 4:4 + M], nhc[o, 8:8 + M], nhc[o, 12:12 + M] = x.v, x.eta, x.vb, x.xi
        nhc[o, 17] = 123.0                                                 # H - Epot of an earlier evaluation: replaced by MD_ABSORB only
        vg[o] = x.Vg
    energy = rng.normal(-100, 10, B).astype(np.float32)
    force = np.ascontiguousarray(np.concatenate(new_f), np.float32)
    if nan_replica is not None:
        force[aoff[nan_replica] + 1, 1] = np.nan
    stress = np.ascontiguousarray(rng.normal(0, 3.0, (B, 3, 3)), np.float32)
    assert np.abs(stress - stress.transpose(0, 2, 1)).max() > 0.1
    frac_next = np.zeros_like(r)
    lat_next = np.zeros((B, 3, 3))
    before = {k: v.copy() for k, v in dict(r=r, p=p, f=f, sd=sd, si=si, nhc=nhc, vg=vg).items()}
    prm = _lib.MdParams(ensemble=CODES[mode], fixcm=0, dt=dt, temperature=t0, taut=100 * dt, taup=50 * dt, pressure=0.5 * md_ref.GPA,
                        compressibility=0.0, kB=md_ref.KB, stress_weight=SW, loginterval=1, ring_frames=1, log_stress=1, log_crystal_fea=0,
                        r_atom=6.0, r_bond=3.0, numerical_tol=1e-8)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    fixed = None
    if masks[0] is not None:
        fixed = np.ascontiguousarray(np.concatenate(masks), np.uint8)
    rc = hip_engine.lib.chg_test_md_step_nhc_flex(
        hip_engine.handle, ctypes.byref(prm), B, aoff.ctypes.data_as(_lib.c_int_p), flags, dp(r), dp(p), dp(f), dp(m), dp(sd),
        si.ctypes.data_as(_lib.c_int_p), fp(energy), fp(force), fp(stress), dp(frac_next), dp(lat_next), M, dp(nhc), dp(vg),
        fixed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if fixed is not None else None)
    out = dict(r=r, p=p, f=f, sd=sd, si=si, nhc=nhc, vg=vg, frac_next=frac_next, lat_next=lat_next, rc=rc)
    return aoff, before, out, refs, cached, new_f, old_stress, stress, energy


def _check_against_restatement(flags, aoff, before, out, refs, cached, new_f, old_stress, stress, energy, skip=()):
    """Every output at relative 1e-12, with the scale conventions of test_gpu_nhc.py: the scale of an array is its largest entry; for a
    sum of terms of either sign (the strain rate, H - Epot) it is the largest term, which bounds the rounding of the sum."""
    worst = {}

    def close(got, want, what, scale=None):
        scale = (np.abs(want).max() if scale is None else scale) + 1e-300
        err = np.abs(got - want).max() / scale
        worst[what] = max(worst.get(what, 0.0), err)
        assert err <= 1e-12, (what, err)

    for o, ref in enumerate(refs):
        if o in skip:
            continue
        ref = copy.deepcopy(ref)
        M = len(ref.v)
        sl = slice(aoff[o], aoff[o + 1])
        fcache, sigma, steps = np.where(ref.mask, 0.0, cached[o]), old_stress[o], ref.nsteps
        vg_terms = [np.abs(ref.Vg).max()]
        tau = 0.5 * ref.dt
        constrained = ref.mask.any()
        dof = ref.nf if constrained else 3 * len(ref.m)

        def kick_size(sig):                                               # the largest term of the barostat kick
            vol = ref.volume()
            return tau * max(np.abs(nhc_flex_ref.sym_outer_sum(ref.p, ref.m)).max(), ref.k2() / ref.nf, abs(ref.pext * vol),
                             vol * np.abs(sig).max()) / ref.Wg

        if flags & ABSORB:
            fcache, sigma = np.where(ref.mask, 0.0, new_f[o].astype(np.float64)), stress[o].astype(np.float64) * SW
            vg_terms.append(kick_size(sigma))
            ref.second_half(fcache, sigma)
            steps += 1
            done = copy.deepcopy(ref)                                      # the end of the step: what sd and H - Epot describe
        if flags & START:
            vg_terms.append(kick_size(sigma))
            ref.first_half(fcache, sigma)
        close(out["r"][sl], ref.r, "r")
        close(out["p"][sl], ref.p, "p")
        close(out["f"][sl], fcache, "f")
        assert not out["p"][sl][ref.mask].any()
        close(out["sd"][o, :9].reshape(3, 3), ref.cell, "cell")
        close(out["sd"][o, 9:18].reshape(3, 3), np.linalg.inv(ref.cell), "cell^-1")
        assert list(out["si"][o]) == [steps, 0, 0, 0], (o, out["si"][o])
        x = out["nhc"][o]
        close(x[0:M], ref.v, "v")
        close(x[4:4 + M], ref.eta, "eta")
        close(x[8:8 + M], ref.vb, "vb")
        close(x[12:12 + M], ref.xi, "xi")
        assert not x[M:4].any() and not x[4 + M:8].any() and not x[8 + M:12].any() and not x[12 + M:17].any() and not x[18:].any()
        g = out["vg"][o]
        close(g, ref.Vg, "Vg", max(vg_terms))
        assert np.array_equal(g, g.T)
        if ref.cell_dof == "axes":
            assert not (g - np.diag(np.diag(g))).any()
        if flags & ABSORB:
            ekin = md_ref.kinetic_energy(done.p, done.m)
            close(out["sd"][o, 18], float(energy[o]), "epot")
            close(out["sd"][o, 19], ekin, "ekin")
            close(out["sd"][o, 20], 2.0 * ekin / (dof * md_ref.KB), "T")
            close(out["sd"][o, 21:30].reshape(3, 3), sigma, "stress")
            close(out["sd"][o, 30:39].reshape(3, 3), nhc_flex_ref.sym_outer_sum(done.p, done.m), "sum p p / m")
            close(x[17], done.extended_energy(), "H - Epot", max(abs(done.extended_energy()), 0.5 * done.k2()))
        else:
            assert np.array_equal(out["sd"][o, 18:], before["sd"][o, 18:]) and x[17] == 123.0
        if flags & START:
            close(out["frac_next"][sl], ref.r @ np.linalg.inv(ref.cell), "frac_next")
            close(out["lat_next"][o], ref.cell, "lat_next")
            assert np.abs(ref.cell - refs[o].cell).max() > 1e-4 * np.abs(ref.cell).max()           # the barostat did act
            held = ref.mask[:, 0]
            if held.any():                                                 # held rows keep their fractional coordinates
                close(out["frac_next"][sl][held], (refs[o].r @ np.linalg.inv(refs[o].cell))[held], "held frac")
        else:
            assert not out["frac_next"][sl].any() and not out["lat_next"][o].any()
            assert np.array_equal(out["sd"][o, :18], before["sd"][o, :18])
        free = ~ref.mask
        assert np.abs(out["p"][sl] - before["p"][sl])[free].max() > 1e-3   # and so did the thermostat and the kick
    return worst


@pytest.mark.parametrize("chain_length", [1, 4])
@pytest.mark.parametrize("cell_dof", MODES)
@pytest.mark.parametrize("flagset", list(FLAGSETS))
def test_step_kernel_matches_restatement(hip_engine, flagset, cell_dof, chain_length):
    flags = FLAGSETS[flagset]
    aoff, before, out, *rest = _run_step_kernel(hip_engine, flags, cell_dof, chain_length)
    hip_engine._check(out["rc"])
    worst = _check_against_restatement(flags, aoff, before, out, *rest)
    print(flagset, cell_dof, "chain", chain_length, "worst relative errors", worst)


# ---- 2. the same with held atoms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain_length", [1, 4])
@pytest.mark.parametrize("cell_dof", MODES)
@pytest.mark.parametrize("flagset", list(FLAGSETS))
def test_step_kernel_with_held_atoms_matches_restatement(hip_engine, flagset, cell_dof, chain_length):
    flags = FLAGSETS[flagset]
    aoff, before, out, refs, *rest = _run_step_kernel(hip_engine, flags, cell_dof, chain_length, mask_kind="held")
    hip_engine._check(out["rc"])
    assert [x.nf for x in refs] == [3, 9, 3 * 295]
    worst = _check_against_restatement(flags, aoff, before, out, refs, *rest)
    print(flagset, cell_dof, "chain", chain_length, "held atoms, worst relative errors", worst)


@pytest.mark.parametrize("cell_dof", MODES)
def test_all_zero_mask_is_bit_identical_and_partial_mask_is_refused(hip_engine, cell_dof):
    flags = ABSORB | KICK2 | START
    _, _, plain, *_ = _run_step_kernel(hip_engine, flags, cell_dof, 3)
    _, before, zero, *_ = _run_step_kernel(hip_engine, flags, cell_dof, 3, mask_kind="zero")
    assert plain["rc"] == 0 and zero["rc"] == 0
    for k in ("r", "p", "f", "sd", "si", "nhc", "vg", "frac_next", "lat_next"):
        assert np.array_equal(plain[k], zero[k]), k
    partial = _masks("zero")
    partial[2][7, 1] = True                                                # one component of one atom
    # the restatement asserts whole atoms, so the refusal is tried on the entry point itself, with the state of the accepted call
    from chgnet_amd import _lib

    fixed = np.ascontiguousarray(np.concatenate(partial), np.uint8)
    n_tot = sum(SIZES)
    prm = _lib.MdParams(ensemble=CODES[cell_dof], fixcm=0, dt=0.2, temperature=300.0, taut=20.0, taup=10.0, pressure=0.0, compressibility=0.0,
                        kB=md_ref.KB, stress_weight=SW, loginterval=1, ring_frames=1, log_stress=1, log_crystal_fea=0, r_atom=6.0, r_bond=3.0,
                        numerical_tol=1e-8)
    z3, z1 = np.zeros((n_tot, 3)), np.ones(n_tot)
    sd, si, nhc, vg = before["sd"].copy(), before["si"].copy(), before["nhc"].copy(), before["vg"].copy()
    aoff = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    rc = hip_engine.lib.chg_test_md_step_nhc_flex(
        hip_engine.handle, ctypes.byref(prm), 3, aoff.ctypes.data_as(_lib.c_int_p), START, dp(z3.copy()), dp(z3.copy()), dp(z3.copy()), dp(z1),
        dp(sd), si.ctypes.data_as(_lib.c_int_p), None, None, None, dp(z3.copy()), dp(np.zeros((3, 9))), 3, dp(nhc), dp(vg),
        fixed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    assert rc != 0
    assert np.array_equal(sd, before["sd"]) and np.array_equal(vg, before["vg"])        # nothing ran


# ---- 3. a non-finite replica -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell_dof", MODES)
def test_step_kernel_nonfinite_replica_is_left_untouched(hip_engine, cell_dof):
    flags, bad = ABSORB | KICK2 | START, 1
    aoff, before, out, *rest = _run_step_kernel(hip_engine, flags, cell_dof, 3, nan_replica=bad)
    hip_engine._check(out["rc"])
    sl = slice(aoff[bad], aoff[bad + 1])
    assert list(out["si"][bad]) == [STEPS0[bad], 1, 0, 0]                      # NONFINITE, the step is not counted
    for k in ("r", "p", "f"):
        assert np.array_equal(out[k][sl], before[k][sl]), k
    for k in ("sd", "nhc", "vg"):
        assert np.array_equal(out[k][bad], before[k][bad]), k                  # neither the chains nor the strain rate moved
    assert not out["frac_next"][sl].any() and not out["lat_next"][bad].any()
    _check_against_restatement(flags, aoff, before, out, *rest, skip=(bad,))   # its neighbours step as usual


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_they_cannot_run(hip_engine):
    from chgnet_amd import _lib
    from chgnet_amd.graph.structure import Lattice, Structure

    one, ints, floats, offs = np.zeros(64), np.zeros(64, np.int32), np.zeros(64, np.float32), np.array([0, 2], np.int32)
    ip, dp = ints.ctypes.data_as(_lib.c_int_p), one.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    fp, aoff = floats.ctypes.data_as(_lib.c_float_p), offs.ctypes.data_as(_lib.c_int_p)
    kw = dict(fixcm=0, dt=0.2, temperature=300.0, taut=20.0, taup=200.0, pressure=0.0, compressibility=0.0, kB=md_ref.KB, stress_weight=SW,
              loginterval=1, ring_frames=1, log_stress=1, log_crystal_fea=0, r_atom=6.0, r_bond=3.0, numerical_tol=1e-8)
    lib, h = hip_engine.lib, hip_engine.handle

    def step(fn, prm, *extra):
        return fn(h, ctypes.byref(prm), 1, aoff, START, dp, dp, dp, dp, dp, ip, fp, fp, fp, dp, dp, *extra)

    for code in (FLEX, AXES):                                                  # the older step entry points have no strain-rate matrix to give
        assert step(lib.chg_test_md_step, _lib.MdParams(ensemble=code, **kw)) != 0
        assert step(lib.chg_test_md_step_nhc, _lib.MdParams(ensemble=code, **kw), 3, dp) != 0
        assert step(lib.chg_test_md_step_fixed, _lib.MdParams(ensemble=code, **kw), 0.0, None, 3, dp, None) != 0
        for m in (0, 5, -1):
            assert step(lib.chg_test_md_step_nhc_flex, _lib.MdParams(ensemble=code, **kw), m, dp, dp, None) != 0
        assert step(lib.chg_test_md_step_nhc_flex, _lib.MdParams(ensemble=code, **dict(kw, temperature=0.0)), 3, dp, dp, None) != 0
        assert step(lib.chg_test_md_step_nhc_flex, _lib.MdParams(ensemble=code, **dict(kw, taup=0.0)), 3, dp, dp, None) != 0
        assert step(lib.chg_test_md_step_nhc_flex, _lib.MdParams(ensemble=code, **kw), 3, dp, None, None) != 0
    for code in (0, 1, 5, NPT_NHC, 9):                                         # and the new one runs nothing else
        assert step(lib.chg_test_md_step_nhc_flex, _lib.MdParams(ensemble=code, **kw), 3, dp, dp, None) != 0

    two = Structure(Lattice(np.eye(3) * 3.5), np.array([3, 3]), np.array([[0, 0, 0], [0.5, 0.5, 0.5]]))
    lone = Structure(Lattice(np.eye(3) * 3.5), np.array([3]), np.array([[0.0, 0.0, 0.0]]))
    ddp = ctypes.POINTER(ctypes.c_double)

    def create(fn, structs, prm, *extra):
        prep = hip_engine.prepare_structures(structs)
        host = prep.host()
        n = int(prep.atom_off[-1])
        masses, mom = np.full(n, 6.94), np.zeros((n, 3))
        handle = ctypes.c_void_p()
        rc = fn(h, ctypes.byref(host), masses.ctypes.data_as(ddp), mom.ctypes.data_as(ddp), ctypes.byref(prm), *extra, ctypes.byref(handle))
        if handle:
            lib.chg_md_free(h, handle)
        return rc

    ckw = dict(kw, loginterval=1, ring_frames=4)
    for code in (FLEX, AXES):
        assert create(lib.chg_md_create, [two], _lib.MdParams(ensemble=code, **ckw)) != 0
        assert create(lib.chg_md_create_nhc, [two], _lib.MdParams(ensemble=code, **ckw), 3) != 0
    good = _lib.MdParams(ensemble=NPT_NHC, **ckw)
    for mode in CELL_MODES.values():
        assert create(lib.chg_md_create_nhc_flex, [two], good, 3, mode) == 0
        assert create(lib.chg_md_create_nhc_flex, [two, lone], good, 3, mode) != 0
        assert create(lib.chg_md_create_nhc_flex, [two], _lib.MdParams(ensemble=NPT_NHC, **dict(ckw, temperature=0.0)), 3, mode) != 0
        assert create(lib.chg_md_create_nhc_flex, [two], _lib.MdParams(ensemble=NPT_NHC, **dict(ckw, temperature=-1.0)), 3, mode) != 0
        assert create(lib.chg_md_create_nhc_flex, [two], _lib.MdParams(ensemble=NPT_NHC, **dict(ckw, taup=0.0)), 3, mode) != 0
        assert create(lib.chg_md_create_nhc_flex, [two], _lib.MdParams(ensemble=NPT_NHC, **dict(ckw, taup=-5.0)), 3, mode) != 0
        for m in (0, 5, -1):
            assert create(lib.chg_md_create_nhc_flex, [two], good, m, mode) != 0
    for mode in (0, 3, -1):
        assert create(lib.chg_md_create_nhc_flex, [two], good, 3, mode) != 0


# ---- 5. MolecularDynamics against the restatement driven by predict_structure --------------------------------------------------------------
@pytest.mark.parametrize("cell_dof", MODES)
def test_run_matches_host_loop(model, calc, cell_dof):
    from chgnet_amd.dynamics import ATOMIC_MASSES, MolecularDynamics

    s = _structure("limno2", (1, 1, 1), rattle=0.05, seed=3)
    steps = 20
    md = MolecularDynamics(s, model=calc, ensemble="npt", thermostat="Nose-Hoover-Chain", cell_dof=cell_dof, temperature=600.0,
                           starting_temperature=200.0, timestep=1.0, taut=50.0, taup=500.0, pressure=0.5, loginterval=1, seed=7)
    traj = md.run(steps)
    p0 = md.traj.momenta[0]
    m = ATOMIC_MASSES[s.atomic_numbers]
    ref = nhc_flex_ref.NHCFlexRef(s.frac_coords @ s.lattice.matrix, s.lattice.matrix, m, p0, cell_dof=cell_dof, dt=1.0 * md_ref.FS,
                                  temperature_k=600.0, taut=50.0 * md_ref.FS, taup=500.0 * md_ref.FS, pressure=0.5 * md_ref.GPA, chain_length=3,
                                  calc=_host_calc(model, s.atomic_numbers))
    frames = ref.run(steps)
    assert len(traj) == len(frames) == len(traj.conserved) == steps + 1
    assert ref.n_evals == steps + 1                                            # one evaluation per step
    assert np.array_equal(traj.cells[0], s.lattice.matrix)
    assert np.abs(traj.atom_positions[0] - frames[0]["positions"]).max() < 1e-12
    assert np.array_equal(traj.momenta[0], frames[0]["momenta"])
    errs = {"pos": 0.0, "mom": 0.0, "cell": 0.0, "e": 0.0, "T": 0.0, "H": 0.0}
    pscale = max(np.abs(fr["momenta"]).max() for fr in frames)
    for k, fr in enumerate(frames):
        errs["pos"] = max(errs["pos"], np.abs(traj.atom_positions[k] - fr["positions"]).max())
        errs["mom"] = max(errs["mom"], np.abs(traj.momenta[k] - fr["momenta"]).max() / pscale)
        errs["cell"] = max(errs["cell"], np.abs(traj.cells[k] - fr["cell"]).max())
        errs["e"] = max(errs["e"], abs(traj.energies[k] - fr["epot"]) / len(s))
        errs["T"] = max(errs["T"], abs(traj.temperatures[k] - fr["temperature"]))
        errs["H"] = max(errs["H"], abs(traj.conserved[k] - fr["conserved"]) / len(s))
    moved = np.abs(traj.cells[-1] - traj.cells[0]).max()
    print("nhc", cell_dof, errs, "T first / last", traj.temperatures[0], traj.temperatures[-1], "cell moved by", moved, "A")
    assert errs["pos"] < 2e-5 and errs["cell"] < 2e-5, errs
    assert errs["mom"] < 1e-4 and errs["e"] < 1e-4 and errs["T"] < 0.05 and errs["H"] < 1e-4, errs
    st = md.thermostat_state
    assert set(st) == {"v", "eta", "vb", "xi", "veps", "vg"} and len(st["v"]) == 3 and st["veps"] == 0.0
    assert st["vg"].shape == (3, 3) and np.array_equal(st["vg"], st["vg"].T)
    assert np.abs(st["v"] - ref.v).max() < 1e-4 * np.abs(ref.v).max() and np.abs(st["eta"] - ref.eta).max() < 1e-4 * np.abs(ref.eta).max()
    assert moved > 1e-4 and np.abs(st["vg"] - ref.Vg).max() < 1e-4 * np.abs(ref.Vg).max()
    lam = np.vdot(traj.cells[-1], traj.cells[0]) / np.vdot(traj.cells[0], traj.cells[0])
    assert np.abs(traj.cells[-1] - lam * traj.cells[0]).max() > 1e-7           # not a mere scaling: the shape moved
    if cell_dof == "axes":
        assert not (st["vg"] - np.diag(np.diag(st["vg"]))).any()


# ---- 6. batch slots and split runs ------------------------------------------------------------------------------------------------------
NHC_KW = dict(ensemble="npt", thermostat="Nose-Hoover-Chain", temperature=500.0, starting_temperature=400.0, timestep=2.0, taut=40.0, taup=400.0,
              pressure=0.5)


def _same(ta, tb, what):
    assert ta.steps == tb.steps, what
    assert len(ta.conserved) == len(ta) == len(tb.conserved)
    assert np.array_equal(ta.momenta[0], tb.momenta[0]), what
    for k in range(len(ta)):
        assert np.abs(ta.atom_positions[k] - tb.atom_positions[k]).max() < 2e-5, (what, k)
        assert np.abs(ta.cells[k] - tb.cells[k]).max() < 2e-5, (what, k)
        assert abs(ta.temperatures[k] - tb.temperatures[k]) < 0.5, (what, k)
        assert abs(ta.conserved[k] - tb.conserved[k]) < 1e-4 * len(ta.atomic_numbers), (what, k)


def _same_state(a, b, what):
    for key in ("v", "eta", "vb", "xi", "vg"):
        assert np.abs(a[key] - b[key]).max() <= 1e-4 * max(np.abs(a[key]).max(), 1e-300), (what, key)
    assert np.array_equal(a["vg"], a["vg"].T) and np.array_equal(b["vg"], b["vg"].T)


@pytest.mark.parametrize("cell_dof", MODES)
def test_batch_equals_single(calc, cell_dof):
    from chgnet_amd.dynamics import MolecularDynamics

    structs = [_structure("limno2", rattle=0.05, seed=1), _structure("li9co7o16", rattle=0.03, seed=2), _structure("limno2", (2, 2, 1), rattle=0.04, seed=3)]
    seeds = [11, 12, 13]
    kw = dict(NHC_KW, cell_dof=cell_dof, loginterval=3)
    batch = MolecularDynamics.run_batch(structs, 12, seeds=seeds, model=calc, **kw)
    turned = MolecularDynamics.run_batch(structs[::-1], 12, seeds=seeds[::-1], model=calc, **kw)[::-1]
    for b, t, s, sd in zip(batch, turned, structs, seeds):
        md = MolecularDynamics(s, model=calc, seed=sd, **kw)
        t1 = md.run(12)
        assert b["status"] == "RUNNING" and b["n_steps"] == 12
        assert b["trajectory"].steps == [0, 3, 6, 9, 12] and len(b["trajectory"].conserved) == 5
        _same(b["trajectory"], t1, "batch vs alone")
        _same(t["trajectory"], t1, "another slot vs alone")
        _same_state(b["thermostat_state"], md.thermostat_state, "batch vs alone")
        _same_state(t["thermostat_state"], md.thermostat_state, "another slot vs alone")


@pytest.mark.parametrize("cell_dof", MODES)
def test_split_run_equals_one_run(calc, cell_dof):
    from chgnet_amd.dynamics import MolecularDynamics

    s = _structure("limno2", (2, 2, 1), rattle=0.04, seed=5)
    one = MolecularDynamics(s, model=calc, seed=21, cell_dof=cell_dof, **NHC_KW)
    t_one = one.run(12)
    two = MolecularDynamics(s, model=calc, seed=21, cell_dof=cell_dof, **NHC_KW)
    two.run(6)
    half = copy.deepcopy(two.thermostat_state)
    t_two = two.run(6)
    assert t_one.steps == t_two.steps == list(range(13))
    _same(t_one, t_two, "run(6); run(6) vs run(12)")
    _same_state(one.thermostat_state, two.thermostat_state, "run(6); run(6) vs run(12)")
    assert np.abs(half["vg"] - two.thermostat_state["vg"]).max() > 0            # the strain rate went on from where it was
    assert half["vg"].any() and np.abs(half["eta"] - two.thermostat_state["eta"]).max() > 0
    two.set_atoms(s)                                                             # a new handle: zeroed chains and strain rate
    assert two.thermostat_state is None
    two.run(0)
    assert not two.thermostat_state["v"].any() and not two.thermostat_state["vg"].any()


def test_held_atoms_follow_the_flexible_cell(calc):
    from chgnet_amd.dynamics import MolecularDynamics

    s = _structure("limno2", (2, 2, 1), rattle=0.04, seed=6)
    md = MolecularDynamics(s, model=calc, seed=4, cell_dof="flexible", fixed_atoms=[0, len(s) - 1], **dict(NHC_KW, taup=100.0))
    traj = md.run(10)
    frac0 = traj.atom_positions[0] @ np.linalg.inv(traj.cells[0])
    frac1 = traj.atom_positions[-1] @ np.linalg.inv(traj.cells[-1])
    held = [0, len(s) - 1]
    assert np.abs(traj.cells[-1] - traj.cells[0]).max() > 1e-4
    assert np.abs(frac1[held] - frac0[held]).max() < 1e-12 and np.abs(frac1 - frac0).max() > 1e-4
    assert not traj.momenta[-1][held].any()


# ---- 7. drift of the conserved energy on the real potential ------------------------------------------------------------------------------
def test_conserved_energy_drifts_no_more_than_twice_the_isotropic_barostat(calc):
    """Same 32-atom start, 200 steps of 1 fs with the isotropic chains and with each flexible form: the largest |H - H_0| may exceed the
    isotropic run's by at most a factor of 2 (both integrators are second order with the same force noise; the factor absorbs the
    six-component barostat).  The figures are printed, and appended to the file CHGNET_MD_NHC_FLEX_PROBE names when it is set
    (profiles/md_nhc_flex_probe.jsonl)."""
    from chgnet_amd.dynamics import MolecularDynamics

    s = _structure("limno2", (2, 2, 1), rattle=0.04, seed=9)
    assert len(s) == 32
    kw = dict(model=calc, ensemble="npt", thermostat="Nose-Hoover-Chain", temperature=300.0, starting_temperature=300.0, timestep=1.0, pressure=0.0,
              seed=3)
    steps = 200
    drift = {}
    for mode in ("isotropic", *MODES):
        h = np.array(MolecularDynamics(s, cell_dof=mode, **kw).run(steps).conserved)
        assert len(h) == steps + 1
        drift[mode] = float(np.abs(h - h[0]).max())
    rec = {"leg": "drift", "structure": "limno2 2x2x1", "atoms": len(s), "steps": steps, "timestep_fs": 1.0,
           **{f"{k}_max_abs_dH_eV": v for k, v in drift.items()}}
    print(json.dumps(rec))
    if os.environ.get("CHGNET_MD_NHC_FLEX_PROBE"):
        with open(os.environ["CHGNET_MD_NHC_FLEX_PROBE"], "a") as fh:
            fh.write(json.dumps(rec) + "\n")
    for mode in MODES:
        assert drift[mode] <= 2.0 * drift["isotropic"], rec
