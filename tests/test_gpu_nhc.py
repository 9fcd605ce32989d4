"""Nose-Hoover-chain NVT and isotropic NPT molecular dynamics on the MI355X: the step kernel against the float64 restatement
(tests/nhc_ref.py) on every flag set, chain length and ensemble, a non-finite replica, MolecularDynamics(thermostat="Nose-Hoover-Chain")
against the restatement driven by predict_structure, run_batch == run per replica, split runs, the cell shape and the total momentum,
the drift of the conserved energy against the NVE path's, and a 64 x 256-atom batch."""

from __future__ import annotations

import copy
import ctypes
import json
import os

import numpy as np
import pytest

import md_ref
import nhc_ref
from conftest import load_case

pytestmark = pytest.mark.gpu

NVT_NHC, NPT_NHC = 5, 6
ABSORB, KICK2, START = 1, 2, 4
SW = 1.0 / 160.21766208
NHC_STATE = 20


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
SIZES = [2, 5, 17, 300, 40]                # 300: rows beyond one pass of the workgroup; 2: the smallest N_f
STEPS0 = [0, 70000, 3, 49, 11]
LEFT_HANDED = 1                            # this replica's cell has a negative determinant
FLAGSETS = {"start_only": START, "finish_only": ABSORB | KICK2, "finish_start": ABSORB | KICK2 | START}


def _run_step_kernel(hip_engine, flags, npt, chain_length, nan_replica=None):
    """One launch of the step kernel on five replicas with non-zero chain state; returns inputs, outputs and the restatement replicas
    before the launch.  taut = 100 dt; taup = 50 dt, so that the barostat moves the cell by about a percent in one step."""
    from chgnet_amd import _lib

    rng = np.random.default_rng(1000 * flags + 10 * chain_length + int(npt))
    dt, t0, M = 2.0 * md_ref.FS, 300.0, chain_length
    refs, cached, new_f = [], [], []
    for o, (n, k) in enumerate(zip(SIZES, STEPS0)):
        cell = np.diag(rng.uniform(5, 9, 3)) + rng.normal(0, 0.5, (3, 3))
        if o == LEFT_HANDED:
            cell[2] = -cell[2]
        m = rng.uniform(1.0, 200.0, n)
        ref = nhc_ref.NHCRef(rng.random((n, 3)) @ cell, cell, m, rng.normal(0, 0.3, (n, 3)) * np.sqrt(m)[:, None], npt=npt, dt=dt,
                             temperature_k=t0, taut=100 * dt, taup=50 * dt, pressure=0.5 * md_ref.GPA, chain_length=M)
        ref.v, ref.eta = rng.normal(0, 0.03, M), rng.normal(0, 0.5, M)
        if npt:
            ref.vb, ref.xi, ref.veps = rng.normal(0, 0.05, M), rng.normal(0, 0.5, M), float(rng.normal(0, 0.02))
        ref.nsteps = k
        refs.append(ref)
        cached.append(rng.normal(0, 0.5, (n, 3)))
        new_f.append(rng.normal(0, 0.5, (n, 3)).astype(np.float32))
    assert np.linalg.det(refs[LEFT_HANDED].cell) < 0 < np.linalg.det(refs[0].cell)
    B = len(SIZES)
    aoff = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    r = np.ascontiguousarray(np.concatenate([x.r for x in refs]))
    p = np.ascontiguousarray(np.concatenate([x.p for x in refs]))
    f = np.ascontiguousarray(np.concatenate(cached))
    m = np.ascontiguousarray(np.concatenate([x.m for x in refs]))
    sd = np.zeros((B, 40))
    si = np.zeros((B, 4), np.int32)
    nhc = np.zeros((B, NHC_STATE))
    old_stress = rng.normal(0, 3.0, (B, 3, 3)) * SW                       # the cached stress MD_START reads
    for o, x in enumerate(refs):
        sd[o, :9] = x.cell.ravel()
        sd[o, 9:18] = np.linalg.inv(x.cell).ravel()
        sd[o, 18] = -50.0 - o
        sd[o, 19] = md_ref.kinetic_energy(x.p, x.m)
        sd[o, 20] = md_ref.temperature(x.p, x.m)
        sd[o, 21:30] = old_stress[o].ravel()
        sd[o, 30:39] = np.einsum("ka,kb,k->ab", x.p, x.p, 1.0 / x.m).ravel()
        si[o] = [x.nsteps, 0, 0, 0]
        nhc[o, 0:M], nhc[o, 4:4 + M], nhc[o, 8:8 + M], nhc[o, 12:12 + M], nhc[o, 16] = x.v, x.eta, x.vb, x.xi, x.veps
        nhc[o, 17] = 123.0                                                 # H - Epot of an earlier evaluation: replaced by MD_ABSORB only
    energy = rng.normal(-100, 10, B).astype(np.float32)
    force = np.ascontiguousarray(np.concatenate(new_f), np.float32)
    if nan_replica is not None:
        force[aoff[nan_replica] + 1, 1] = np.nan
    stress = np.ascontiguousarray(rng.normal(0, 3.0, (B, 3, 3)), np.float32)
    frac_next = np.zeros_like(r)
    lat_next = np.zeros((B, 3, 3))
    before = {k: v.copy() for k, v in dict(r=r, p=p, f=f, sd=sd, si=si, nhc=nhc).items()}
    prm = _lib.MdParams(ensemble=NPT_NHC if npt else NVT_NHC, fixcm=0, dt=dt, temperature=t0, taut=100 * dt, taup=50 * dt,
                        pressure=0.5 * md_ref.GPA, compressibility=0.0, kB=md_ref.KB, stress_weight=SW, loginterval=1, ring_frames=1,
                        log_stress=1, log_crystal_fea=0, r_atom=6.0, r_bond=3.0, numerical_tol=1e-8)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    hip_engine._check(hip_engine.lib.chg_test_md_step_nhc(
        hip_engine.handle, ctypes.byref(prm), B, aoff.ctypes.data_as(_lib.c_int_p), flags, dp(r), dp(p), dp(f), dp(m), dp(sd),
        si.ctypes.data_as(_lib.c_int_p), fp(energy), fp(force), fp(stress), dp(frac_next), dp(lat_next), M, dp(nhc)))
    out = dict(r=r, p=p, f=f, sd=sd, si=si, nhc=nhc, frac_next=frac_next, lat_next=lat_next)
    return aoff, before, out, refs, cached, new_f, old_stress, stress, energy


def _check_against_restatement(flags, aoff, before, out, refs, cached, new_f, old_stress, stress, energy, skip=()):
    """Every output at relative 1e-12.  The scale of an array is its largest entry; for a sum of terms of either sign (the strain rate,
    H - Epot) it is the largest term, which bounds the rounding of the sum."""
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
        fcache, sigma, steps = cached[o], old_stress[o], ref.nsteps
        veps_terms = [abs(ref.veps)]
        tau = 0.5 * ref.dt

        def kick_size(sig):                                               # the three terms of the barostat kick
            vol = ref.volume()
            return tau * max(ref.alpha * ref.k2(), abs(vol * np.trace(sig)), abs(3 * ref.pext * vol)) / ref.W

        if flags & ABSORB:
            fcache, sigma = new_f[o].astype(np.float64), stress[o].astype(np.float64) * SW
            veps_terms.append(kick_size(sigma))
            ref.second_half(fcache, sigma)
            steps += 1
            done = copy.deepcopy(ref)                                      # the end of the step: what sd and H - Epot describe
        if flags & START:
            veps_terms.append(kick_size(sigma))
            ref.first_half(fcache, sigma)
        close(out["r"][sl], ref.r, "r")
        close(out["p"][sl], ref.p, "p")
        close(out["f"][sl], fcache, "f")
        close(out["sd"][o, :9].reshape(3, 3), ref.cell, "cell")
        close(out["sd"][o, 9:18].reshape(3, 3), np.linalg.inv(ref.cell), "cell^-1")
        assert list(out["si"][o]) == [steps, 0, 0, 0], (o, out["si"][o])
        x = out["nhc"][o]
        close(x[0:M], ref.v, "v")
        close(x[4:4 + M], ref.eta, "eta")
        assert not x[M:4].any() and not x[4 + M:8].any() and not x[18:].any()
        if ref.npt:
            close(x[8:8 + M], ref.vb, "vb")
            close(x[12:12 + M], ref.xi, "xi")
            close(x[16], ref.veps, "veps", max(veps_terms))
        else:
            assert not x[8:17].any()                                       # NVT never touches the barostat
            assert np.array_equal(out["sd"][o, :18], before["sd"][o, :18])
        if flags & ABSORB:
            close(out["sd"][o, 18], float(energy[o]), "epot")
            close(out["sd"][o, 19], md_ref.kinetic_energy(done.p, done.m), "ekin")
            close(out["sd"][o, 20], md_ref.temperature(done.p, done.m), "T")
            close(out["sd"][o, 21:30].reshape(3, 3), sigma, "stress")
            close(out["sd"][o, 30:39].reshape(3, 3), np.einsum("ka,kb,k->ab", done.p, done.p, 1.0 / done.m), "sum p p / m")
            close(x[17], done.extended_energy(), "H - Epot", max(abs(done.extended_energy()), 0.5 * done.k2()))
        else:
            assert np.array_equal(out["sd"][o, 18:], before["sd"][o, 18:]) and x[17] == 123.0
        if flags & START:
            close(out["frac_next"][sl], ref.r @ np.linalg.inv(ref.cell), "frac_next")
            close(out["lat_next"][o], ref.cell, "lat_next")
            if ref.npt:
                assert np.abs(ref.cell - refs[o].cell).max() > 1e-4 * np.abs(ref.cell).max()       # the barostat did act
        else:
            assert not out["frac_next"][sl].any() and not out["lat_next"][o].any()
        assert np.abs(out["p"][sl] - before["p"][sl]).max() > 1e-3        # and so did the thermostat and the kick
    return worst


@pytest.mark.parametrize("chain_length", [1, 3, 4])
@pytest.mark.parametrize("npt", [False, True], ids=["nvt", "npt"])
@pytest.mark.parametrize("mode", list(FLAGSETS))
def test_step_kernel_matches_restatement(hip_engine, mode, npt, chain_length):
    flags = FLAGSETS[mode]
    aoff, before, out, *rest = _run_step_kernel(hip_engine, flags, npt, chain_length)
    worst = _check_against_restatement(flags, aoff, before, out, *rest)
    print(mode, "npt" if npt else "nvt", "chain", chain_length, "worst relative errors", worst)


@pytest.mark.parametrize("npt", [False, True], ids=["nvt", "npt"])
def test_step_kernel_nonfinite_replica_is_left_untouched(hip_engine, npt):
    flags, bad = ABSORB | KICK2 | START, 2
    aoff, before, out, *rest = _run_step_kernel(hip_engine, flags, npt, 3, nan_replica=bad)
    sl = slice(aoff[bad], aoff[bad + 1])
    assert list(out["si"][bad]) == [STEPS0[bad], 1, 0, 0]                      # NONFINITE, the step is not counted
    for k in ("r", "p", "f"):
        assert np.array_equal(out[k][sl], before[k][sl]), k
    assert np.array_equal(out["sd"][bad], before["sd"][bad])
    assert np.array_equal(out["nhc"][bad], before["nhc"][bad])                 # the chains did not move either
    assert not out["frac_next"][sl].any() and not out["lat_next"][bad].any()
    _check_against_restatement(flags, aoff, before, out, *rest, skip=(bad,))   # its neighbours step as usual


def test_entry_points_refuse_what_they_cannot_run(hip_engine):
    from chgnet_amd import _lib

    one, ints, floats, offs = np.zeros(64), np.zeros(64, np.int32), np.zeros(64, np.float32), np.array([0, 2], np.int32)
    ip, dp = ints.ctypes.data_as(_lib.c_int_p), one.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    fp, aoff = floats.ctypes.data_as(_lib.c_float_p), offs.ctypes.data_as(_lib.c_int_p)
    kw = dict(fixcm=0, dt=0.2, temperature=300.0, taut=20.0, taup=200.0, pressure=0.0, compressibility=0.0, kB=md_ref.KB, stress_weight=SW,
              loginterval=1, ring_frames=1, log_stress=1, log_crystal_fea=0, r_atom=6.0, r_bond=3.0, numerical_tol=1e-8)
    lib, h = hip_engine.lib, hip_engine.handle

    def step(fn, prm, *extra):
        return fn(h, ctypes.byref(prm), 1, aoff, START, dp, dp, dp, dp, dp, ip, fp, fp, fp, dp, dp, *extra)

    for code in (NVT_NHC, NPT_NHC):                                            # the plain entry point has no chain length to give
        assert step(lib.chg_test_md_step, _lib.MdParams(ensemble=code, **kw)) != 0
    assert step(lib.chg_test_md_step_nhc, _lib.MdParams(ensemble=1, **kw), 3, dp) != 0
    for m in (0, 5, -1):
        assert step(lib.chg_test_md_step_nhc, _lib.MdParams(ensemble=NVT_NHC, **kw), m, dp) != 0
    assert step(lib.chg_test_md_step_nhc, _lib.MdParams(ensemble=NVT_NHC, **dict(kw, temperature=0.0)), 3, dp) != 0


# ---- 2. MolecularDynamics against the restatement driven by predict_structure ----------------------------------------------------------
@pytest.mark.parametrize("ensemble", ["nvt", "npt"])
@pytest.mark.parametrize("struct", [("limno2", (1, 1, 1)), ("li9co7o16", (2, 2, 2))])
def test_run_matches_host_loop(model, calc, struct, ensemble):
    from chgnet_amd.dynamics import ATOMIC_MASSES, MolecularDynamics

    s = _structure(struct[0], struct[1], rattle=0.05, seed=3)
    steps = 20
    md = MolecularDynamics(s, model=calc, ensemble=ensemble, thermostat="Nose-Hoover-Chain", temperature=600.0, starting_temperature=200.0,
                           timestep=1.0, taut=50.0, taup=500.0, pressure=0.5, loginterval=1, seed=7)
    traj = md.run(steps)
    p0 = md.traj.momenta[0]
    m = ATOMIC_MASSES[s.atomic_numbers]
    assert np.abs((p0).sum(axis=0)).max() < 1e-12 * np.abs(p0).sum()           # removed once, when the atoms were set
    ref = nhc_ref.NHCRef(s.frac_coords @ s.lattice.matrix, s.lattice.matrix, m, p0, npt=ensemble == "npt", dt=1.0 * md_ref.FS,
                         temperature_k=600.0, taut=50.0 * md_ref.FS, taup=500.0 * md_ref.FS, pressure=0.5 * md_ref.GPA, chain_length=3,
                         calc=_host_calc(model, s.atomic_numbers))
    frames = ref.run(steps)
    assert len(traj) == len(frames) == len(traj.conserved) == steps + 1
    assert ref.n_evals == steps + 1                                            # one evaluation per step, NPT included
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
    print("nhc", ensemble, struct, errs, "T first / last", traj.temperatures[0], traj.temperatures[-1], "cell moved by", moved, "A")
    assert errs["pos"] < 2e-5 and errs["cell"] < 2e-5, errs
    assert errs["mom"] < 1e-4 and errs["e"] < 1e-4 and errs["T"] < 0.05 and errs["H"] < 1e-4, errs
    st = md.thermostat_state
    assert set(st) == {"v", "eta", "vb", "xi", "veps"} and len(st["v"]) == 3
    assert np.abs(st["v"] - ref.v).max() < 1e-4 * np.abs(ref.v).max() and np.abs(st["eta"] - ref.eta).max() < 1e-4 * np.abs(ref.eta).max()
    if ensemble == "npt":
        assert moved > 1e-4 and abs(st["veps"] - ref.veps) < 1e-4 * abs(ref.veps)
    else:
        assert moved == 0.0 and st["veps"] == 0.0 and not st["vb"].any()


# ---- 3. batch slots and split runs ------------------------------------------------------------------------------------------------------
NHC_KW = dict(thermostat="Nose-Hoover-Chain", temperature=500.0, starting_temperature=400.0, timestep=2.0, taut=40.0, taup=400.0, pressure=0.5)


def _same(ta, tb, what):
    assert ta.steps == tb.steps, what
    assert np.array_equal(ta.momenta[0], tb.momenta[0]), what
    for k in range(len(ta)):
        assert np.abs(ta.atom_positions[k] - tb.atom_positions[k]).max() < 2e-5, (what, k)
        assert np.abs(ta.cells[k] - tb.cells[k]).max() < 2e-5, (what, k)
        assert abs(ta.temperatures[k] - tb.temperatures[k]) < 0.5, (what, k)
        assert abs(ta.conserved[k] - tb.conserved[k]) < 1e-4 * len(ta.atomic_numbers), (what, k)


def _same_state(a, b, what):
    for key in ("v", "eta", "vb", "xi"):
        assert np.abs(a[key] - b[key]).max() <= 1e-4 * max(np.abs(a[key]).max(), 1e-300), (what, key)
    assert abs(a["veps"] - b["veps"]) <= 1e-4 * abs(a["veps"]), what


@pytest.mark.parametrize("ensemble", ["nvt", "npt"])
def test_batch_equals_single(calc, ensemble):
    from chgnet_amd.dynamics import MolecularDynamics

    structs = [_structure("limno2", rattle=0.05, seed=1), _structure("li9co7o16", rattle=0.03, seed=2),
               _structure("limno2", (2, 2, 1), rattle=0.04, seed=3), _structure("li9co7o16", (2, 1, 1), rattle=0.02, seed=4)]
    seeds = [11, 12, 13, 14]
    kw = dict(NHC_KW, ensemble=ensemble, loginterval=3)
    batch = MolecularDynamics.run_batch(structs, 15, seeds=seeds, model=calc, **kw)
    turned = MolecularDynamics.run_batch(structs[::-1], 15, seeds=seeds[::-1], model=calc, **kw)[::-1]
    for b, t, s, sd in zip(batch, turned, structs, seeds):
        md = MolecularDynamics(s, model=calc, seed=sd, **kw)
        t1 = md.run(15)
        assert b["status"] == "RUNNING" and b["n_steps"] == 15
        assert b["trajectory"].steps == [0, 3, 6, 9, 12, 15] and len(b["trajectory"].conserved) == 6
        _same(b["trajectory"], t1, "batch vs alone")
        _same(t["trajectory"], t1, "another slot vs alone")
        _same_state(b["thermostat_state"], md.thermostat_state, "batch vs alone")
        _same_state(t["thermostat_state"], md.thermostat_state, "another slot vs alone")


@pytest.mark.parametrize("ensemble", ["nvt", "npt"])
def test_split_run_equals_one_run(calc, ensemble):
    from chgnet_amd.dynamics import MolecularDynamics

    s = _structure("limno2", (2, 2, 1), rattle=0.04, seed=5)
    one = MolecularDynamics(s, model=calc, seed=21, ensemble=ensemble, **NHC_KW)
    t_one = one.run(12)
    two = MolecularDynamics(s, model=calc, seed=21, ensemble=ensemble, **NHC_KW)
    two.run(6)
    half = copy.deepcopy(two.thermostat_state)
    t_two = two.run(6)
    assert t_one.steps == t_two.steps == list(range(13))
    _same(t_one, t_two, "run(6); run(6) vs run(12)")
    _same_state(one.thermostat_state, two.thermostat_state, "run(6); run(6) vs run(12)")
    assert np.abs(half["eta"] - two.thermostat_state["eta"]).max() > 0           # the chains went on from where they were
    two.set_atoms(s)                                                             # a new handle: zeroed chains
    assert two.thermostat_state is None
    two.run(0)
    assert not two.thermostat_state["v"].any() and not two.thermostat_state["eta"].any() and two.thermostat_state["veps"] == 0.0


# ---- 4. the cell only scales, nothing pushes the centre of mass --------------------------------------------------------------------------
def test_cell_shape_and_total_momentum(calc):
    from chgnet_amd.dynamics import MolecularDynamics

    s = _structure("li9co7o16", (2, 1, 1), rattle=0.03, seed=8)
    md = MolecularDynamics(s, model=calc, seed=5, ensemble="npt", **dict(NHC_KW, taup=100.0))
    traj = md.run(30)
    h0 = s.lattice.matrix
    assert abs(h0[1, 0]) + abs(h0[2, 0]) + abs(h0[2, 1]) > 0.1 or abs(h0[0, 1]) + abs(h0[0, 2]) + abs(h0[1, 2]) > 0.1      # not diagonal
    lams = []
    for c in traj.cells:
        lam = np.vdot(c, h0) / np.vdot(h0, h0)
        lams.append(lam)
        assert np.abs(c - lam * h0).max() <= 1e-13 * np.abs(c).max()         # 30 multiplications of 9 numbers by one factor each
    print("npt cell scale over 30 steps: min", min(lams), "max", max(lams))
    assert max(lams) - min(lams) > 1e-4
    for p in traj.momenta:
        assert np.abs(p.sum(axis=0)).max() < 1e-6 * np.abs(p).sum()          # no per-step removal: sum f = 0 to the fp32 rounding


# ---- 5. drift of the conserved energy on the real potential ------------------------------------------------------------------------------
def test_conserved_energy_drifts_no_more_than_nve(calc):
    """Same structure, time step and step count on the NVE path and with the chain thermostat: the standard deviation of H (NVT chains)
    against that of Epot + Ekin (NVE).  The chains add only work terms built from the same fp32 forces, so a ratio above 4 would be a
    bookkeeping error, not noise.  NPT is recorded, not asserted: the fp32 stress is not the exact volume derivative of the fp32
    energy.  The figures are printed, and appended to the file CHGNET_MD_NHC_PROBE names when it is set (profiles/md_nhc_probe.jsonl)."""
    from chgnet_amd.dynamics import MolecularDynamics

    s = _structure("limno2", (2, 2, 1), rattle=0.04, seed=9)
    kw = dict(model=calc, temperature=300.0, starting_temperature=300.0, timestep=1.0, seed=3)
    steps = 200
    nve = MolecularDynamics(s, ensemble="nve", **kw).run(steps)
    etot = np.array(nve.energies) + np.array(nve.kinetic_energies)
    nvt = MolecularDynamics(s, ensemble="nvt", thermostat="Nose-Hoover-Chain", **kw).run(steps)
    npt = MolecularDynamics(s, ensemble="npt", thermostat="Nose-Hoover-Chain", pressure=0.0, **kw).run(steps)
    rec = {"leg": "drift", "structure": "limno2 2x2x1", "atoms": len(s), "steps": steps, "timestep_fs": 1.0, "nve_etot_std_eV": float(etot.std()),
           "nvt_nhc_H_std_eV": float(np.std(nvt.conserved)), "npt_nhc_H_std_eV": float(np.std(npt.conserved)),
           "nve_etot_drift_eV": float(etot[-1] - etot[0]), "nvt_nhc_H_drift_eV": float(nvt.conserved[-1] - nvt.conserved[0]),
           "npt_nhc_H_drift_eV": float(npt.conserved[-1] - npt.conserved[0])}
    print(json.dumps(rec))
    if os.environ.get("CHGNET_MD_NHC_PROBE"):
        with open(os.environ["CHGNET_MD_NHC_PROBE"], "a") as fh:
            fh.write(json.dumps(rec) + "\n")
    assert len(nvt.conserved) == steps + 1 and nve.conserved == []
    assert rec["nvt_nhc_H_std_eV"] <= 4 * rec["nve_etot_std_eV"], rec


# ---- 6. scale -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ensemble", ["nvt", "npt"])
def test_large_batch_64_replicas(calc, ensemble):
    from chgnet_amd.dynamics import MolecularDynamics

    structs = [_structure("li9co7o16", (2, 2, 2), rattle=0.02, seed=100 + i) for i in range(64)]
    out = MolecularDynamics.run_batch(structs, 5, seeds=list(range(64)), model=calc, ensemble=ensemble, thermostat="Nose-Hoover-Chain",
                                      temperature=300.0, starting_temperature=300.0, loginterval=5)
    assert len(out) == 64
    for o in out:
        assert o["status"] == "RUNNING" and o["n_steps"] == 5
        assert len(o["trajectory"]) == 2 and len(o["trajectory"].conserved) == 2
        assert np.all(np.isfinite(o["final_structure"].frac_coords)) and np.all(np.isfinite(o["momenta"]))
        assert np.all(np.isfinite(o["trajectory"].temperatures)) and np.all(np.isfinite(o["trajectory"].conserved))
