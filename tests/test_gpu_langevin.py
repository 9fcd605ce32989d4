"""Langevin NVT molecular dynamics on the MI355X: the step kernel against the float64 restatement (tests/langevin_ref.py) on every
flag set, MolecularDynamics(thermostat="Langevin") against the restatement driven by predict_structure with the same noise,
run_batch == run per replica, split runs, distinct seeds, thermalisation of 64 replicas to the canonical kinetic energy, and a
64 x 256-atom batch."""

from __future__ import annotations

import copy
import ctypes

import numpy as np
import pytest

import langevin_ref
import md_ref
from conftest import load_case

pytestmark = pytest.mark.gpu

LANGEVIN = 4
ABSORB, KICK2, START = 1, 2, 4
SW = 1.0 / 160.21766208


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
SIZES = [1, 5, 17, 300, 40]                # 300: rows beyond one pass of the workgroup; 1: COM removal leaves p = 0
SEEDS = [7, (1 << 32) + 12345, 0, (1 << 64) - 1, 99]
STEPS0 = [0, 70000, 3, 49, 11]             # si[0] on entry: the noise counter (one above 2^16)
FLAGSETS = {"start_only": START, "finish_only": ABSORB | KICK2, "finish_start": ABSORB | KICK2 | START}


def _run_step_kernel(hip_engine, flags, fixcm, friction, nan_replica=None):
    """One launch of the step kernel on five replicas; returns (inputs, outputs, restatement replicas after the same launch)."""
    from chgnet_amd import _lib

    rng = np.random.default_rng(1000 * flags + 10 * fixcm + (1 if friction > 0 else 0))
    dt, t0 = 2.0 * md_ref.FS, 300.0
    refs, cached, new_f = [], [], []
    for n, seed, k in zip(SIZES, SEEDS, STEPS0):
        cell = np.diag(rng.uniform(5, 9, 3)) + rng.normal(0, 0.5, (3, 3))
        m = rng.uniform(1.0, 200.0, n)
        ref = langevin_ref.LangevinRef(rng.random((n, 3)) @ cell, cell, m, rng.normal(0, 0.3, (n, 3)) * np.sqrt(m)[:, None], dt=dt,
                                       temperature_k=t0, friction=friction, seed=seed, fixcm=bool(fixcm))
        ref.nsteps = k
        refs.append(ref)
        cached.append(rng.normal(0, 0.5, (n, 3)))
        new_f.append(rng.normal(0, 0.5, (n, 3)).astype(np.float32))
    B = len(SIZES)
    aoff = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    r = np.ascontiguousarray(np.concatenate([x.r for x in refs]))
    p = np.ascontiguousarray(np.concatenate([x.p for x in refs]))
    f = np.ascontiguousarray(np.concatenate(cached))
    m = np.ascontiguousarray(np.concatenate([x.m for x in refs]))
    sd = np.zeros((B, 40))
    si = np.zeros((B, 4), np.int32)
    for o, x in enumerate(refs):
        sd[o, :9] = x.cell.ravel()
        sd[o, 9:18] = np.linalg.inv(x.cell).ravel()
        sd[o, 19] = md_ref.kinetic_energy(x.p, x.m)
        sd[o, 20] = md_ref.temperature(x.p, x.m)
        si[o] = [x.nsteps, 0, 0, 0]
    energy = rng.normal(-100, 10, B).astype(np.float32)
    force = np.ascontiguousarray(np.concatenate(new_f), np.float32)
    if nan_replica is not None:
        force[aoff[nan_replica] + 2, 1] = np.nan
    stress = np.ascontiguousarray(rng.normal(0, 3.0, (B, 3, 3)), np.float32)
    frac_next = np.zeros_like(r)
    lat_next = np.zeros((B, 3, 3))
    seeds = np.array(SEEDS, np.uint64)
    before = {k: v.copy() for k, v in dict(r=r, p=p, f=f, sd=sd, si=si).items()}
    prm = _lib.MdParams(ensemble=LANGEVIN, fixcm=fixcm, dt=dt, temperature=t0, taut=0.0, taup=0.0, pressure=0.0, compressibility=0.0,
                        kB=md_ref.KB, stress_weight=SW, loginterval=1, ring_frames=1, log_stress=1, log_crystal_fea=0, r_atom=6.0,
                        r_bond=3.0, numerical_tol=1e-8)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    hip_engine._check(hip_engine.lib.chg_test_md_step_langevin(
        hip_engine.handle, ctypes.byref(prm), B, aoff.ctypes.data_as(_lib.c_int_p), flags, dp(r), dp(p), dp(f), dp(m), dp(sd),
        si.ctypes.data_as(_lib.c_int_p), fp(energy), fp(force), fp(stress), dp(frac_next), dp(lat_next), friction,
        seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
    out = dict(r=r, p=p, f=f, sd=sd, si=si, frac_next=frac_next, lat_next=lat_next)
    return aoff, before, out, refs, cached, new_f, stress


def _check_against_restatement(flags, aoff, out, refs, cached, new_f, stress, skip=()):
    worst = {}

    def close(got, want, what, scale=None):
        scale = (np.abs(want).max() if scale is None else scale) + 1e-300
        err = np.abs(got - want).max() / scale
        worst[what] = max(worst.get(what, 0.0), err)
        assert err <= 1e-12, (what, err)

    for o, ref in enumerate(refs):
        if o in skip:
            continue
        sl = slice(aoff[o], aoff[o + 1])
        fcache, steps, ek = cached[o], ref.nsteps, None
        if flags & ABSORB:
            fcache = new_f[o].astype(np.float64)
            ref.second_half(fcache)
            steps += 1
            ek = (md_ref.kinetic_energy(ref.p, ref.m), md_ref.temperature(ref.p, ref.m))
        pscale = np.abs(ref.p).max()
        if flags & START:
            free = copy.deepcopy(ref)            # the momenta before the centre-of-mass removal set the rounding scale of p
            free.fixcm = False
            free.first_half(fcache)
            ref.first_half(fcache)
            pscale = max(np.abs(free.p).max(), np.abs(ref.p).max())
        close(out["r"][sl], ref.r, "r")
        close(out["p"][sl], ref.p, "p", pscale)
        close(out["f"][sl], fcache, "f")
        close(out["sd"][o, :9].reshape(3, 3), ref.cell, "cell")
        close(out["sd"][o, 9:18].reshape(3, 3), np.linalg.inv(ref.cell), "cell^-1")
        assert list(out["si"][o, :3]) == [steps, 0, 0], (o, out["si"][o])
        if flags & KICK2:
            close(out["sd"][o, 19], ek[0], "ekin")
            close(out["sd"][o, 20], ek[1], "T")
        if flags & START:
            close(out["frac_next"][sl], ref.r @ np.linalg.inv(ref.cell), "frac_next")
            close(out["lat_next"][o], ref.cell, "lat_next")
            if ref.fixcm:
                assert np.abs(out["p"][sl].sum(0)).max() <= 1e-12 * np.abs(free.p).sum(), o
                if len(ref.m) == 1:
                    assert np.abs(out["p"][sl]).max() <= 1e-12 * pscale
        if flags & ABSORB:
            close(out["sd"][o, 21:30].reshape(3, 3), stress[o].astype(np.float64) * SW, "stress")
    return worst


@pytest.mark.parametrize("friction_fs", [0.0, 0.01])
@pytest.mark.parametrize("fixcm", [0, 1])
@pytest.mark.parametrize("mode", list(FLAGSETS))
def test_step_kernel_matches_restatement(hip_engine, mode, fixcm, friction_fs):
    flags = FLAGSETS[mode]
    aoff, before, out, refs, cached, new_f, stress = _run_step_kernel(hip_engine, flags, fixcm, friction_fs / md_ref.FS)
    quiet = copy.deepcopy(refs[3])               # the same launch without friction: velocity Verlet
    quiet.friction = 0.0
    worst = _check_against_restatement(flags, aoff, out, refs, cached, new_f, stress)
    print(mode, "fixcm", fixcm, "friction", friction_fs, "worst relative errors", worst)
    if friction_fs > 0 and flags & START:        # the noise did act (its scale here is sqrt(0.04 m kB T) ~ 0.1)
        if flags & ABSORB:
            quiet.second_half(new_f[3].astype(np.float64))
        quiet.first_half(new_f[3].astype(np.float64) if flags & ABSORB else cached[3])
        assert np.abs(out["p"][aoff[3]:aoff[4]] - quiet.p).max() > 1e-3


def test_step_kernel_nonfinite_replica_is_left_untouched(hip_engine):
    flags, bad = ABSORB | KICK2 | START, 2
    aoff, before, out, refs, cached, new_f, stress = _run_step_kernel(hip_engine, flags, 1, 0.01 / md_ref.FS, nan_replica=bad)
    sl = slice(aoff[bad], aoff[bad + 1])
    assert list(out["si"][bad]) == [STEPS0[bad], 1, 0, 0]                      # NONFINITE, the step is not counted
    for k in ("r", "p", "f"):
        assert np.array_equal(out[k][sl], before[k][sl]), k
    assert np.array_equal(out["sd"][bad], before["sd"][bad])
    assert not out["frac_next"][sl].any() and not out["lat_next"][bad].any()
    _check_against_restatement(flags, aoff, out, refs, cached, new_f, stress, skip=(bad,))      # its neighbours step as usual


# ---- 2. MolecularDynamics against the restatement driven by predict_structure, same noise on both sides -----------------------------
@pytest.mark.parametrize("struct", [("limno2", (1, 1, 1)), ("li9co7o16", (2, 2, 2))])
def test_run_matches_host_loop(model, calc, struct):
    from chgnet_amd.dynamics import ATOMIC_MASSES, MolecularDynamics

    s = _structure(struct[0], struct[1], rattle=0.05, seed=3)
    steps, friction = 20, 0.02
    md = MolecularDynamics(s, model=calc, ensemble="nvt", thermostat="Langevin", temperature=600.0, starting_temperature=200.0,
                           friction=friction, timestep=1.0, loginterval=1, seed=7)
    assert md.thermostat_seed == 7
    traj = md.run(steps)
    p0 = md.traj.momenta[0]
    m = ATOMIC_MASSES[s.atomic_numbers]
    ref = langevin_ref.LangevinRef(s.frac_coords @ s.lattice.matrix, s.lattice.matrix, m, p0, dt=1.0 * md_ref.FS, temperature_k=600.0,
                                   friction=friction / md_ref.FS, seed=7, fixcm=True, calc=_host_calc(model, s.atomic_numbers))
    frames = ref.run(steps)
    assert len(traj) == len(frames) == steps + 1
    assert ref.n_evals == steps + 1                                            # one evaluation per step
    assert np.array_equal(traj.cells[0], s.lattice.matrix)
    assert np.abs(traj.atom_positions[0] - frames[0]["positions"]).max() < 1e-12
    assert np.array_equal(traj.momenta[0], frames[0]["momenta"])
    errs = {"pos": 0.0, "mom": 0.0, "cell": 0.0, "e": 0.0, "T": 0.0}
    pscale = max(np.abs(fr["momenta"]).max() for fr in frames)
    for k, fr in enumerate(frames):
        errs["pos"] = max(errs["pos"], np.abs(traj.atom_positions[k] - fr["positions"]).max())
        errs["mom"] = max(errs["mom"], np.abs(traj.momenta[k] - fr["momenta"]).max() / pscale)
        errs["cell"] = max(errs["cell"], np.abs(traj.cells[k] - fr["cell"]).max())
        errs["e"] = max(errs["e"], abs(traj.energies[k] - fr["epot"]) / len(s))
        errs["T"] = max(errs["T"], abs(traj.temperatures[k] - fr["temperature"]))
    print("langevin", struct, errs, "T first / last", traj.temperatures[0], traj.temperatures[-1])
    # both sides draw the same noise: what is left is the fp32 force noise that test_gpu_md.py::test_run_matches_host_loop bounds
    assert errs["pos"] < 2e-5 and errs["cell"] < 2e-5, errs
    assert errs["mom"] < 1e-4 and errs["e"] < 1e-4 and errs["T"] < 0.05, errs


# ---- 3. the noise is a function of (seed, atom, step): batch slots, split runs, seeds ------------------------------------------------
LANGEVIN_KW = dict(ensemble="nvt", thermostat="Langevin", temperature=500.0, starting_temperature=400.0, timestep=2.0, friction=0.01)


def _same(ta, tb, what):
    assert ta.steps == tb.steps, what
    assert np.array_equal(ta.momenta[0], tb.momenta[0]), what
    for k in range(len(ta)):
        assert np.abs(ta.atom_positions[k] - tb.atom_positions[k]).max() < 2e-5, (what, k)
        assert np.abs(ta.cells[k] - tb.cells[k]).max() < 2e-5, (what, k)
        assert abs(ta.temperatures[k] - tb.temperatures[k]) < 0.5, (what, k)


def test_batch_equals_single(calc):
    from chgnet_amd.dynamics import MolecularDynamics

    structs = [_structure("limno2", rattle=0.05, seed=1), _structure("li9co7o16", rattle=0.03, seed=2),
               _structure("limno2", (2, 2, 1), rattle=0.04, seed=3), _structure("li9co7o16", (2, 1, 1), rattle=0.02, seed=4)]
    seeds = [11, (1 << 33) + 12, 13, 14]
    kw = dict(LANGEVIN_KW, loginterval=3)
    batch = MolecularDynamics.run_batch(structs, 15, seeds=seeds, model=calc, **kw)
    turned = MolecularDynamics.run_batch(structs[::-1], 15, seeds=seeds[::-1], model=calc, **kw)[::-1]
    for b, t, s, sd in zip(batch, turned, structs, seeds):
        md = MolecularDynamics(s, model=calc, seed=sd, **kw)
        t1 = md.run(15)
        assert b["status"] == "RUNNING" and b["n_steps"] == 15
        assert b["trajectory"].steps == [0, 3, 6, 9, 12, 15]
        _same(b["trajectory"], t1, "batch vs alone")
        _same(t["trajectory"], t1, "another slot vs alone")


def test_split_run_equals_one_run(calc):
    from chgnet_amd.dynamics import MolecularDynamics

    s = _structure("limno2", (2, 2, 1), rattle=0.04, seed=5)
    one = MolecularDynamics(s, model=calc, seed=21, **LANGEVIN_KW)
    t_one = one.run(20)
    two = MolecularDynamics(s, model=calc, seed=21, **LANGEVIN_KW)
    two.run(10)
    t_two = two.run(10)
    assert t_one.steps == t_two.steps == list(range(21))
    _same(t_one, t_two, "run(10); run(10) vs run(20)")


def test_seeds_matter(calc):
    """Same structure, same (zero) initial momenta, two thermostat seeds: after 20 steps at 300 K, 2 fs, 0.01 / fs the positions
    differ by more than 100 times the bar under which trajectories count as equal."""
    from chgnet_amd.dynamics import MolecularDynamics

    s = _structure("limno2", (2, 2, 1), rattle=0.04, seed=6)
    a, b = MolecularDynamics.run_batch([s, s], 20, seeds=[31, 32], model=calc, ensemble="nvt", thermostat="Langevin", temperature=300.0,
                                       timestep=2.0, friction=0.01, loginterval=20)
    assert np.array_equal(a["trajectory"].atom_positions[0], b["trajectory"].atom_positions[0])
    diff = np.abs(a["trajectory"].atom_positions[-1] - b["trajectory"].atom_positions[-1]).max()
    print("two seeds, 20 steps: max position difference", diff, "A")
    assert diff > 2e-3


# ---- 4. physics: the canonical kinetic energy ------------------------------------------------------------------------------------
def test_thermalises_to_the_canonical_kinetic_energy(calc):
    """64 replicas of a 40-atom LiMnO2 cell from 0 K to 600 K: 0.5 fs (keeps BAOAB's O(dt^2) kinetic bias out of the picture), friction
    0.05 / fs, 200 fs = 10 / friction.  With the centre of mass at rest each replica has 3 (n - 1) Gaussian momenta, so the reported
    T = 2 Ekin / (3 n kB) has mean T0 (n - 1) / n and relative width sqrt(2 / (3 (n - 1))); the mean over 64 independent replicas
    must lie within 5 of its standard deviations, 5 sqrt(2 / (3 * 39 * 64)) = 8.2 %."""
    from chgnet_amd.dynamics import MolecularDynamics

    n, R, t0 = 40, 64, 600.0
    structs = [_structure("limno2", (5, 1, 1), rattle=0.02, seed=200 + i) for i in range(R)]
    assert len(structs[0]) == n
    out = MolecularDynamics.run_batch(structs, 400, seeds=[1000 + i for i in range(R)], model=calc, ensemble="nvt", thermostat="Langevin",
                                      temperature=t0, timestep=0.5, friction=0.05, loginterval=400)
    assert all(o["status"] == "RUNNING" and o["n_steps"] == 400 for o in out)
    first = np.array([o["trajectory"].temperatures[0] for o in out])
    last = np.array([o["trajectory"].temperatures[-1] for o in out])
    mean, want = float(last.mean()), t0 * (n - 1) / n
    print("thermalisation: mean T of 64 replicas", mean, "K, expected", want, "K, spread over replicas", float(last.std()), "K")
    assert np.all(first == 0.0)
    assert abs(mean - want) < 5 * np.sqrt(2 / (3 * (n - 1) * R)) * want
    # the total momentum is removed after every noise step; the half kick that follows adds dt/2 sum f, zero to the fp32 rounding
    # of the forces (~1e-6 of sum |f|, and dt/2 sum |f| < sum |p| here).  Without the removal it would wander to ~sum |p| / sqrt(3 n)
    for o in out[:4]:
        assert np.abs(o["momenta"].sum(0)).max() < 1e-6 * np.abs(o["momenta"]).sum()


# ---- 5. scale ---------------------------------------------------------------------------------------------------------------------
def test_large_batch_64_replicas(calc):
    from chgnet_amd.dynamics import MolecularDynamics

    structs = [_structure("li9co7o16", (2, 2, 2), rattle=0.02, seed=100 + i) for i in range(64)]
    out = MolecularDynamics.run_batch(structs, 5, seeds=list(range(64)), model=calc, ensemble="nvt", thermostat="Langevin",
                                      temperature=300.0, starting_temperature=300.0, loginterval=5)
    assert len(out) == 64
    for o in out:
        assert o["status"] == "RUNNING" and o["n_steps"] == 5
        assert len(o["trajectory"]) == 2
        assert np.all(np.isfinite(o["final_structure"].frac_coords)) and np.all(np.isfinite(o["momenta"]))
        assert np.all(np.isfinite(o["trajectory"].temperatures))
