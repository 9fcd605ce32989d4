"""Batched molecular dynamics on the MI355X: the step kernel against the float64 restatement (tests/md_ref.py) for every ensemble,
MolecularDynamics.run against the restatement driven by predict_structure, run_batch == run per replica, NVE energy conservation,
NVT temperature relaxation, NPT compression, and a 64 x 256-atom batch."""

from __future__ import annotations

import ctypes
import zlib

import numpy as np
import pytest

import md_ref
from conftest import load_case

pytestmark = pytest.mark.gpu

ENS = {md_ref.NVE: 0, md_ref.NVT: 1, md_ref.NPT_INHOM: 2, md_ref.NPT_ISO: 3}
ABSORB, KICK2, START = 1, 2, 4
SW = 1.0 / 160.21766208


def _params(ensemble, dt, t0=300.0, taut=None, taup=None, pressure=0.0, kappa=0.0):
    from chgnet_amd import _lib

    return _lib.MdParams(ensemble=ENS[ensemble], fixcm=1, dt=dt, temperature=t0, taut=taut or 100 * dt, taup=taup or 1000 * dt,
                         pressure=pressure, compressibility=kappa, kB=md_ref.KB, stress_weight=SW, loginterval=1, ring_frames=1,
                         log_stress=1, log_crystal_fea=0, r_atom=6.0, r_bond=3.0, numerical_tol=1e-8)


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


# ---- 1. the step kernel on its own ---------------------------------------------------------------------------------------------
def _pack(refs, forces_cached):
    sizes = [len(r.m) for r in refs]
    aoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    r = np.ascontiguousarray(np.concatenate([x.r for x in refs]))
    p = np.ascontiguousarray(np.concatenate([x.p for x in refs]))
    f = np.ascontiguousarray(np.concatenate(forces_cached))
    m = np.ascontiguousarray(np.concatenate([x.m for x in refs]))
    sd = np.zeros((len(refs), 40))
    si = np.zeros((len(refs), 4), np.int32)
    for o, x in enumerate(refs):
        sd[o, :9] = x.cell.ravel()
        sd[o, 9:18] = np.linalg.inv(x.cell).ravel()
        sd[o, 19] = md_ref.kinetic_energy(x.p, x.m)
        sd[o, 20] = md_ref.temperature(x.p, x.m)
        sd[o, 21:30] = x.stress_cached.ravel()
        sd[o, 30:39] = np.einsum("ka,kb,k->ab", x.p, x.p, 1.0 / x.m).ravel()
        si[o] = [x.nsteps, 0, x.phase, 0]
    return aoff, r, p, f, m, sd, si


KERNEL_CASES = [(e, m) for e in (md_ref.NVE, md_ref.NVT, md_ref.NPT_INHOM, md_ref.NPT_ISO) for m in ("finish_start", "start_only", "finish_only")]
KERNEL_CASES += [(md_ref.NPT_INHOM, "npt_mid"), (md_ref.NPT_ISO, "npt_mid")]     # phase 1 exists only for NPT


@pytest.mark.parametrize(("ensemble", "mode"), KERNEL_CASES)
def test_step_kernel_matches_restatement(hip_engine, ensemble, mode):
    from chgnet_amd import _lib

    npt = ensemble in (md_ref.NPT_INHOM, md_ref.NPT_ISO)
    rng = np.random.default_rng(zlib.crc32(f"{ensemble}/{mode}".encode()))
    sizes = [5, 300, 17, 1, 40]          # 300: rows beyond one pass of the workgroup; 1: a single atom
    dt = 2.0 * md_ref.FS
    kappa, pressure = 1.0 / (80.0 / 160.2176), 2.0 * md_ref.GPA
    refs, cached, new_f, new_s = [], [], [], []
    for k, n in enumerate(sizes):
        cell = np.diag(rng.uniform(5, 9, 3)) + rng.normal(0, 0.5, (3, 3))
        ref = md_ref.MDRef(rng.random((n, 3)) @ cell, cell, rng.uniform(1.0, 200.0, n), ensemble=ensemble, dt=dt, temperature_k=300.0,
                           pressure=pressure, compressibility=kappa)
        ref.p = rng.normal(0, 0.3, (n, 3)) * np.sqrt(ref.m)[:, None]
        if k == 2:
            ref.p[:] = 0.0                 # T = 0: lambda clamps to 1.1
        if k == 4:
            ref.p *= 0.02                  # cold: lambda clamps to 1.1 as well
        ref.nsteps = int(rng.integers(0, 50))
        ref.phase = 1 if mode == "npt_mid" else 0
        s = rng.normal(0, 0.02, (3, 3))
        ref.stress_cached = (s + s.T) / 2
        refs.append(ref)
        cached.append(rng.normal(0, 0.5, (n, 3)))
        new_f.append(rng.normal(0, 0.5, (n, 3)).astype(np.float32))
        s2 = rng.normal(0, 3.0, (3, 3))
        new_s.append(((s2 + s2.T) / 2).astype(np.float32))
    aoff, r, p, f, m, sd, si = _pack(refs, cached)
    energy = rng.normal(-100, 10, len(sizes)).astype(np.float32)
    force = np.ascontiguousarray(np.concatenate(new_f), np.float32)
    stress = np.ascontiguousarray(np.stack(new_s), np.float32)
    frac_next = np.zeros_like(r)
    lat_next = np.zeros((len(sizes), 3, 3))
    flags = {"finish_start": ABSORB | KICK2 | START, "start_only": START, "finish_only": ABSORB | KICK2, "npt_mid": ABSORB}[mode]
    prm = _params(ensemble, dt, pressure=pressure, kappa=kappa)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    hip_engine._check(hip_engine.lib.chg_test_md_step(hip_engine.handle, ctypes.byref(prm), len(sizes), aoff.ctypes.data_as(_lib.c_int_p), flags,
                                                      dp(r), dp(p), dp(f), dp(m), dp(sd), si.ctypes.data_as(_lib.c_int_p), fp(energy), fp(force),
                                                      fp(stress), dp(frac_next), dp(lat_next)))

    def close(got, want, what):
        scale = np.abs(want).max() + 1e-300
        assert np.abs(got - want).max() <= 1e-12 * scale, (what, np.abs(got - want).max() / scale)

    for o, ref in enumerate(refs):
        sl = slice(aoff[o], aoff[o + 1])
        fcache = cached[o]
        writes_next, phase, steps = False, ref.phase, ref.nsteps
        if flags & ABSORB:
            fcache = new_f[o].astype(np.float64)
            stress_now = new_s[o].astype(np.float64) * SW
            if ref.phase == 1:
                ref.first_half(fcache)
                writes_next, phase = True, 0
            else:
                ref.second_half(fcache)
                steps += 1
                ek = (md_ref.kinetic_energy(ref.p, ref.m), md_ref.temperature(ref.p, ref.m))    # before the next step's lambda
        else:
            stress_now = ref.stress_cached
        if flags & START and not (flags & ABSORB and ref.phase == 1):
            if ensemble != md_ref.NVE:
                ref.scale_velocities()
            if npt:
                ref.scale_positions_and_cell(stress_now)
                phase = 1
            else:
                ref.first_half(fcache)
            writes_next = True
        close(r[sl], ref.r, "r")
        close(p[sl], ref.p, "p")
        close(f[sl], fcache, "f")
        close(sd[o, :9].reshape(3, 3), ref.cell, "cell")
        close(sd[o, 9:18].reshape(3, 3), np.linalg.inv(ref.cell), "cell^-1")
        assert list(si[o, :3]) == [steps, 0, phase], (o, si[o])
        if flags & KICK2:
            close(sd[o, 19], ek[0], "ekin")
            close(sd[o, 20], ek[1], "T")
        if writes_next:
            close(frac_next[sl], ref.r @ np.linalg.inv(ref.cell), "frac_next")
            close(lat_next[o], ref.cell, "lat_next")
        if flags & ABSORB:
            close(sd[o, 21:30].reshape(3, 3), stress_now, "stress")


# ---- 2. MolecularDynamics.run against the restatement driven by predict_structure -------------------------------------------------
def _host_calc(model, z):
    from chgnet_amd.graph.structure import Lattice, Structure

    def calc(r, cell):
        pred = model.predict_structure(Structure(Lattice(cell), z, r @ np.linalg.inv(cell)), task="efs")
        e = float(pred["e"]) * (len(z) if model.is_intensive else 1)
        return e, np.asarray(pred["f"], np.float64), np.asarray(pred["s"], np.float64) * SW
    return calc


CASES = {"nve": dict(ensemble="nve", starting_temperature=300.0),
         "nvt": dict(ensemble="nvt", temperature=600.0, starting_temperature=200.0, taut=20.0),
         "nvt_cold": dict(ensemble="nvt", temperature=300.0),
         "npt_inhom": dict(ensemble="npt", thermostat="Berendsen_inhomogeneous", temperature=300.0, starting_temperature=300.0,
                           pressure=5.0, bulk_modulus=100.0, taup=200.0),
         "npt_iso": dict(ensemble="npt", thermostat="npt_berendsen", temperature=300.0, starting_temperature=300.0, pressure=5.0,
                         bulk_modulus=100.0, taup=200.0)}
REF_KIND = {"nve": md_ref.NVE, "nvt": md_ref.NVT, "nvt_cold": md_ref.NVT, "npt_inhom": md_ref.NPT_INHOM, "npt_iso": md_ref.NPT_ISO}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("struct", [("limno2", (1, 1, 1)), ("li9co7o16", (2, 2, 2))])
def test_run_matches_host_loop(model, calc, case, struct):
    from chgnet_amd.dynamics import ATOMIC_MASSES, MolecularDynamics

    s = _structure(struct[0], struct[1], rattle=0.05, seed=3)
    kw = dict(CASES[case])
    steps = 20
    md = MolecularDynamics(s, model=calc, timestep=1.0, loginterval=1, seed=7, **kw)
    traj = md.run(steps)
    p0 = md.traj.momenta[0]
    m = ATOMIC_MASSES[s.atomic_numbers]
    dt = 1.0 * md_ref.FS
    ref = md_ref.MDRef(s.frac_coords @ s.lattice.matrix, s.lattice.matrix, m, p0, ensemble=REF_KIND[case], dt=dt,
                       temperature_k=kw.get("temperature", 300.0), taut=kw["taut"] * md_ref.FS if "taut" in kw else None,
                       taup=kw["taup"] * md_ref.FS if "taup" in kw else None, pressure=kw.get("pressure", 1.01325e-4) * md_ref.GPA,
                       compressibility=1.0 / (kw["bulk_modulus"] / 160.2176) if "bulk_modulus" in kw else None,
                       calc=_host_calc(model, s.atomic_numbers))
    frames = ref.run(steps)
    assert len(traj) == len(frames) == steps + 1
    # frame 0: the given configuration and the drawn momenta, exactly; the evaluation to the engine's fp32
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
    print(case, struct, errs, "n_evals", ref.n_evals)
    # the engine's fp32 forces carry ~1e-6 relative noise (atomic accumulation order); over 20 steps of 1 fs that moves atoms by
    # ~dt^2 / m * |dF| * steps^2 ~ 1e-7 A (measured: <= 1e-7 A, momenta <= 1e-6 of their scale).  The bars leave two orders on top
    assert errs["pos"] < 2e-5 and errs["cell"] < 2e-5, errs
    assert errs["mom"] < 1e-4 and errs["e"] < 1e-4 and errs["T"] < 0.05, errs
    if case.startswith("npt"):
        assert ref.n_evals == 2 * steps + 1


# ---- 3. run_batch == run per replica ----------------------------------------------------------------------------------------------
def test_batch_equals_single(calc):
    from chgnet_amd.dynamics import MolecularDynamics

    structs = [_structure("limno2", rattle=0.05, seed=1), _structure("li9co7o16", rattle=0.03, seed=2),
               _structure("limno2", (2, 2, 1), rattle=0.04, seed=3), _structure("li9co7o16", (2, 1, 1), rattle=0.02, seed=4)]
    seeds = [11, 12, 13, 14]
    kw = dict(ensemble="npt", thermostat="Berendsen_inhomogeneous", temperature=500.0, starting_temperature=400.0, timestep=2.0,
              pressure=1.0, bulk_modulus=120.0, loginterval=3)
    batch = MolecularDynamics.run_batch(structs, 15, seeds=seeds, model=calc, **kw)
    for b, s, sd in zip(batch, structs, seeds):
        md = MolecularDynamics(s, model=calc, seed=sd, **kw)
        t1 = md.run(15)
        tb = b["trajectory"]
        assert b["status"] == "RUNNING" and b["n_steps"] == 15
        assert tb.steps == t1.steps == [0, 3, 6, 9, 12, 15]
        assert np.array_equal(tb.momenta[0], t1.momenta[0])
        for k in range(len(t1)):
            assert np.abs(tb.atom_positions[k] - t1.atom_positions[k]).max() < 2e-5
            assert np.abs(tb.cells[k] - t1.cells[k]).max() < 2e-5
            assert abs(tb.temperatures[k] - t1.temperatures[k]) < 0.5


# ---- 4. physics: NVE conservation, NVT relaxation, NPT compression -----------------------------------------------------------------
def test_nve_energy_drift(calc):
    from chgnet_amd.dynamics import MolecularDynamics

    s = _structure("li9co7o16", (2, 2, 2), rattle=0.02, seed=5)
    md = MolecularDynamics(s, model=calc, ensemble="nve", starting_temperature=300.0, timestep=0.5, loginterval=10, seed=1)
    tr = md.run(200)
    etot = np.array(tr.energies) + np.array(tr.kinetic_energies)
    drift = np.abs(etot - etot[0]).max() / len(s)
    print("NVE drift eV/atom", drift, "T", tr.temperatures[0], tr.temperatures[-1])
    assert len(tr) == 21
    assert drift < 2e-3                      # eV/atom over 100 fs at 0.5 fs


def test_nvt_relaxes_to_target(calc):
    from chgnet_amd.dynamics import MolecularDynamics

    s = _structure("li9co7o16", (2, 2, 2), rattle=0.02, seed=6)
    md = MolecularDynamics(s, model=calc, ensemble="nvt", temperature=900.0, starting_temperature=100.0, timestep=1.0, taut=10.0,
                           loginterval=5, seed=2)
    tr = md.run(150)
    late = float(np.mean(tr.temperatures[-10:]))
    print("NVT T", tr.temperatures[0], late)
    assert abs(tr.temperatures[0] - 100.0) < 1e-6
    assert abs(late - 900.0) < 0.25 * 900.0


def test_npt_compresses_under_pressure(calc):
    from chgnet_amd.dynamics import MolecularDynamics

    for thermostat in ("Berendsen_inhomogeneous", "npt_berendsen"):
        s = _structure("li9co7o16", (2, 2, 2), rattle=0.02, seed=7)
        md = MolecularDynamics(s, model=calc, ensemble="npt", thermostat=thermostat, temperature=300.0, starting_temperature=300.0,
                               timestep=1.0, pressure=20.0, bulk_modulus=100.0, taup=50.0, loginterval=10, seed=3)
        tr = md.run(60)
        v = [abs(np.linalg.det(c)) for c in tr.cells]
        print(thermostat, "volume", v[0], v[-1])
        assert v[-1] < 0.95 * v[0]              # 20 GPa on a cell near zero pressure


# ---- 5. scale ---------------------------------------------------------------------------------------------------------------------
def test_large_batch_64_replicas(calc):
    from chgnet_amd.dynamics import MolecularDynamics

    structs = [_structure("li9co7o16", (2, 2, 2), rattle=0.02, seed=100 + i) for i in range(64)]
    out = MolecularDynamics.run_batch(structs, 20, seeds=list(range(64)), model=calc, ensemble="nvt", temperature=300.0,
                                      starting_temperature=300.0, loginterval=10)
    assert len(out) == 64
    for o in out:
        assert o["status"] == "RUNNING" and o["n_steps"] == 20
        assert len(o["trajectory"]) == 3 and np.all(np.isfinite(o["final_structure"].frac_coords))


# ---- 6. isolated atoms -------------------------------------------------------------------------------------------------------------
def test_isolated_atoms_reported_once_per_structure(model, capsys):
    """A batch with one structure holding isolated atoms: the converter's message once on stderr under "warn", ValueError under "error"."""
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.graph.structure import Lattice, Structure

    lone = Structure(Lattice(np.eye(3) * 20.0), ["H", "O"], [[0, 0, 0], [0.5, 0.5, 0.5]])
    structs = [_structure("limno2", rattle=0.05, seed=1), lone, _structure("li9co7o16", rattle=0.03, seed=2)]
    try:
        capsys.readouterr()
        MolecularDynamics.run_batch(structs, 2, model=model, on_isolated_atoms="warn", ensemble="nve", starting_temperature=300.0, seeds=[1, 2, 3])
        assert capsys.readouterr().err.count("has 2 isolated atom") == 1
        with pytest.raises(ValueError, match="has 2 isolated atom"):
            MolecularDynamics.run_batch(structs, 2, model=model, on_isolated_atoms="error", ensemble="nve", seeds=[1, 2, 3])
    finally:
        model.graph_converter.set_isolated_atom_response("warn")
