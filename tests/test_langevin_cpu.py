"""CPU checks of the Langevin NVT restatement (tests/langevin_ref.py) and of its plumbing without a GPU: Philox4x32-10 against
known vectors, the normals' values and moments, friction = 0 against velocity Verlet, the counter semantics (same seed, split runs,
zero total momentum), argument validation, and the two entry points added to the C-ABI at interface version 5."""

from __future__ import annotations

import numpy as np
import pytest

import langevin_ref
import md_ref


def _system(n=12, seed=0, box=5.0):
    rng = np.random.default_rng(seed)
    cell = np.eye(3) * box
    r = rng.random((n, 3)) * box
    m = rng.uniform(6, 60, n)
    p = md_ref.maxwell_boltzmann(m, 300.0, rng)
    return r, cell, m, p


# ---- 1. the generator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("counter", "key", "want"), [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_vectors(counter, key, want):
    assert " ".join("%08x" % w for w in langevin_ref.philox4x32_10(counter, key)) == want


def test_normals_known_values():
    assert np.abs(np.array(langevin_ref.normals(7, 0, 0)) - [0.2297081605550599, 0.20041438525856892, -0.44499077181983376]).max() < 1e-14
    assert np.abs(np.array(langevin_ref.normals(7, 3, 11)) - [1.5194969039132005, -1.568051604120783, -1.3914748345355854]).max() < 1e-14
    # the key is the whole 64-bit seed
    assert langevin_ref.normals(7, 0, 0) != langevin_ref.normals(7 + (1 << 32), 0, 0)


def test_normals_moments():
    """30,000 values; the bars are 5 sigma of each estimator for exact standard normals (var of x^2 is 2, of x^4 is 96)."""
    z = np.array([langevin_ref.normals(12345, i, k) for i in range(200) for k in range(50)]).ravel()
    n = z.size
    mean, var, m4 = z.mean(), z.var(), (z ** 4).mean()
    print("normals: n", n, "mean", mean, "var", var, "m4", m4)
    assert n == 30000
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)
    assert abs(m4 - 3) < 5 * np.sqrt(96 / n)


# ---- 2. the integrator ---------------------------------------------------------------------------------------------------------
def test_zero_friction_is_velocity_verlet():
    r, cell, m, p = _system()
    calc = md_ref.pair_potential()
    nve = md_ref.MDRef(r, cell, m, p, ensemble=md_ref.NVE, dt=2.0 * md_ref.FS, calc=calc)
    lan = langevin_ref.LangevinRef(r, cell, m, p, dt=2.0 * md_ref.FS, temperature_k=300.0, friction=0.0, seed=5, fixcm=False, calc=calc)
    fa, fb = nve.run(50), lan.run(50)
    assert len(fa) == len(fb) == 51
    for a, b in zip(fa, fb):
        for key in ("positions", "momenta"):
            err = np.abs(a[key] - b[key]).max() / np.abs(a[key]).max()
            assert err < 1e-12, (a["step"], key, err)
        assert abs(a["epot"] - b["epot"]) <= 1e-12 * abs(a["epot"])


def test_counter_semantics():
    r, cell, m, p = _system(seed=1)
    calc = md_ref.pair_potential()
    kw = dict(dt=2.0 * md_ref.FS, temperature_k=300.0, friction=0.01 / md_ref.FS, calc=calc)
    a = langevin_ref.LangevinRef(r, cell, m, p, seed=42, **kw)
    b = langevin_ref.LangevinRef(r, cell, m, p, seed=42, **kw)
    c = langevin_ref.LangevinRef(r, cell, m, p, seed=43, **kw)
    fa = a.run(20)
    fb = b.run(10) + b.run(10)
    fc = c.run(20)
    assert len(fa) == len(fb) == 21
    for x, y in zip(fa, fb):                                       # same seed, split run: bit for bit
        assert x["step"] == y["step"]
        assert np.array_equal(x["positions"], y["positions"]) and np.array_equal(x["momenta"], y["momenta"])
    assert np.abs(fa[-1]["positions"] - fc[-1]["positions"]).max() > 1e-3     # another seed, another trajectory
    d = langevin_ref.LangevinRef(r, cell, m, p, seed=42, **kw)
    d.evaluate()
    for _ in range(20):                                            # fixcm: the total momentum vanishes after every step
        d.step()
        assert np.abs(d.p.sum(0)).max() < 1e-12 * np.abs(d.p).sum()
    free = langevin_ref.LangevinRef(r, cell, m, p, seed=42, fixcm=False, **kw)
    free.run(20)
    assert np.abs(free.p.sum(0)).max() > 1e-6 * np.abs(free.p).sum()


def test_langevin_heats_the_restatement_towards_the_target():
    """From 0 K with strong friction the kinetic temperature of the restatement reaches the order of the target."""
    r, cell, m, _ = _system(n=24, seed=2, box=7.0)
    lan = langevin_ref.LangevinRef(r, cell, m, None, dt=1.0 * md_ref.FS, temperature_k=500.0, friction=0.1 / md_ref.FS, seed=3,
                                   calc=md_ref.pair_potential())
    frames = lan.run(100)
    late = np.mean([f["temperature"] for f in frames[50:]])
    assert frames[0]["temperature"] == 0.0
    # 50 frames, each 2 Ekin / (3 n kB) of 3 (n - 1) Gaussian momenta; consecutive frames are correlated over 1 / friction = 10
    # steps, so ~5 independent samples: relative width sqrt(2 / (69 * 5)) = 7.6 %, bar at 5 widths around T0 (n - 1) / n
    assert abs(late - 500.0 * 23 / 24) < 5 * np.sqrt(2 / (69 * 5)) * 500.0, late


# ---- 3. chgnet_amd.dynamics and the C-ABI without a GPU ------------------------------------------------------------------------
def _li2():
    from chgnet_amd.graph.structure import Lattice, Structure

    return Structure(Lattice(np.eye(3) * 3.5), np.array([3, 3]), np.array([[0, 0, 0], [0.5, 0.5, 0.5]]))


def test_resolve_and_codes():
    from chgnet_amd.dynamics import ENSEMBLE_CODES, _resolve

    assert _resolve("nvt", "Langevin", None) == _resolve("NVT", "langevin", 10.0) == "nvt_langevin"
    assert ENSEMBLE_CODES["nvt_langevin"] == 4
    assert _resolve("nve", "Langevin", None) == "nve"
    with pytest.raises(ValueError, match="Thermostat not supported"):
        _resolve("npt", "Langevin", 100.0)
    with pytest.raises(ValueError, match="Thermostat not supported"):
        _resolve("npt", "Langevin", None)


@pytest.mark.parametrize(("kwargs", "match"), [
    (dict(ensemble="nvt", thermostat="Langevin", friction=-0.01), "friction"),
    (dict(ensemble="nvt", thermostat="Langevin", friction=float("nan")), "friction"),
    (dict(ensemble="nvt", thermostat="Langevin", friction=float("inf")), "friction"),
    (dict(ensemble="nvt", thermostat="Berendsen", friction=0.01), "friction"),
    (dict(ensemble="nve", friction=0.01), "friction"),
    (dict(ensemble="npt", thermostat="Berendsen_inhomogeneous", bulk_modulus=100.0, friction=0.01), "friction"),
    (dict(ensemble="npt", thermostat="Langevin", bulk_modulus=100.0), "Thermostat not supported"),
    (dict(ensemble="npt", thermostat="Langevin"), "Thermostat not supported"),
])
def test_argument_validation(kwargs, match):
    from chgnet_amd.dynamics import MolecularDynamics

    with pytest.raises(ValueError, match=match):
        MolecularDynamics(_li2(), model=object(), **kwargs)


def test_friction_default_units_and_seed():
    from chgnet_amd.calculator import CHGNetCalculator
    from chgnet_amd.dynamics import FS, MolecularDynamics

    calc = CHGNetCalculator.__new__(CHGNetCalculator)            # no engine: nothing runs here
    md = MolecularDynamics(_li2(), model=calc, ensemble="nvt", thermostat="Langevin", seed=7)
    assert md.kind == "nvt_langevin" and md.friction == 0.01 and md.cfg["friction"] == 0.01 / FS
    assert md.thermostat_seed == 7
    md = MolecularDynamics(_li2(), model=calc, ensemble="nvt", thermostat="Langevin", friction=0.0, seed=(1 << 40) + 3)
    assert md.cfg["friction"] == 0.0 and md.thermostat_seed == (1 << 40) + 3
    a = MolecularDynamics(_li2(), model=calc, ensemble="nvt", thermostat="Langevin")
    b = MolecularDynamics(_li2(), model=calc, ensemble="nvt", thermostat="Langevin")
    assert 0 <= a.thermostat_seed < 1 << 64 and a.thermostat_seed != b.thermostat_seed       # seed=None: 64 fresh bits each
    assert MolecularDynamics(_li2(), model=calc, ensemble="nvt", seed=7).thermostat_seed is None


def test_abi_gains_entry_points_without_a_bump():
    from chgnet_amd import _lib

    assert _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert int(lib.chg_abi_version()) == 5
    for name in ("chg_md_create_langevin", "chg_test_md_step_langevin"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert len(lib.chg_md_create_langevin.argtypes) == len(lib.chg_md_create.argtypes) + 2
    assert len(lib.chg_test_md_step_langevin.argtypes) == len(lib.chg_test_md_step.argtypes) + 2
