"""CPU checks of the molecular-dynamics restatement (tests/md_ref.py) and of chgnet_amd.dynamics without a GPU: energy conservation
of the NVE integrator, the Berendsen factor and its clamps, fixcm, both barostats, the ideal-gas stress, ASE's units, argument
validation, the logfile and pickle formats, and the interface version of the C-ABI."""

from __future__ import annotations

import os
import pickle
import re

import numpy as np
import pytest

import md_ref
from conftest import REPO


def _lattice_cell(n_side=2, a=3.3, jitter=0.05, seed=0):
    rng = np.random.default_rng(seed)
    g = np.array([[i, j, k] for i in range(n_side) for j in range(n_side) for k in range(n_side)], np.float64)
    pos = g * a + rng.normal(0, jitter, g.shape)
    return pos, np.eye(3) * a * n_side


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_units_are_ase_codata_2014():
    from chgnet_amd import dynamics
    from chgnet_amd.calculator import GPA_TO_EV_A3

    assert md_ref.KB == pytest.approx(8.6173303e-5, rel=1e-9)
    assert md_ref.FS == pytest.approx(0.09822694788464063, rel=1e-14)
    assert md_ref.GPA == pytest.approx(1 / 160.21766208, rel=1e-14) and md_ref.GPA == pytest.approx(GPA_TO_EV_A3, rel=1e-14)
    assert (dynamics.FS, dynamics.KB, dynamics.GPA) == (md_ref.FS, md_ref.KB, md_ref.GPA)


def test_nve_conserves_energy_to_second_order():
    pos, cell = _lattice_cell(jitter=0.15, seed=1)
    m = np.full(len(pos), 20.0)
    calc = md_ref.pair_potential(eps=0.5, rc=3.6)
    drifts = []
    for dt_fs in (2.0, 1.0):
        ref = md_ref.MDRef(pos, cell, m, ensemble=md_ref.NVE, dt=dt_fs * md_ref.FS, calc=calc)
        steps = int(round(100 / dt_fs))
        frames = ref.run(steps)
        etot = np.array([f["epot"] + f["ekin"] for f in frames])
        drifts.append(np.abs(etot - etot[0]).max())
    assert drifts[0] < 1e-3
    # velocity Verlet: the energy error scales as dt^2 (halving dt cuts it about fourfold)
    assert 2.5 < drifts[0] / drifts[1] < 6.0, drifts


def test_berendsen_lambda_and_clamps():
    dt, taut = 1.0, 10.0
    assert md_ref.berendsen_lambda(300.0, 300.0, dt, taut) == 1.0
    assert md_ref.berendsen_lambda(290.0, 300.0, dt, taut) == pytest.approx(np.sqrt(1 + (300 / 290 - 1) * 0.1))
    assert md_ref.berendsen_lambda(1.0, 300.0, dt, taut) == 1.1
    assert md_ref.berendsen_lambda(0.0, 300.0, dt, taut) == 1.1        # T = 0: inf -> 1.1
    assert md_ref.berendsen_lambda(1e5, 300.0, dt, 1.0) == 0.9          # dt / taut = 1: lambda^2 = T0 / T
    assert md_ref.berendsen_lambda(0.0, 0.0, dt, taut) == 1.0


def test_fixcm_removes_mean_momentum_not_mass_weighted():
    rng = np.random.default_rng(2)
    pos, cell = _lattice_cell()
    m = rng.uniform(1, 100, len(pos))
    ref = md_ref.MDRef(pos, cell, m, rng.normal(0, 1, (len(pos), 3)), ensemble=md_ref.NVT, dt=md_ref.FS)
    ref.first_half(rng.normal(0, 1, (len(pos), 3)))
    assert np.abs(ref.p.sum(0)).max() < 1e-12
    assert np.abs((ref.p / m[:, None] * m[:, None]).sum(0)).max() < 1e-12
    nve = md_ref.MDRef(pos, cell, m, rng.normal(0, 1, (len(pos), 3)), ensemble=md_ref.NVE, dt=md_ref.FS)
    nve.first_half(np.zeros((len(pos), 3)))
    assert np.abs(nve.p.sum(0)).max() > 1e-3                          # VelocityVerlet has no fixcm


@pytest.mark.parametrize("ensemble", [md_ref.NPT_INHOM, md_ref.NPT_ISO])
def test_barostats_move_the_cell_the_right_way(ensemble):
    pos, cell = _lattice_cell()
    m = np.full(len(pos), 10.0)
    kappa = 1 / (100 / 160.2176)
    for p_ext, sign in ((10.0, -1), (-10.0, 1)):                      # external pressure above / below the internal one
        ref = md_ref.MDRef(pos, cell, m, ensemble=ensemble, dt=2 * md_ref.FS, pressure=p_ext * md_ref.GPA, compressibility=kappa)
        frac0 = pos @ np.linalg.inv(cell)
        ref.scale_positions_and_cell(np.zeros((3, 3)))
        dv = abs(np.linalg.det(ref.cell)) - abs(np.linalg.det(cell))
        assert np.sign(dv) == sign
        assert np.allclose(ref.r @ np.linalg.inv(ref.cell), frac0, atol=1e-13)    # scale_atoms=True keeps fractional coordinates
    # anisotropic internal stress: only the inhomogeneous barostat scales the axes differently
    ref = md_ref.MDRef(pos, cell, m, ensemble=ensemble, dt=2 * md_ref.FS, pressure=0.0, compressibility=kappa)
    ref.scale_positions_and_cell(np.diag([1.0, 0.0, -1.0]) * md_ref.GPA)          # sigma_xx = -1 GPa: compressive along x
    s = np.diag(ref.cell) / np.diag(cell)
    if ensemble == md_ref.NPT_INHOM:
        assert s[0] < s[1] < s[2] and s[1] == 1.0
    else:
        assert s[0] == s[1] == s[2] == 1.0                           # the trace is zero


def test_ideal_gas_term_matches_direct_sum():
    rng = np.random.default_rng(3)
    pos, cell = _lattice_cell()
    cell = cell + rng.normal(0, 0.3, (3, 3))
    m = rng.uniform(1, 50, len(pos))
    p = rng.normal(0, 1, (len(pos), 3))
    got = md_ref.ideal_gas_stress(p, m, cell)
    vol = abs(np.linalg.det(cell))
    want = np.zeros((3, 3))
    for k in range(len(m)):
        for a in range(3):
            for b in range(3):
                want[a, b] -= p[k, a] * p[k, b] / m[k] / vol
    assert np.allclose(got, want, rtol=1e-13, atol=0)
    assert md_ref.temperature(p, m) == pytest.approx(2 * md_ref.kinetic_energy(p, m) / (3 * len(m) * md_ref.KB))


def test_maxwell_boltzmann_forces_temperature_and_is_stationary():
    from chgnet_amd.dynamics import maxwell_boltzmann

    m = np.random.default_rng(4).uniform(1, 200, 50)
    p = maxwell_boltzmann(m, 450.0, np.random.default_rng(9))
    assert md_ref.temperature(p, m) == pytest.approx(450.0, rel=1e-12)
    assert np.abs(p.sum(0)).max() < 1e-10
    assert np.array_equal(p, md_ref.maxwell_boltzmann(m, 450.0, np.random.default_rng(9)))


# ---- chgnet_amd.dynamics without a GPU -----------------------------------------------------------------------------------------
def _li2():
    from chgnet_amd.graph.structure import Lattice, Structure

    return Structure(Lattice(np.eye(3) * 3.5), np.array([3, 3]), np.array([[0, 0, 0], [0.5, 0.5, 0.5]]))


@pytest.mark.parametrize(("kwargs", "match"), [
    (dict(ensemble="nvt", thermostat="Nose-Hoover"), "Nose-Hoover"),
    (dict(ensemble="npt", thermostat="Nose-Hoover", bulk_modulus=100.0), "Nose-Hoover"),
    (dict(ensemble="npt"), "bulk_modulus"),
    (dict(ensemble="npt", thermostat="npt_berendsen"), "bulk_modulus"),
    (dict(ensemble="nvt", thermostat="Andersen"), "Thermostat not supported"),
    (dict(ensemble="npt", thermostat="Berendsen", bulk_modulus=100.0), "Thermostat not supported"),
    (dict(ensemble="nph"), "Ensemble"),
    (dict(loginterval=0), "loginterval"),
])
def test_argument_validation(kwargs, match):
    from chgnet_amd.dynamics import MolecularDynamics

    with pytest.raises(ValueError, match=match):
        MolecularDynamics(_li2(), model=object(), **kwargs)


def test_resolve_maps_the_reference_thermostats():
    from chgnet_amd.dynamics import _resolve

    assert _resolve("NVE", "Nose-Hoover", None) == "nve"
    assert _resolve("nvt", "Berendsen", None) == _resolve("nvt", "Berendsen_inhomogeneous", None) == "nvt"
    assert _resolve("npt", "Berendsen_inhomogeneous", 10.0) == "npt_inhomogeneous"
    assert _resolve("npt", "NPT_Berendsen", 10.0) == "npt_berendsen"


def test_logfile_format(tmp_path):
    from chgnet_amd.dynamics import MDLogger

    path = str(tmp_path / "md.log")
    log = MDLogger(path, natoms=8)
    log.rows([0.0, 0.002], [-10.123456, -10.2], [0.5, 0.6], [300.04, 301.0])
    lines = open(path).read().splitlines()
    assert lines[0] == "Time[ps]      Etot[eV]     Epot[eV]     Ekin[eV]    T[K]"
    assert lines[1] == "0.0000" + " " * 4 + " " + "%12s" % "-9.6235" + " " + "%12s" % "-10.1235" + " " + "%12s" % "0.5000" + "  " + " 300.0"
    assert re.fullmatch(r"0\.0020 +-9\.6000 +-10\.2000 +0\.6000 +301\.0", lines[2])
    big = MDLogger(str(tmp_path / "big.log"), natoms=256)
    assert big.fmt == "%-10.4f %12.3f %12.3f %12.3f  %6.1f\n"


def test_trajectory_pickle_keys(tmp_path):
    from chgnet_amd.dynamics import MDTrajectory

    tr = MDTrajectory([3, 3])
    tr.energies.append(-1.0)
    path = str(tmp_path / "t.pkl")
    tr.save(path)
    with open(path, "rb") as fh:
        d = pickle.load(fh)
    assert set(d) == {"energy", "forces", "stresses", "magmoms", "atom_positions", "cell", "atomic_number", "momenta", "temperature"}


def test_md_abi_version_and_symbols():
    from chgnet_amd import _lib

    with open(os.path.join(REPO, "include", "chgnet_hip.h")) as fh:
        text = fh.read()
    assert int(re.search(r"#define\s+CHG_ABI_VERSION\s+(\d+)", text).group(1)) == 5 == _lib.ABI_VERSION
    names = ("chg_md_create", "chg_md_run", "chg_md_download", "chg_md_free", "chg_test_md_step")
    lib = _lib.load()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n), n
