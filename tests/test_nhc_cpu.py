"""CPU checks of the Nose-Hoover-chain restatement (tests/nhc_ref.py) and of its plumbing without a GPU: second-order conservation
of the extended energy, time reversal, NPT -> NVT when the barostat decouples, mean pressure and temperature of the sampled
ensembles, the cell only ever scaling, argument validation, and the three entry points added to the C-ABI at interface version 5.

The system is an 8-atom jittered lattice (like ``_lattice_cell`` of test_md_cpu.py) in a sheared, non-triangular cell with the soft
repulsive ``md_ref.pair_potential``: eps = 5 eV and rc = 4.5 A make it stiff enough that the NPT volume stays where the potential's 27
images suffice (checked below)."""

from __future__ import annotations

import copy
import os
import re

import numpy as np
import pytest

import md_ref
import nhc_ref
from conftest import REPO

FS, GPA = md_ref.FS, md_ref.GPA
RC = 4.5
T0 = 300.0
PEXT = 0.02                                    # eV/A^3: the NVT mean pressure of this system at 300 K is 0.0203
SHEAR = np.array([[0.0, 0.4, -0.3], [0.5, 0.0, 0.2], [-0.2, 0.3, 0.0]])


def _system(seed=0, n_side=2, a=3.0, jitter=0.1):
    rng = np.random.default_rng(seed)
    g = np.array([[i, j, k] for i in range(n_side) for j in range(n_side) for k in range(n_side)], np.float64)
    cell = np.eye(3) * a * n_side + SHEAR
    assert abs(cell[1, 0]) > 0.1 and abs(cell[0, 1]) > 0.1                # neither triangular form
    frac = g / n_side + rng.normal(0, jitter / (a * n_side), g.shape)
    m = rng.uniform(10, 40, len(g))
    p = nhc_ref.remove_com_momentum(md_ref.maxwell_boltzmann(m, T0, rng), m)
    return frac @ cell, cell, m, p


def _ref(npt, dt_fs, *, taup_fs=200.0, chain_length=3, seed=0):
    r, cell, m, p = _system(seed)
    return nhc_ref.NHCRef(r, cell, m, p, npt=npt, dt=dt_fs * FS, temperature_k=T0, taut=20 * FS, taup=taup_fs * FS, pressure=PEXT,
                          chain_length=chain_length, calc=md_ref.pair_potential(eps=5.0, rc=RC))


def _min_height(cell):
    vol = abs(np.linalg.det(cell))
    return min(vol / np.linalg.norm(np.cross(cell[i - 1], cell[i - 2])) for i in range(3))


# ---- (a) second order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npt", [False, True])
def test_conserved_quantity_is_second_order(npt):
    """std of H over 200 fs at dt and dt / 2: a second-order integrator quarters it."""
    stds = []
    for dt_fs in (1.0, 0.5):
        frames = _ref(npt, dt_fs).run(int(round(200 / dt_fs)))
        stds.append(np.std([f["conserved"] for f in frames]))
    print("npt" if npt else "nvt", "std of H at 1 fs and 0.5 fs", stds, "ratio", stds[0] / stds[1])
    assert stds[0] < 5e-3                                                 # eV, of a kinetic energy of 0.27 eV
    assert 3.0 <= stds[0] / stds[1] <= 5.0, stds


# ---- (b) time reversal -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npt", [False, True])
@pytest.mark.parametrize("chain_length", [1, 3, 4])
def test_time_reversal(npt, chain_length):
    ref = _ref(npt, 2.0, chain_length=chain_length)
    start = copy.deepcopy(ref)
    ref.run(25)
    moved = np.abs(ref.r - start.r).max()
    ref.reverse()
    ref.run(25)
    ref.reverse()
    assert moved > 0.05
    for name in ("r", "p", "cell", "v", "eta", "vb", "xi"):
        a, b = getattr(ref, name), getattr(start, name)
        scale = max(np.abs(b).max(), np.abs(getattr(ref, name)).max(), 1e-300)
        if name in ("v", "vb", "eta", "xi"):                             # start at 0: relative to what they reached on the way
            scale = max(scale, 1e-3)
        assert np.abs(a - b).max() <= 1e-9 * scale, name
    assert abs(ref.veps - start.veps) <= 1e-9 * 1e-3


# ---- (c) decoupling --------------------------------------------------------------------------------------------------------------
def test_npt_with_a_decoupled_barostat_is_nvt():
    nvt, npt = _ref(False, 2.0), _ref(True, 2.0, taup_fs=1e12)
    fa, fb = nvt.run(20), npt.run(20)
    for a, b in zip(fa, fb):
        assert np.abs(a["positions"] - b["positions"]).max() <= 1e-10 * np.abs(a["positions"]).max()
        assert np.abs(a["momenta"] - b["momenta"]).max() <= 1e-10 * np.abs(a["momenta"]).max()


# ---- (d), (e), (f) the sampled ensembles ---------------------------------------------------------------------------------------------
def _block_test(x, want, what):
    """Mean of the second half of x against ``want``: within 3 standard errors, the standard error from 8 block means."""
    x = np.asarray(x[len(x) // 2:])
    blocks = x[: len(x) // 8 * 8].reshape(8, -1).mean(axis=1)
    se = blocks.std(ddof=1) / np.sqrt(8)
    print(what, "mean", x.mean(), "expected", want, "standard error", se, "deviation / se", (x.mean() - want) / se)
    assert abs(x.mean() - want) <= 3 * se, what


def _sample(ref, steps):
    pres, temp, cells = [], [], []
    ref.evaluate()
    for _ in range(steps):
        ref.step()
        _, _, s = ref.evaluate()
        pres.append(-float(np.trace(s)) / 3 + ref.k2() / (3 * ref.volume()))     # -tr(sigma + ideal gas) / 3
        temp.append(md_ref.temperature(ref.p, ref.m))
        cells.append(ref.cell.copy())
    return np.array(pres), np.array(temp), cells


def test_npt_mean_pressure_temperature_and_cell_shape():
    ref = _ref(True, 2.0)
    h0, n = ref.cell.copy(), len(ref.m)
    pres, temp, cells = _sample(ref, 4000)
    assert min(_min_height(c) for c in cells) > RC                        # the potential's 27 images suffice throughout
    _block_test(pres, PEXT, "NPT pressure")
    _block_test(temp, T0 * (n - 1) / n, "NPT temperature")
    vols = np.array([abs(np.linalg.det(c)) for c in cells]) / abs(np.linalg.det(h0))
    assert vols.max() - vols.min() > 0.05                                 # the cell did breathe
    for c in cells:                                                        # (f): a scalar multiple of the initial cell
        lam = np.vdot(c, h0) / np.vdot(h0, h0)
        assert np.abs(c - lam * h0).max() <= 1e-14 * np.abs(c).max()


def test_nvt_mean_temperature():
    ref = _ref(False, 2.0)
    h0, n = ref.cell.copy(), len(ref.m)
    _, temp, cells = _sample(ref, 2000)
    _block_test(temp, T0 * (n - 1) / n, "NVT temperature")
    assert np.array_equal(cells[-1], h0)
    assert np.abs(ref.p.sum(axis=0)).max() <= 1e-10 * np.abs(ref.p).sum()  # nothing pushes the centre of mass


# ---- (g) chgnet_amd.dynamics and the C-ABI without a GPU ------------------------------------------------------------------------
def _li2():
    from chgnet_amd.graph.structure import Lattice, Structure

    return Structure(Lattice(np.eye(3) * 3.5), np.array([3, 3]), np.array([[0, 0, 0], [0.5, 0.5, 0.5]]))


def _calc():
    from chgnet_amd.calculator import CHGNetCalculator

    return CHGNetCalculator.__new__(CHGNetCalculator)                     # no engine: nothing runs here


def test_resolve_and_codes():
    from chgnet_amd.dynamics import ENSEMBLE_CODES, _resolve

    assert _resolve("nvt", "Nose-Hoover-Chain", None) == _resolve("NVT", "nose-hoover-chain", 10.0) == "nvt_nhc"
    assert _resolve("npt", "Nose-Hoover-Chain", None) == _resolve("npt", "NOSE-HOOVER-CHAIN", 100.0) == "npt_nhc"
    assert ENSEMBLE_CODES["nvt_nhc"] == 5 and ENSEMBLE_CODES["npt_nhc"] == 6
    assert _resolve("nve", "Nose-Hoover-Chain", None) == "nve"
    for ens in ("nvt", "npt"):
        with pytest.raises(ValueError, match="Nose-Hoover") as exc:
            _resolve(ens, "Nose-Hoover", 100.0)
        assert "'Nose-Hoover-Chain'" in str(exc.value)


@pytest.mark.parametrize(("kwargs", "match"), [
    (dict(ensemble="nvt", thermostat="Nose-Hoover-Chain", chain_length=0), "chain_length"),
    (dict(ensemble="nvt", thermostat="Nose-Hoover-Chain", chain_length=5), "chain_length"),
    (dict(ensemble="npt", thermostat="Nose-Hoover-Chain", chain_length=2.5), "chain_length"),
    (dict(ensemble="nvt", thermostat="Berendsen", chain_length=3), "chain_length"),
    (dict(ensemble="nvt", thermostat="Langevin", chain_length=3), "chain_length"),
    (dict(ensemble="nve", thermostat="Nose-Hoover-Chain", chain_length=3), "chain_length"),
    (dict(ensemble="npt", thermostat="Nose-Hoover-Chain", pressure=np.full(3, 1e-4)), "pressure"),
    (dict(ensemble="npt", thermostat="Nose-Hoover-Chain", pressure=[1e-4] * 6), "pressure"),
    (dict(ensemble="nvt", thermostat="Nose-Hoover-Chain", temperature=0), "temperature"),
    (dict(ensemble="npt", thermostat="Nose-Hoover-Chain", temperature=-5.0), "temperature"),
    (dict(ensemble="nvt", thermostat="Nose-Hoover-Chain", friction=0.01), "friction"),
])
def test_argument_validation(kwargs, match):
    from chgnet_amd.dynamics import MolecularDynamics

    with pytest.raises(ValueError, match=match):
        MolecularDynamics(_li2(), model=_calc(), **kwargs)


def test_single_atom_is_refused():
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.graph.structure import Lattice, Structure

    one = Structure(Lattice(np.eye(3) * 3.5), np.array([3]), np.array([[0.0, 0.0, 0.0]]))
    for ens in ("nvt", "npt"):
        with pytest.raises(ValueError, match="one atom"):
            MolecularDynamics(one, model=_calc(), ensemble=ens, thermostat="Nose-Hoover-Chain")
    MolecularDynamics(one, model=_calc(), ensemble="nvt", thermostat="Berendsen")          # the others take it


def test_defaults_units_and_initial_momentum():
    from chgnet_amd.dynamics import FS as DFS, GPA as DGPA, MolecularDynamics
    from chgnet_amd.graph.structure import Lattice, Structure

    md = MolecularDynamics(_li2(), model=_calc(), ensemble="npt", thermostat="Nose-Hoover-Chain", timestep=1.5)
    assert md.kind == "npt_nhc" and md.chain_length == 3 and md.bulk_modulus is None            # bulk_modulus=None is accepted
    assert md.cfg["taut"] == 150 * DFS and md.cfg["taup"] == 1500 * DFS and md.cfg["pressure"] == 1.01325e-4 * DGPA
    assert md.thermostat_state is None and md.traj.conserved == []
    md = MolecularDynamics(_li2(), model=_calc(), ensemble="nvt", thermostat="nose-hoover-chain", chain_length=4, bulk_modulus=50.0)
    assert md.kind == "nvt_nhc" and md.chain_length == 4
    assert MolecularDynamics(_li2(), model=_calc(), ensemble="nvt").chain_length is None

    class Moving:                                                          # atoms-like: masses and momenta of its own
        def __init__(self):
            self.s = Structure(Lattice(np.eye(3) * 5.0), np.array([3, 8, 27]), np.array([[0, 0, 0], [0.5, 0.5, 0.5], [0.2, 0.7, 0.1]]))
            self.frac_coords, self.lattice, self.atomic_numbers = self.s.frac_coords, self.s.lattice, self.s.atomic_numbers

        def __len__(self):
            return 3

        def get_masses(self):
            return np.array([7.0, 16.0, 59.0])

        def get_momenta(self):
            return np.array([[1.0, 0.0, 2.0], [0.5, -1.0, 0.0], [3.0, 1.0, 1.0]])

    atoms = Moving()
    md = MolecularDynamics(atoms, model=_calc(), ensemble="nvt", thermostat="Nose-Hoover-Chain")
    want = nhc_ref.remove_com_momentum(atoms.get_momenta(), atoms.get_masses())
    assert np.abs(md.momenta - want).max() < 1e-15 and np.abs(md.momenta.sum(axis=0)).max() < 1e-14
    kept = MolecularDynamics(atoms, model=_calc(), ensemble="nvt", thermostat="Berendsen")
    assert np.array_equal(kept.momenta, atoms.get_momenta())               # the other ensembles keep what they are given


def test_conserved_joins_the_pickle_only_when_present(tmp_path):
    import pickle

    from chgnet_amd.dynamics import MDTrajectory

    tr = MDTrajectory([3, 3])
    tr.energies.append(-1.0)
    tr.save(str(tmp_path / "a.pkl"))
    with open(tmp_path / "a.pkl", "rb") as fh:
        assert "conserved" not in pickle.load(fh)
    tr.conserved.append(-0.5)
    tr.save(str(tmp_path / "b.pkl"))
    with open(tmp_path / "b.pkl", "rb") as fh:
        assert pickle.load(fh)["conserved"] == [-0.5]


def test_abi_gains_entry_points_without_a_bump():
    from chgnet_amd import _lib

    with open(os.path.join(REPO, "include", "chgnet_hip.h")) as fh:
        header = fh.read()
    assert int(re.search(r"#define\s+CHG_ABI_VERSION\s+(\d+)", header).group(1)) == 5 == _lib.ABI_VERSION
    lib = _lib.load()
    assert int(lib.chg_abi_version()) == 5
    for name in ("chg_md_create_nhc", "chg_md_download_nhc", "chg_test_md_step_nhc"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(rf"\b{name}\s*\(", header), name
    assert len(lib.chg_md_create_nhc.argtypes) == len(lib.chg_md_create.argtypes) + 1
    assert len(lib.chg_md_download_nhc.argtypes) == 5
    assert len(lib.chg_test_md_step_nhc.argtypes) == len(lib.chg_test_md_step.argtypes) + 2
    # null arguments are refused before anything touches a device
    assert lib.chg_md_create_nhc(None, None, None, None, None, 3, None) != 0
    assert lib.chg_md_download_nhc(None, None, None, None, 0) != 0
