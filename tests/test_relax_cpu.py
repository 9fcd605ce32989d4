"""Batched relaxation, CPU side: the float64 restatement (tests/relax_ref.py) against central differences of the float64 oracle,
FIRE's branches on an analytic quadratic, argument validation of StructOptimizer and the trajectory file."""

from __future__ import annotations

import pickle

import numpy as np
import pytest
import torch
from scipy.linalg import expm

from conftest import load_case
from relax_ref import FIRE, GPA, Relaxation, fire_step


def _oracle_energy_fs(oracle, conv, z, frac, lattice):
    from chgnet_amd.graph.structure import Lattice, Structure

    g = conv(Structure(Lattice(lattice), z, frac))
    g.atom_frac_coord, g.lattice = np.asarray(frac, np.float64), np.asarray(lattice, np.float64)   # the graph keeps fp32 copies
    out = oracle.predict_graph(g, "efs")
    n = len(z)
    return float(out["e"]) * n, np.asarray(out["f"], np.float64), np.asarray(out["s"], np.float64)


@pytest.mark.parametrize("sheared", [False, True])
def test_generalized_forces_are_minus_energy_gradient(trained_like_weights, sheared):
    """g of the restatement == -dE/d(u, X) by central differences of the float64 oracle energy (graph rebuilt per displacement)."""
    from chgnet_amd import CrystalGraphConverter
    from oracle.chgnet_oracle import OracleCHGNet

    _, d = load_case("limno2")
    z = d["atomic_number"].astype(np.int32)
    oracle = OracleCHGNet(trained_like_weights, dtype=torch.float64)
    conv = CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3)
    r = Relaxation(d["frac_coord_f64"], d["lattice_f64"])
    if sheared:
        r.q[r.n:] = r.c * np.array([[0.03, 0.02, -0.01], [0.015, -0.025, 0.01], [-0.02, 0.005, 0.04]])
        r.q[:r.n] += np.random.default_rng(0).normal(0, 0.05, (r.n, 3))

    def energy(q):
        r2 = Relaxation(d["frac_coord_f64"], d["lattice_f64"])
        r2.q = q
        return _oracle_energy_fs(oracle, conv, z, r2.frac(), r2.lattice())

    _, f, s = energy(r.q.copy())
    g = r.generalized_forces(f, s * GPA)
    h = 1e-4
    num = np.zeros_like(g)
    for i in range(r.n + 3):
        for j in range(3):
            qp, qm = r.q.copy(), r.q.copy()
            qp[i, j] += h
            qm[i, j] -= h
            num[i, j] = -(energy(qp)[0] - energy(qm)[0]) / (2 * h)
    scale = np.abs(g).max()
    assert np.abs(num - g).max() < 1e-5 * scale + 1e-8, (num, g)
    assert np.abs(g[r.n:]).max() > 1e-3        # the cell rows carry a real force


def _quadratic(k):
    return lambda x: -k * x            # E = k |x|^2 / 2


def test_fire_first_step_and_dt_growth_only_after_nmin():
    """Downhill on a quadratic: v starts at 0, dt grows (and a shrinks) only once Nsteps > Nmin."""
    grad = _quadratic(0.05)
    x = np.array([1.0, -0.5, 0.25])
    v, dt, a, n = None, FIRE["dt"], FIRE["astart"], 0
    dts, alphas = [], []
    for k in range(12):
        g = grad(x)
        dr, v, dt, a, n = fire_step(g, v if v is not None else np.zeros(3), k == 0, dt, a, n)
        if k == 0:
            assert np.allclose(v, FIRE["dt"] * g)          # v = 0 + dt g
        x = x + dr
        dts.append(dt)
        alphas.append(a)
    # Nsteps counts the downhill steps after the first; dt stays until Nsteps > Nmin = 5 (ASE: growth on the 7th downhill update)
    assert dts[:7] == [FIRE["dt"]] * 7
    assert dts[7] == pytest.approx(FIRE["dt"] * FIRE["finc"])
    assert alphas[7] == pytest.approx(FIRE["astart"] * FIRE["fa"])


def test_fire_uphill_resets():
    g = np.array([1.0, 0.0, 0.0])
    v = np.array([-2.0, 0.0, 0.0])                        # P = g.v < 0
    dr, v2, dt, a, n = fire_step(g, v, False, 0.2, 0.05, 9)
    assert dt == pytest.approx(0.1) and a == FIRE["astart"] and n == 0
    assert np.allclose(v2, dt * g)                        # v reset to 0, then v += dt g


def test_fire_maxstep_clamp():
    g = np.array([30.0, -40.0, 0.0])
    dr, v, dt, a, n = fire_step(g, np.zeros(3), True, 0.1, 0.1, 0)
    assert np.linalg.norm(dr) == pytest.approx(FIRE["maxstep"])
    assert np.allclose(dr / np.linalg.norm(dr), g / np.linalg.norm(g))


def test_relaxation_converges_on_quadratic_cell_free():
    """Restatement end to end on a harmonic well (no cell): converges, first evaluation converged -> 0 steps."""
    rng = np.random.default_rng(1)
    L = np.eye(3) * 5.0
    frac0 = np.full((4, 3), 0.5)
    r = Relaxation(frac0 + rng.normal(0, 0.02, (4, 3)), L, relax_cell=False, fmax=1e-3, steps=500)
    while r.status == 0:
        x = r.positions() - frac0 @ L
        r.advance(-0.8 * x, np.zeros((3, 3)))
    assert r.status == 1 and 0 < r.steps < 500
    r0 = Relaxation(frac0, L, relax_cell=False, fmax=1e-3)
    assert r0.advance(np.zeros((4, 3)), np.zeros((3, 3))) == 1 and r0.steps == 0
    r1 = Relaxation(frac0, L, relax_cell=False, fmax=1e-3, steps=0)
    assert r1.advance(np.ones((4, 3)), np.zeros((3, 3))) == 2
    r2 = Relaxation(frac0, L, relax_cell=False)
    assert r2.advance(np.full((4, 3), np.nan), np.zeros((3, 3))) == 3


def test_cell_rows_start_at_identity():
    _, d = load_case("limno2")
    r = Relaxation(d["frac_coord_f64"], d["lattice_f64"])
    assert np.array_equal(r.lattice(), d["lattice_f64"]) and r.c == 8.0
    r.q[r.n:] = 0.08 * np.eye(3)
    assert np.allclose(r.lattice(), d["lattice_f64"] @ expm(0.01 * np.eye(3)).T)
    assert np.allclose(r.frac(), d["frac_coord_f64"])   # frac = u L0^-1 does not depend on F


# ---- StructOptimizer argument validation (no GPU: the engine is never created) -------------------------------------------------
@pytest.fixture()
def optimizer():
    from chgnet_amd import CHGNet
    from chgnet_amd.relax import StructOptimizer

    return StructOptimizer(model=CHGNet())


def test_exported_lazily():
    import chgnet_amd
    from chgnet_amd.relax import StructOptimizer, TrajectoryObserver

    assert chgnet_amd.StructOptimizer is StructOptimizer and chgnet_amd.TrajectoryObserver is TrajectoryObserver


def test_unknown_optimizer_rejected():
    from chgnet_amd import CHGNet
    from chgnet_amd.relax import StructOptimizer

    with pytest.raises(ValueError, match=r"Optimizer instance not found. Select from \['FIRE'\]"):
        StructOptimizer(model=CHGNet(), optimizer_class="BFGS")


def test_invalid_filter_and_arguments_rejected(optimizer):
    from chgnet_amd.graph.structure import Lattice, Structure

    s = Structure(Lattice(np.eye(3) * 4), [3], [[0, 0, 0]])
    with pytest.raises(ValueError, match=r"Invalid ase_filter='ExpCellFilter', "):
        optimizer.relax(s, ase_filter="ExpCellFilter")
    with pytest.raises(ValueError, match="Invalid ase_filter="):
        optimizer.relax_batch([s], ase_filter="UnitCellFilter")
    with pytest.raises(TypeError, match="unexpected keyword"):
        optimizer.relax(s, dtt=0.2)
    with pytest.raises(ValueError, match="loginterval"):
        optimizer.relax(s, loginterval=0)
    with pytest.raises(ValueError, match="non-negative"):
        optimizer.relax(s, fmax=-1.0)


def test_calculator_is_reused():
    from chgnet_amd import CHGNet, CHGNetCalculator
    from chgnet_amd.relax import StructOptimizer

    calc = CHGNetCalculator(model=CHGNet(), stress_weight=0.5)
    opt = StructOptimizer(model=calc)
    assert opt.calculator is calc and opt.n_params == calc.n_params


def test_trajectory_save_round_trip(tmp_path):
    from chgnet_amd.relax import TrajectoryObserver

    obs = TrajectoryObserver([3, 8])
    rng = np.random.default_rng(0)
    for _ in range(3):
        obs.append(rng.normal(), rng.normal(size=(2, 3)), rng.normal(size=6), rng.normal(size=2), rng.normal(size=(2, 3)), rng.normal(size=(3, 3)))
    path = tmp_path / "traj.pkl"
    obs.save(str(path))
    with open(path, "rb") as fh:
        got = pickle.load(fh)
    assert set(got) == {"energy", "forces", "stresses", "magmoms", "atom_positions", "cell", "atomic_number"}
    assert len(obs) == 3 and got["energy"] == obs.energies
    for key, mine in (("forces", obs.forces), ("stresses", obs.stresses), ("magmoms", obs.magmoms), ("atom_positions", obs.atom_positions),
                      ("cell", obs.cells)):
        assert all(np.array_equal(a, b) for a, b in zip(got[key], mine))
    assert np.array_equal(got["atomic_number"], [3, 8])


def test_structure_site_properties():
    from chgnet_amd.graph.structure import Lattice, Structure

    s = Structure(Lattice(np.eye(3) * 4), [3, 8], [[0, 0, 0], [0.5, 0.5, 0.5]])
    assert s.site_properties == {}
    s.add_site_property("magmom", [0.1, 0.2])
    assert s.site_properties["magmom"] == [0.1, 0.2]
    with pytest.raises(ValueError):
        s.add_site_property("magmom", [0.1])
    s.remove_site_property("magmom")
    assert s.site_properties == {}
