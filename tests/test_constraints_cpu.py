"""Fixed atoms, CPU side: the entry points added to the C-ABI at interface version 5, the mask normalisation of the Python layer
(every accepted form, selective_dynamics, stand-ins for ASE's FixAtoms / FixCartesian, every refusal), and the physics of the
float64 restatement (tests/constraint_ref.py) on analytic potentials: held coordinates never move, FIRE and L-BFGS converge on
the free ones, NVE conserves energy, the Nose-Hoover-chain energy is conserved with N_f = dof, Langevin thermalises dof components."""

from __future__ import annotations

import os
import re
import warnings

import numpy as np
import pytest

import constraint_ref as cref
import md_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("chg_relax_set_fixed", "chg_md_set_fixed", "chg_test_relax_step_fixed", "chg_test_lbfgs_step_fixed", "chg_test_md_step_fixed")


# ---- 1. the C-ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_gains_the_constraint_entry_points_without_a_bump():
    from chgnet_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "chgnet_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+CHG_ABI_VERSION\s+5\b", header) and _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert int(lib.chg_abi_version()) == 5
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(rf"\bint\s+{name}\s*\(", header), name
    assert re.search(r"chg_relax_set_fixed\s*\(\s*chg_engine\*\s*\w+,\s*chg_relax\*\s*\w+,\s*const uint8_t\*\s*\w+\s*\)", header)
    assert re.search(r"chg_md_set_fixed\s*\(\s*chg_engine\*\s*\w+,\s*chg_md\*\s*\w+,\s*const uint8_t\*\s*\w+\s*\)", header)
    assert len(lib.chg_relax_set_fixed.argtypes) == len(lib.chg_md_set_fixed.argtypes) == 3
    assert len(lib.chg_test_relax_step_fixed.argtypes) == len(lib.chg_test_relax_step.argtypes) + 1
    assert len(lib.chg_test_lbfgs_step_fixed.argtypes) == len(lib.chg_test_lbfgs_step.argtypes) + 1
    assert len(lib.chg_test_md_step_fixed.argtypes) == len(lib.chg_test_md_step.argtypes) + 5      # friction, seeds, chain_length, nhc, fixed
    # null arguments are refused before anything touches a device
    assert lib.chg_relax_set_fixed(None, None, None) != 0
    assert lib.chg_md_set_fixed(None, None, None) != 0


# ---- 2. the Python layer without a GPU ---------------------------------------------------------------------------------------------
def _li4():
    from chgnet_amd.graph.structure import Lattice, Structure

    return Structure(Lattice(np.eye(3) * 5.0), np.array([3, 3, 8, 8]), np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]]))


def test_every_accepted_form_gives_the_same_mask():
    from chgnet_amd.calculator import join_fixed, normalize_fixed

    want = np.array([[1, 1, 1], [0, 0, 0], [1, 1, 1], [0, 0, 0]], np.uint8)
    for entry in ([0, 2], (2, 0), np.array([0, 2]), [-4, 2], np.array([True, False, True, False]), want.astype(bool)):
        got = normalize_fixed(entry, 4)
        assert got.dtype == np.uint8 and got.shape == (4, 3) and np.array_equal(got, want), entry
    per_component = np.zeros((4, 3), bool)
    per_component[1, 2] = per_component[3, 0] = True
    assert np.array_equal(normalize_fixed(per_component, 4), per_component.astype(np.uint8))
    assert normalize_fixed(None, 4) is None
    assert not normalize_fixed([], 4).any() and not normalize_fixed(np.zeros(4, bool), 4).any()
    # one array for the handle: None entries hold nothing, and a batch that holds nothing at all has no mask
    joined = join_fixed([None, want, normalize_fixed([], 2)], [3, 4, 2])
    assert joined.shape == (9, 3) and joined.flags.c_contiguous and np.array_equal(joined[3:7], want) and not joined[:3].any() and not joined[7:].any()
    assert join_fixed([None, normalize_fixed([], 2)], [3, 2]) is None


@pytest.mark.parametrize(("entry", "match"), [
    ([0, 4], "out of range"), ([-5], "out of range"), (np.zeros(3, bool), "shape"), (np.zeros((4, 2), bool), "shape"),
    (np.zeros((3, 3), bool), "shape"), ([0.5, 1.0], "indices"), ([[0, 1], [2, 3]], "indices"), ("ab", "indices"),
])
def test_bad_entries_are_refused(entry, match):
    from chgnet_amd.calculator import normalize_fixed

    with pytest.raises(ValueError, match=match):
        normalize_fixed(entry, 4)


def test_selective_dynamics_is_honoured_and_the_keyword_wins():
    from chgnet_amd.calculator import structure_fixed

    s = _li4()
    assert structure_fixed(s) is None
    s.add_site_property("selective_dynamics", [[True, True, True], [False, False, False], [True, False, True], [True, True, True]])
    assert np.array_equal(structure_fixed(s), [[0, 0, 0], [1, 1, 1], [0, 1, 0], [0, 0, 0]])          # True = free: pymatgen's convention
    assert np.array_equal(structure_fixed(s, [3]), [[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 1, 1]])
    s.add_site_property("selective_dynamics", [[True, True]] * 4)
    with pytest.raises(ValueError, match="selective_dynamics"):
        structure_fixed(s)


class FixAtoms:                                   # stand-ins: ASE is matched by class name
    def __init__(self, indices=None, mask=None):
        self.index = np.flatnonzero(mask) if mask is not None else np.asarray(indices)


class FixCartesian:
    def __init__(self, a, mask=(True, True, True)):
        self.index = np.atleast_1d(np.asarray(a))
        self.mask = np.asarray(mask, bool)


class FixBondLength:
    def __init__(self, a, b):
        self.pairs = [(a, b)]


class _Atoms:
    def __init__(self, constraints):
        self.constraints = constraints

    def get_cell(self):
        return np.eye(3) * 5.0

    def get_atomic_numbers(self):
        return np.array([3, 3, 8, 8])

    def get_scaled_positions(self, wrap=False):  # noqa: ARG002
        return np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]], np.float64)


def test_ase_constraints_are_translated_by_class_name():
    from chgnet_amd.calculator import atoms_to_structure, structure_fixed

    s = atoms_to_structure(_Atoms([FixAtoms(indices=[1]), FixCartesian([0, 3], mask=(True, False, True)), FixAtoms(mask=[False, False, False, True])]))
    assert np.array_equal(structure_fixed(s), [[1, 0, 1], [1, 1, 1], [0, 0, 0], [1, 1, 1]])
    assert s.site_properties["selective_dynamics"][0] == [False, True, False]
    assert structure_fixed(atoms_to_structure(_Atoms([]))) is None
    with pytest.warns(UserWarning, match="FixBondLength"):
        s = atoms_to_structure(_Atoms([FixBondLength(0, 1), FixAtoms(indices=[2])]))
    assert np.array_equal(structure_fixed(s), [[0, 0, 0], [0, 0, 0], [1, 1, 1], [0, 0, 0]])         # the rest is still honoured
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        atoms_to_structure(_Atoms([FixAtoms(indices=[0])]))                                           # nothing to report
    with pytest.raises(ValueError, match="names atom 7 "):
        atoms_to_structure(_Atoms([FixAtoms(indices=[7])]))
    with pytest.raises(ValueError, match="names atom -9 "):
        atoms_to_structure(_Atoms([FixAtoms(indices=[1, -9])]))


def test_relaxation_refusals_come_before_the_device():
    from chgnet_amd.model import CHGNet
    from chgnet_amd.relax import StructOptimizer

    s = _li4()
    partial = np.zeros((4, 3), bool)
    partial[1, 0] = True
    for name in ("FIRE", "LBFGS"):
        opt = StructOptimizer(model=CHGNet(), optimizer_class=name)
        with pytest.raises(ValueError, match="only some cartesian components"):
            opt.relax(s, fixed_atoms=partial, verbose=False)                                  # relax_cell defaults to True
        with pytest.raises(ValueError, match="out of range"):
            opt.relax(s, fixed_atoms=[4], relax_cell=False, verbose=False)
        with pytest.raises(ValueError, match="shape"):
            opt.relax_batch([s, s], fixed_atoms=[None, np.zeros(5, bool)])
        with pytest.raises(ValueError, match="entries for 2 structures"):
            opt.relax_batch([s, s], fixed_atoms=[[0]])
        with pytest.raises(ValueError, match="structure 1 holds only some"):
            opt.relax_batch([s, s], fixed_atoms=[[0], partial])
    masks = StructOptimizer._fixed([s, s], [None, partial], relax_cell=False)                # a fixed cell takes per-component masks
    assert masks[0] is None and np.array_equal(masks[1], partial)


def _calc():
    from chgnet_amd.calculator import CHGNetCalculator

    return CHGNetCalculator.__new__(CHGNetCalculator)                     # no engine: nothing runs here


def test_md_refusals_momenta_and_centre_of_mass():
    from chgnet_amd.dynamics import MolecularDynamics

    s = _li4()
    partial = np.zeros((4, 3), bool)
    partial[2, 1] = True
    moving = [dict(ensemble="npt", thermostat="Berendsen_inhomogeneous", bulk_modulus=100.0), dict(ensemble="npt", thermostat="npt_berendsen", bulk_modulus=100.0),
              dict(ensemble="npt", thermostat="Nose-Hoover-Chain")]
    for kw in moving:
        with pytest.raises(ValueError, match="only some cartesian components"):
            MolecularDynamics(s, model=_calc(), fixed_atoms=partial, **kw)
        MolecularDynamics(s, model=_calc(), fixed_atoms=[2], **kw)                            # whole atoms scale with the cell
    for kw in (dict(ensemble="nvt"), dict(ensemble="nvt", thermostat="Langevin"), dict(ensemble="nvt", thermostat="Nose-Hoover-Chain"), *moving):
        with pytest.raises(ValueError, match="no free component"):
            MolecularDynamics(s, model=_calc(), fixed_atoms=[0, 1, 2, 3], **kw)
    assert not MolecularDynamics(s, model=_calc(), ensemble="nve", fixed_atoms=[0, 1, 2, 3], starting_temperature=300.0, seed=1).momenta.any()
    with pytest.raises(ValueError, match="out of range"):
        MolecularDynamics(s, model=_calc(), ensemble="nve", fixed_atoms=[9])
    with pytest.raises(ValueError, match="entries for 2 structures"):
        MolecularDynamics.run_batch([s, s], 1, model=_calc(), fixed_atoms=[[0]])
    # momenta are masked after they are drawn; md.atoms carries the mask; the caller's structure is left alone
    free = MolecularDynamics(s, model=_calc(), ensemble="nvt", starting_temperature=300.0, seed=5)
    md = MolecularDynamics(s, model=_calc(), ensemble="nvt", starting_temperature=300.0, seed=5, fixed_atoms=partial)
    assert np.array_equal(md.momenta, np.where(partial, 0.0, free.momenta)) and md.momenta[2, 1] == 0.0 and md.momenta[2, 0] != 0.0
    assert md.atoms.site_properties["selective_dynamics"][2] == [True, False, True] and "selective_dynamics" not in s.site_properties
    # Nose-Hoover chains: the centre-of-mass momentum is removed once unless something is pinned
    nhc = dict(ensemble="nvt", thermostat="Nose-Hoover-Chain", starting_temperature=300.0, seed=5)
    unpinned = MolecularDynamics(s, model=_calc(), **nhc)
    pinned = MolecularDynamics(s, model=_calc(), fixed_atoms=[0], **nhc)
    assert np.abs(unpinned.momenta.sum(0)).max() < 1e-12 * np.abs(unpinned.momenta).sum()
    assert np.array_equal(pinned.momenta[1:], free.momenta[1:]) and not pinned.momenta[0].any()
    # the copy that carries the mask keeps the other site properties
    mag = _li4()
    mag.add_site_property("magmom", [1.0, 2.0, 3.0, 4.0])
    kept = MolecularDynamics(mag, model=_calc(), ensemble="nvt", fixed_atoms=[1]).atoms
    assert kept.site_properties["magmom"] == [1.0, 2.0, 3.0, 4.0] and kept.site_properties["selective_dynamics"][1] == [False] * 3
    # selective_dynamics without the keyword
    sd = _li4()
    sd.add_site_property("selective_dynamics", [[True] * 3, [False] * 3, [True] * 3, [True] * 3])
    assert not MolecularDynamics(sd, model=_calc(), ensemble="nvt", starting_temperature=300.0, seed=5).momenta[1].any()


# ---- 3. the restatement behaves physically -------------------------------------------------------------------------------------------
def _quadratic(n, seed):
    """E = 1/2 (x - x0)^T H (x - x0) with a random SPD H coupling all coordinates: forces -H (x - x0)."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(3 * n, 3 * n))
    H = a @ a.T / (3 * n) + 0.5 * np.eye(3 * n)
    x0 = rng.uniform(1.0, 5.0, (n, 3))
    return H, x0, lambda x: -(H @ (x - x0).ravel()).reshape(n, 3)


@pytest.mark.parametrize("optimizer", ["FIRE", "LBFGS"])
@pytest.mark.parametrize("kind", ["atoms", "components"])
def test_relaxation_converges_on_the_free_coordinates_only(optimizer, kind):
    n = 7
    H, x0, force = _quadratic(n, 3)
    rng = np.random.default_rng(4)
    mask = np.zeros((n, 3), bool)
    if kind == "atoms":
        mask[[0, 3, 6]] = True
    else:
        mask[1, 0] = mask[2, 1:] = mask[5] = mask[6, 2] = True
    cell = np.eye(3) * 20.0
    start = x0 + rng.normal(0, 0.4, (n, 3))
    cls = cref.FixedLbfgsRelaxation if optimizer == "LBFGS" else cref.FixedRelaxation
    r = cls(start @ np.linalg.inv(cell), cell, mask, relax_cell=False, fmax=1e-6, steps=2000)
    q0 = r.q[:n].copy()
    for _ in range(2001):
        if r.status != 0:
            break
        r.advance(force(r.q[:n]), np.zeros((3, 3)))
        assert np.array_equal(r.q[:n][mask], q0[mask])                     # held coordinates never move
    assert r.status == 1, (r.status, r.steps)
    f = force(r.q[:n])
    assert np.sqrt((cref.project(f, mask) ** 2).sum(1).max()) < 1e-6       # converged on the free ones ...
    assert np.abs(f[mask]).max() > 1e-2                                    # ... while the held ones still carry force
    # and it is the constrained minimum: the free block of H solves for the free coordinates
    fr = ~mask.ravel()
    d = np.zeros(3 * n)
    d[~fr] = (q0 - x0).ravel()[~fr]
    d[fr] = -np.linalg.solve(H[np.ix_(fr, fr)], H[np.ix_(fr, ~fr)] @ d[~fr])
    assert np.abs((r.q[:n] - x0).ravel() - d).max() < 1e-5
    # a structure whose only large forces sit on held atoms is converged as it stands
    big = np.where(mask, 5.0, 1e-9)
    r2 = cls(start @ np.linalg.inv(cell), cell, mask, relax_cell=False, fmax=0.05, steps=10)
    assert r2.advance(big, np.zeros((3, 3))) == 1 and r2.steps == 0
    # the finiteness test still sees the raw forces
    r3 = cls(start @ np.linalg.inv(cell), cell, mask, relax_cell=False, fmax=0.05, steps=10)
    bad = force(start)
    bad[np.argwhere(mask)[0][0], np.argwhere(mask)[0][1]] = np.nan
    assert r3.advance(bad, np.zeros((3, 3))) == 3


def test_cell_relaxation_keeps_held_fractional_coordinates():
    """A held atom follows the cell affinely: u is untouched, so frac = u L0^-1 is the same number at every step, while the cell and
    the free atoms move under a force field and a constant stress."""
    n = 5
    _, x0, force = _quadratic(n, 8)
    rng = np.random.default_rng(9)
    cell = np.diag([6.0, 7.0, 8.0]) + rng.normal(0, 0.3, (3, 3))
    mask = np.zeros((n, 3), bool)
    mask[[1, 4]] = True
    for cls in (cref.FixedRelaxation, cref.FixedLbfgsRelaxation):
        r = cls(rng.random((n, 3)), cell, mask, relax_cell=True, fmax=1e-9, steps=50)
        f0 = r.frac().copy()
        for _ in range(25):
            r.advance(force(r.positions()), -0.01 * np.eye(3))
        assert r.steps == 25 and np.abs(r.lattice() - cell).max() > 1e-3
        assert np.array_equal(r.frac()[[1, 4]], f0[[1, 4]]) and np.abs(r.frac()[[0, 2, 3]] - f0[[0, 2, 3]]).max() > 1e-3
    with pytest.raises(AssertionError):
        cref.FixedRelaxation(rng.random((n, 3)), cell, np.eye(n, 3, dtype=bool), relax_cell=True)


def _system(n=12, seed=0, box=5.0):
    rng = np.random.default_rng(seed)
    cell = np.eye(3) * box
    r = rng.random((n, 3)) * box
    m = rng.uniform(6, 60, n)
    p = md_ref.maxwell_boltzmann(m, 300.0, rng)
    return r, cell, m, p


def test_degrees_of_freedom_and_temperature():
    _, _, m, p = _system()
    none = np.zeros((12, 3), bool)
    some = none.copy()
    some[[0, 5]] = True
    some[7, 1] = True
    assert cref.degrees_of_freedom(none) == 36 and cref.degrees_of_freedom(some) == 29
    assert cref.temperature(p, m, none) == md_ref.temperature(p, m)                      # nothing held: exactly as before
    pm = cref.project(p, some)
    assert cref.temperature(pm, m, some) == pytest.approx(md_ref.temperature(pm, m) * 36 / 29, rel=1e-14)
    assert cref.temperature(np.zeros_like(p), m, ~none) == 0.0


def test_nve_conserves_energy_with_pinned_atoms():
    r, cell, m, p = _system(seed=3)
    mask = np.zeros((12, 3), bool)
    mask[[1, 4, 8]] = True
    mask[10, 2] = True
    ref = cref.FixedMDRef(r, cell, m, p, mask, ensemble=md_ref.NVE, dt=2.0 * md_ref.FS, calc=md_ref.pair_potential())
    frames = ref.run(150)
    etot = np.array([f["epot"] + f["ekin"] for f in frames])
    ekin = np.array([f["ekin"] for f in frames])
    for f in frames:
        assert np.array_equal(f["positions"][mask], r[mask]) and not f["momenta"][mask].any() and not f["forces"][mask].any()
    assert np.abs(frames[-1]["positions"][~mask] - r[~mask]).max() > 0.1
    # velocity Verlet: the total energy fluctuates at O((w dt)^2) of the energy that kinetic and potential exchange
    exchange = ekin.max() - ekin.min()
    print("NVE pinned: |dE| max", np.abs(etot - etot[0]).max(), "exchange", exchange)
    assert np.abs(etot - etot[0]).max() < 1e-2 * exchange


def _secular_drift(h, blocks=10):
    """Drift of H over the run and its standard error: the slope of a line fitted to the means of `blocks` consecutive blocks (each
    spans two thermostat periods, so the O(dt^2) oscillation averages out inside a block and the block means scatter independently
    about the line), times the length of the run."""
    h = np.asarray(h[1:], np.float64)
    length = len(h) // blocks
    means = h[:blocks * length].reshape(blocks, length).mean(axis=1)
    t = (np.arange(blocks) + 0.5) * length
    design = np.vstack([t, np.ones(blocks)]).T
    coef = np.linalg.lstsq(design, means, rcond=None)[0]
    resid = means - design @ coef
    se = np.sqrt(resid @ resid / (blocks - 2) / ((t - t.mean()) ** 2).sum())
    return abs(coef[0]) * len(h), se * len(h)


@pytest.mark.parametrize("npt", [False, True], ids=["nvt", "npt"])
def test_nhc_conserved_energy_drifts_no_more_than_unconstrained(npt):
    """The same system with and without four pinned atoms, one statistic on both runs and no number of its own: the secular drift of
    H over 400 steps (_secular_drift) of the constrained run is no larger than that of the unconstrained run, beyond what the two
    runs' own standard errors (two of each) leave open.  Measured, eV over the run: NVT 2.0e-5 +- 0.9e-5 constrained against
    1.1e-5 +- 0.3e-5 unconstrained, NPT 1.0e-5 +- 0.6e-5 against 6.4e-5 +- 2.2e-5.  (The largest excursion of H is no such statistic:
    it is the amplitude of the O(dt^2) oscillation, which belongs to the trajectory -- 6.1e-5 against 2.9e-5 NVT, 3.0e-5 against
    7.3e-5 NPT -- and shrinks fourfold with half the step in both runs.)"""
    import nhc_ref

    r, cell, m, p = _system(seed=5)
    mask = np.zeros((12, 3), bool)
    rows = [0, 3, 7, 9]
    mask[rows] = True

    def runs(dt_fs, steps):
        kw = dict(npt=npt, dt=dt_fs * md_ref.FS, temperature_k=300.0, taut=20.0 * md_ref.FS, taup=200.0 * md_ref.FS, chain_length=3,
                  calc=md_ref.pair_potential())
        free = nhc_ref.NHCRef(r, cell, m, nhc_ref.remove_com_momentum(p, m), **kw)
        fixed = cref.FixedNHCRef(r, cell, m, p, mask, **kw)
        return free, fixed, free.run(steps), fixed.run(steps)

    free, fixed, ff, fx = runs(1.0, 400)
    assert fixed.nf == 24 and free.nf == 33 and fixed.alpha == 1 + 3 / 24 and fixed.Q[0] == 24 * fixed.Q[1] and fixed.W == 27 * fixed.Qb[0]
    h = lambda frames: np.array([f["conserved"] for f in frames]) - frames[0]["conserved"]  # noqa: E731
    excursion = lambda frames: np.abs(h(frames)).max()  # noqa: E731
    (d_ff, se_ff), (d_fx, se_fx) = _secular_drift(h(ff)), _secular_drift(h(fx))
    print("NHC", "npt" if npt else "nvt", "secular drift of H over the run: unconstrained", d_ff, "+-", se_ff, "constrained", d_fx, "+-", se_fx,
          "largest excursion: unconstrained", excursion(ff), "constrained", excursion(fx))
    assert d_fx <= d_ff + 2.0 * (se_fx + se_ff)
    _, _, _, fx_half = runs(0.5, 400)                                        # the first 200 fs once more at half the step
    assert 3.0 < excursion(fx[:201]) / excursion(fx_half) < 5.0             # second order: a quarter of the error
    for f in fx:
        assert not f["momenta"][mask].any()
        assert np.abs(f["positions"][rows] @ np.linalg.inv(f["cell"]) - r[rows] @ np.linalg.inv(cell)).max() < 1e-13    # scale with the cell
    if not npt:
        assert all(np.array_equal(f["positions"][rows], r[rows]) for f in fx)
    # with 3 (n - 1) = 33 in the N_f kT eta_1 term the same trajectory would be off by 9 kT eta_1: far more than it wanders
    assert 9 * fixed.kt * abs(fixed.eta[0]) > 10 * excursion(fx), (fixed.eta, excursion(fx))


def test_langevin_thermalises_the_free_components():
    """Six of twelve atoms pinned, harmonic wells (w dt = 0.02: no visible discretisation bias), no fixcm.  The estimator
    2 Ekin / (dof kB) averages 18 Gaussian momenta per frame; frames are correlated over 1 / (2 friction dt) = 5 steps, so the 2700
    frames after equilibration hold ~270 independent samples: relative width sqrt(2 / (18 * 270)) = 2.0 %, bar at 5 widths.  With
    3 n in the denominator the same run reads half the target."""
    rng = np.random.default_rng(11)
    n, t0 = 12, 400.0
    cell = np.eye(3) * 30.0
    wells = rng.uniform(5, 25, (n, 3))
    m = rng.uniform(15, 40, n)
    mask = np.zeros((n, 3), bool)
    mask[::2] = True

    def calc(r, cell):  # noqa: ARG001
        d = r - wells
        return 0.5 * float((d ** 2).sum()), -d, np.zeros((3, 3))

    lan = cref.FixedLangevinRef(wells + rng.normal(0, 0.05, (n, 3)), cell, m, None, mask, dt=1.0 * md_ref.FS, temperature_k=t0,
                                friction=0.1 / md_ref.FS, seed=17, fixcm=False, calc=calc)
    start = lan.r.copy()
    frames = lan.run(3000)
    late = frames[300:]
    t_dof = np.mean([f["temperature"] for f in late])
    t_3n = np.mean([md_ref.temperature(f["momenta"], m) for f in late])
    print("Langevin pinned: T with dof", t_dof, "with 3n", t_3n, "target", t0)
    assert abs(t_dof - t0) < 5 * np.sqrt(2 / (18 * 270)) * t0
    assert abs(t_3n - 0.5 * t0) < 5 * np.sqrt(2 / (18 * 270)) * 0.5 * t0
    assert all(np.array_equal(f["positions"][mask], start[mask]) and not f["momenta"][mask].any() for f in frames)
    # the noise of a free atom does not depend on the mask: the same seed without a mask moves atom 1 the same way in the first step
    free = cref.FixedLangevinRef(start, cell, m, None, None, dt=1.0 * md_ref.FS, temperature_k=t0, friction=0.1 / md_ref.FS, seed=17,
                                 fixcm=False, calc=calc)
    assert np.array_equal(free.run(1)[1]["momenta"][1], frames[1]["momenta"][1])
