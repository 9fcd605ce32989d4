"""CPU checks of the flexible-cell Nose-Hoover-chain NPT restatement (tests/nhc_flex_ref.py) and of its plumbing without a GPU: second
order of the conserved energy, time reversal, symmetry of the strain-rate matrix, the isotropic limit of every piece against
tests/nhc_ref.py, the matrix exponential, the sampled pressure tensor, keyword validation and held atoms.

The system is a four-atom close-packed cell (a = 5.2 A, nearest neighbours at 3.7 A) with ``md_ref.pair_potential(eps=200, rc=4.5)``: a
purely repulsive solid is stable against shear only when close packed -- a simple cubic or fluid arrangement lets a flexible cell
collapse to a needle within picoseconds, where the potential's 27 images no longer suffice.  The static pressure of this lattice is
0.23 eV/A^3, which is the external pressure used, so the volume stays where it starts.  Every run asserts that the cell stays wider
than the cutoff."""

from __future__ import annotations

import copy
import os
import re

import numpy as np
import pytest

import md_ref
import nhc_flex_ref
import nhc_ref
from conftest import REPO

FS = md_ref.FS
RC, EPS = 4.5, 200.0
T0 = 300.0
PEXT = 0.23                                    # eV/A^3
SHEAR = 0.15 * np.array([[0.0, 0.4, -0.3], [0.5, 0.0, 0.2], [-0.2, 0.3, 0.0]])
MODES = ("flexible", "axes")


def _system(sheared, seed=0, a=5.2, jitter=0.05):
    rng = np.random.default_rng(seed)
    frac = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]], np.float64)
    cell = np.eye(3) * a + (SHEAR if sheared else 0.0)
    r = frac @ cell + rng.normal(0, jitter, (4, 3))
    m = rng.uniform(10, 40, 4)
    p = nhc_ref.remove_com_momentum(md_ref.maxwell_boltzmann(m, T0, rng), m)
    return r, cell, m, p


def _ref(mode, dt_fs, *, sheared=True, chain_length=3, mask=None, seed=0):
    r, cell, m, p = _system(sheared, seed)
    return nhc_flex_ref.NHCFlexRef(r, cell, m, p, cell_dof=mode, mask=mask, dt=dt_fs * FS, temperature_k=T0, taut=20 * FS, taup=100 * FS,
                                   pressure=PEXT, chain_length=chain_length, calc=md_ref.pair_potential(eps=EPS, rc=RC))


def _min_height(cell):
    vol = abs(np.linalg.det(cell))
    return min(vol / np.linalg.norm(np.cross(cell[i - 1], cell[i - 2])) for i in range(3))


# ---- 1. second order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_conserved_quantity_is_second_order(mode):
    """max |H - H_0| over 200 fs at 2, 1 and 0.5 fs: each halving divides it by 3.5 to 4.5."""
    drift = []
    for dt_fs in (2.0, 1.0, 0.5):
        frames = _ref(mode, dt_fs).run(int(round(200 / dt_fs)))
        h = np.array([f["conserved"] for f in frames])
        drift.append(np.abs(h - h[0]).max())
        margin = min(_min_height(f["cell"]) for f in frames) - RC
        print(mode, dt_fs, "fs: max |H - H0|", drift[-1], "eV, cell wider than the cutoff by", margin, "A")
        assert margin > 0.1                                               # the 27-image sum stays valid with room to spare
    print(mode, "ratios", drift[0] / drift[1], drift[1] / drift[2])
    assert 3.5 <= drift[0] / drift[1] <= 4.5 and 3.5 <= drift[1] / drift[2] <= 4.5, drift


# ---- 2. time reversal ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chain_length", [1, 4])
def test_time_reversal(mode, chain_length):
    ref = _ref(mode, 2.0, chain_length=chain_length)
    start = copy.deepcopy(ref)
    ref.run(50)
    moved, sheared = np.abs(ref.r - start.r).max(), np.abs(ref.cell - start.cell).max()
    assert _min_height(ref.cell) > RC
    ref.reverse()
    ref.run(50)
    ref.reverse()
    assert moved > 0.05 and sheared > 0.01
    errs = {name: np.abs(getattr(ref, name) - getattr(start, name)).max() / np.abs(getattr(start, name)).max() for name in ("r", "cell", "p")}
    print(mode, chain_length, errs)
    assert errs["r"] <= 1e-11 and errs["cell"] <= 1e-11 and errs["p"] <= 1e-9, errs
    assert np.abs(ref.Vg - start.Vg).max() <= 1e-9 * 1e-3                   # starts at 0: against the 1e-3 / fs it reaches on the way


# ---- 3. symmetry of the strain rate ---------------------------------------------------------------------------------------------------
def test_strain_rate_stays_symmetric_and_axes_keep_the_angles():
    flex = _ref("flexible", 2.0)
    for _ in range(40):
        flex.step()
        assert np.array_equal(flex.Vg, flex.Vg.T)
    assert np.abs(flex.Vg - np.diag(np.diag(flex.Vg))).max() > 1e-3 * np.abs(flex.Vg).max()      # the angles do move
    axes = _ref("axes", 2.0, sheared=False)
    h0 = axes.cell.copy()
    for _ in range(40):
        axes.step()
        assert not (axes.Vg - np.diag(np.diag(axes.Vg))).any()            # exactly 0
        assert not (axes.cell - np.diag(np.diag(axes.cell))).any()        # an orthorhombic cell stays orthorhombic
    lengths = np.diag(axes.cell) / np.diag(h0)
    assert np.ptp(lengths) > 1e-3                                          # and its axes move independently


# ---- 4. the isotropic limit of the pieces ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_pieces_reduce_to_the_isotropic_integrator(mode):
    r, cell, m, p = _system(True)
    kw = dict(dt=2.0 * FS, temperature_k=T0, taut=20 * FS, taup=100 * FS, pressure=PEXT, chain_length=3)
    rng = np.random.default_rng(5)
    forces, stress = rng.normal(0, 0.5, r.shape), rng.normal(0, 0.05, (3, 3))
    veps, tau = 3e-3, FS
    iso, flex = nhc_ref.NHCRef(r, cell, m, p, npt=True, **kw), nhc_flex_ref.NHCFlexRef(r, cell, m, p, cell_dof=mode, **kw)
    iso.veps, flex.Vg = veps, veps * np.eye(3)

    def rel(a, b):
        return np.abs(a - b).max() / np.abs(b).max()

    iso.particle_kick(forces, tau)
    flex.particle_kick(forces, tau)
    assert rel(flex.p, iso.p) <= 1e-15
    e = np.exp(0.5 * iso.veps * iso.dt)                                    # NHCRef's drift
    r_iso, h_iso = (iso.r * e + iso.dt * iso.p / iso.m[:, None]) * e, iso.cell * np.exp(iso.veps * iso.dt)
    flex.p = iso.p.copy()
    flex.drift()
    assert rel(flex.r, r_iso) <= 1e-15 and rel(flex.cell, h_iso) <= 1e-15
    # the barostat kick with the isotropic part of the stress: its trace / 3 is the veps kick, its deviator only the kinetic one's
    iso, flex = nhc_ref.NHCRef(r, cell, m, p, npt=True, **kw), nhc_flex_ref.NHCFlexRef(r, cell, m, p, cell_dof=mode, **kw)
    iso.veps, flex.Vg = veps, veps * np.eye(3)
    iso.barostat_kick(stress, tau)
    flex.barostat_kick(np.trace(stress) / 3.0 * np.eye(3), tau)
    terms = tau * max(iso.alpha * iso.k2(), abs(iso.volume() * np.trace(stress)), 3 * iso.pext * iso.volume()) / iso.W
    assert abs(np.trace(flex.Vg) / 3.0 - iso.veps) <= 4e-16 * max(terms, abs(veps))
    assert flex.W == iso.W and flex.Wg == iso.W / 3.0 and flex.db == (6 if mode == "flexible" else 3)
    assert flex.Qb[0] == flex.db * flex.kt * flex.taup ** 2 and np.all(flex.Qb[1:] == flex.kt * flex.taup ** 2)


# ---- 5. the matrix exponential ---------------------------------------------------------------------------------------------------------
def test_matrix_exponential_against_scipy():
    from scipy.linalg import expm

    q, _ = np.linalg.qr(np.random.default_rng(2).normal(size=(3, 3)))
    cases = {"zero": np.zeros((3, 3)), "multiple of I": -0.37 * np.eye(3), "two equal eigenvalues": q @ np.diag([0.2, 0.2, -0.5]) @ q.T,
             "a strain-rate step": 1e-3 * np.array([[1.0, 0.3, -0.2], [0.3, -2.0, 0.5], [-0.2, 0.5, 0.7]])}
    for name, a in cases.items():
        a = 0.5 * (a + a.T)
        got = nhc_flex_ref.expm_sym(a)
        assert np.array_equal(got, got.T), name
        assert np.abs(got - expm(a)).max() <= 1e-14, name
        assert np.abs(got @ nhc_flex_ref.expm_sym(-a) - np.eye(3)).max() <= 1e-14, name
    assert np.array_equal(nhc_flex_ref.expm_sym(np.zeros((3, 3))), np.eye(3))


# ---- 6. the sampled pressure tensor (statistical, fixed seed) ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_mean_pressure_tensor_is_the_external_pressure(mode):
    """A statistical check with a fixed seed: 6 ps at 2 fs, the second half in 8 blocks.  Every free component of the mean pressure
    tensor (``NHCFlexRef.pressure_tensor``) lies within 3 standard errors of Pext delta_ab, the standard error from the block means, as
    ``_block_test`` of test_nhc_cpu.py does for the isotropic barostat.  For "axes" the cell is orthorhombic and only the diagonal is
    free: nothing relaxes a shear stress there."""
    ref = _ref(mode, 2.0, sheared=mode == "flexible")
    pres, heights = [], []
    ref.evaluate()
    for _ in range(3000):
        ref.step()
        pres.append(ref.pressure_tensor())
        heights.append(_min_height(ref.cell))
    assert min(heights) > RC + 0.1
    pres = np.array(pres[len(pres) // 2:])
    blocks = pres[: len(pres) // 8 * 8].reshape(8, -1, 3, 3).mean(axis=1)
    se = blocks.std(axis=0, ddof=1) / np.sqrt(8)
    dev = (pres.mean(axis=0) - PEXT * np.eye(3)) / se
    print(mode, "mean pressure tensor", pres.mean(axis=0).tolist(), "deviation / standard error", dev.tolist())
    assert np.all(np.abs(dev[ref.free]) <= 3.0), dev
    assert np.all(se[ref.free] < 0.01 * PEXT)                             # and the run resolves a percent of Pext


# ---- 7. keyword validation ---------------------------------------------------------------------------------------------------------------
def _li2():
    from chgnet_amd.graph.structure import Lattice, Structure

    return Structure(Lattice(np.eye(3) * 3.5), np.array([3, 3]), np.array([[0, 0, 0], [0.5, 0.5, 0.5]]))


def _calc():
    from chgnet_amd.calculator import CHGNetCalculator

    return CHGNetCalculator.__new__(CHGNetCalculator)                     # no engine: nothing runs here


NPT_CHAIN = dict(ensemble="npt", thermostat="Nose-Hoover-Chain")


@pytest.mark.parametrize(("kwargs", "match"), [
    (dict(NPT_CHAIN, cell_dof="triclinic"), "cell_dof"),
    (dict(NPT_CHAIN, cell_dof="Flexible"), "cell_dof"),
    (dict(NPT_CHAIN, cell_dof=None), "cell_dof"),
    (dict(ensemble="nvt", thermostat="Nose-Hoover-Chain", cell_dof="flexible"), "cell_dof"),
    (dict(ensemble="npt", thermostat="Berendsen_inhomogeneous", bulk_modulus=100.0, cell_dof="axes"), "cell_dof"),
    (dict(ensemble="npt", thermostat="npt_berendsen", bulk_modulus=100.0, cell_dof="flexible"), "cell_dof"),
    (dict(ensemble="nvt", thermostat="Langevin", cell_dof="axes"), "cell_dof"),
    (dict(ensemble="nve", cell_dof="flexible"), "cell_dof"),
    (dict(NPT_CHAIN, cell_dof="flexible", pressure=np.full((3, 3), 1e-4)), "pressure"),
    (dict(NPT_CHAIN, cell_dof="axes", pressure=[1e-4] * 3), "pressure"),
    (dict(NPT_CHAIN, cell_dof="flexible", chain_length=5), "chain_length"),
    (dict(NPT_CHAIN, cell_dof="flexible", temperature=0.0), "temperature"),
])
def test_keyword_validation(kwargs, match):
    from chgnet_amd.dynamics import MolecularDynamics

    with pytest.raises(ValueError, match=match):
        MolecularDynamics(_li2(), model=_calc(), **kwargs)


def test_isotropic_is_what_omitting_the_keyword_gives():
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.graph.structure import Lattice, Structure

    plain = MolecularDynamics(_li2(), model=_calc(), timestep=1.5, **NPT_CHAIN)
    named = MolecularDynamics(_li2(), model=_calc(), timestep=1.5, cell_dof="isotropic", **NPT_CHAIN)
    assert named.kind == plain.kind == "npt_nhc" and named.cfg == plain.cfg and "cell_dof" not in plain.cfg
    assert named.cell_dof == plain.cell_dof == "isotropic" and named.chain_length == plain.chain_length == 3
    for ens, th in (("nvt", "Berendsen"), ("nve", "Berendsen"), ("nvt", "Langevin"), ("nvt", "Nose-Hoover-Chain")):
        assert MolecularDynamics(_li2(), model=_calc(), ensemble=ens, thermostat=th, cell_dof="isotropic").cell_dof == "isotropic"
    for mode in MODES:
        md = MolecularDynamics(_li2(), model=_calc(), cell_dof=mode, **NPT_CHAIN)
        assert md.kind == "npt_nhc" and md.cfg["cell_dof"] == mode and md.bulk_modulus is None and md.thermostat_state is None
    one = Structure(Lattice(np.eye(3) * 3.5), np.array([3]), np.array([[0.0, 0.0, 0.0]]))
    with pytest.raises(ValueError, match="one atom"):
        MolecularDynamics(one, model=_calc(), cell_dof="flexible", **NPT_CHAIN)
    with pytest.raises(ValueError, match="only some cartesian components"):           # a partially held atom under a moving cell
        MolecularDynamics(_li2(), model=_calc(), cell_dof="flexible", fixed_atoms=np.array([[True, False, False], [False] * 3]), **NPT_CHAIN)


def test_abi_gains_entry_points_without_a_bump():
    from chgnet_amd import _lib

    with open(os.path.join(REPO, "include", "chgnet_hip.h")) as fh:
        header = fh.read()
    assert int(re.search(r"#define\s+CHG_ABI_VERSION\s+(\d+)", header).group(1)) == 5 == _lib.ABI_VERSION
    lib = _lib.load()
    for name in ("chg_md_create_nhc_flex", "chg_md_download_vg", "chg_test_md_step_nhc_flex"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(rf"\b{name}\s*\(", header), name
    assert len(lib.chg_md_create_nhc_flex.argtypes) == len(lib.chg_md_create_nhc.argtypes) + 1
    assert len(lib.chg_test_md_step_nhc_flex.argtypes) == len(lib.chg_test_md_step_nhc.argtypes) + 2
    assert int(re.search(r"#define\s+CHG_MD_VG\s+(\d+)", header).group(1)) == _lib.MD_VG == 9
    assert lib.chg_md_create_nhc_flex(None, None, None, None, None, 3, 1, None) != 0       # null arguments: refused before any device call
    assert lib.chg_md_download_vg(None, None, None) != 0


# ---- 8. held atoms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_held_atoms_follow_the_cell_and_leave_the_sums(mode):
    mask = np.zeros((4, 3), bool)
    mask[[0, 3]] = True
    ref = _ref(mode, 1.0, mask=mask)
    free = ~mask[:, 0]
    assert ref.nf == 6 and ref.alpha == 1.5                                # the free components, not 3 (n - 1) = 9
    for got, want in ((ref.Q[0], 6 * ref.kt * ref.taut ** 2), (ref.W, 9 * ref.kt * ref.taup ** 2), (ref.Wg, 3 * ref.kt * ref.taup ** 2)):
        assert abs(got - want) <= 4e-16 * want
    assert not ref.p[~free].any()
    frac0, h0 = ref.r @ np.linalg.inv(ref.cell), ref.cell.copy()
    # one first half by hand, from the equations, with the held rows left out of every sum
    e0, f0, s0 = ref.evaluate()
    assert not f0[~free].any()
    by_hand = copy.deepcopy(ref)
    tau = 0.5 * ref.dt
    pf, mf = ref.p[free], ref.m[free]
    by_hand.p = by_hand.p * by_hand.chain(by_hand.v, by_hand.eta, by_hand.Q, float(np.vdot(pf, pf / mf[:, None])), 6, tau)
    pf = by_hand.p[free]
    k2, vol = float(np.vdot(pf, pf / mf[:, None])), abs(np.linalg.det(h0))
    g = np.einsum("ka,kb,k->ab", pf, pf, 1.0 / mf) + (k2 / 6 - PEXT * vol) * np.eye(3) - vol * 0.5 * (s0 + s0.T)
    vg = np.where(ref.free, tau * g / ref.Wg, 0.0)
    ref.first_half(f0, s0)
    assert np.abs(ref.Vg - vg).max() <= 1e-14 * np.abs(vg).max()
    assert np.abs(ref.cell - h0 @ nhc_flex_ref.expm_sym(vg * ref.dt)).max() <= 1e-14 * np.abs(h0).max()
    ref.second_half(*ref.evaluate()[1:])
    for _ in range(30):
        ref.step()
        assert not ref.p[~free].any()
        assert ref.k2() == float(np.vdot(ref.p[free], ref.p[free] / ref.m[free][:, None]))
    assert np.abs(ref.cell - h0).max() > 1e-3 and _min_height(ref.cell) > RC
    held_frac = ref.r[~free] @ np.linalg.inv(ref.cell)
    assert np.abs(held_frac - frac0[~free]).max() <= 1e-12                 # affine: the held rows keep their fractional coordinates
    assert np.abs(ref.r[free] @ np.linalg.inv(ref.cell) - frac0[free]).max() > 1e-3
    fr = ref.frame()
    assert abs(fr["temperature"] - 2.0 * fr["ekin"] / (6 * md_ref.KB)) <= 1e-12 * fr["temperature"]
