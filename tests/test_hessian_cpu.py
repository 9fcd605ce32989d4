"""Hessian-vector products and force constants, CPU part: the C-ABI entry point is declared, bound and exported; the Gamma
frequencies of a two-mass spring; argument validation; the float64 finite-difference reference the GPU tests compare against is
converged, also at the exactly collinear triplets of rock salt."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO


def test_hessian_vector_entry_point_is_declared_bound_and_exported():
    from chgnet_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "chgnet_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+chg_hessian_vector\s*\(\s*chg_engine\*\s*\w+,\s*chg_batch\*\s*\w+,\s*const float\*\s*\w+,\s*float\*\s*\w+\)", text)
    assert "chg_hessian_vector" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "chg_hessian_vector") and len(lib.chg_hessian_vector.argtypes) == 4
    assert _lib.ABI_VERSION == 5


def test_gamma_frequencies_of_a_two_mass_spring():
    from chgnet_amd import Structure, gamma_frequencies
    from chgnet_amd.dynamics import ATOMIC_MASSES

    s = Structure(np.eye(3) * 10.0, ["Li", "F"], [[0, 0, 0], [0.2, 0, 0]])
    for k in (3.7, -0.8):                       # eV/A^2; a negative spring gives an unstable mode
        h = np.zeros((6, 6))
        h[np.ix_([0, 3], [0, 3])] = k * np.array([[1.0, -1.0], [-1.0, 1.0]])
        mu = 1.0 / (1.0 / ATOMIC_MASSES[3] + 1.0 / ATOMIC_MASSES[9])
        # omega = sqrt(k / mu) in sqrt(eV / (A^2 amu)) -> rad/s -> THz (CODATA 2014: e, amu)
        want = np.sqrt(abs(k) / mu * 1.6021766208e-19 / (1e-20 * 1.660539040e-27)) / (2 * np.pi * 1e12)
        f = gamma_frequencies(s, h)
        assert f.shape == (6,) and np.all(np.diff(f) >= 0)
        if k > 0:
            assert np.allclose(f[:5], 0.0, atol=1e-6) and f[5] == pytest.approx(want, rel=1e-12)
        else:
            assert f[0] == pytest.approx(-want, rel=1e-12) and np.allclose(f[1:], 0.0, atol=1e-6)
    assert want == pytest.approx(6.20, abs=0.01)   # 0.8 eV/A^2 between Li and F (reduced mass 5.08 amu): 6.2 THz
    with pytest.raises(ValueError, match="needs"):
        gamma_frequencies(s, np.zeros((5, 5)))


def test_hessian_vector_product_validates_its_arguments():
    from chgnet_amd import CHGNet
    from chgnet_amd.model import random_state_dict
    from hessian_ref import lif_structure

    model = CHGNet(state_dict=random_state_dict({}, seed=0))
    prim, conv = lif_structure(False), lif_structure(True)
    with pytest.raises(ValueError, match=r"expected \(2, 3\)"):
        model.hessian_vector_product(prim, np.zeros((3, 3)))
    with pytest.raises(ValueError, match=r"expected \(8, 3\)"):
        model.hessian_vector_product([prim, conv], [np.zeros((2, 3)), np.zeros(8)])
    with pytest.raises(ValueError, match="2 structures but 1 directions"):
        model.hessian_vector_product([prim, conv], [np.zeros((2, 3))])
    with pytest.raises(TypeError, match="Structure or a CrystalGraph"):
        model.predict_hessian([prim, "LiF"])
    assert model._engine is None                  # nothing reached the device


@pytest.mark.parametrize("weights", ["weights_seed0.npz", "weights_trained_like.npz"])
def test_finite_difference_reference_is_converged(weights):
    """The GPU tests' reference: central differences of the float64 oracle's forces at 1e-5 A.  Halving the step changes it by
    <= 3e-5 max|H| (a tenth of the GPU bar) -- also on rock salt, whose collinear triplets have an angle curvature scale of only
    sin(theta) ~ 1.4e-3 rad; the reference is symmetric and obeys the acoustic sum rule to that level too."""
    import torch

    from chgnet_amd.graph.converter import CrystalGraphConverter
    from hessian_ref import fd_hessian, lif_structure
    from oracle.chgnet_oracle import OracleCHGNet

    torch.set_num_threads(8)
    oracle = OracleCHGNet(dict(np.load(os.path.join(GOLDEN, weights))), dtype=torch.float64)
    conv = CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3)
    for structure in (lif_structure(True), lif_structure(True, rattle=0.01), lif_structure(False)):
        g = conv(structure)
        assert len(g.bond_graph) > 0
        h1, h2 = fd_hessian(oracle, g, 1e-5), fd_hessian(oracle, g, 5e-6)
        scale = float(np.abs(h1).max())
        assert np.abs(h1 - h2).max() <= 3e-5 * scale
        assert np.abs(h1 - h1.T).max() <= 3e-5 * scale
        assert np.abs(h1.reshape(3 * len(g.atomic_number), -1, 3).sum(1)).max() <= 3e-5 * scale


def test_rock_salt_cell_has_exactly_collinear_triplets():
    from chgnet_amd.graph.converter import CrystalGraphConverter
    from hessian_ref import lif_structure

    g = CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3)(lif_structure(True))
    lat = np.asarray(g.lattice, np.float64)
    cart = np.asarray(g.atom_frac_coord, np.float64) @ lat
    ag = np.asarray(g.atom_graph)
    v = cart[ag[:, 0]] - cart[ag[:, 1]] - np.asarray(g.neighbor_image, np.float64) @ lat
    u = v / np.linalg.norm(v, axis=1, keepdims=True)
    bg = np.asarray(g.bond_graph)
    c = (u[bg[:, 2]] * u[bg[:, 4]]).sum(1)
    assert np.isclose(c, -1.0, atol=1e-12).sum() >= 8
