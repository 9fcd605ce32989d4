"""Strain blocks of the Hessian and elastic constants, CPU part: the C-ABI entry point is declared, bound and exported; the host
algebra (Voigt strains, relaxed-ion correction, Voigt / Reuss / Hill moduli); argument validation; the float64 finite-difference
reference the GPU tests compare against is converged, symmetric and agrees with second differences of the energy."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO


def _oracle(weights="weights_seed0.npz"):
    import torch

    from oracle.chgnet_oracle import OracleCHGNet

    torch.set_num_threads(8)
    return OracleCHGNet(dict(np.load(os.path.join(GOLDEN, weights))), dtype=torch.float64)


def _lif(conventional, rattle=0.0, seed=0):
    from chgnet_amd.graph.converter import CrystalGraphConverter
    from hessian_ref import lif_structure

    return CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3)(lif_structure(conventional, rattle, seed))


def test_hessian_vector_strain_entry_point_is_declared_bound_and_exported():
    import chgnet_amd
    from chgnet_amd import _lib
    from chgnet_amd.elastic import elastic_moduli

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "chgnet_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+chg_hessian_vector_strain\s*\(\s*chg_engine\*\s*\w+,\s*chg_batch\*\s*\w+,\s*const float\*\s*\w+,\s*"
                     r"const float\*\s*\w+,\s*float\*\s*\w+,\s*float\*\s*\w+\)", text)
    assert "chg_hessian_vector_strain" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "chg_hessian_vector_strain") and len(lib.chg_hessian_vector_strain.argtypes) == 6
    assert _lib.ABI_VERSION == 5
    assert chgnet_amd.elastic_moduli is elastic_moduli


def test_voigt_strains_and_the_moduli_of_a_cubic_tensor():
    from chgnet_amd.elastic import elastic_moduli, to_voigt, voigt_strains

    w = voigt_strains()
    assert np.array_equal(w[0], np.diag([1.0, 0, 0])) and np.array_equal(w[2], np.diag([0, 0, 1.0]))
    assert w[3][1, 2] == w[3][2, 1] == 0.5 and w[4][0, 2] == w[4][2, 0] == 0.5 and w[5][0, 1] == w[5][1, 0] == 0.5
    assert np.array_equal(to_voigt([[1, 6, 5], [6, 2, 4], [5, 4, 3]]), [1, 2, 3, 4, 5, 6])
    c11, c12, c44 = 250.0, 110.0, 80.0
    c = np.zeros((6, 6))
    c[:3, :3] = c12
    c[np.arange(3), np.arange(3)] = c11
    c[np.arange(3, 6), np.arange(3, 6)] = c44
    m = elastic_moduli(c)
    assert m["K_V"] == pytest.approx((c11 + 2 * c12) / 3, rel=1e-12)
    assert m["K_R"] == pytest.approx((c11 + 2 * c12) / 3, rel=1e-12)
    assert m["G_V"] == pytest.approx((c11 - c12 + 3 * c44) / 5, rel=1e-12)
    assert m["G_R"] == pytest.approx(5 * (c11 - c12) * c44 / (4 * c44 + 3 * (c11 - c12)), rel=1e-12)
    assert m["K_VRH"] == pytest.approx(0.5 * (m["K_V"] + m["K_R"])) and m["G_VRH"] == pytest.approx(0.5 * (m["G_V"] + m["G_R"]))
    assert m["G_R"] < m["G_V"]
    with pytest.raises(ValueError, match="expected"):
        elastic_moduli(np.eye(3))


def test_relaxed_ion_correction_of_a_two_atom_spring():
    """Two atoms joined by an isotropic spring k: Phi = k [[I, -I], [-I, I]], Lambda = [a; -a] -> Lambda^T Phi^+ Lambda = a^T a / k
    (the relative coordinate carries stiffness 2k and coupling 2a); the translations do not enter."""
    from chgnet_amd.elastic import EV_A3_TO_GPA, min_phonon_eigenvalue, relaxed_ion_tensor

    rng = np.random.default_rng(0)
    k, vol = 3.0, 40.0
    phi = k * np.block([[np.eye(3), -np.eye(3)], [-np.eye(3), np.eye(3)]])
    a = rng.normal(size=(3, 6))
    lam = np.concatenate([a, -a])
    clamped = np.diag(np.full(6, 500.0))
    got = relaxed_ion_tensor(clamped, lam, phi, vol)
    assert np.allclose(got, clamped - a.T @ a / k * EV_A3_TO_GPA / vol, rtol=1e-12, atol=1e-9)
    assert min_phonon_eigenvalue(phi) == pytest.approx(2 * k, rel=1e-12)
    assert np.array_equal(relaxed_ion_tensor(clamped, lam[:3], phi[:3, :3], vol), clamped)   # one atom: nothing to relax
    assert np.isnan(min_phonon_eigenvalue(phi[:3, :3]))


def test_strain_products_validate_their_arguments():
    from chgnet_amd import CHGNet
    from chgnet_amd.model import random_state_dict
    from hessian_ref import lif_structure

    model = CHGNet(state_dict=random_state_dict({}, seed=0))
    prim, conv = lif_structure(False), lif_structure(True)
    with pytest.raises(ValueError, match=r"expected \(2, 3\)"):
        model.hessian_vector_product_with_strain(prim, np.zeros((3, 3)), np.zeros((3, 3)))
    with pytest.raises(ValueError, match=r"strain 0 has shape \(2, 3\)"):
        model.hessian_vector_product_with_strain(prim, np.zeros((2, 3)), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="2 structures but 1 strains"):
        model.hessian_vector_product_with_strain([prim, conv], [np.zeros((2, 3)), np.zeros((8, 3))], [np.eye(3)])
    with pytest.raises(ValueError, match="2 structures but 1 directions"):
        model.hessian_vector_product_with_strain([prim, conv], [np.zeros((2, 3))], [np.eye(3)] * 2)
    with pytest.raises(TypeError, match="Structure or a CrystalGraph"):
        model.predict_elastic_tensor([prim, "LiF"])
    assert model._engine is None                  # nothing reached the device


@pytest.mark.parametrize("weights", ["weights_seed0.npz", "weights_trained_like.npz"])
def test_strain_reference_is_converged(weights):
    """Halving the 1e-5 step changes hx and hs by <= 3e-5 of their scales (a tenth of the GPU bar), on the primitive LiF cell
    (self-image bonds only), rattled conventional LiF and a golden graph."""
    from conftest import load_case
    from elastic_ref import fd_hvp_strain

    oracle = _oracle(weights)
    graphs = [_lif(False), _lif(True, 0.01), load_case("limno2")[0]]
    rng = np.random.default_rng(1)
    dirs = [rng.normal(size=(len(g.atomic_number), 3)) for g in graphs]
    ws = [rng.normal(size=(3, 3)) for _ in graphs]
    a, b = fd_hvp_strain(oracle, graphs, dirs, ws, 1e-5), fd_hvp_strain(oracle, graphs, dirs, ws, 5e-6)
    for (hx1, hs1), (hx2, hs2) in zip(a, b):
        assert np.abs(hx1 - hx2).max() <= 3e-5 * np.abs(hx1).max()
        assert np.abs(hs1 - hs2).max() <= 3e-5 * np.abs(hs1).max()


def test_strain_reference_converges_for_the_scaled_weights_legs():
    """The references of tests/test_gpu_elastic.py's scaled-weights legs, along the strain directions that test uses: linear weights
    x 4 at the 1e-5 step (limno2, s16tri), x 100 on limno2 at 2.5e-7 -- halving the step changes hx and hs by <= 3e-5 of scale.
    (x 100 at the 1e-6 step of the position-only test is still 2.5e-4 off along these directions: not a reference at 3e-4.)"""
    import torch

    from conftest import load_case
    from elastic_ref import fd_hvp_strain
    from oracle.chgnet_oracle import OracleCHGNet

    torch.set_num_threads(8)
    golden = dict(np.load(os.path.join(GOLDEN, "weights_seed0.npz")))

    def scaled(k):
        return {name: ((v * k).astype(v.dtype) if name.endswith(".weight") and v.ndim == 2 and "embedding" not in name
                       and "composition" not in name else v) for name, v in golden.items()}

    graphs = [load_case(n)[0] for n in ("limno2", "s16tri")]
    rng = np.random.default_rng(25)                # tests/test_gpu_elastic.py::_directions(graphs, 25)
    dirs = [rng.normal(size=(len(g.atomic_number), 3)).astype(np.float32) for g in graphs]
    ws = [rng.normal(size=(3, 3)).astype(np.float32) for _ in graphs]
    for k, idx, step in ((4.0, (0, 1), 1e-5), (100.0, (0,), 2.5e-7)):
        oracle = OracleCHGNet(scaled(k), dtype=torch.float64)
        g, d, w = [graphs[i] for i in idx], [dirs[i] for i in idx], [ws[i] for i in idx]
        for (hx1, hs1), (hx2, hs2) in zip(fd_hvp_strain(oracle, g, d, w, step), fd_hvp_strain(oracle, g, d, w, step / 2)):
            assert np.abs(hx1 - hx2).max() <= 3e-5 * np.abs(hx1).max(), k
            assert np.abs(hs1 - hs2).max() <= 3e-5 * np.abs(hs1).max(), k


def test_strain_reference_is_symmetric():
    """(u', W') . H (u, W) = u' . hx(u, W) + W' : hs(u, W) is symmetric in the two directions, and the mixed blocks are each
    other's transposes: W' : hs(u, 0) = u . hx(0, W')."""
    from elastic_ref import fd_hvp_strain

    oracle = _oracle()
    g = _lif(True, 0.02, seed=3)
    n = len(g.atomic_number)
    rng = np.random.default_rng(2)
    for _ in range(2):
        u1, u2 = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
        w1, w2 = rng.normal(size=(3, 3)), rng.normal(size=(3, 3))
        (hx1, hs1), (hx2, hs2), (hxu, hsu), (hxw, hsw) = fd_hvp_strain(
            oracle, [g] * 4, [u1, u2, u1, np.zeros((n, 3))], [w1, w2, np.zeros((3, 3)), w2])
        a, b = float((u2 * hx1).sum() + (w2 * hs1).sum()), float((u1 * hx2).sum() + (w1 * hs2).sum())
        assert abs(a - b) <= 3e-5 * max(abs(a), abs(b))
        c, d = float((w2 * hsu).sum()), float((u1 * hxw).sum())
        assert abs(c - d) <= 3e-5 * max(np.abs(hsu).max(), np.abs(hxw).max()) * np.abs(w2).sum()


def test_strain_reference_agrees_with_second_differences_of_the_energy():
    """W_i : hs(0, W_j) against central second differences of the oracle's total energy in eps (h = 3e-5, fp64 energies): the
    diagonal and, by polarisation, one off-diagonal pair, for the Voigt strains and a non-symmetric W."""
    from elastic_ref import fd_hvp_strain, strained, total_energy, voigt_strains

    oracle = _oracle("weights_trained_like.npz")
    g = _lif(True, 0.01)
    n = len(g.atomic_number)
    rng = np.random.default_rng(4)
    ws = list(voigt_strains()[[0, 3]]) + [rng.normal(size=(3, 3))]
    hs = [r[1] for r in fd_hvp_strain(oracle, [g] * len(ws), [np.zeros((n, 3))] * len(ws), ws)]
    h = 3e-5                     # the h^2 term of the second difference is still 3e-4 of the value at h = 1e-3
    zero = np.zeros((n, 3))
    for w, s in zip(ws, hs):
        e = total_energy(oracle, [strained(g, zero, h * w), strained(g, zero, 0 * w), strained(g, zero, -h * w)])
        d2 = (e[0] - 2 * e[1] + e[2]) / h**2
        assert float((w * s).sum()) == pytest.approx(d2, rel=1e-4, abs=1e-4 * np.abs(s).max())
    wp, wm = ws[0] + ws[2], ws[0] - ws[2]
    e = total_energy(oracle, [strained(g, zero, h * wp), strained(g, zero, -h * wp), strained(g, zero, h * wm), strained(g, zero, -h * wm)])
    d2 = (e[0] + e[1] - e[2] - e[3]) / (4 * h**2)
    assert float((ws[0] * hs[2]).sum()) == pytest.approx(d2, rel=1e-4, abs=1e-4 * np.abs(hs[2]).max())
