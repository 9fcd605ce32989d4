"""Exact Hessian-vector products on the device (chg_hessian_vector, CHGNet.hessian_vector_product / predict_hessian) against
central differences of the float64 oracle's forces on the fixed graph (tests/hessian_ref.py; converged to 3e-5 of scale,
tests/test_hessian_cpu.py).  Tolerance: max|got - ref| <= 3e-4 max|ref| per structure, the REL_TOL_B of the second-order
fine-tuning tests (tests/test_gpu_train.py)."""

from __future__ import annotations

import os

import numpy as np
import pytest

from conftest import GOLDEN, load_case

pytestmark = pytest.mark.gpu

REL_TOL = 3e-4
FIVE = ("limno2", "noangle", "s16tri", "s40", "li9co7o16")


def _oracle(w, **kw):
    import torch

    from oracle.chgnet_oracle import OracleCHGNet

    torch.set_num_threads(8)
    return OracleCHGNet(w, dtype=torch.float64, **kw)


def _close(got, ref, what, tol=REL_TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    assert np.isfinite(got).all() and err <= tol * scale, f"{what}: max|d|={err:.3e} scale={scale:.3e} rel={err / max(scale, 1e-300):.2e}"


def _directions(graphs, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(len(g.atomic_number), 3)).astype(np.float32) for g in graphs]


def _engine_hvp(weights, graphs, dirs, **desc):
    from chgnet_amd.engine import Engine
    from chgnet_amd.pack import pack_weights

    eng = Engine(pack_weights(weights, desc or None), 0)
    try:
        batch = eng.upload(graphs)
        try:
            eng.predict(batch, "ef")
            h = eng.hessian_vector(batch, np.concatenate(dirs))
            off = batch.packed.atom_off
        finally:
            batch.free()
    finally:
        eng.close()
    return [h[off[i]:off[i + 1]] for i in range(len(graphs))]


def test_hvp_of_the_five_golden_graphs_vs_fp64_oracle(golden_weights, trained_like_weights):
    """One mixed batch per weight set (seed-0 and trained-checkpoint magnitudes), seeded random directions."""
    from hessian_ref import fd_hvp

    graphs = [load_case(n)[0] for n in FIVE]
    dirs = _directions(graphs, 11)
    for name, w in (("seed0", golden_weights), ("trained_like", trained_like_weights)):
        got = _engine_hvp(w, graphs, dirs)
        ref = fd_hvp(_oracle(w), graphs, dirs)
        for n, g, r in zip(FIVE, got, ref):
            _close(g, r, f"{name}/{n}")


def test_hvp_on_the_020_architecture_and_an_extensive_model_without_atomref():
    from chgnet_amd.model import CHGNet, random_state_dict
    from hessian_ref import fd_hvp
    from test_v020 import V020_ARGS, load_case_v020

    w020 = dict(np.load(os.path.join(GOLDEN, "weights_v020.npz")))
    graphs = [load_case_v020(n)[0] for n in FIVE]
    dirs = _directions(graphs, 12)
    model = CHGNet(state_dict=w020, **V020_ARGS)
    try:
        got = model.hessian_vector_product(graphs, dirs)
    finally:
        model.engine.close()
    ref = fd_hvp(_oracle(w020, atom_graph_cutoff=5.0, bond_graph_cutoff=3.0, cutoff_coeff=5), graphs, dirs)
    for n, g, r in zip(FIVE, got, ref):
        _close(g, r, f"0.2.0/{n}")

    args = dict(n_conv=3, is_intensive=False, composition_model=None)        # as tests/test_gpu_train.py
    sd = random_state_dict({"n_conv": 3, **args}, seed=21)
    rng = np.random.default_rng(22)
    for k, v in sd.items():
        if ".bn" in k or k.startswith("readout_norm") or k.endswith("frequencies"):
            sd[k] = (v + 0.1 * rng.normal(size=v.shape)).astype(np.float32)
    sd.pop("composition_model.fc.weight", None)
    graphs = [load_case(n)[0] for n in ("limno2", "s16tri")]
    dirs = _directions(graphs, 13)
    model = CHGNet(state_dict=sd, **args)
    try:
        got = model.hessian_vector_product(graphs, dirs)
    finally:
        model.engine.close()
    ref = fd_hvp(_oracle(sd, is_intensive=False), graphs, dirs)
    for n, g, r in zip(("limno2", "s16tri"), got, ref):
        _close(g, r, f"extensive/{n}")


@pytest.fixture(scope="module")
def models(golden_weights, trained_like_weights):
    from chgnet_amd.model import CHGNet

    ms = {"seed0": CHGNet(state_dict=golden_weights), "trained_like": CHGNet(state_dict=trained_like_weights)}
    yield ms
    for m in ms.values():
        if m._engine is not None:
            m._engine.close()


def _lif_graph(conventional, rattle=0.0):
    from chgnet_amd.graph.converter import CrystalGraphConverter
    from hessian_ref import lif_structure

    return CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3)(lif_structure(conventional, rattle))


@pytest.mark.parametrize("which", ["seed0", "trained_like"])
def test_full_hessian_of_a_cell_bonded_to_its_own_images(models, golden_weights, trained_like_weights, which):
    """Primitive rock-salt LiF (2 atoms): every bond of an atom to its own periodic image contributes nothing to rdot; the raw
    (unsymmetrised) Hessian is symmetric and obeys the acoustic sum rule within the same bar."""
    from hessian_ref import fd_hessian

    w = golden_weights if which == "seed0" else trained_like_weights
    g = _lif_graph(False)
    h = models[which].predict_hessian(g, symmetrize=False)
    ref = fd_hessian(_oracle(w), g)
    assert h.shape == (6, 6) and h.dtype == np.float64
    _close(h, ref, "H")
    scale = float(np.abs(ref).max())
    assert np.abs(h - h.T).max() <= REL_TOL * scale
    assert np.abs(h.reshape(6, 2, 3).sum(1)).max() <= REL_TOL * scale
    hs = models[which].predict_hessian([g], symmetrize=True)[0]
    assert np.abs(hs - 0.5 * (h + h.T)).max() <= 3e-5 * scale      # a second run: fp32 atomics in another order


@pytest.mark.parametrize("which", ["seed0", "trained_like"])
@pytest.mark.parametrize("rattle", [0.0, 0.01])
def test_rock_salt_with_collinear_triplets_and_its_gamma_modes(models, golden_weights, trained_like_weights, which, rattle):
    """Conventional LiF (a = 4.03 A): F-Li-F triplets at exactly 180 degrees, where the angle's second derivative is dominated by
    1/sin(theta) terms.  Full Hessian against the reference; the mass-weighted eigenvalues against the reference's, three of them
    (the uniform translations) zero, all within 3e-4 max|lambda| -- at any geometry, not only at a minimum."""
    from chgnet_amd import gamma_frequencies
    from chgnet_amd.phonons import _THZ
    from hessian_ref import fd_hessian, mass_weighted_eigenvalues

    w = golden_weights if which == "seed0" else trained_like_weights
    g = _lif_graph(True, rattle)
    h = models[which].predict_hessian(g, symmetrize=False)
    ref = fd_hessian(_oracle(w), g)
    _close(h, ref, f"LiF rattle={rattle}")
    scale = float(np.abs(ref).max())
    assert np.abs(h.reshape(24, 8, 3).sum(1)).max() <= REL_TOL * scale
    z = np.asarray(g.atomic_number)
    lam, lam_ref = mass_weighted_eigenvalues(z, h), mass_weighted_eigenvalues(z, ref)
    big = float(np.abs(lam_ref).max())
    assert np.abs(lam - lam_ref).max() <= REL_TOL * big, (lam, lam_ref)
    assert np.sort(np.abs(lam))[:3].max() <= REL_TOL * big
    f = gamma_frequencies(g, h)
    assert np.allclose(f, np.sign(lam) * np.sqrt(np.abs(lam)) * _THZ, rtol=1e-12, atol=1e-12)


def test_isolated_atoms_and_batch_equals_single(models, golden_weights):
    from chgnet_amd import Structure
    from chgnet_amd.graph.converter import CrystalGraphConverter
    from hessian_ref import fd_hvp

    conv = CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3, on_isolated_atoms="ignore")
    lone = conv(Structure(np.eye(3) * 20.0, ["Li"], [[0, 0, 0]]))
    # a Li-F dimer and an atom 11 A from both (and from every image): one structure with an isolated atom
    mixed = conv(Structure(np.eye(3) * 14.0, ["Li", "F", "O"], [[0, 0, 0], [2.0 / 14, 0, 0], [0.5, 0.5, 0.5]]))
    normal = load_case("s16tri")[0]
    graphs = [lone, normal, mixed]
    dirs = _directions(graphs, 14)
    model = models["seed0"]
    got = model.hessian_vector_product(graphs, dirs)
    assert np.array_equal(got[0], np.zeros((1, 3), np.float32)) and np.array_equal(got[2][2], np.zeros(3, np.float32))
    assert np.abs(got[2][:2]).max() > 0
    single = model.hessian_vector_product(normal, dirs[1])
    _close(single, got[1], "batch vs single", tol=1e-5)
    ref = fd_hvp(_oracle(golden_weights), graphs[1:], dirs[1:])
    _close(got[1], ref[0], "s16tri next to isolated atoms")
    _close(got[2], ref[1], "dimer with an isolated atom")


def test_scaled_weights_product_and_wide_range_sweeps(golden_weights):
    """Linear weights x 4: the batch stays on the product sweep; x 100: the product sweep leaves the f16 operand range and
    chg_hessian_vector forms the HVP again on the wide-range sweep (as chg_batch_download does for predictions,
    tests/test_gpu_round4.py).  Both against the fp64 oracle."""
    from chgnet_amd.engine import Engine
    from chgnet_amd.pack import pack_weights
    from hessian_ref import fd_hvp

    graphs = [load_case(n)[0] for n in ("limno2", "s16tri")]
    dirs = _directions(graphs, 15)

    def scaled(k):
        out = {}
        for name, v in golden_weights.items():
            lin = name.endswith(".weight") and v.ndim == 2 and "embedding" not in name and "composition" not in name
            out[name] = (v * k).astype(v.dtype) if lin else v
        return out

    for k, wide in ((4.0, 0), (100.0, 1)):
        w = scaled(k)
        eng = Engine(pack_weights(w), 0)
        try:
            batch = eng.upload(graphs)
            try:
                eng.predict(batch, "ef")
                h = eng.hessian_vector(batch, np.concatenate(dirs))
                assert int(eng.debug_fetch_i32(batch, "wide_range", 1)[0]) == wide, k
                off = batch.packed.atom_off
            finally:
                batch.free()
        finally:
            eng.close()
        # x 100 makes the energy so curved that the 1e-5 A central difference is off by 16 % on limno2 (1e-6 A agrees with 1e-7 A
        # to 3e-5 of scale there); on s16tri no step between 1e-5 and 1e-7 A converges, so the x 100 leg checks limno2 at 1e-6 A
        check = range(len(graphs)) if k < 10 else [0]
        ref = fd_hvp(_oracle(w), [graphs[i] for i in check], [dirs[i] for i in check], 1e-5 if k < 10 else 1e-6)
        # tests/test_gpu_round4.py's rule: within 50x the fp32 oracle's own error (here: of the forces, relative to their scale), at
        # least REL_TOL.  x 100: the fp32 forces are 1.3e-4 of scale off their fp64 values on limno2 (x 1: ~1e-7)
        import torch

        from oracle.chgnet_oracle import OracleCHGNet

        f32 = OracleCHGNet(w).predict_graph(graphs[0], "ef")["f"]
        f64 = _oracle(w).predict_graph(graphs[0], "ef")["f"]
        tol = max(REL_TOL, 50 * float(np.abs(f32 - f64).max() / np.abs(f64).max()))
        torch.set_num_threads(8)
        for i, r in zip(check, ref):
            _close(h[off[i]:off[i + 1]], r, f"x{k:g}/{i}", tol)
        assert np.isfinite(h).all()


def test_hvp_skips_the_weight_gradients_and_leaves_the_batch_intact(hip_engine, golden_weights):
    graphs = [load_case(n)[0] for n in ("limno2", "noangle", "s16tri")]
    batch = hip_engine.upload(graphs)
    try:
        pb = batch.packed
        rng = np.random.default_rng(16)
        ce, gf = rng.normal(size=pb.n_struct).astype(np.float32), rng.normal(size=(pb.n_atoms, 3)).astype(np.float32)
        u = rng.normal(size=(pb.n_atoms, 3)).astype(np.float32)
        hip_engine.predict(batch, "efs")
        before = hip_engine.download(batch, "efs")
        blob = hip_engine.backward(batch, ce, None, gf, None)
        h0 = hip_engine.hessian_vector(batch, u)
        hip_engine.profile(True)
        hip_engine.profile_reset()
        try:
            h1 = hip_engine.hessian_vector(batch, u)
            labels = hip_engine.profile_read()
        finally:
            hip_engine.profile(False)
        assert {"hvp_bond", "hvp_angle", "hvp_scatter"} <= set(labels), labels
        assert not {"t2_wgrad", "t2_freq", "wgrad_atom_embed"} & set(labels), labels
        assert np.abs(h1 - h0).max() <= 1e-5 * np.abs(h0).max()
        again = hip_engine.backward(batch, ce, None, gf, None)
        assert np.abs(again - blob).max() <= 2e-5 * np.abs(blob).max()
        after = hip_engine.download(batch, "efs")
        for k in ("e", "f", "s"):
            assert np.abs(after[k] - before[k]).max() <= 1e-6 * max(1.0, float(np.abs(before[k]).max())), k
        # energy-only last prediction: the HVP runs the force prediction first, same result
        hip_engine.predict(batch, "e")
        _close(hip_engine.hessian_vector(batch, u), h0, "after an energy-only prediction", tol=1e-5)
        with pytest.raises(ValueError, match="expected"):
            hip_engine.hessian_vector(batch, u[:-1])
    finally:
        batch.free()
