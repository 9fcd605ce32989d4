"""Strain blocks of the exact Hessian on the device (chg_hessian_vector_strain, CHGNet.hessian_vector_product_with_strain /
predict_elastic_tensor) against central differences of the float64 oracle's forces and stress on the fixed graph
(tests/elastic_ref.py; converged to 3e-5 of scale, tests/test_elastic_cpu.py).  Tolerance: max|got - ref| <= 3e-4 max|ref|, the bar
of tests/test_gpu_hessian.py."""

from __future__ import annotations

import os

import numpy as np
import pytest

from conftest import GOLDEN, load_case

pytestmark = pytest.mark.gpu

REL_TOL = 3e-4
FIVE = ("limno2", "noangle", "s16tri", "s40", "li9co7o16")
GPA = 160.21766208


def _oracle(w, **kw):
    import torch

    from oracle.chgnet_oracle import OracleCHGNet

    torch.set_num_threads(8)
    return OracleCHGNet(w, dtype=torch.float64, **kw)


def _close(got, ref, what, tol=REL_TOL, scale=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) if scale is None else scale
    err = float(np.abs(got - ref).max())
    assert np.isfinite(got).all() and err <= tol * scale, f"{what}: max|d|={err:.3e} scale={scale:.3e} rel={err / max(scale, 1e-300):.2e}"


def _directions(graphs, seed):
    rng = np.random.default_rng(seed)
    return ([rng.normal(size=(len(g.atomic_number), 3)).astype(np.float32) for g in graphs],
            [rng.normal(size=(3, 3)).astype(np.float32) for _ in graphs])


def _split(hx, hs, off, k):
    return [(hx[off[i]:off[i + 1]], hs[i]) for i in range(k)]


def _volume(g):
    return abs(float(np.linalg.det(np.asarray(g.lattice, np.float64).reshape(3, 3))))


def _lif_graph(conventional, rattle=0.0, seed=0, rotation=None):
    from chgnet_amd.graph.converter import CrystalGraphConverter
    from chgnet_amd.graph.structure import Structure
    from hessian_ref import lif_structure

    s = lif_structure(conventional, rattle, seed)
    if rotation is not None:
        s = Structure(s.lattice.matrix @ rotation.T, s.atomic_numbers, s.frac_coords)
    return CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3)(s)


def test_strain_products_of_the_five_golden_graphs_vs_fp64_oracle(golden_weights, trained_like_weights):
    """One mixed batch per weight set: random (u, W), u = 0 and W = 0.  With W = 0, hx is chg_hessian_vector's H u."""
    from chgnet_amd.engine import Engine
    from chgnet_amd.pack import pack_weights
    from elastic_ref import fd_hvp_strain

    graphs = [load_case(n)[0] for n in FIVE]
    dirs, ws = _directions(graphs, 21)
    zu = [np.zeros_like(u) for u in dirs]
    zw = [np.zeros((3, 3), np.float32) for _ in ws]
    for name, w in (("seed0", golden_weights), ("trained_like", trained_like_weights)):
        eng = Engine(pack_weights(w), 0)
        try:
            batch = eng.upload(graphs)
            try:
                eng.predict(batch, "ef")
                off = batch.packed.atom_off
                runs = {kind: _split(*eng.hessian_vector_strain(batch, np.concatenate(u), np.stack(s)), off, len(graphs))
                        for kind, u, s in (("uW", dirs, ws), ("W", zu, ws), ("u", dirs, zw))}
                hu = eng.hessian_vector(batch, np.concatenate(dirs))
            finally:
                batch.free()
        finally:
            eng.close()
        oracle = _oracle(w)
        refs = {kind: fd_hvp_strain(oracle, graphs, u, s) for kind, u, s in (("uW", dirs, ws), ("W", zu, ws), ("u", dirs, zw))}
        for i, n in enumerate(FIVE):
            # per structure one scale for each output over the three kinds: a block can vanish by symmetry (noangle's two atoms are
            # inversion centres, so d2E/dx deps = 0 and the u = 0 run's hx is rounding noise around zero)
            sx = max(float(np.abs(refs[k][i][0]).max()) for k in refs)
            ss = max(float(np.abs(refs[k][i][1]).max()) for k in refs)
            for kind in refs:
                _close(runs[kind][i][0], refs[kind][i][0], f"{name}/{kind}/{n} hx", scale=sx)
                _close(runs[kind][i][1], refs[kind][i][1], f"{name}/{kind}/{n} hs", scale=ss)
        for i, n in enumerate(FIVE):
            _close(runs["u"][i][0], hu[off[i]:off[i + 1]], f"{name}/{n}: W = 0 vs chg_hessian_vector", tol=1e-5)


def test_strain_products_on_the_020_architecture_and_an_extensive_model_without_atomref():
    from chgnet_amd.model import CHGNet, random_state_dict
    from elastic_ref import fd_hvp_strain
    from test_v020 import V020_ARGS, load_case_v020

    w020 = dict(np.load(os.path.join(GOLDEN, "weights_v020.npz")))
    graphs = [load_case_v020(n)[0] for n in FIVE]
    dirs, ws = _directions(graphs, 22)
    model = CHGNet(state_dict=w020, **V020_ARGS)
    try:
        got = model.hessian_vector_product_with_strain(graphs, dirs, ws)
    finally:
        model.engine.close()
    ref = fd_hvp_strain(_oracle(w020, atom_graph_cutoff=5.0, bond_graph_cutoff=3.0, cutoff_coeff=5), graphs, dirs, ws)
    for n, (gx, gs), (rx, rs) in zip(FIVE, got, ref):
        _close(gx, rx, f"0.2.0/{n} hx")
        _close(gs, rs, f"0.2.0/{n} hs")

    args = dict(n_conv=3, is_intensive=False, composition_model=None)        # as tests/test_gpu_hessian.py
    sd = random_state_dict({"n_conv": 3, **args}, seed=21)
    rng = np.random.default_rng(22)
    for k, v in sd.items():
        if ".bn" in k or k.startswith("readout_norm") or k.endswith("frequencies"):
            sd[k] = (v + 0.1 * rng.normal(size=v.shape)).astype(np.float32)
    sd.pop("composition_model.fc.weight", None)
    graphs = [load_case(n)[0] for n in ("limno2", "s16tri")]
    dirs, ws = _directions(graphs, 23)
    model = CHGNet(state_dict=sd, **args)
    try:
        got = model.hessian_vector_product_with_strain(graphs, dirs, ws)
    finally:
        model.engine.close()
    ref = fd_hvp_strain(_oracle(sd, is_intensive=False), graphs, dirs, ws)
    for n, (gx, gs), (rx, rs) in zip(("limno2", "s16tri"), got, ref):
        _close(gx, rx, f"extensive/{n} hx")
        _close(gs, rs, f"extensive/{n} hs")


@pytest.fixture(scope="module")
def models(golden_weights, trained_like_weights):
    from chgnet_amd.model import CHGNet

    ms = {"seed0": CHGNet(state_dict=golden_weights), "trained_like": CHGNet(state_dict=trained_like_weights)}
    yield ms
    for m in ms.values():
        if m._engine is not None:
            m._engine.close()


def _ref_tensors(oracle, g):
    """Clamped / relaxed tensors (GPa), Lambda and Phi by the host formula on the oracle's full (3n + 6)^2 Hessian."""
    from chgnet_amd.elastic import relaxed_ion_tensor
    from elastic_ref import fd_full_hessian

    phi, lam, ss = fd_full_hessian(oracle, g)
    v = _volume(g)
    clamped = 0.5 * (ss + ss.T) * GPA / v
    phi = 0.5 * (phi + phi.T)
    return clamped, relaxed_ion_tensor(clamped, lam, phi, v), lam, phi


@pytest.mark.parametrize("which", ["seed0", "trained_like"])
@pytest.mark.parametrize("conventional", [False, True])
def test_rock_salt_elastic_tensor(models, golden_weights, trained_like_weights, which, conventional):
    """Rock-salt LiF, the 2-atom primitive cell (self-image bonds only: zero position tangent, non-zero strain tangent) and the
    8-atom cell (collinear triplets): against the oracle; the cubic pattern; every atom an inversion centre, so Lambda ~ 0 and the
    relaxed-ion tensor is the clamped one."""
    w = golden_weights if which == "seed0" else trained_like_weights
    g = _lif_graph(conventional)
    n = len(g.atomic_number)
    r = models[which].predict_elastic_tensor(g)
    clamped, relaxed, lam, phi = _ref_tensors(_oracle(w), g)
    assert r["clamped_ion"].shape == (6, 6) and r["internal_strain"].shape == (3 * n, 6) and r["force_constants"].shape == (3 * n, 3 * n)
    c = r["clamped_ion"]
    scale = float(np.abs(clamped).max())
    _close(c, clamped, "clamped")
    _close(r["force_constants"], phi, "force constants")
    _close(r["relaxed_ion"], relaxed, "relaxed", scale=scale)
    d, o, s = np.diag(c)[:3], c[[0, 0, 1], [1, 2, 2]], np.diag(c)[3:]
    tol = REL_TOL * scale
    assert np.ptp(d) <= tol and np.ptp(o) <= tol and np.ptp(s) <= tol, c
    mask = np.ones((6, 6), bool)
    mask[:3, :3] = False
    mask[np.arange(3, 6), np.arange(3, 6)] = False
    assert np.abs(c[mask]).max() <= tol, c
    # Lambda = d2E/dx deps is a force-constant block times bond vectors (eV/A^2 x A): its zero is judged on that scale, with the
    # longest bond of this graph as the length
    assert np.abs(r["internal_strain"]).max() <= REL_TOL * float(np.abs(phi).max()) * _longest_bond(g)
    _close(r["relaxed_ion"], c, "relaxed == clamped", scale=scale)
    assert r["volume"] == pytest.approx(_volume(g), rel=1e-6) and r["stress"].shape == (6,)
    assert np.isfinite(r["min_phonon_eigenvalue"])


def _longest_bond(g):
    lat = np.asarray(g.lattice, np.float64).reshape(3, 3)
    cart = np.asarray(g.atom_frac_coord, np.float64).reshape(-1, 3) @ lat
    ag = np.asarray(g.atom_graph).reshape(-1, 2)
    v = cart[ag[:, 0]] - cart[ag[:, 1]] - np.asarray(g.neighbor_image, np.float64).reshape(-1, 3) @ lat
    return float(np.linalg.norm(v, axis=1).max())


def _phi_condition(phi):
    """Condition number of the symmetrised force constants off the translations: what the relaxed-ion correction inverts."""
    from chgnet_amd.elastic import translation_complement

    q = translation_complement(phi.shape[0] // 3)
    ev = np.abs(np.linalg.eigvalsh(q.T @ (0.5 * (phi + phi.T)) @ q))
    return float(ev.max() / ev.min())


def _voigt_to_full(c):
    pairs = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
    idx = np.zeros((3, 3), int)
    for i, (a, b) in enumerate(pairs):
        idx[a, b] = idx[b, a] = i
    return c[idx[:, :, None, None], idx[None, None, :, :]], pairs


def test_rotated_cell_rotates_the_tensor_as_rank_four(models):
    """A random rotation R of a rattled cell: C'_ijkl = R_ia R_jb R_kc R_ld C_abcd, for both tensors.  The relaxed one's correction
    inverts Phi, so its bar is scaled by Phi's condition number off the translations; this cell's is 1.7 (float64 reference: all
    21 modes between 0.22 and 0.38 eV/A^2, seed-0 weights), and the test refuses to run with one above 10, where that bar would
    stop meaning anything."""
    rng = np.random.default_rng(5)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    rot = q * np.sign(np.linalg.det(q))
    base = models["seed0"].predict_elastic_tensor(_lif_graph(True, 0.02, seed=7))
    turned = models["seed0"].predict_elastic_tensor(_lif_graph(True, 0.02, seed=7, rotation=rot))
    kappa = _phi_condition(base["force_constants"])
    assert kappa <= 10, kappa
    scale = float(np.abs(base["clamped_ion"]).max())
    for key, tol in (("clamped_ion", REL_TOL), ("relaxed_ion", REL_TOL * kappa)):
        full, pairs = _voigt_to_full(base[key])
        f2 = np.einsum("ia,jb,kc,ld,abcd->ijkl", rot, rot, rot, rot, full)
        want = np.array([[f2[a, b, c, d] for (c, d) in pairs] for (a, b) in pairs])
        _close(turned[key], want, key, tol=tol, scale=scale)


def test_relaxed_ion_tensor_of_a_low_symmetry_cell(models, golden_weights):
    """limno2 (no symmetry, not at a minimum): the device tensors against the host formula on the oracle's full Hessian.  The
    relaxed-ion correction inverts Phi, so its bar is scaled by Phi's condition number off the translations: 29 here (float64
    reference, seed-0 weights: |eigenvalues| 0.038 .. 1.09 eV/A^2, three of them negative); the test refuses one above 50."""
    from chgnet_amd.elastic import translation_complement

    g = load_case("limno2")[0]
    n = len(g.atomic_number)
    r = models["seed0"].predict_elastic_tensor(g)
    clamped, relaxed, lam, phi = _ref_tensors(_oracle(golden_weights), g)
    _close(r["clamped_ion"], clamped, "clamped")
    _close(r["internal_strain"], lam, "Lambda")
    _close(r["force_constants"], phi, "Phi")
    ev = np.abs(np.linalg.eigvalsh(translation_complement(n).T @ phi @ translation_complement(n)))
    kappa = _phi_condition(phi)
    assert kappa <= 50, kappa
    _close(r["relaxed_ion"], relaxed, f"relaxed (cond(Phi) = {kappa:.1f})", tol=REL_TOL * kappa)
    assert r["min_phonon_eigenvalue"] == pytest.approx(float(np.linalg.eigvalsh(translation_complement(n).T @ phi @ translation_complement(n))[0]),
                                                       abs=REL_TOL * ev.max())
    clamped_only = models["seed0"].predict_elastic_tensor(g, relaxed_ion=False)
    assert clamped_only["relaxed_ion"] is None and "force_constants" not in clamped_only and clamped_only["min_phonon_eigenvalue"] is None
    _close(clamped_only["clamped_ion"], r["clamped_ion"], "clamped-only run", tol=1e-5)


def test_internal_strain_from_either_block(models):
    """Lambda^T from the position columns' hs (d2E/deps dx . e_k) equals Lambda from the strain columns' hx (d2E/dx deps : W_j)."""
    from chgnet_amd.elastic import voigt_strains

    g = _lif_graph(True, 0.02, seed=9)
    n = len(g.atomic_number)
    model = models["trained_like"]
    r = model.predict_elastic_tensor(g, relaxed_ion=False)
    eye = np.eye(3 * n, dtype=np.float32).reshape(3 * n, n, 3)
    res = model.hessian_vector_product_with_strain([g] * (3 * n), list(eye), [np.zeros((3, 3), np.float32)] * (3 * n))
    wv = voigt_strains()
    lam_t = np.array([[float((wv[j] * hs).sum()) for j in range(6)] for _, hs in res])
    _close(lam_t, r["internal_strain"], "Lambda from hs vs from hx")


def test_isolated_atoms_and_batch_equals_single(models, golden_weights):
    from chgnet_amd import Structure
    from chgnet_amd.graph.converter import CrystalGraphConverter
    from elastic_ref import fd_hvp_strain

    conv = CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3, on_isolated_atoms="ignore")
    lone = conv(Structure(np.eye(3) * 20.0, ["Li"], [[0, 0, 0]]))
    mixed = conv(Structure(np.eye(3) * 14.0, ["Li", "F", "O"], [[0, 0, 0], [2.0 / 14, 0, 0], [0.5, 0.5, 0.5]]))
    normal = load_case("s16tri")[0]
    graphs = [lone, normal, mixed]
    dirs, ws = _directions(graphs, 24)
    model = models["seed0"]
    got = model.hessian_vector_product_with_strain(graphs, dirs, ws)
    assert np.array_equal(got[0][0], np.zeros((1, 3), np.float32)) and np.array_equal(got[0][1], np.zeros((3, 3), np.float32))
    assert np.array_equal(got[2][0][2], np.zeros(3, np.float32)) and np.abs(got[2][0][:2]).max() > 0 and np.abs(got[2][1]).max() > 0
    hx1, hs1 = model.hessian_vector_product_with_strain(normal, dirs[1], ws[1])
    _close(hx1, got[1][0], "batch vs single hx", tol=1e-5)
    _close(hs1, got[1][1], "batch vs single hs", tol=1e-5)
    ref = fd_hvp_strain(_oracle(golden_weights), graphs[1:], dirs[1:], ws[1:])
    for (gx, gs), (rx, rs), what in zip(got[1:], ref, ("s16tri next to isolated atoms", "dimer with an isolated atom")):
        _close(gx, rx, what + " hx")
        _close(gs, rs, what + " hs")
    # a batch of several structures' replicas gives each structure's own tensor
    lif = _lif_graph(False)
    both = model.predict_elastic_tensor([lif, normal], relaxed_ion=False)
    alone = model.predict_elastic_tensor(lif, relaxed_ion=False)
    _close(both[0]["clamped_ion"], alone["clamped_ion"], "LiF next to s16tri", tol=1e-5)


def test_scaled_weights_product_and_wide_range_sweeps(golden_weights, monkeypatch):
    """The strain products on both sweeps of engine_train_wide.hip's two compilations.

    (i) Accuracy of the wide-range compilation: CHGNET_WIDE_RANGE=1 puts the batch on the wide-range sweeps from its first
    prediction; with weights x 1 and x 4 its products match the float64 reference at the suite's bar.  (ii) Linear weights x 4 on
    the product sweep, same bar.  (iii) Linear weights x 100: the prediction stays on the product sweep, the strain product leaves
    the f16 operand range, and chg_hessian_vector_strain moves the batch and forms both outputs again on the wide-range sweep.

    References (tests/test_elastic_cpu.py checks their convergence along these strain directions): x 1 and x 4 at the 1e-5 step
    (halving it changes them by ~2e-7 of scale); x 100 on limno2 at 2.5e-7, where halving changes them by 1.4e-6 (the 1e-6 step of
    the position-only test is still 2.5e-4 off there).  s16tri x 100 converges at no step and is left out, as in
    tests/test_gpu_hessian.py.

    Bars, from repeated device runs (8 per weight set, two engines): x 4 on the product sweep is 1.0e-5 .. 1.4e-5 of scale off the
    reference, with 3e-6 between runs, inside REL_TOL = 3e-4.  x 100 is not reproducible to better than 1.6e-3 (hx) and 2.8e-3
    (hs) of scale between runs: fp32 sums in arrival order, amplified by the cancellations of a x 100 network (the same spread
    is in chg_hessian_vector's H u there).  Its error is 4.6e-3 .. 7.0e-3 of scale, so it is held to X100_TOL = 2e-2: about 3x the
    largest error seen and 7x the run-to-run spread.  A bar tied to the fp32 oracle's force error (50 x 1.33e-4) sat inside that
    spread and failed intermittently."""
    from chgnet_amd.engine import Engine
    from chgnet_amd.pack import pack_weights
    from elastic_ref import fd_hvp_strain

    X100_TOL = 2e-2
    graphs = [load_case(n)[0] for n in ("limno2", "s16tri")]
    dirs, ws = _directions(graphs, 25)

    def scaled(k):
        out = {}
        for name, v in golden_weights.items():
            lin = name.endswith(".weight") and v.ndim == 2 and "embedding" not in name and "composition" not in name
            out[name] = (v * k).astype(v.dtype) if lin else v
        return out

    def run(w, force_wide=False):
        if force_wide:
            monkeypatch.setenv("CHGNET_WIDE_RANGE", "1")      # read when the engine is created
        try:
            eng = Engine(pack_weights(w), 0)
        finally:
            monkeypatch.delenv("CHGNET_WIDE_RANGE", raising=False)
        try:
            batch = eng.upload(graphs)
            try:
                eng.predict(batch, "ef")
                before = int(eng.debug_fetch_i32(batch, "wide_range", 1)[0])
                hx, hs = eng.hessian_vector_strain(batch, np.concatenate(dirs), np.stack(ws))
                after = int(eng.debug_fetch_i32(batch, "wide_range", 1)[0])
                off = batch.packed.atom_off
            finally:
                batch.free()
        finally:
            eng.close()
        assert np.isfinite(hx).all() and np.isfinite(hs).all()
        return hx, hs, off, (before, after)

    for k, force_wide, flags, check, step, tol in ((1.0, True, (1, 1), (0, 1), 1e-5, REL_TOL),
                                                   (4.0, True, (1, 1), (0, 1), 1e-5, REL_TOL),
                                                   (4.0, False, (0, 0), (0, 1), 1e-5, REL_TOL),
                                                   (100.0, False, (0, 1), (0,), 2.5e-7, X100_TOL)):
        w = scaled(k)
        hx, hs, off, got_flags = run(w, force_wide)
        what = f"x{k:g}{' wide' if force_wide else ''}"
        assert got_flags == flags, (what, got_flags)
        ref = fd_hvp_strain(_oracle(w), [graphs[i] for i in check], [dirs[i] for i in check], [ws[i] for i in check], step)
        for i, (rx, rs) in zip(check, ref):
            _close(hx[off[i]:off[i + 1]], rx, f"{what}/{i} hx", tol)
            _close(hs[i], rs, f"{what}/{i} hs", tol)


def test_strain_scatter_runs_in_the_product_and_leaves_the_batch_intact(hip_engine):
    graphs = [load_case(n)[0] for n in ("limno2", "noangle", "s16tri")]
    batch = hip_engine.upload(graphs)
    try:
        pb = batch.packed
        rng = np.random.default_rng(26)
        u = rng.normal(size=(pb.n_atoms, 3)).astype(np.float32)
        w = rng.normal(size=(pb.n_struct, 3, 3)).astype(np.float32)
        hip_engine.predict(batch, "efs")
        before = hip_engine.download(batch, "efs")
        hx0, hs0 = hip_engine.hessian_vector_strain(batch, u, w)
        h0 = hip_engine.hessian_vector(batch, u)
        hx1, hs1 = hip_engine.hessian_vector_strain(batch, u, w)
        _close(hx1, hx0, "repeat hx", tol=1e-5)
        _close(hs1, hs0, "repeat hs", tol=1e-5)
        _close(hip_engine.hessian_vector(batch, u), h0, "H u after a strain product", tol=1e-5)
        after = hip_engine.download(batch, "efs")
        for k in ("e", "f", "s"):
            assert np.abs(after[k] - before[k]).max() <= 1e-6 * max(1.0, float(np.abs(before[k]).max())), k
        with pytest.raises(ValueError, match="expected"):
            hip_engine.hessian_vector_strain(batch, u, w[:-1])
    finally:
        batch.free()
