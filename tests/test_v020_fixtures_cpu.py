"""The fixtures of tests/test_gpu_v020_paths.py (tests/v020_fixtures.py) keep their meaning at the released 0.2.0 architecture's
5 A / 3 A cutoffs, a pass there is not vacuous (the ``mlp_out`` biases and the batch-level switch of the shift move every energy
far past the tolerance), and the batch semantics the GPU matrix checks are the reference's: a recording of the unmodified
reference (tests/golden/make_golden_v020.py -> batch_v020_low.npz) pins the oracle, the oracle pins the float64 models of the
kernel pipeline."""

from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import angle_fixtures as af
import neighbor_ref
import v020_fixtures as vf
from chgnet_amd.graph.converter import build_graph_arrays
from conftest import GOLDEN
from test_gpu_parity import TOL
from test_v020 import DEAD, TOL_ORACLE, TOL_ORACLE_TL, V020_ARGS, _blob_from, _oracle


@pytest.fixture(scope="module")
def graphs():
    conv = vf.converter()
    return {name: [conv(s) for s in structs] for name, structs in vf.structure_groups().items()}


@pytest.fixture(scope="module")
def weight_sets():
    return {w: dict(np.load(os.path.join(GOLDEN, f"weights_{w}.npz"))) for w in vf.WEIGHTS}


def _short_counts(s):
    a = build_graph_arrays(s.frac_coords, s.lattice.matrix, vf.R_ATOM, vf.R_BOND)
    d, c = a["distance"], a["atom_graph"][:, 0]
    return np.bincount(c[d < vf.R_BOND], minlength=len(s)), int((d == vf.R_BOND).sum())


def _rows_per_centre(g):
    return np.bincount(np.asarray(g.bond_graph).reshape(-1, 5)[:, 0], minlength=len(g.atomic_number))


def _canonical(s, g) -> bool:
    """The predicates of tests/test_angle_fixtures_cpu.py: complete n (n - 1) blocks of distinct (centre, b1, b2) rows at every atom,
    no bond exactly at the bond cutoff, and no atom with more than WIN_LIST = 32 short bonds."""
    n, ties = _short_counts(s)
    bg = np.asarray(g.bond_graph).reshape(-1, 5)
    blocks = np.array_equal(_rows_per_centre(g), n * (n - 1)) and len(np.unique(bg[:, [0, 2, 4]], axis=0)) == len(bg)
    return blocks and ties == 0 and int(n.max()) <= 32


def test_shell_centres_have_k_short_bonds_at_5_3(graphs):
    for s, g, k in zip(vf.structure_groups()["shell"] + vf.structure_groups()["shell_33"], graphs["shell"] + graphs["shell_33"],
                       vf.SHELL_KS + (33,)):
        n, ties = _short_counts(s)
        assert n[0] == k and ties == 0 and len(s) == k + 1
        assert _rows_per_centre(g)[0] == k * (k - 1)
        assert af.short_bond_counts(g)[0] == k
    sizes = [len(s) for s in vf.structure_groups()["shell"]]
    angles = [len(np.asarray(g.bond_graph).reshape(-1, 5)) for g in graphs["shell"]]
    assert (min(sizes), max(sizes)) == (3, 33) and min(angles) == 2 and max(angles) == 6792


def test_canonical_and_non_canonical_groups(graphs):
    groups = vf.structure_groups()
    for name, structs in groups.items():
        canon = [_canonical(s, g) for s, g in zip(structs, graphs[name])]
        if name in vf.NONCANONICAL:
            assert not any(canon), name
        else:
            assert all(canon), name
    for s, per_atom in zip(groups["tie"], (6, 2)):            # bonds exactly at the bond cutoff that own angles (as at 6 / 3)
        n, ties = _short_counts(s)
        assert ties == per_atom * len(s) and n.min() >= 12
    assert _short_counts(groups["shell_33"][0])[0][0] == 33


def test_zero_angle_batches_and_the_zero_angle_structure_that_rides_along(graphs):
    angles = {name: [len(np.asarray(g.bond_graph).reshape(-1, 5)) for g in gs] for name, gs in graphs.items()}
    assert angles["noangle"] == [0] and angles["noangle_2"] == [0, 0]
    assert angles["low"][0] == 0 and sum(angles["low"]) > 0 and angles["low"][1] == 2 and angles["low"][2] == 20
    assert all(len(np.asarray(g.atom_graph).reshape(-1, 2)) > 0 for gs in graphs.values() for g in gs)       # every structure has bonds
    assert [len(g.atomic_number) for g in graphs["md"]] == [256]
    for name, gs in graphs.items():
        if name not in ("low", "noangle", "noangle_2"):
            assert min(angles[name]) > 0, name


def test_long_batch_is_the_shortest_prefix_past_the_capped_grids():
    import bench
    from chgnet_amd.pack import pack_batch

    structs = vf.long_structures()
    conv = vf.converter()
    n = len(structs)
    full = bench.workload_structures(n, vf.LONG_SEED)
    assert all(np.array_equal(a.frac_coords, b.frac_coords) for a, b in zip(structs, full))    # the generator's prefixes nest
    assert all(len(s) == 40 for s in structs)
    gs = [conv(s) for s in structs]
    pb = pack_batch(gs)
    assert pb.n_directed > vf.LONG_LIMIT and pb.n_angles > vf.LONG_LIMIT and pb.n_angles % 32 != 0
    ed = np.cumsum([len(np.asarray(g.atom_graph).reshape(-1, 2)) for g in gs])
    a = np.cumsum([len(np.asarray(g.bond_graph).reshape(-1, 5)) for g in gs])
    assert not np.any((ed[:-1] > vf.LONG_LIMIT) & (a[:-1] > vf.LONG_LIMIT) & (a[:-1] % 32 != 0))          # no shorter prefix does
    assert min(len(np.asarray(g.bond_graph).reshape(-1, 5)) for g in gs) > 0                               # the loss is additive
    print(f"long: n = {n}, Ed = {pb.n_directed}, A = {pb.n_angles}")


def test_no_edge_within_the_oracle_margin_of_the_atom_cutoff(graphs):
    """Brute-force neighbour oracle (tests/neighbor_ref.py): the smallest |d - 5.0| over every pair it evaluates is far above what
    float64 arithmetic can move a distance by (the bound of tests/graph_hard_cases.required_margin), so the device builder and the
    host converter must produce the same rows -- a disagreement is a finding, not a tie.  The rows equal the host converter's."""
    groups = dict(vf.structure_groups(), long=list(vf.long_structures()))
    conv = vf.converter()
    worst = float("inf")
    for name, structs in groups.items():
        for i, s in enumerate(structs):
            rows, margin = neighbor_ref.brute_neighbors(s.frac_coords, s.lattice.matrix, vf.R_ATOM)
            need = max(1e-9, 100.0 * neighbor_ref.cart_bound(s.frac_coords, s.lattice.matrix))
            assert margin > need, (name, i, margin, need)
            worst = min(worst, margin / need)
            g = graphs[name][i] if name in graphs else conv(s)
            ag = np.asarray(g.atom_graph).reshape(-1, 2)
            got = np.concatenate([ag, np.asarray(g.neighbor_image, np.int64).reshape(-1, 3)], 1)
            assert np.array_equal(got[np.lexsort(got.T[::-1])], rows.table), (name, i)
    print(f"smallest margin / required margin: {worst:.3g}")


def _energies(oracle, gs):
    return np.array([float(p["e"]) for p in oracle.predict_graph(gs, "e", batch_size=len(gs))])


@pytest.mark.parametrize("wname", vf.WEIGHTS)
def test_biases_and_batch_switch_move_every_energy_far_past_the_tolerance(graphs, weight_sets, wname):
    """The GPU matrix is not vacuous: with the float64 oracle, zeroing the seven ``mlp_out`` biases changes every structure's energy
    in every group with angles by more than 100 x TOL["e"] (measured minimum over both weight sets: 6.3e-3 eV/atom), and the pair
    alone differs from the pair inside ``low`` by more than 10 x TOL["e"] (2.5e-4 eV/atom with weights_v020.npz)."""
    torch.set_num_threads(8)
    w = weight_sets[wname]
    assert set(vf.MLP_OUT_BIASES) <= set(w) and all(np.abs(w[k]).max() > 0 for k in vf.MLP_OUT_BIASES)
    w0 = {k: (np.zeros_like(v) if k in vf.MLP_OUT_BIASES else v) for k, v in w.items()}
    o, o0 = _oracle(w, torch.float64), _oracle(w0, torch.float64)
    sets = dict(graphs, long=[vf.converter()(s) for s in vf.long_structures()])
    least = float("inf")
    for name, gs in sets.items():
        if name.startswith("noangle"):
            continue
        d = np.abs(_energies(o, gs) - _energies(o0, gs))
        least = min(least, float(d.min()))
        assert d.min() > 100 * TOL["e"], (name, d)
    alone, inside = _energies(o, graphs["noangle"])[0], _energies(o, graphs["low"])[0]
    print(f"{wname}: least effect of the biases {least:.3e} eV/atom; pair alone vs in low {abs(alone - inside):.3e} eV/atom")
    assert abs(alone - inside) > 10 * TOL["e"]
    two = _energies(o, graphs["noangle_2"])
    assert abs(two[0] - alone) < 1e-12 and abs(two[1] - alone) < 1e-12       # a batch of zero-angle structures: no shift for any


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_oracle_reproduces_the_references_batch_semantics(graphs, weight_sets, dtype):
    """The unmodified reference's own predictions (batch_v020_low.npz): pair + trimer + chain in ONE call -- the zero-angle pair
    receives the BondConv biases (model.py:459 tests the batch) -- and the pair alone, which does not."""
    torch.set_num_threads(1)
    d = np.load(os.path.join(GOLDEN, "batch_v020_low.npz"))
    assert np.array_equal(d["n_atoms"], [len(g.atomic_number) for g in graphs["low"]])
    assert np.array_equal(d["n_angles"], [len(np.asarray(g.bond_graph).reshape(-1, 5)) for g in graphs["low"]])
    for wname, prefix, tol in ((vf.WEIGHTS[0], "", TOL_ORACLE), (vf.WEIGHTS[1], "tl_", TOL_ORACLE_TL)):
        o = _oracle(weight_sets[wname], dtype)
        trio = o.predict_graph(graphs["low"], "efsm", batch_size=3)
        alone = o.predict_graph(graphs["noangle"][0], "efsm")
        for k in ("e", "f", "s", "m"):
            for i, out in enumerate(trio):
                err = float(np.abs(np.asarray(out[k], np.float64) - d[f"{prefix}trio_{i}_{k}"]).max())
                assert err <= tol[k], (wname, "trio", i, k, err)
            err = float(np.abs(np.asarray(alone[k], np.float64) - d[f"{prefix}alone_{k}"]).max())
            assert err <= tol[k], (wname, "alone", k, err)
        # the recording itself separates the two semantics by far more than the oracle's tolerance
        assert abs(float(d[f"{prefix}trio_0_e"]) - float(d[f"{prefix}alone_e"])) > 10 * TOL["e"]


@pytest.mark.parametrize("wname", vf.WEIGHTS)
@pytest.mark.parametrize("name", ["low", "noangle", "noangle_2"])
def test_pipeline_models_equal_the_oracle_on_the_batch_switch_fp64(graphs, weight_sets, wname, name):
    """StagedModel / StagedTrainer in float64 (what the kernels compute: q_bias switched by the batch's angle count) == the float64
    autograd oracle on ``low`` and on the zero-angle batches, predictions and all 141 gradient tensors, at the bars of
    tests/test_v020.py (1e-12 / 1e-11 outputs, 1e-10 first order, 2e-9 second order).  Without angles the three BondConv ``mlp_out``
    bias gradients are exactly zero."""
    from chgnet_amd.pack import pack_batch, pack_weights, unpack_weight_grads
    from oracle.staged_ref import StagedModel
    from oracle.staged_train import StagedTrainer

    torch.set_num_threads(4)
    w = weight_sets[wname]
    pw = pack_weights(w, V020_ARGS)
    gs = graphs[name]
    pb = pack_batch(gs)
    o = _oracle(w, torch.float64)
    ref = o.forward(gs, "efsm", return_site_energies=True)
    out = StagedModel(pw).run(pb)
    cat = lambda parts: np.concatenate([np.atleast_1d(p) for p in parts])  # noqa: E731
    assert np.abs(out["e"] - np.array(ref["e"])).max() < 1e-12
    assert np.abs(out["f"] - cat(ref["f"])).max() < 1e-12
    assert np.abs(out["s"] - np.stack(ref["s"])).max() < 1e-11
    assert np.abs(out["m"] - cat(ref["m"])).max() < 1e-12
    assert np.abs(out["site_energies"] - cat(ref["site_energies"])).max() < 1e-12

    rng = np.random.default_rng(47)
    gE, gF, gS = rng.normal(size=pb.n_struct), rng.normal(size=(pb.n_atoms, 3)), rng.normal(size=(pb.n_struct, 3, 3))
    tE, tF, tS = torch.tensor(gE), torch.tensor(gF), torch.tensor(gS)

    def check(got, want, tol, first_order):
        assert set(got) == set(want) == set(w) and len(want) == 141
        for k, r in want.items():
            if k.startswith(DEAD) or (first_order and k.startswith("site_wise")):
                assert not np.any(got[k]), k
                continue
            scale = np.abs(r).max()
            if scale == 0:
                assert np.abs(got[k]).max() < 1e-12, k
            else:
                assert np.abs(got[k] - r).max() < tol * scale, (k, np.abs(got[k] - r).max(), scale)
            if pb.n_angles == 0 and k in vf.BOND_BIASES:
                assert scale == 0 and not np.any(got[k]), k

    want = o.parameter_gradients(gs, lambda r: (r["e"] * tE).sum())
    got = StagedModel(pw).run(pb, e_cot=gE)
    check(unpack_weight_grads(_blob_from(got["wgrad"], pw), pw), want, 1e-10, True)
    if pb.n_angles:
        assert all(np.abs(want[k]).max() > 0 for k in vf.BOND_BIASES)
    want = o.parameter_gradients(gs, lambda r: (r["e"] * tE).sum() + (r["f"] * tF).sum() + (r["s"] * tS).sum(), task="efs")
    got = StagedTrainer(pw).run(pb, gE=gE, gF=gF, gS=gS)
    check(unpack_weight_grads(_blob_from(got["wgrad"], pw), pw), want, 2e-9, True)
