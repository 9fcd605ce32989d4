"""The fixtures of tests/test_gpu_angle_paths.py (tests/angle_fixtures.py) have the properties that make a pass there mean what it
claims: the coordination numbers either side of the kernels' limits, bonds exactly at the bond cutoff that own angles, the defect
each malformed angle set is meant to carry, and an fp32 oracle close enough to the fp64 one for the parity criterion to bite."""

from __future__ import annotations

import numpy as np
import pytest

import angle_fixtures as af
from chgnet_amd.graph.converter import build_graph_arrays, graph_arrays_from_neighbors


def _short_counts(s):
    """float64 host converter: bonds shorter than the bond cutoff per atom, and the number of bonds at exactly the cutoff."""
    a = build_graph_arrays(s.frac_coords, s.lattice.matrix, af.R_ATOM, af.R_BOND)
    d, c = a["distance"], a["atom_graph"][:, 0]
    return np.bincount(c[d < af.R_BOND], minlength=len(s)), int((d == af.R_BOND).sum())


def _rows_per_centre(g):
    return np.bincount(np.asarray(g.bond_graph).reshape(-1, 5)[:, 0], minlength=len(g.atomic_number))


@pytest.mark.parametrize("k", af.SHELL_KS)
def test_shell_cluster_centre_has_k_short_bonds(k):
    s = af.shell_cluster(k)
    n, ties = _short_counts(s)
    assert n[0] == k and ties == 0
    assert n[1:].min() >= 1 and n[1:].max() <= 19
    g = af.converter()(s)
    rows = _rows_per_centre(g)
    assert rows[0] == k * (k - 1)                                # the complete n (n - 1) block at the centre
    assert np.array_equal(rows, n * (n - 1))                     # ... and at every shell atom
    bg = np.asarray(g.bond_graph).reshape(-1, 5)
    assert len(np.unique(bg[:, [0, 2, 4]], axis=0)) == len(bg)


def test_cutoff_tie_cells_have_bonds_at_exactly_the_cutoff_that_own_angles():
    for s, per_atom in zip(af.tie_cells(), (6, 2)):
        n, ties = _short_counts(s)
        assert ties == per_atom * len(s) and n.min() >= 12
        g = af.converter()(s)
        d = af.directed_lengths(g)                       # also exactly 3.0 from the graph's own float32 coordinates
        tie = np.flatnonzero(d == af.R_BOND)
        assert len(tie) == per_atom * len(s)
        bg = np.asarray(g.bond_graph).reshape(-1, 5)
        assert np.isin(tie, bg[:, 2]).all()              # every bond at the cutoff is the first bond of angles ...
        assert not np.isin(tie, bg[:, 4]).any()          # ... and never a second bond
        assert len(bg) != int((n * (n - 1)).sum())       # so the angle sets are not the n (n - 1) blocks


def test_dense_cells_have_42_short_bonds_per_atom():
    for s in af.dense_cells():
        n, ties = _short_counts(s)
        assert (n == 42).all() and ties == 0
        assert np.array_equal(_rows_per_centre(af.converter()(s)), n * (n - 1))


def test_low_coordination_cells():
    pair, trimer, chain, big = af.low_coordination_cells()
    for s, want in ((pair, [1, 1]), (trimer, [1, 2, 1]), (chain, [2] * 10)):
        n, _ = _short_counts(s)
        assert n.tolist() == want
        assert _rows_per_centre(af.converter()(s)).max() <= 2
    assert len(big) == 100


def test_md_cells_and_large_batch():
    md = af.md_cells()
    assert [len(s) for s in md] == [256, 512]
    assert all(_short_counts(s)[0].max() <= 32 for s in md)
    large = af.large_batch()
    assert sum(len(s) for s in large) + 1 > 8192


def test_host_bond_graph_equals_the_references_compiled_builder():
    """Same neighbour list -> the reference's create_graph.c (when it is available) builds the same angle rows, ties included."""
    from oracle import ref_graph

    if not (ref_graph.available() or ref_graph.build() is not None):
        pytest.skip("the reference's graph builder is not available")
    structs = [s for v in af.structure_groups().values() for s in v] + af.malformed_bases()
    for s in structs:
        a = build_graph_arrays(s.frac_coords, s.lattice.matrix, af.R_ATOM, af.R_BOND)
        c, nb, im, d = a["atom_graph"][:, 0], a["atom_graph"][:, 1], a["image"], a["distance"]
        ours = graph_arrays_from_neighbors(len(s), c, nb, im, d, r_bond=af.R_BOND)
        ref = ref_graph.reference_graph(len(s), c, nb, im, d, af.R_BOND)
        assert np.array_equal(ref["bond_graph"].reshape(-1, 5), ours["bond_graph"])
        assert np.array_equal(af.converter()(s).bond_graph, ours["bond_graph"])


def test_malformed_sets_pass_packing_and_carry_their_defect():
    from chgnet_amd.pack import pack_batch

    conv = af.converter()
    bases = [conv(s) for s in af.malformed_bases()]
    sets = af.malformed_graphs()
    for kind in af.MALFORMED_KINDS:
        pack_batch(sets[kind])                                  # the consistency checks of an upload pass
    for g0, ga, gb, gc, gd in zip(bases, *(sets[k] for k in af.MALFORMED_KINDS)):
        bg0 = np.asarray(g0.bond_graph).reshape(-1, 5)
        key = lambda bg: sorted(map(tuple, bg.tolist()))        # noqa: E731
        # (a) the same rows in another order
        bga = np.asarray(ga.bond_graph).reshape(-1, 5)
        assert key(bga) == key(bg0) and not np.array_equal(bga, bg0)
        # (b) one (centre, b1, b2) triple twice, one missing, the row count unchanged, each group still n - 1 rows
        bgb = np.asarray(gb.bond_graph).reshape(-1, 5)
        assert len(bgb) == len(bg0) and np.array_equal(_rows_per_centre(gb), _rows_per_centre(g0))
        trip, cnt = np.unique(bgb[:, [0, 2, 4]], axis=0, return_counts=True)
        assert sorted(cnt.tolist())[-2:] == [1, 2] and (cnt == 2).sum() == 1
        assert len(trip) == len(bg0) - 1
        assert (bgb[:, 4] != bgb[:, 2]).all()
        # (c) one row fewer at one centre
        d_rows = _rows_per_centre(g0) - _rows_per_centre(gc)
        assert d_rows.sum() == 1 and d_rows.min() == 0
        # (d) one row's second bond does not start at the row's centre (but is a short bond of another atom)
        bgd = np.asarray(gd.bond_graph).reshape(-1, 5)
        ag = np.asarray(gd.atom_graph).reshape(-1, 2)
        foreign = ag[bgd[:, 4], 0] != bgd[:, 0]
        assert foreign.sum() == 1 and len(bgd) == len(bg0)
        assert np.isin(bgd[foreign, 4], bg0[:, 2]).all()


@pytest.mark.parametrize("which", ["seed0", "trained_like"])
def test_fp32_oracle_is_close_to_fp64_on_the_fixtures(golden_weights, trained_like_weights, which):
    """The GPU criterion is max(TOL x scale, 20 x |fp32 oracle - fp64 oracle|): on these fixtures it stays below 1e-3 of each
    output's scale (no near-contact or saturated gate lets a kernel error of that size through).  The MD cells and the large batch
    are thermalised or perturbed crystals of the golden kind and are left to the GPU test."""
    import torch

    from oracle.chgnet_oracle import OracleCHGNet
    from test_gpu_parity import TOL

    weights = golden_weights if which == "seed0" else trained_like_weights
    groups = af.structure_groups()
    conv = af.converter()
    gs = [conv(s) for name in ("shell_le32", "shell_33", "shell_40", "tie", "dense", "low") for s in groups[name]]
    gs += [g for v in af.malformed_graphs().values() for g in v]
    torch.set_num_threads(8)
    kw = dict(return_site_energies=True, batch_size=64)
    o64 = OracleCHGNet(weights, dtype=torch.float64).predict_graph(gs, "efsm", **kw)
    o32 = OracleCHGNet(weights).predict_graph(gs, "efsm", **kw)
    for i, (a, b) in enumerate(zip(o64, o32)):
        for key in ("e", "f", "s", "m", "site_energies"):
            ref = np.asarray(a[key], np.float64)
            if ref.size == 0:
                continue
            assert np.isfinite(ref).all()
            scale = max(1.0, float(np.abs(ref).max()))
            bar = max(TOL[key] * scale, 20 * float(np.abs(np.asarray(b[key], np.float64) - ref).max()))
            assert bar < 1e-3 * scale, (i, key, bar, scale)
