"""The host graph builder (csrc/host_graph.cpp, both searches) against a brute-force neighbour oracle that shares none of its
reasoning (tests/neighbor_ref.py), on the hard cell shapes of tests/graph_hard_cases.py -- and the oracle itself against
known answers."""

from __future__ import annotations

import numpy as np
import pytest

import graph_hard_cases as hard
import neighbor_ref
from chgnet_amd.graph.converter import build_graph_arrays

CASE_CUTS = [(name, r_atom, r_bond) for name, _, cuts in hard.cases() for r_atom, r_bond in cuts]


# ---- the oracle against known answers (none of our code) -------------------------------------------------------------------------
def _shells(rows, centre=0):
    d = np.asarray(rows.distance[rows.center == centre], np.float64)
    vals, counts = np.unique(np.round(d, 9), return_counts=True)
    return vals, counts


def test_oracle_shell_counts_fcc_and_simple_cubic():
    a = 4.0
    fcc = [[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]]
    rows, margin = neighbor_ref.brute_neighbors(fcc, np.eye(3) * a, 5.0)            # shells at a/sqrt2, a, a*sqrt(3/2) = 2.83, 4, 4.90
    for centre in range(4):
        vals, counts = _shells(rows, centre)
        assert counts.tolist() == [12, 6, 24]
        assert np.allclose(vals, [a / 2 ** 0.5, a, a * 1.5 ** 0.5], atol=1e-9)
    assert abs(margin - (5.0 - a * 1.5 ** 0.5)) < 1e-9
    rows, _ = neighbor_ref.brute_neighbors([[0.3, 0.7, 0.1]], np.eye(3) * 3.0, 5.5)    # 3, 4.24, 5.20
    vals, counts = _shells(rows)
    assert counts.tolist() == [6, 12, 8] and np.allclose(vals, [3.0, 3.0 * 2 ** 0.5, 3.0 * 3 ** 0.5], atol=1e-9)


def test_oracle_rows_are_sorted_paired_and_description_independent():
    per_atom = {}
    for m in hard.UNIMODULAR:
        name = f"tri8_{m}"
        s, _ = hard.case(name)
        rows, _ = hard.oracle_rows(name, 6.0)
        t = rows.table
        assert np.array_equal(t, t[np.lexsort(t.T[::-1])])                           # (centre, neighbour, ia, ib, ic)
        have = {tuple(r) for r in t.tolist()}
        assert len(have) == len(t)
        assert all((j, i, -a, -b, -c) in have for i, j, a, b, c in have)             # every row has its reverse
        # the long-double distance is the geometry of the coordinates as given
        v = (s.frac_coords[rows.neighbor] + rows.image - s.frac_coords[rows.center]) @ s.lattice.matrix
        assert np.abs(np.linalg.norm(v, axis=1) - np.asarray(rows.distance, np.float64)).max() < 1e-9
        per_atom[m] = [np.sort(np.asarray(rows.distance[rows.center == i], np.float64)) for i in range(len(s))]
    for m in hard.UNIMODULAR:                                                        # same crystal: same distances per atom
        for a, b in zip(per_atom["id"], per_atom[m]):
            assert len(a) == len(b) and np.abs(a - b).max() < 1e-9
    reach = {f"{b}_{m}": int(np.abs(hard.oracle_rows(f"{b}_{m}", r)[0].image).max()) for b, r in (("tri8", 11.0), ("lmo40", 6.0)) for m in hard.UNIMODULAR}
    print("largest image index per description:", reach)
    assert max(reach.values()) >= 20 and reach["tri8_id"] <= 3                       # the skewed descriptions are the hard ones


@pytest.mark.parametrize("name", hard.TIES)
def test_oracle_tie_cases_equal_integer_arithmetic(name):
    _, cuts = hard.case(name)
    rows, margin = hard.oracle_rows(name, cuts[0][0])
    want = hard.integer_tie_rows(name)
    assert np.array_equal(rows.table, want)
    assert margin == 0.0                                                             # a shell lies exactly on the cutoff, and is out
    assert len(want) == {"tie_sc3": 26, "tie_fcc4": 48, "tie_tet": 36}[name]


def test_line_graph_rules_restate_the_compiled_reference():
    """The pure-Python restatement used where oracle/_ref is absent gives what the reference's C builder gives."""
    from oracle import ref_graph

    if not ref_graph.available() and ref_graph.build() is None:
        pytest.fail("the reference's compiled builder is neither built nor buildable here")
    for name, r_atom, r_bond in (("tri8_m130", 6.0, 3.0), ("tie_tet", 6.0, 3.0), ("thin_needle", 4.0, 4.0), ("left_handed", 5.0, 3.0)):
        s, _ = hard.case(name)
        rows, _ = hard.oracle_rows(name, r_atom)
        ref = neighbor_ref.line_graph_ref(len(s), rows, r_bond)
        own = neighbor_ref.line_graph_rules(len(s), rows.center, rows.neighbor, rows.image, rows.distance, r_bond)
        for key in ("directed2undirected", "undirected2directed", "bond_graph"):
            assert np.array_equal(ref[key], own[key]), (name, key)
        assert len(ref["bond_graph"]) > 0


# ---- the condition on the inputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r_atom,r_bond", CASE_CUTS)
def test_cases_keep_their_distance_from_the_cutoffs(name, r_atom, r_bond):
    """Every case (the ties apart) has no distance within max(1e-9 A, 100 x the float64 error bound) of either cutoff, so the
    comparison below does not depend on the last bits of anybody's arithmetic."""
    m_atom, m_bond = hard.margins(name, r_atom, r_bond)
    need = hard.required_margin(name)
    print(f"{name} r={r_atom:g}/{r_bond:g}: margin {m_atom:.3e} / {m_bond:.3e}, required {need:.3e}")
    if name in hard.TIES:
        return
    assert m_atom >= need and m_bond >= need


def test_sort_limit_cutoffs_put_exactly_1024_and_1025_rows_on_the_busiest_centre():
    for K in (1024, 1025):
        _, cuts = hard.case(f"sort_{K}")
        rows, _ = hard.oracle_rows(f"sort_{K}", cuts[0][0])
        assert np.bincount(rows.center).max() == K


# ---- the host builder, both searches, against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("search", ["pairs", "cells"])
@pytest.mark.parametrize("name,r_atom,r_bond", CASE_CUTS)
def test_host_builder_equals_the_oracle(name, r_atom, r_bond, search):
    s, _ = hard.case(name)
    want = hard.oracle_graph(name, r_atom, r_bond)
    got = build_graph_arrays(s.frac_coords, s.lattice.matrix, r_atom, r_bond, search=search)
    assert np.array_equal(got["atom_graph"], want["atom_graph"]), "rows (centre, neighbour)"
    assert np.array_equal(got["image"], want["image"]), "images"
    tol = 64 * np.finfo(np.float64).eps * max(1.0, float(np.abs(s.frac_coords @ s.lattice.matrix).max()))
    if len(got["distance"]):
        assert float(np.abs(got["distance"].astype(np.longdouble) - want["rows"].distance).max()) <= tol
    for key in ("directed2undirected", "undirected2directed"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["bond_graph"].reshape(-1, 5), want["bond_graph"]), "bond_graph"
