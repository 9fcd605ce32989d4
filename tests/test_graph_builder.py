"""Native graph builder (csrc/host_graph.cpp) vs the reference's graph semantics."""

from __future__ import annotations

import os

import numpy as np
import pytest

from chgnet_amd import CrystalGraphConverter, Structure
from chgnet_amd.graph.converter import build_graph_arrays, graph_arrays_from_neighbors
from chgnet_amd.graph.structure import Lattice
from conftest import GOLDEN, load_case


def limno2() -> Structure:
    _, d = load_case("limno2")
    return Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"])


def test_toy_bigraph_known_answers():
    """Known-answer vectors of reference tests/test_graph.py:52-97 (3 nodes, 8 directed edges incl. a
    periodic self-pair), fed through the from-neighbours entry point."""
    center = [0, 0, 1, 1, 1, 1, 2, 2]
    nbr = [1, 2, 0, 2, 1, 1, 0, 1]
    image = [[0, 0, 0]] * 4 + [[0, 0, 1], [0, 0, -1]] + [[0, 0, 0]] * 2
    dist = [1, 2, 1, 5, 4, 4, 2, 5]
    g = graph_arrays_from_neighbors(3, center, nbr, image, dist, r_bond=7)
    assert len(g["atom_graph"]) == 8 and len(g["undirected2directed"]) == 4
    assert g["atom_graph"][0].tolist() == [0, 1] and g["atom_graph"][1].tolist() == [0, 2]
    assert g["atom_graph"][2].tolist() == [1, 0] and g["atom_graph"][6].tolist() == [2, 0]
    assert g["directed2undirected"][:3].tolist() == [0, 1, 0]
    bg = g["bond_graph"]
    assert len(bg) == 16
    assert bg[0].tolist() == [0, 0, 0, 1, 1]
    assert bg[5].tolist() == [2, 1, 6, 2, 7]
    assert bg[10].tolist() == [1, 3, 4, 0, 2]
    assert g["undirected2directed"][:3].tolist() == [0, 1, 3]


def test_limno2_count_goldens():
    """Counts asserted by reference tests/test_crystal_graph.py:22-65 (cutoffs 5 / 3)."""
    g = CrystalGraphConverter(atom_graph_cutoff=5, bond_graph_cutoff=3)(limno2())
    assert g.composition == "Li2 Mn2 O4"
    assert g.atomic_number.tolist() == [3, 3, 25, 25, 8, 8, 8, 8]
    assert g.atom_frac_coord.shape == (8, 3)
    assert g.atom_graph.shape == (384, 2)
    for atom in (0, 4, 7):
        assert (g.atom_graph[:, 0] == atom).sum() == 48
    assert (g.atom_graph[:, 1] == 0).sum() == 48
    assert g.bond_graph.shape == (744, 5)
    assert (g.bond_graph[:, 0] == 1).sum() == 72
    assert g.lattice.shape == (3, 3)
    assert g.undirected2directed.shape == (192,) and g.directed2undirected.shape == (384,)
    assert g.atom_graph.dtype == np.int32 and g.neighbor_image.dtype == np.float32


def test_supercell_count_goldens():
    """2x3x4 supercell: reference tests/test_crystal_graph.py:255-303."""
    g = CrystalGraphConverter(atom_graph_cutoff=5, bond_graph_cutoff=3)(limno2().make_supercell([2, 3, 4]))
    assert g.atom_graph.shape == (9216, 2)
    assert g.bond_graph.shape == (17856, 5)
    assert g.undirected2directed.shape == (4608,)
    assert (g.atom_graph[:, 0] == 4).sum() == 48 and (g.atom_graph[:, 1] == 100).sum() == 48


@pytest.mark.parametrize("name", ["limno2", "s16tri", "noangle"])
def test_indexing_bit_exact_vs_reference_converter(name):
    """Same (shuffled) neighbour list in -> element-for-element the graph the reference's
    CrystalGraphConverter produced (tests/golden/graph_*.npz)."""
    d = np.load(os.path.join(GOLDEN, f"graph_{name}.npz"))
    g = graph_arrays_from_neighbors(int(d["n_atoms"]), d["nl_center"], d["nl_neighbor"], d["nl_image"], d["nl_distance"], r_bond=3)
    assert np.array_equal(g["atom_graph"], d["atom_graph"])
    assert np.array_equal(g["directed2undirected"], d["directed2undirected"])
    assert np.array_equal(g["undirected2directed"], d["undirected2directed"])
    assert np.array_equal(g["bond_graph"].reshape(-1, 5), d["bond_graph"].reshape(-1, 5))
    assert np.array_equal(g["image"].astype(np.float32), d["neighbor_image"])


def test_graph_invariants_and_sortedness():
    s = limno2().make_supercell([2, 2, 1]).perturb(0.03, np.random.default_rng(1))
    a = build_graph_arrays(s.frac_coords, s.lattice.matrix, 6.0, 3.0)
    ag, d2u, u2d, bg = a["atom_graph"], a["directed2undirected"], a["undirected2directed"], a["bond_graph"]
    assert len(ag) == 2 * len(u2d)
    assert np.all(np.diff(ag[:, 0]) >= 0)                       # centre-major
    assert np.all(np.bincount(d2u) == 2)                        # every bond has exactly two directions
    assert np.array_equal(d2u[u2d], np.arange(len(u2d)))
    assert np.all(np.diff(bg[:, 1]) >= 0)                       # angles sorted by owning bond
    assert np.array_equal(ag[bg[:, 2], 0], bg[:, 0]) and np.array_equal(ag[bg[:, 4], 0], bg[:, 0])
    assert np.array_equal(d2u[bg[:, 2]], bg[:, 1]) and np.array_equal(d2u[bg[:, 4]], bg[:, 3])
    assert np.all(bg[:, 2] != bg[:, 4])
    # reverse edge has the negated image and the same length
    for k in range(0, len(u2d), 97):
        e1, e2 = np.flatnonzero(d2u == k)
        assert np.array_equal(a["image"][e1], -a["image"][e2]) and abs(a["distance"][e1] - a["distance"][e2]) < 1e-9
        assert ag[e1, 0] == ag[e2, 1] and ag[e1, 1] == ag[e2, 0]
    # distances agree with the geometry
    cart = s.cart_coords
    v = cart[ag[:, 1]] + a["image"] @ s.lattice.matrix - cart[ag[:, 0]]
    assert np.abs(np.linalg.norm(v, axis=1) - a["distance"]).max() < 1e-9
    assert a["distance"].max() < 6.0 and a["distance"].min() > 1e-8


def test_unwrapped_fractional_coordinates_give_the_same_bonds():
    s = limno2()
    shifted = Structure(s.lattice, s.atomic_numbers, s.frac_coords + np.array([[1, -2, 0]] * 4 + [[0, 0, 3]] * 4))
    a = build_graph_arrays(s.frac_coords, s.lattice.matrix, 5.0, 3.0)
    b = build_graph_arrays(shifted.frac_coords, shifted.lattice.matrix, 5.0, 3.0)
    assert len(a["atom_graph"]) == len(b["atom_graph"]) and len(a["bond_graph"]) == len(b["bond_graph"])
    assert np.allclose(np.sort(a["distance"]), np.sort(b["distance"]), atol=1e-9)


@pytest.mark.parametrize("on_isolated_atoms", ["ignore", "warn", "error"])
def test_isolated_atom_policy(on_isolated_atoms, capsys):
    """reference tests/test_converter.py:65-100 (NaCl, a = 4 A, 5x strain -> both atoms isolated)."""
    nacl = Structure(Lattice(np.eye(3) * 4.0), ["Na", "Cl"], [[0, 0, 0], [0.5, 0.5, 0.5]]).apply_strain(5)
    atom_graph_cutoff = 5
    conv = CrystalGraphConverter(atom_graph_cutoff=atom_graph_cutoff, bond_graph_cutoff=3, on_isolated_atoms=on_isolated_atoms)
    graph_id = "strained"
    err_msg = (f"Structure {graph_id=} has 2 isolated atom(s) with {atom_graph_cutoff=}. "
               f"CHGNet calculation will likely go wrong")
    if on_isolated_atoms == "error":
        with pytest.raises(ValueError, match="has 2 isolated atom") as exc:
            conv.forward(nacl, graph_id=graph_id)
        assert err_msg in str(exc.value)
    else:
        g = conv.forward(nacl, graph_id=graph_id)
        assert len(g.atom_graph) == 0 and g.num_isolated_atoms == 2
        out, err = capsys.readouterr()
        assert out == ""
        assert (err_msg in err) if on_isolated_atoms == "warn" else err == ""


def test_graph_builder_error_codes():
    with pytest.raises(ValueError, match="singular lattice|invalid argument"):
        build_graph_arrays(np.zeros((1, 3)), np.zeros((3, 3)), 5.0, 3.0)
    with pytest.raises(ValueError, match="not complete|2 \\* number"):
        graph_arrays_from_neighbors(2, [0], [1], [[0, 0, 0]], [1.0], r_bond=3)   # dangling directed edge


def test_crystal_graph_file_round_trip_and_reference_format(tmp_path):
    """On-disk format of reference crystalgraph.py:138-167: torch.save(to_dict()) with tensor values."""
    import torch

    g, _ = load_case("s16tri")
    path = g.save(fname="g.pt", save_dir=str(tmp_path))
    raw = torch.load(path, weights_only=False)
    assert isinstance(raw, dict) and isinstance(raw["atom_graph"], torch.Tensor) and raw["atom_graph"].dtype == torch.int32
    assert raw["atom_frac_coord"].dtype == torch.float32 and raw["atom_graph_cutoff"] == 6
    from chgnet_amd import CrystalGraph

    g2 = CrystalGraph.from_file(path)
    for key in ("atomic_number", "atom_frac_coord", "atom_graph", "neighbor_image", "directed2undirected",
                "undirected2directed", "bond_graph", "lattice"):
        assert np.array_equal(getattr(g, key), getattr(g2, key)), key
    assert repr(g2).startswith("CrystalGraph(composition=") and "n_atoms=16" in repr(g2)
    # a file written the way the reference writes it (tensor dict incl. grad-tracking floats) loads too
    ref_style = {k: (torch.tensor(v, requires_grad=v.dtype == np.float32) if isinstance(v, np.ndarray) else v)
                 for k, v in g.to_dict().items()}
    torch.save(ref_style, tmp_path / "ref.pt")
    g3 = CrystalGraph.from_file(str(tmp_path / "ref.pt"))
    assert np.array_equal(g3.bond_graph, g.bond_graph) and g3.lattice.dtype == np.float32


def _cases_for_native_reference():
    rng = np.random.default_rng(5)
    out = []
    for name in ("limno2", "s16tri", "noangle", "li9co7o16"):
        _, d = load_case(name)
        out.append(Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]))
    out.append(out[0].make_supercell([3, 2, 1]).perturb(0.02, rng))
    out.append(Structure(Lattice(np.eye(3) * 2.5), ["Fe"], [[0.1, 0.2, 0.3]]))          # periodic self-pairs only
    out.append(Structure(Lattice([[3.1, 0.2, 0.0], [0.4, 2.9, 0.3], [0.1, 0.5, 3.3]]), ["Li", "O"], [[0, 0, 0], [0.45, 0.55, 0.5]]))
    return out


def test_builder_matches_the_references_compiled_c_algorithm():
    """What the reference's create_graph.c built (tests/golden/ref_graph_c.json, make_ref_graph_golden.py: the library compiled
    from where it lies) from the same neighbour list, in our order and in a shuffled order: every array identical."""
    import json

    from golden.make_golden_helpers import array_digest

    with open(os.path.join(GOLDEN, "ref_graph_c.json")) as fh:
        fx = json.load(fh)
    rng = np.random.default_rng(3)                      # the shuffles the fixture was made with
    for i, s in enumerate(_cases_for_native_reference()):
        for j, (r_atom, r_bond) in enumerate(((6.0, 3.0), (5.0, 3.0), (4.0, 4.0))):
            a = build_graph_arrays(s.frac_coords, s.lattice.matrix, r_atom, r_bond)
            nl = {"center": a["atom_graph"][:, 0].astype(np.int64), "neighbor": a["atom_graph"][:, 1].astype(np.int64),
                  "image": a["image"].astype(np.int64), "distance": a["distance"]}
            for shuffle in (0, 1):
                if shuffle and len(nl["center"]):
                    perm = np.concatenate([rng.permutation(np.flatnonzero(nl["center"] == c)) for c in range(len(s))])
                    nl = {k: v[perm] for k, v in nl.items()}
                ref = fx[f"cpu_{i}_{j}_{shuffle}"]
                for key in ("center", "neighbor", "image", "distance"):          # the list the reference was fed
                    assert array_digest(nl[key]) == ref[key], (key, i, r_atom, r_bond, shuffle)
                got = graph_arrays_from_neighbors(len(s), nl["center"], nl["neighbor"], nl["image"], nl["distance"], r_bond)
                for key in ("atom_graph", "directed2undirected", "undirected2directed", "bond_graph"):
                    assert array_digest(got[key]) == ref[key], (key, i, r_atom, r_bond, shuffle)


def test_cutoff_boundary_rules_known_answer():
    """Bond-graph cutoff boundary, hand-made (reference graph.py:283-327 / create_graph.c via cygraph): an
    undirected bond whose length EQUALS the cutoff still owns angles (it is skipped only when dist > cutoff), but
    is never the second bond of an angle (a neighbour qualifies only when dist < cutoff).  Atom-graph boundary:
    the neighbour list keeps d < r_atom strictly (host_graph.cpp: d2 < r2); pymatgen's own inequality at
    exactly d == r cannot be pinned offline (pymatgen is not installed) and cannot change E/F/S because the
    envelope and its derivative vanish at the cutoff (basis.py:197-205).  Our own strict ``<`` is pinned by exact integer
    arithmetic on the tie cases of tests/graph_hard_cases.py (a shell exactly on the cutoff is out: test_neighbor_oracle_cpu.py,
    test_gpu_graph_oracle.py)."""
    # triangle A(0) B(1) C(2): |AB| = 3.0 (== cutoff), |AC| = 2.0, |BC| = 2.5
    center = [0, 0, 1, 1, 2, 2]
    nbr = [1, 2, 0, 2, 0, 1]
    dist = [3.0, 2.0, 3.0, 2.5, 2.0, 2.5]
    g = graph_arrays_from_neighbors(3, center, nbr, [[0, 0, 0]] * 6, dist, r_bond=3.0)
    d2u, bg = g["directed2undirected"], g["bond_graph"]
    ab, ac, bc = d2u[0], d2u[1], d2u[3]
    assert (ab, ac, bc) == (0, 1, 2)
    assert sorted(bg[:, 1].tolist()) == [0, 0, 1, 2]          # AB owns an angle at A and one at B; AC, BC one each (at C)
    assert ab not in bg[:, 3].tolist()                         # ... but never appears as the SECOND bond
    assert bg.tolist() == [[0, 0, 0, 1, 1], [1, 0, 2, 2, 3], [2, 1, 4, 2, 5], [2, 2, 5, 1, 4]]
    from oracle import ref_graph

    if ref_graph.available() or ref_graph.build() is not None:  # the reference's compiled C says the same
        ref = ref_graph.reference_graph(3, center, nbr, [[0, 0, 0]] * 6, dist, 3.0)
        assert np.array_equal(ref["bond_graph"].reshape(-1, 5), bg)
    # one ulp above the cutoff: the bond drops out of the bond graph entirely
    dist2 = [np.nextafter(3.0, 4.0) if x == 3.0 else x for x in dist]
    g2 = graph_arrays_from_neighbors(3, center, nbr, [[0, 0, 0]] * 6, dist2, r_bond=3.0)
    assert g2["bond_graph"].tolist() == [[2, 1, 4, 2, 5], [2, 2, 5, 1, 4]]
    # atom-graph boundary of our own neighbour list: strict d < r
    s = Structure(Lattice(np.eye(3) * 3.0), ["Fe"], [[0, 0, 0]])     # images at exactly 3.0
    assert len(build_graph_arrays(s.frac_coords, s.lattice.matrix, 3.0, 3.0)["atom_graph"]) == 0
    assert len(build_graph_arrays(s.frac_coords, s.lattice.matrix, np.nextafter(3.0, 4.0), 3.0)["atom_graph"]) == 6


def _random_cells():
    rng = np.random.default_rng(21)
    out = [s for s in _cases_for_native_reference()]
    out.append(limno2().make_supercell([4, 3, 2]).perturb(0.05, rng))                       # 192 atoms, orthorhombic
    out.append(Structure(Lattice([[7.1, 0.3, -0.4], [2.2, 6.5, 0.6], [-1.7, 2.4, 8.3]]), rng.choice([3, 8, 25], 40),
                         rng.random((40, 3)) * 3 - 1))                                     # skewed, unwrapped coordinates
    out.append(Structure(Lattice(np.diag([30.0, 3.2, 3.4])), rng.choice([3, 8], 24), rng.random((24, 3))))   # needle: 1 bin on two axes
    out.append(Structure(Lattice(np.diag([12.0, 12.0, 12.0])), ["O"] * 8,
                         [[0, 0, 0], [0.5, 0, 0], [1.0 - 1e-17, 0.5, 0.5], [-1e-17, 0.25, 0.75], [0.999999999999, 0.1, 0.1],
                          [0.5, 0.5, 1.0], [2.5, -1.5, 0.5], [0.25, 0.25, 0.25]]))          # coordinates on / across the cell faces
    return out


def test_cell_list_equals_all_pairs_bit_for_bit():
    """The O(n) cell-list search returns the rows of the all-pairs search in the same order with bit-identical
    distances and images (any cell shape, unwrapped / on-the-boundary coordinates, cells smaller than the cutoff)."""
    for s in _random_cells():
        for r_atom, r_bond in ((6.0, 3.0), (3.7, 3.7), (11.0, 2.0)):
            a = build_graph_arrays(s.frac_coords, s.lattice.matrix, r_atom, r_bond, search="pairs")
            b = build_graph_arrays(s.frac_coords, s.lattice.matrix, r_atom, r_bond, search="cells")
            for key in ("atom_graph", "image", "distance", "directed2undirected", "undirected2directed", "bond_graph"):
                assert np.array_equal(a[key], b[key]), (len(s), r_atom, key)


def test_cell_list_scales_linearly_to_thousands_of_atoms():
    """2,048-atom cell: the automatic choice is the cell list; build time grows ~linearly with the atom count
    (the all-pairs search grows quadratically), and a sub-sampled comparison with all pairs still matches."""
    import time

    base = limno2().make_supercell([4, 4, 2]).perturb(0.03, np.random.default_rng(9))      # 256 atoms
    big = base.make_supercell([2, 2, 2])                                                   # 2048 atoms
    def best_of(n, s):            # best of n: a busy test machine (parallel builds, other ranks) must not decide a scaling claim
        best, out = float("inf"), None
        for _ in range(n):
            t = time.perf_counter()
            out = build_graph_arrays(s.frac_coords, s.lattice.matrix, 6.0, 3.0)
            best = min(best, time.perf_counter() - t)
        return best, out

    t_small, small = best_of(5, base)
    t_large, large = best_of(3, big)
    assert len(large["atom_graph"]) == 8 * len(small["atom_graph"]) and len(large["bond_graph"]) == 8 * len(small["bond_graph"])
    assert t_large < 24 * max(t_small, 1e-3)                                                # 8x the atoms: nowhere near 64x
    pairs = build_graph_arrays(big.frac_coords, big.lattice.matrix, 6.0, 3.0, search="pairs")
    for key in ("atom_graph", "image", "distance", "bond_graph"):
        assert np.array_equal(pairs[key], large[key]), key
