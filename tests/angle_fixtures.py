"""Structures and graphs at the coordination numbers, cutoff ties and angle-set shapes where the angle kernels branch
(tests/test_gpu_angle_paths.py, checked on the CPU by tests/test_angle_fixtures_cpu.py).

Limits of the angle kernels these fixtures straddle (chgnet_amd/csrc): NS = 13 / 14 private LDS rows in the per-atom and team
adjoints, FA_NSL = 15 LDS rows in the per-atom forward, WIN_LIST = 32 short bonds per atom in the centre-major index, the
blocked-tile shapes of blk_shape_of, and the bond exactly at the bond cutoff that owns angles but is nobody's second bond."""

from __future__ import annotations

import copy

import numpy as np

R_ATOM, R_BOND = 6.0, 3.0
SHELL_KS = (2, 3, 6, 12, 13, 14, 15, 16, 17, 24, 31, 32, 33, 40)


def _structure(lattice, species, frac):
    from chgnet_amd import Structure
    from chgnet_amd.graph.structure import Lattice

    return Structure(Lattice(lattice), species, frac)


def _from_cart(lattice, species, cart):
    lattice = np.asarray(lattice, np.float64)
    return _structure(lattice, species, np.asarray(cart, np.float64) @ np.linalg.inv(lattice))


def converter(r_atom: float = R_ATOM, r_bond: float = R_BOND):
    from chgnet_amd import CrystalGraphConverter

    return CrystalGraphConverter(atom_graph_cutoff=r_atom, bond_graph_cutoff=r_bond)


def shell_cluster(k: int, seed: int = 0):
    """One Co at the centre of a 14 A cubic cell, k O on a Fibonacci sphere of radius 2.3 A, rattled by ~0.02 A: the centre
    has exactly k short bonds (3 A), the shell atoms 5-18 each; the clusters of neighbouring cells are > 6 A apart."""
    i = np.arange(k) + 0.5
    z = 1 - 2 * i / k
    phi = np.pi * (1 + 5 ** 0.5) * i
    rho = np.sqrt(1 - z * z)
    pts = 2.3 * np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1)
    pts += np.random.default_rng([77, k, seed]).normal(0, 0.02, pts.shape)
    cart = np.concatenate([[[0.0, 0.0, 0.0]], pts]) + 7.0
    return _from_cart(np.eye(3) * 14.0, ["Co"] + ["O"] * k, cart)


def fcc_li(a: float):
    """Conventional fcc cell (4 atoms), fractional coordinates in {0, 1/2}: exact in float32 and float64."""
    return _structure(np.eye(3) * a, ["Li"] * 4, [[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])


def tie_cells():
    """fcc Li at a = 3.0 A: 12 bonds of 2.12 A and 6 image bonds of EXACTLY 3.0 A (= the bond cutoff) per atom.  The 3 x 3 x 1
    supercell is rattled in the a-b plane only: the bond of every atom to its own image along c (frac difference (0, 0, 1),
    c = 3.0 A) stays exactly at the cutoff, the other bonds move off it.  (3 x 3 in the plane: no image of an atom's own at
    exactly the atom-graph cutoff in a direction the rattle touches.)"""
    base = fcc_li(3.0)
    sc = base.make_supercell([3, 3, 1])
    d = np.random.default_rng(11).normal(0, 0.03, (len(sc), 3))
    d[:, 2] = 0.0
    rattled = _structure(sc.lattice.matrix, sc.atomic_numbers, sc.frac_coords + d @ np.linalg.inv(sc.lattice.matrix))
    return [base, rattled]


def dense_cells():
    """fcc Li at a = 2.4 A: 12 + 6 + 24 = 42 bonds shorter than 3 A at every atom (past WIN_LIST): the whole graph is
    non-canonical for the centre-major index."""
    base = fcc_li(2.4)
    return [base, base.make_supercell([2, 1, 1])]


def low_coordination_cells():
    """0-2 angles per atom: an isolated pair, a linear trimer, a 10-atom zigzag chain (periodic along a) with exactly 2 short
    bonds per atom; and, at the other extreme, one 100-atom cell of the C3 sweep."""
    import bench

    pair = _from_cart(np.eye(3) * 12.0, ["Li", "O"], [[5.0, 6.0, 6.0], [7.0, 6.0, 6.0]])
    trimer = _from_cart(np.eye(3) * 14.0, ["O", "Co", "O"], [[5.0, 7.0, 7.0], [7.0, 7.0, 7.0], [9.0, 7.0, 7.0]])
    x = 1.9 * np.arange(10) + 0.5
    y = 6.0 + 0.6 * (-1.0) ** np.arange(10)
    chain = _from_cart(np.diag([19.0, 12.0, 12.0]), ["Li", "O"] * 5, np.stack([x, y, np.full(10, 6.0)], 1))
    big = next(bench.sweep_structure(i) for i in range(1000) if bench.sweep_atom_count(i) == 100)
    return [pair, trimer, chain, big]


def md_cells():
    """Li9Co7O16 2 x 2 x 2 (256 atoms) and 4 x 2 x 2 (512 atoms), thermalised with sigma = 0.01 A."""
    import bench

    out = []
    for i, scale in enumerate(((2, 2, 2), (4, 2, 2))):
        s = bench.li9co7o16_supercell(scale)
        d = np.random.default_rng([5, i]).normal(0, 0.01, (len(s), 3))
        out.append(_structure(s.lattice.matrix, s.atomic_numbers, s.frac_coords + d @ np.linalg.inv(s.lattice.matrix)))
    return out


def large_batch():
    """210 perturbed LiMnO2 5 x 1 x 1 cells (bench.py's headline generator): 8,400 atoms, past the 8,191 the builder emits the
    blocked tiles and the per-atom index for -- the index of the per-atom windows comes from the k_win_* kernels."""
    import bench

    return bench.workload_structures(210, 1000)


# ---- malformed uploaded angle sets (only an upload can carry them) ---------------------------------------------------------------
# bond_graph rows: [centre, bond 1 (bond-graph node), bond 1 (directed), bond 2 (bond-graph node), bond 2 (directed)]

def malformed_bases():
    return [shell_cluster(12, 1), shell_cluster(6, 1)]


def _groups(bg):
    """(centre, directed first bond) -> row indices, in row order."""
    out: dict = {}
    for r, row in enumerate(bg):
        out.setdefault((int(row[0]), int(row[2])), []).append(r)
    return out


def _with_bond_graph(g, bg):
    g = copy.copy(g)
    g.bond_graph = np.ascontiguousarray(bg, dtype=np.int32)
    return g


def malformed_graph(g, kind: str, seed: int = 0):
    """The host converter's graph ``g`` with its angle rows edited:
    a: rows shuffled; b: one row's second bond replaced by the second bond of another row of its group -- one (b1, b2) pair
    twice, one missing, the row count unchanged; c: one row of a group removed; d: one row's second bond replaced by a short
    bond that does not start at the centre."""
    bg = np.array(g.bond_graph, dtype=np.int32).reshape(-1, 5)
    rng = np.random.default_rng([31, seed, ord(kind)])
    groups = _groups(bg)
    big = max(groups.values(), key=len)                       # the centre's largest group (>= 2 rows)
    if kind == "a":
        bg = bg[rng.permutation(len(bg))]
    elif kind == "b":
        r, src = big[1], big[len(big) // 2 + 1]
        bg[r, 3:5] = bg[src, 3:5]
    elif kind == "c":
        bg = np.delete(bg, big[len(big) // 2], axis=0)
    elif kind == "d":
        r = big[0]
        other = next(i for i in range(len(bg)) if bg[i, 0] != bg[r, 0])
        bg[r, 3:5] = bg[other, 1:3]
    else:
        raise ValueError(kind)
    return _with_bond_graph(g, bg)


MALFORMED_KINDS = ("a", "b", "c", "d")


def malformed_graphs():
    conv = converter()
    return {kind: [malformed_graph(conv(s), kind, i) for i, s in enumerate(malformed_bases())] for kind in MALFORMED_KINDS}


# ---- the fixture groups of the GPU matrix ------------------------------------------------------------------------------------

def structure_groups() -> dict:
    """name -> list of structures (the groups that run through both the device builder and the host converter)."""
    canon = [shell_cluster(k) for k in SHELL_KS if k <= 32]
    return {
        "shell_le32": canon,
        "shell_33": [shell_cluster(33)],
        "shell_40": [shell_cluster(40)],
        "shell_mixed": canon + [shell_cluster(33)],
        "tie": tie_cells(),
        "dense": dense_cells(),
        "low": low_coordination_cells(),
        "md": md_cells(),
    }


def short_bond_counts(g) -> np.ndarray:
    """Short (< bond cutoff or == it) bonds per atom as the angle rows see them: the number of distinct first bonds of each
    centre plus one (an atom with n short bonds has groups of n - 1 rows)."""
    bg = np.asarray(g.bond_graph).reshape(-1, 5)
    n = np.zeros(len(g.atomic_number), np.int64)
    for (c, _), rows in _groups(bg).items():
        n[c] = max(n[c], len(rows) + 1)
    return n


def directed_lengths(g) -> np.ndarray:
    """float64 length of every directed edge from the graph's own (float32) coordinates."""
    frac = np.asarray(g.atom_frac_coord, np.float64)
    lat = np.asarray(g.lattice, np.float64)
    ag = np.asarray(g.atom_graph).reshape(-1, 2)
    v = (frac[ag[:, 1]] + np.asarray(g.neighbor_image, np.float64) - frac[ag[:, 0]]) @ lat
    return np.linalg.norm(v, axis=1)
