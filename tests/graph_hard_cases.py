"""Hard cell shapes for the graph builders (seeded, deterministic): ``cases()`` -> [(name, Structure, [(r_atom, r_bond), ...])].

Shared by tests/test_neighbor_oracle_cpu.py (host builder, both searches) and tests/test_gpu_graph_oracle.py (device
builder, every route); the expected graphs come from tests/neighbor_ref.py and are computed once per session.
Apart from the tie cases every case keeps its distances away from its cutoffs (``margins`` / ``required_margin``): the builders' float64
arithmetic and the oracle's long double then agree on every comparison, whatever the last bits.
"""

from __future__ import annotations

import functools

import numpy as np

import neighbor_ref

SMALL = ((6.0, 3.0), (5.0, 3.0), (4.0, 4.0), (11.0, 2.0), (1.0, 1.0))
MEDIUM = ((6.0, 3.0), (5.0, 3.0), (1.0, 1.0))
DENSE = ((2.0, 0.6),)

# unimodular re-descriptions of one crystal (determinant +1): lattice M @ L, coordinates frac @ inv(M)
UNIMODULAR = {"id": ((1, 0, 0), (0, 1, 0), (0, 0, 1)), "m130": ((1, 3, 0), (0, 1, 0), (2, 0, 1)),
              "m121": ((1, 2, 1), (0, 1, 2), (0, 0, 1)), "mneg": ((1, 0, -4), (3, 1, 0), (0, 0, 1))}
TIES = ("tie_sc3", "tie_fcc4", "tie_tet")
LANE_SIZES = (1, 2, 63, 64, 65, 128, 129)


def _S(lattice, species, frac):
    from chgnet_amd import Structure
    from chgnet_amd.graph.structure import Lattice

    return Structure(lattice if isinstance(lattice, Lattice) else Lattice(lattice), species, frac)


def redescribe(s, M):
    """The same crystal in the cell M @ L (M integer, det +1)."""
    M = np.asarray(M, np.float64)
    assert round(float(np.linalg.det(M))) == 1
    return _S(M @ s.lattice.matrix, s.atomic_numbers, s.frac_coords @ np.round(np.linalg.inv(M)))


def _jittered(n: int, jitter: float, rng) -> np.ndarray:
    m = int(np.ceil(n ** (1 / 3)))
    grid = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    pick = rng.choice(len(grid), size=n, replace=False) if n < len(grid) else np.arange(n)
    return (grid[pick] + 0.5 + rng.uniform(-jitter, jitter, (n, 3))) / m


def tri8():
    """8-atom triclinic cell (0.046 atoms / A^3)."""
    rng = np.random.default_rng(11)
    return _S([[5.1, 0.3, -0.2], [0.8, 5.6, 0.4], [-0.5, 1.1, 6.2]], [3, 3, 25, 25, 8, 8, 8, 8], _jittered(8, 0.15, rng))


def lmo40():
    import bench

    return bench.limno2((5, 1, 1)).perturb(0.01, np.random.default_rng(3))


def _sheared(a, b, c, al, be, ga, seed):
    from chgnet_amd.graph.structure import Lattice

    return _S(Lattice.from_parameters(a, b, c, al, be, ga), [3, 3, 25, 25, 8, 8, 8, 8], _jittered(8, 0.08, np.random.default_rng(seed)))


def physics_cases():
    """case name -> the case whose float64 oracle result is its truth (the identity description of the same crystal; a
    sheared cell is its own): the cases that are predicted, not only built (tests/test_gpu_graph_oracle.py)."""
    out = {}
    for base in ("tri8", "lmo40"):
        for m in UNIMODULAR:
            out[f"{base}_{m}"] = f"{base}_id"
    for name in ("shear_30", "shear_150", "shear_mixed"):
        out[name] = name
    return out


@functools.lru_cache(maxsize=None)
def _sort_limit():
    """Rattled 96-atom LiMnO2 cell and the two cutoffs at which its busiest centre has exactly 1,024 / 1,025 rows (no centre
    has more): from the oracle's own per-centre sorted distances."""
    import bench

    s = bench.limno2((3, 2, 2)).perturb(0.03, np.random.default_rng(1))
    rows, _ = neighbor_ref.brute_neighbors(s.frac_coords, s.lattice.matrix, 13.6)
    per = [np.sort(rows.distance[rows.center == i]) for i in range(len(s))]
    cut = {}
    for K in (1024, 1025):
        assert min(len(p) for p in per) > K
        c = int(np.argmin([p[K] for p in per]))                      # smallest (K + 1)-th distance over all centres
        hi, lo = per[c][K], per[c][K - 1]
        assert float(hi - lo) >= 1e-6, (K, float(hi - lo))
        cut[K] = float((lo + hi) / 2)
    return s, cut


@functools.lru_cache(maxsize=None)
def cases():
    import bench

    out = []
    # ---- unimodular family: same crystal, image indices up to about +-30
    for base, s, cuts in (("tri8", tri8(), SMALL), ("lmo40", lmo40(), MEDIUM)):
        for m, M in UNIMODULAR.items():
            out.append((f"{base}_{m}", redescribe(s, M), cuts))
    # ---- sheared (35 / 120 / 75 degrees cannot be the three angles of a cell -- 120 > 35 + 75 -- so the mixed cell is 35 / 100 / 75)
    out.append(("shear_30", _sheared(7.0, 7.2, 5.8, 90, 90, 30, 21), SMALL))
    out.append(("shear_150", _sheared(7.0, 7.2, 5.8, 90, 90, 150, 22), SMALL))
    out.append(("shear_mixed", _sheared(7.5, 7.0, 8.0, 35, 100, 75, 23), SMALL))
    # ---- thin cells
    rng = np.random.default_rng(31)
    out.append(("thin_cube16", _S(np.eye(3) * 1.6, ["Fe"], [[0.1, 0.2, 0.3]]), ((6.0, 3.0), (5.0, 3.0), (4.0, 4.0), (1.0, 1.0))))
    fz = (np.arange(8) + 0.5 + rng.uniform(-0.2, 0.2, 8)) / 8
    out.append(("thin_needle", _S(np.diag([1.7, 1.8, 30.0]), rng.choice([3, 8], 8), np.stack([rng.random(8), rng.random(8), fz], 1)), SMALL))
    out.append(("thin_slab", _S(np.diag([25.0, 25.0, 1.9]), rng.choice([3, 8, 25], 40), rng.random((40, 3))), MEDIUM))
    out.append(("thin_rod_a", _S(np.diag([25.0, 1.9, 2.03]), rng.choice([3, 8], 8), np.stack([fz, rng.random(8), rng.random(8)], 1)), SMALL))
    # ---- left-handed description of tri8 (two lattice rows swapped)
    t = tri8()
    out.append(("left_handed", _S(t.lattice.matrix[[1, 0, 2]], t.atomic_numbers, t.frac_coords[:, [1, 0, 2]]), SMALL))
    # ---- coordinates on and across faces, shifted, either side of the sort-key guard, one atom far away
    faces = [[0, 0, 0], [0.5, 0, 0], [1.0 - 1e-17, 0.5, 0.5], [-1e-17, 0.25, 0.75], [0.999999999999, 0.1, 0.1], [0.5, 0.5, 1.0],
             [2.5, -1.5, 0.5], [0.25, 0.25, 0.25]]
    out.append(("coord_faces", _S([[11.3, 0.2, 0.0], [0.1, 12.1, 0.3], [0.0, -0.2, 12.7]], ["O"] * 8, faces), SMALL))
    alt = np.where(np.arange(8) % 2 == 0, 1.0, -1.0)[:, None]
    out.append(("coord_shift5", _S(t.lattice, t.atomic_numbers, t.frac_coords + 5.0 * alt), SMALL))
    for tag, sh in (("p3999", 3999.5), ("m3999", -3999.5), ("p4000", 4000.5), ("m4000", -4000.5)):
        out.append((f"coord_{tag}", _S(t.lattice, t.atomic_numbers, t.frac_coords + sh), MEDIUM))
    # both signs in one cell, every floor inside the guard: images near +-8,000, the edge of the packed sort key
    out.append(("coord_mixed3999", _S(t.lattice, t.atomic_numbers, t.frac_coords + np.where(alt > 0, 3998.5, -3998.5)), MEDIUM))
    far = t.frac_coords.copy()
    far[3] += np.array([1e6, 0.0, -1e6])
    out.append(("coord_far1e6", _S(t.lattice, t.atomic_numbers, far), MEDIUM))
    # ---- ties by construction (expected rows from integer arithmetic: integer_tie_rows)
    out.append(("tie_sc3", _S(np.eye(3) * 3.0, ["Fe"], [[0, 0, 0]]), ((6.0, 3.0),)))
    out.append(("tie_fcc4", _S(np.eye(3) * 4.0, ["Cu"] * 4, [[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]]), ((4.0, 3.0),)))
    out.append(("tie_tet", _S(np.diag([3.0, 3.0, 2.5]), ["Fe"], [[0, 0, 0]]), ((6.0, 3.0),)))   # bonds AT r_bond own angles with the 2.5 A ones
    # ---- lane strides of the all-pairs loop (64 neighbours per wave pass)
    for n in LANE_SIZES:
        rng = np.random.default_rng(100 + n)
        a = (n / 0.09) ** (1 / 3)
        lat = np.eye(3) * a + rng.normal(0, 0.04 * a, (3, 3))
        out.append((f"lanes_{n}", _S(lat, rng.choice([3, 25, 8], n), _jittered(n, 0.2, rng)), ((6.0, 3.0), (5.0, 3.0))))
    # ---- more than 64 atoms per bin (graph only: 700 atoms in 91 A^3 is no crystal)
    rng = np.random.default_rng(41)
    out.append(("dense_bins", _S(np.eye(3) * 4.5, rng.choice([3, 8], 700), rng.random((700, 3))), DENSE))
    out.append(("dense_companion", tri8(), DENSE))
    # ---- the 1,024-row limit of the in-LDS sort
    s, cut = _sort_limit()
    out.append(("sort_1024", s, ((cut[1024], 3.0),)))
    out.append(("sort_1025", s, ((cut[1025], 3.0),)))
    # ---- isolated atoms only
    out.append(("isolated", _S(np.eye(3) * 20.0, ["H", "O"], [[0, 0, 0], [0.5, 0.5, 0.5]]), SMALL + DENSE))
    # ---- one large sheared cell: the automatic search picks the cell list by itself
    big = bench.limno2((8, 8, 4)).perturb(0.01, np.random.default_rng(5))
    lat = big.lattice.matrix.copy()
    lat[2] += [np.linalg.norm(lat[2]), 0.0, 0.0]                     # c leans 45 degrees towards a
    out.append(("large_sheared", _S(lat, big.atomic_numbers, big.frac_coords), ((6.0, 3.0),)))
    assert len({n for n, _, _ in out}) == len(out)
    return tuple(out)


def case(name: str):
    for n, s, cuts in cases():
        if n == name:
            return s, cuts
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_rows(name: str, r_atom: float):
    """(Rows, margin) of a case, once per session."""
    s, _ = case(name)
    return neighbor_ref.brute_neighbors(s.frac_coords, s.lattice.matrix, r_atom)


@functools.lru_cache(maxsize=None)
def oracle_graph(name: str, r_atom: float, r_bond: float) -> dict:
    """Everything the builders must reproduce for (case, cutoffs): rows + bond bookkeeping + line graph."""
    s, _ = case(name)
    rows, _ = oracle_rows(name, r_atom)
    lg = neighbor_ref.line_graph_ref(len(s), rows, r_bond)
    n_iso = len(s) - len(np.unique(rows.center))
    return {"rows": rows, "atom_graph": np.stack([rows.center, rows.neighbor], 1), "image": rows.image, "n_isolated": n_iso, **lg}


def required_margin(name: str) -> float:
    s, _ = case(name)
    return max(1e-9, 100.0 * neighbor_ref.cart_bound(s.frac_coords, s.lattice.matrix))


def margins(name: str, r_atom: float, r_bond: float) -> tuple[float, float]:
    rows, m_atom = oracle_rows(name, r_atom)
    return m_atom, neighbor_ref.bond_margin(rows, r_bond)


def integer_tie_rows(name: str) -> np.ndarray:
    """Expected [E,5] rows of a tie case from exact integer arithmetic, strict ``<``: positions and periods in integer
    units, squared lengths weighted by integer metric entries."""
    points, period, weight, r2 = {
        "tie_sc3": ([(0, 0, 0)], 1, (9, 9, 9), 36),                                                    # a^2 n.n < r^2
        "tie_fcc4": ([(0, 0, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1)], 2, (4, 4, 4), 16),                  # units of a / 2
        "tie_tet": ([(0, 0, 0)], 1, (36, 36, 25), 144),                                                # 4 x (9, 9, 6.25) < 4 x 36
    }[name]
    rows = []
    span = range(-8, 9)
    for i, pi in enumerate(points):
        for j, pj in enumerate(points):
            for ia in span:
                for ib in span:
                    for ic in span:
                        d = [pj[k] - pi[k] + period * n for k, n in enumerate((ia, ib, ic))]
                        d2 = sum(w * x * x for w, x in zip(weight, d))
                        if 0 < d2 < r2:
                            rows.append((i, j, ia, ib, ic))
    return np.asarray(sorted(rows), np.int64).reshape(-1, 5)
