"""Brute-force periodic neighbour oracle (plain numpy, none of the project's code).

``brute_neighbors`` finds every pair closer than a cutoff by visiting every image in a cube bounded by the smallest
singular value of the lattice -- nothing of the plane-spacing argument, the image windows or the bins the builders
rely on -- with distances in ``np.longdouble``.  ``line_graph_ref`` turns such rows into the expected bond bookkeeping
and line graph through the reference's compiled C builder (``oracle/_ref``), or through the restatement of its rules
below where that library is absent.  TEST INFRASTRUCTURE ONLY.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

LD = np.longdouble
LONG_DOUBLE_ATOMS = 300          # above this many atoms the pair loop runs in float64 chunks (the margin condition of the
                                 # case family makes the answer independent of the last bits)


class Rows(NamedTuple):
    center: np.ndarray           # [E] int64
    neighbor: np.ndarray         # [E] int64
    image: np.ndarray            # [E,3] int64, relative to the coordinates AS GIVEN (unwrapped)
    distance: np.ndarray         # [E] long double (float64 for large structures)

    @property
    def table(self) -> np.ndarray:
        """[E,5] (centre, neighbour, ia, ib, ic)."""
        return np.concatenate([self.center[:, None], self.neighbor[:, None], self.image], 1)


def _wrap(frac: np.ndarray):
    """Fractional coordinates -> (w in [0, 1) as long double, integer floors) with frac = w + floor."""
    frac = np.asarray(frac, np.float64).reshape(-1, 3)
    fl = np.floor(frac)
    w = frac.astype(LD) - fl.astype(LD)
    up = w >= 1                                   # -1e-30 - floor(-1e-30) rounds to 1 even in long double
    w = np.where(up, w - 1, w)
    fl = np.where(up, fl + 1, fl)
    return w, fl.astype(np.int64)


def _images(lattice: np.ndarray, reach: float) -> np.ndarray:
    """Every integer triple n with |n @ L| <= reach, from the cube |n_k| <= ceil(reach / sigma_min) + 1."""
    L = np.asarray(lattice, np.float64).reshape(3, 3)
    sigma_min = float(np.linalg.svd(L, compute_uv=False).min())
    if not sigma_min > 0:
        raise ValueError("singular lattice")
    m = int(np.ceil(reach / sigma_min)) + 1
    ax = np.arange(-m, m + 1, dtype=np.int64)
    grid_bc = np.stack(np.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)
    keep = []
    slack = reach * (1 + 1e-9) + 1e-9
    for ia in ax:                                 # one slab of the cube at a time: (2 m + 1)^2 rows
        n = np.concatenate([np.full((len(grid_bc), 1), ia, np.int64), grid_bc], 1)
        length = np.linalg.norm(n.astype(np.float64) @ L, axis=1)
        keep.append(n[length <= slack])           # triangle inequality: beyond r + diameter no pair can be inside r
    return np.concatenate(keep, 0)


def brute_neighbors(frac, lattice, r: float, tol: float = 1e-8):
    """-> (Rows sorted by (centre, neighbour, ia, ib, ic), margin = smallest |d - r| over everything evaluated).
    A pair is a row when ``tol < d < r``."""
    L64 = np.asarray(lattice, np.float64).reshape(3, 3)
    w, fl = _wrap(frac)
    n = len(w)
    big = n > LONG_DOUBLE_ATOMS
    ft = np.float64 if big else LD
    L = L64.astype(ft)
    wc = w.astype(ft) @ L                                              # wrapped Cartesian positions
    wc64 = wc.astype(np.float64)
    diameter = 0.0
    for s in range(0, n, 512):
        d = wc64[s:s + 512, None, :] - wc64[None, :, :]
        diameter = max(diameter, float(np.sqrt((d * d).sum(-1).max())))
    diameter = diameter * (1 + 1e-9) + 1e-9
    imgs = _images(L64, float(r) + diameter)
    shift = imgs.astype(ft) @ L                                        # [I,3]
    r_ft, tol_ft = ft(r), ft(tol)
    margin = float("inf")
    out_c, out_n, out_img, out_d = [], [], [], []
    centre_chunk = n if not big else 64
    img_chunk = max(1, int(2e6 // max(1, min(n, centre_chunk) * n)))
    for c0 in range(0, n, centre_chunk):
        c1 = min(n, c0 + centre_chunk)
        base = wc[None, :, :] - wc[c0:c1, None, :]                     # [C,n,3]: w_j - w_i
        for k0 in range(0, len(imgs), img_chunk):
            sh = shift[k0:k0 + img_chunk]
            v = base[None, :, :, :] + sh[:, None, None, :]             # [K,C,n,3]
            d = np.sqrt((v * v).sum(-1))
            margin = min(margin, float(np.abs(d - r_ft).min()))
            hit = (d < r_ft) & (d > tol_ft)
            if hit.any():
                kk, ii, jj = np.nonzero(hit)
                out_c.append(ii + c0)
                out_n.append(jj)
                out_img.append(imgs[k0 + kk] - fl[jj] + fl[ii + c0])   # back to the unwrapped description
                out_d.append(d[kk, ii, jj])
    if not out_c:
        z = np.zeros(0, np.int64)
        return Rows(z, z.copy(), np.zeros((0, 3), np.int64), np.zeros(0, ft)), margin
    c, nb, img, dist = np.concatenate(out_c), np.concatenate(out_n), np.concatenate(out_img, 0), np.concatenate(out_d)
    order = np.lexsort((img[:, 2], img[:, 1], img[:, 0], nb, c))
    return Rows(c[order].astype(np.int64), nb[order].astype(np.int64), img[order].astype(np.int64), dist[order]), margin


def bond_margin(rows: Rows, r_bond: float) -> float:
    """Smallest |d - r_bond| over the rows (inf without rows)."""
    return float(np.abs(rows.distance - rows.distance.dtype.type(r_bond)).min()) if len(rows.center) else float("inf")


def cart_bound(frac, lattice) -> float:
    """How far float64 arithmetic on the unwrapped Cartesian coordinates can be from long double:
    64 * 2^-53 * max(1, max|cart|)."""
    cart = np.asarray(frac, np.float64).reshape(-1, 3) @ np.asarray(lattice, np.float64).reshape(3, 3)
    return 64.0 * 2.0 ** -53 * max(1.0, float(np.abs(cart).max()))


# ---------------------------------------------------------------------------------------------------
# bond bookkeeping and line graph from a row list
# ---------------------------------------------------------------------------------------------------
def line_graph_rules(n_atoms: int, center, neighbor, image, distance, r_bond: float) -> dict:
    """The reference's rules restated (tests/test_graph_builder.py::test_cutoff_boundary_rules_known_answer spells them out):

    * rows are taken in the order given; a directed edge (i -> j, image) closes the undirected bond that an EARLIER edge
      (j -> i, -image) opened, otherwise it opens a new one; bonds are numbered in the order they are opened and
      ``undirected2directed`` is the edge that opened the bond; every bond must end up with exactly two edges;
    * bond k owns angles only if its length is not ABOVE the cutoff (``>`` skips); at each of its two ends (the end its
      opening edge leaves from first) the other edges leaving that atom -- grouped by neighbour in order of first
      appearance, row order inside a group -- form an angle if they are strictly SHORTER than the cutoff (``<``);
      an angle is (centre atom, bond, its edge leaving the centre, the other bond, the other edge)."""
    center, neighbor = np.asarray(center, np.int64), np.asarray(neighbor, np.int64)
    image = np.asarray(image, np.int64).reshape(-1, 3)
    distance = np.asarray(distance, np.float64)
    E = len(center)
    opened: dict = {}
    d2u = np.zeros(E, np.int32)
    u2d, closing = [], []
    for e in range(E):
        i, j, im = int(center[e]), int(neighbor[e]), tuple(int(x) for x in image[e])
        k = opened.get((j, i, (-im[0], -im[1], -im[2])))
        if k is not None:
            if closing[k] >= 0:
                raise ValueError("a third directed edge on one bond")
            closing[k] = e
        else:
            k = len(u2d)
            u2d.append(e)
            closing.append(-1)
            opened[(i, j, im)] = k
        d2u[e] = k
    if any(c < 0 for c in closing):
        raise ValueError("directed edges are not complete")
    leaving = [[] for _ in range(n_atoms)]
    for e in range(E):
        leaving[center[e]].append(e)
    for i in range(n_atoms):
        rank: dict = {}
        for e in leaving[i]:
            rank.setdefault(int(neighbor[e]), len(rank))
        leaving[i].sort(key=lambda e: rank[int(neighbor[e])])          # stable: row order inside a neighbour group
    bg = []
    for k, first in enumerate(u2d):
        if distance[first] > r_bond:
            continue
        for de in (first, closing[k]):
            ctr = int(center[de])
            for other in leaving[ctr]:
                if other != de and distance[other] < r_bond:
                    bg.append((ctr, k, de, int(d2u[other]), other))
    return {"directed2undirected": d2u, "undirected2directed": np.asarray(u2d, np.int32).reshape(-1),
            "bond_graph": np.asarray(bg, np.int32).reshape(-1, 5)}


def line_graph_ref(n_atoms: int, rows: Rows, r_bond: float) -> dict:
    """Expected ``directed2undirected``, ``undirected2directed``, ``bond_graph`` of a row list: the reference's compiled
    C builder where it is available, the restated rules otherwise.  Never the project's own builder."""
    from oracle import ref_graph

    dist = np.asarray(rows.distance, np.float64)
    if len(rows.center) and ref_graph.available():
        ref = ref_graph.reference_graph(n_atoms, rows.center, rows.neighbor, rows.image, dist, float(r_bond))
        return {"directed2undirected": ref["directed2undirected"], "undirected2directed": ref["undirected2directed"],
                "bond_graph": ref["bond_graph"].reshape(-1, 5)}
    return line_graph_rules(n_atoms, rows.center, rows.neighbor, rows.image, dist, r_bond)
