"""Reference Hessians for the HVP tests: central differences of the float64 oracle's forces on a FIXED graph (the displaced
positions go into ``atom_frac_coord``; the neighbour list, images and angles stay those of the undisplaced structure -- the
reference's autograd semantics).  Also the rock-salt LiF cells whose F-Li-F triplets are exactly collinear."""

from __future__ import annotations

import types

import numpy as np

GRAPH_KEYS = ("atomic_number", "atom_graph", "neighbor_image", "directed2undirected", "undirected2directed", "bond_graph")


def lif_structure(conventional: bool = True, rattle: float = 0.0, seed: int = 0, a: float = 4.03):
    """Rock-salt LiF: the 8-atom conventional cell or the 2-atom primitive one (every atom bonds to its own images).  Li-F
    bonds of a/2 = 2.015 A lie inside the 3 A bond-graph cutoff, so F-Li-F / Li-F-Li triplets at 180 degrees exist.  ``rattle``:
    every atom displaced by that length (A) in a seeded random direction."""
    from chgnet_amd.graph.structure import Structure

    if conventional:
        lat = np.eye(3) * a
        frac = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.5, .5, .5], [.5, 0, 0], [0, .5, 0], [0, 0, .5]], float)
        species = ["Li"] * 4 + ["F"] * 4
    else:
        lat = 0.5 * a * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], float)
        frac = np.array([[0, 0, 0], [.5, .5, .5]], float)
        species = ["Li", "F"]
    if rattle:
        d = np.random.default_rng(seed).normal(size=frac.shape)
        d *= rattle / np.linalg.norm(d, axis=1, keepdims=True)
        frac = (frac @ lat + d) @ np.linalg.inv(lat)
    return Structure(lat, species, frac)


def displaced(g, dcart):
    """``g`` with every atom moved by dcart [n,3] (A), same graph; float64 coordinates (a CrystalGraph rounds to float32)."""
    lat = np.asarray(g.lattice, np.float64).reshape(3, 3)
    frac = np.asarray(g.atom_frac_coord, np.float64).reshape(-1, 3) + np.asarray(dcart, np.float64) @ np.linalg.inv(lat)
    return types.SimpleNamespace(**{k: getattr(g, k) for k in GRAPH_KEYS}, atom_frac_coord=frac, lattice=lat)


def fd_hvp(oracle, graphs, directions, delta: float = 1e-5, batch_size: int = 64) -> list[np.ndarray]:
    """H u ~ -(F(x + d u) - F(x - d u)) / (2 d) per graph, u scaled to a largest atom displacement of 1 (d in A).  ``batch_size``: the
    oracle's chunk (an architecture with ``mlp_out`` biases switches them per chunk: model.py:459)."""
    jobs, scale = [], []
    for g, u in zip(graphs, directions):
        u = np.asarray(u, np.float64)
        s = float(np.abs(u).max()) or 1.0
        scale.append(s)
        jobs += [displaced(g, delta * u / s), displaced(g, -delta * u / s)]
    f = [np.asarray(p["f"], np.float64) for p in oracle.predict_graph(jobs, "ef", batch_size=batch_size)]
    return [-(f[2 * i] - f[2 * i + 1]) / (2 * delta) * scale[i] for i in range(len(graphs))]


def fd_hessian(oracle, g, delta: float = 1e-5) -> np.ndarray:
    """[3n,3n] float64, column 3j+beta = H e_(3j+beta)."""
    n = len(g.atomic_number)
    eye = np.eye(3 * n).reshape(3 * n, n, 3)
    cols = fd_hvp(oracle, [g] * (3 * n), list(eye), delta)
    return np.stack([c.reshape(-1) for c in cols], axis=1)


def mass_weighted_eigenvalues(z, h) -> np.ndarray:
    """Eigenvalues of M^-1/2 H M^-1/2 (symmetrised), ascending: what phonons.gamma_frequencies takes the roots of."""
    from chgnet_amd.dynamics import ATOMIC_MASSES

    w = np.repeat(1.0 / np.sqrt(ATOMIC_MASSES[np.asarray(z)]), 3)
    h = np.asarray(h, np.float64)
    return np.linalg.eigvalsh(0.5 * (h + h.T) * w[:, None] * w[None, :])
