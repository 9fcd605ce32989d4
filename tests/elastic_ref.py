"""Reference strain-block Hessian products for the elastic tests: central differences, on a FIXED graph, of the float64 oracle's first
derivatives along a direction (u, W).  The energy is E(x, eps) with the lattice L (I + eps) and the atoms at fixed fractional
coordinates (every bond vector v0 (I + eps)).  At the displaced point the graph gets the lattice L (I + h W) and the fractional
coordinates of x + h u; the oracle's forces F and stress s there map back to this parameterisation as

    dE/dx   = -F (I + eps)^T                 (positions x (I + eps))
    dE/deps = (I + eps)^-T G',  G' = s det(L (I + eps)) / 160.21766208    (G' the oracle's dE/dstrain at the strained cell)

The step and scaling are those of hessian_ref.fd_hvp."""

from __future__ import annotations

import types

import numpy as np

from hessian_ref import GRAPH_KEYS

EV_A3_TO_GPA = 160.21766208


def strained(g, dcart, w):
    """``g`` with the lattice L (I + w) and the fractional coordinates of x + dcart, same graph, float64."""
    lat = np.asarray(g.lattice, np.float64).reshape(3, 3)
    frac = np.asarray(g.atom_frac_coord, np.float64).reshape(-1, 3) + np.asarray(dcart, np.float64) @ np.linalg.inv(lat)
    return types.SimpleNamespace(**{k: getattr(g, k) for k in GRAPH_KEYS}, atom_frac_coord=frac,
                                 lattice=lat @ (np.eye(3) + np.asarray(w, np.float64)))


def first_derivatives(oracle, jobs, strains, batch_size: int = 64):
    """(dE/dx [n,3], dE/deps [3,3]) of every strained graph in ``jobs`` (eps = its strain) in this parameterisation."""
    out = []
    for p, w in zip(oracle.predict_graph(jobs, "efs", batch_size=batch_size), strains):
        i_eps = np.eye(3) + np.asarray(w, np.float64)
        gx = -np.asarray(p["f"], np.float64) @ i_eps.T
        gs = np.asarray(p["s"], np.float64).reshape(3, 3) * np.linalg.det(np.asarray(jobs[len(out)].lattice)) / EV_A3_TO_GPA
        out.append((gx, np.linalg.inv(i_eps).T @ gs))
    return out


def fd_hvp_strain(oracle, graphs, directions, strains, delta: float = 1e-5, batch_size: int = 64):
    """[(hx [n,3], hs [3,3])] per graph: central differences along (u, W), scaled so that the largest of |u| and |W| is 1."""
    jobs, ws, scale = [], [], []
    for g, u, w in zip(graphs, directions, strains):
        u, w = np.asarray(u, np.float64), np.asarray(w, np.float64).reshape(3, 3)
        s = max(float(np.abs(u).max()) if u.size else 0.0, float(np.abs(w).max())) or 1.0
        scale.append(s)
        for h in (delta / s, -delta / s):
            jobs.append(strained(g, h * u, h * w))
            ws.append(h * w)
    d = first_derivatives(oracle, jobs, ws, batch_size)
    return [((d[2 * i][0] - d[2 * i + 1][0]) / (2 * delta) * scale[i], (d[2 * i][1] - d[2 * i + 1][1]) / (2 * delta) * scale[i])
            for i in range(len(graphs))]


def voigt_strains() -> np.ndarray:
    w = np.zeros((6, 3, 3))
    for i, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))):
        w[i, a, b] += 0.5
        w[i, b, a] += 0.5
    return w


def fd_full_hessian(oracle, g, delta: float = 1e-5):
    """The full (3n + 6)^2 Hessian in the basis (unit displacements, Voigt unit strains) -> (Phi [3n,3n], Lambda [3n,6] from the
    strain columns' hx, the eps-eps block [6,6] W_i : hs(0, W_j))."""
    n = len(g.atomic_number)
    eye = np.eye(3 * n).reshape(3 * n, n, 3)
    wv = voigt_strains()
    dirs = list(eye) + [np.zeros((n, 3))] * 6
    ws = [np.zeros((3, 3))] * (3 * n) + list(wv)
    cols = fd_hvp_strain(oracle, [g] * len(dirs), dirs, ws, delta)
    phi = np.stack([c[0].reshape(-1) for c in cols[:3 * n]], axis=1)
    lam = np.stack([c[0].reshape(-1) for c in cols[3 * n:]], axis=1)
    ss = np.array([[float((wv[i] * cols[3 * n + j][1]).sum()) for j in range(6)] for i in range(6)])
    return phi, lam, ss


def total_energy(oracle, jobs) -> np.ndarray:
    """Total energy (eV) of every job: the per-atom energy times n for an intensive oracle."""
    e = np.array([float(p["e"]) for p in oracle.predict_graph(jobs, "e", batch_size=64)])
    n = np.array([len(j.atomic_number) for j in jobs])
    return e * n if oracle.is_intensive else e
