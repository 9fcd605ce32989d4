"""Float64 NumPy restatement of the MD observables (include/chgnet_hip.h "MD observables"; csrc/kernels_md_obs.h): plain loops over
samples, lags, atoms and pairs, written from the definitions and sharing nothing with the kernels' ring, reductions or shift search.

``correlations`` returns, beside the sums, the sums of the ABSOLUTE values of their terms (every product of two components): the
tests bound the float64 reordering error of the device by ``1e-12 * sum|terms|``.  The centres of mass are summed in long double, so
the restatement's own rounding stays far below that bound.

``pair_histogram`` enumerates a generous range of lattice shifts around the raw, unwrapped difference of every ordered pair
(``wrap=True``: around the difference wrapped with ``np.round``, for inputs shifted by so many lattice vectors that the range would
explode).  It ASSERTS that no pair distance lies within ``EDGE_GUARD`` of a bin edge or of ``rmax``: an input on an edge fails here,
on the CPU, instead of depending on the last bit of a square root on the device.
"""

from __future__ import annotations

import numpy as np

EDGE_GUARD = 1e-9   # A


def centre_of_mass(r: np.ndarray, m: np.ndarray) -> np.ndarray:
    acc = np.zeros(3, np.longdouble)
    tot = np.longdouble(0)
    for i in range(len(m)):
        acc += np.longdouble(m[i]) * r[i].astype(np.longdouble)
        tot += np.longdouble(m[i])
    return (acc / tot).astype(np.float64)


def correlations(positions, momenta, status, atom_off, species, masses, n_species: int, n_lags: int, subtract_com: bool) -> dict:
    """positions / momenta [T, N, 3], status [T, B] (0 = running) -> msd, vacf [B, L, S], cnt [B, L] and msd_abs, vacf_abs."""
    T, B, L, S = len(positions), len(atom_off) - 1, n_lags, n_species
    out = {"msd": np.zeros((B, L, S)), "vacf": np.zeros((B, L, S)), "cnt": np.zeros((B, L), np.int64),
           "msd_abs": np.zeros((B, L, S)), "vacf_abs": np.zeros((B, L, S))}
    for o in range(B):
        sl = slice(atom_off[o], atom_off[o + 1])
        m, sp = masses[sl], species[sl]
        vel = [momenta[k][sl] / m[:, None] for k in range(T)]
        com = [centre_of_mass(positions[k][sl], m) if subtract_com else np.zeros(3) for k in range(T)]
        for k in range(T):
            if status[k][o] != 0:
                continue
            for lag in range(min(k, L - 1) + 1):
                k0 = k - lag
                assert status[k0][o] == 0
                for i in range(len(m)):
                    d = (positions[k][sl][i] - com[k]) - (positions[k0][sl][i] - com[k0])
                    vv = vel[k][i] * vel[k0][i]
                    out["msd"][o, lag, sp[i]] += d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                    out["msd_abs"][o, lag, sp[i]] += d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                    out["vacf"][o, lag, sp[i]] += vv[0] + vv[1] + vv[2]
                    out["vacf_abs"][o, lag, sp[i]] += abs(vv[0]) + abs(vv[1]) + abs(vv[2])
                out["cnt"][o, lag] += 1
    return out


def heights(cell: np.ndarray) -> np.ndarray:
    """Distance between the two faces of the cell that lattice vector a does not lie in, for a = 0, 1, 2."""
    return 1.0 / np.linalg.norm(np.linalg.inv(cell), axis=0)


def pair_histogram_one(r: np.ndarray, cell: np.ndarray, sp: np.ndarray, n_species: int, bins: int, rmax: float, wrap: bool = False) -> np.ndarray:
    """One configuration -> ordered-pair counts [S, S, bins] (uint64)."""
    hist = np.zeros((n_species, n_species, bins), np.uint64)
    n = len(r)
    inv = np.linalg.inv(cell)
    reach = np.ceil(rmax / heights(cell)).astype(int) + 2
    width = rmax / bins
    for i in range(n):
        for j in range(n):
            diff = r[j] - r[i]
            f = diff @ inv
            if wrap:
                diff = (f - np.round(f)) @ cell
                span = reach
            else:
                span = reach + np.ceil(np.abs(f)).astype(int)
            na, nb, nc = (np.arange(-s, s + 1) for s in span)
            shifts = np.stack(np.meshgrid(na, nb, nc, indexing="ij"), -1).reshape(-1, 3)
            if i == j:
                shifts = shifts[np.any(shifts != 0, axis=1)]   # an atom is no neighbour of itself, its images are
            d = np.linalg.norm(diff[None, :] + shifts @ cell, axis=1)
            near = d[d < rmax + 1e-6]
            x = near / width
            off_edge = np.abs(x - np.round(x)) * width
            assert np.all(off_edge > EDGE_GUARD), f"pair ({i}, {j}): a distance lies {off_edge.min():.2e} A from a bin edge"
            inside = d[d < rmax]
            idx = np.floor(inside / rmax * bins).astype(int)
            assert np.all(idx < bins)
            np.add.at(hist[sp[i], sp[j]], idx, np.uint64(1))
    return hist


def pair_histogram(positions, cells, status, atom_off, species, n_species: int, bins: int, rmax: float, wrap: bool = False) -> dict:
    """positions [T, N, 3], cells [T, B, 3, 3], status [T, B] -> rdf [B, S, S, bins], rdf_samples [B], vol_sum [B]."""
    T, B = len(positions), len(atom_off) - 1
    out = {"rdf": np.zeros((B, n_species, n_species, bins), np.uint64), "rdf_samples": np.zeros(B, np.int64), "vol_sum": np.zeros(B)}
    for k in range(T):
        for o in range(B):
            if status[k][o] != 0:
                continue
            sl = slice(atom_off[o], atom_off[o + 1])
            cell = np.asarray(cells[k][o], np.float64).reshape(3, 3)
            out["rdf"][o] += pair_histogram_one(positions[k][sl], cell, species[sl], n_species, bins, rmax, wrap)
            out["rdf_samples"][o] += 1
            out["vol_sum"][o] += abs(np.linalg.det(cell))
    return out
