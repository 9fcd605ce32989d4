"""Float64 NumPy restatement of the charge-state observers (include/chgnet_hip.h "Charge-informed MD"; csrc/kernels_md_magmom.h): plain
loops over samples, lags and atoms, written from the definitions and sharing nothing with the kernels' rings or reductions.

Beside every float sum ``charge_states`` returns the sum of the ABSOLUTE values of its terms (``msum_abs``, ``msq_abs``, ``mcorr_abs``),
which bounds the float64 reordering error of the device, as tests/md_transport_ref.py does.

Edge guard.  A moment that lies within ``MAG_GUARD`` of a state boundary, of a histogram edge or of ``mag_max``, and a distance that
lies within ``EDGE_GUARD`` of an edge of the state-resolved pair histogram or of ``srdf_rmax``, would make the expected integer
depend on the last bit of a division.  With ``guard=True`` such an input fails here, on the CPU.  Deliberate ties are named in
``allow``, a set of ``(sample, atom)``: their moments are float32 values that ARE the boundary or ``mag_max`` exactly, for which the
comparisons ``bound <= m`` and ``m < mag_max`` have one answer.  With ``guard=False`` nothing is asserted and the ``*_doubt`` arrays
mark what a caller comparing values it did not choose has to leave out: ``doubt_atoms`` -- the (sample, atom) pairs whose STATE is in
doubt -- and ``mhist_doubt`` / ``shist_doubt``, the two bins on either side of a guarded value.
"""

from __future__ import annotations

import numpy as np

from md_observe_ref import EDGE_GUARD, heights

Q = 4                # state slots
MAG_GUARD = 1e-9     # mu_B; float32 moments of order 1 are spaced 1e-7 apart


def state_of(m: float, bounds) -> int:
    """The number of boundaries that are <= m; -1 for a non-finite moment."""
    if not np.isfinite(m):
        return -1
    return int(sum(1 for b in bounds if b <= m))


def _centre_distances(r: np.ndarray, cell: np.ndarray, i: int, shifts: np.ndarray) -> tuple:
    """For centre i: the distances |r_j - r_i + n L| [n, shifts] over the given lattice shifts around the wrapped difference, and the
    mask [n, shifts] of what counts (i == j with n == 0 does not)."""
    inv = np.linalg.inv(cell)
    f = (r - r[i]) @ inv
    f = f - np.round(f)
    d = np.linalg.norm((f[:, None, :] + shifts[None, :, :]) @ cell, axis=2)
    counts = np.ones(d.shape, bool)
    counts[i, np.all(shifts == 0, axis=1)] = False
    return d, counts


def charge_states(magmoms, positions, cells, status, atom_off, species, n_species: int, n_lags: int, n_bounds, bounds, mag_bins: int = 0,
                  mag_max: float = 0.0, center: int = -1, srdf_bins: int = 0, srdf_rmax: float = 0.0, guard: bool = True,
                  allow=frozenset()) -> dict:
    """magmoms [T, N] (float32), positions [T, N, 3], cells [T, B, 3, 3], status [T, B] (0 = running), bounds [S, 3] -> the sums of
    chg_md_charge_host with ``_abs`` companions of the float sums, cnt [B, L] and the doubt marks."""
    T, B, L, S = len(magmoms), len(atom_off) - 1, n_lags, n_species
    N = int(atom_off[-1])
    mag = np.asarray(magmoms, np.float32).astype(np.float64)
    out = {"mhist": np.zeros((B, S, mag_bins), np.uint64), "msum": np.zeros((B, S)), "msq": np.zeros((B, S)),
           "msum_abs": np.zeros((B, S)), "msq_abs": np.zeros((B, S)),
           "pop": np.zeros((B, S, Q), np.int64), "trans": np.zeros((B, S, Q, Q), np.int64), "occ": np.zeros((N, Q), np.int64),
           "mcorr": np.zeros((B, L, S)), "mcorr_abs": np.zeros((B, L, S)), "same": np.zeros((B, L, S, Q), np.int64),
           "shist": np.zeros((B, Q, S, srdf_bins), np.uint64), "samples": np.zeros(B, np.int64), "skipped": np.zeros(B, np.int64),
           "vol_sum": np.zeros(B), "cnt": np.zeros((B, L), np.int64),
           "doubt_atoms": np.zeros((T, N), bool), "mhist_doubt": np.zeros((B, S, mag_bins), bool),
           "shist_doubt": np.zeros((B, Q, S, srdf_bins), bool)}
    width = mag_max / mag_bins if mag_bins else 0.0
    swidth = srdf_rmax / srdf_bins if srdf_bins else 0.0
    state = np.full((T, N), -1, np.int64)
    for k in range(T):
        for g in range(N):
            m, sp = mag[k, g], species[g]
            bs = [float(b) for b in bounds[sp][:n_bounds[sp]]]
            state[k, g] = state_of(m, bs)
            if np.isfinite(m) and (k, g) not in allow and any(abs(m - b) <= MAG_GUARD for b in bs):
                assert not guard, f"sample {k}, atom {g}: the moment {m!r} lies within {MAG_GUARD} of a boundary"
                out["doubt_atoms"][k, g] = True
    for o in range(B):
        a0, a1 = int(atom_off[o]), int(atom_off[o + 1])
        for k in range(T):
            if status[k][o] != 0:
                continue
            cell = np.asarray(cells[k][o], np.float64).reshape(3, 3)
            out["samples"][o] += 1
            out["vol_sum"][o] += abs(np.linalg.det(cell))
            for g in range(a0, a1):
                m, sp, q = mag[k, g], species[g], state[k, g]
                if q < 0:
                    out["skipped"][o] += 1
                    continue
                out["msum"][o, sp] += m
                out["msum_abs"][o, sp] += abs(m)
                out["msq"][o, sp] += m * m
                out["msq_abs"][o, sp] += m * m
                out["pop"][o, sp, q] += 1
                out["occ"][g, q] += 1
                if k >= 1 and state[k - 1, g] >= 0:
                    assert status[k - 1][o] == 0
                    out["trans"][o, sp, state[k - 1, g], q] += 1
                if mag_bins > 0:
                    x = m / width
                    edge = int(np.round(x))
                    if (k, g) not in allow and m > -1e-6 and m < mag_max + 1e-6 and abs(x - edge) * width <= MAG_GUARD:
                        assert not guard, f"sample {k}, atom {g}: the moment {m!r} lies within {MAG_GUARD} of a histogram edge"
                        for b in (edge - 1, edge):
                            if 0 <= b < mag_bins:
                                out["mhist_doubt"][o, sp, b] = True
                    if 0.0 <= m < mag_max:
                        b = int(np.floor(m / mag_max * mag_bins))
                        assert b < mag_bins
                        out["mhist"][o, sp, b] += np.uint64(1)
            for lag in range(min(k, L - 1) + 1):
                k0 = k - lag
                assert status[k0][o] == 0
                for g in range(a0, a1):
                    q1, q0, sp = state[k, g], state[k0, g], species[g]
                    if q1 < 0 or q0 < 0:
                        continue
                    out["mcorr"][o, lag, sp] += mag[k, g] * mag[k0, g]
                    out["mcorr_abs"][o, lag, sp] += abs(mag[k, g] * mag[k0, g])
                    if q1 == q0:
                        out["same"][o, lag, sp, q1] += 1
                out["cnt"][o, lag] += 1
            if srdf_bins > 0:
                r = np.asarray(positions[k][a0:a1], np.float64)
                reach = np.ceil(srdf_rmax / heights(cell)).astype(int) + 1
                shifts = np.stack(np.meshgrid(*(np.arange(-s, s + 1) for s in reach), indexing="ij"), -1).reshape(-1, 3)
                sj = np.broadcast_to(np.asarray(species[a0:a1])[:, None], (a1 - a0, len(shifts)))
                for i in range(a1 - a0):
                    if species[a0 + i] != center or state[k, a0 + i] < 0:
                        continue
                    qi = state[k, a0 + i]
                    d, counts = _centre_distances(r, cell, i, shifts)
                    x = d / swidth
                    near = counts & (d < srdf_rmax + 1e-6) & (np.abs(x - np.round(x)) * swidth <= EDGE_GUARD)
                    if near.any():
                        assert not guard, f"replica {o}, sample {k}, centre {i}: a distance lies within {EDGE_GUARD} A of a bin edge"
                        for s_j, e in zip(sj[near], np.round(x[near]).astype(int)):
                            for b in (e - 1, e):
                                if 0 <= b < srdf_bins:
                                    out["shist_doubt"][o, qi, s_j, b] = True
                    inside = counts & (d < srdf_rmax)
                    idx = np.floor(d[inside] / srdf_rmax * srdf_bins).astype(int)
                    assert np.all(idx < srdf_bins)
                    np.add.at(out["shist"][o, qi], (sj[inside], idx), np.uint64(1))
    return out
