"""Float64 NumPy restatement of the transport observables (include/chgnet_hip.h "MD observables"; csrc/kernels_md_transport.h): plain
loops over samples, lags and atoms, written from the definitions and sharing nothing with the kernels' rings or reductions.

Beside every float sum ``transport`` returns the sum of the ABSOLUTE values of its terms, which bounds the float64 reordering error
of the device: ``msd4_abs`` is ``msd4`` itself (its terms are positive), ``cmsd_abs[a, b] = sum_c (sum_{i in a} |u_ic|) (sum_{j in b}
|u_jc|)`` and ``jacf_abs`` likewise from ``|v_ic|``.  The centres of mass come from ``md_observe_ref`` (long double).

For the van Hove histogram it ASSERTS that no ``|u_i|`` lies within ``EDGE_GUARD`` of a bin edge or of ``vh_rmax``: an input on an
edge fails here, on the CPU, instead of depending on the last bit of a square root on the device.  Displacements that are exactly
zero by construction -- lag 0, and a single-atom replica under ``subtract_com`` -- are exempt and belong to bin 0.  With
``guard=False`` nothing is asserted and ``vh_doubt`` [B, vh_lags, S, bins] marks the two bins on either side of every guarded
displacement instead: a caller that compares frames it did not choose leaves those bins out.
"""

from __future__ import annotations

import numpy as np

from md_observe_ref import EDGE_GUARD, centre_of_mass


def transport(positions, momenta, cells, status, atom_off, species, masses, n_species: int, n_lags: int, subtract_com: bool,
              vh_bins: int = 0, vh_rmax: float = 0.0, vh_lags: int = 0, vh_stride: int = 1, guard: bool = True) -> dict:
    """positions / momenta [T, N, 3], cells [T, B, 3, 3], status [T, B] (0 = running) -> msd4 [B, L, S], cmsd / jacf [B, L, S, S] with
    their ``_abs`` companions, vh [B, vh_lags, S, vh_bins] (uint64), samples [B], vol_sum [B], cnt [B, L] and vh_doubt."""
    T, B, L, S = len(positions), len(atom_off) - 1, n_lags, n_species
    out = {"msd4": np.zeros((B, L, S)), "cmsd": np.zeros((B, L, S, S)), "jacf": np.zeros((B, L, S, S)),
           "cmsd_abs": np.zeros((B, L, S, S)), "jacf_abs": np.zeros((B, L, S, S)), "cnt": np.zeros((B, L), np.int64),
           "vh": np.zeros((B, vh_lags, S, vh_bins), np.uint64), "vh_doubt": np.zeros((B, vh_lags, S, vh_bins), bool),
           "samples": np.zeros(B, np.int64), "vol_sum": np.zeros(B)}
    width = vh_rmax / vh_bins if vh_bins else 0.0
    for o in range(B):
        sl = slice(atom_off[o], atom_off[o + 1])
        m, sp = masses[sl], species[sl]
        n = len(m)
        r = [np.asarray(positions[k][sl], np.float64) for k in range(T)]
        vel = [momenta[k][sl] / m[:, None] for k in range(T)]
        com = [centre_of_mass(positions[k][sl], m) if subtract_com else np.zeros(3) for k in range(T)]
        for k in range(T):
            if status[k][o] != 0:
                continue
            out["samples"][o] += 1
            out["vol_sum"][o] += abs(np.linalg.det(np.asarray(cells[k][o], np.float64).reshape(3, 3)))
            for lag in range(min(k, L - 1) + 1):
                k0 = k - lag
                assert status[k0][o] == 0
                U, Uabs = np.zeros((S, 3)), np.zeros((S, 3))
                J1, J0, J1abs, J0abs = np.zeros((S, 3)), np.zeros((S, 3)), np.zeros((S, 3)), np.zeros((S, 3))
                binned = vh_bins > 0 and lag % vh_stride == 0 and lag // vh_stride < vh_lags
                zero_by_construction = lag == 0 or (subtract_com and n == 1)
                for i in range(n):
                    u = (r[k][i] - com[k]) - (r[k0][i] - com[k0])
                    d2 = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
                    out["msd4"][o, lag, sp[i]] += d2 * d2
                    U[sp[i]] += u
                    Uabs[sp[i]] += np.abs(u)
                    J1[sp[i]] += vel[k][i]
                    J0[sp[i]] += vel[k0][i]
                    J1abs[sp[i]] += np.abs(vel[k][i])
                    J0abs[sp[i]] += np.abs(vel[k0][i])
                    if not binned:
                        continue
                    d = np.sqrt(d2)
                    j = lag // vh_stride
                    if zero_by_construction:
                        assert d == 0.0
                        out["vh"][o, j, sp[i], 0] += np.uint64(1)
                        continue
                    x = d / width
                    edge = int(np.round(x))
                    if d < vh_rmax + 1e-6 and abs(x - edge) * width <= EDGE_GUARD:
                        assert not guard, f"replica {o}, sample {k}, lag {lag}, atom {i}: |u| lies {abs(x - edge) * width:.2e} A from a bin edge"
                        for b in (edge - 1, edge):
                            if 0 <= b < vh_bins:
                                out["vh_doubt"][o, j, sp[i], b] = True
                    if d < vh_rmax:
                        b = int(np.floor(d / vh_rmax * vh_bins))
                        assert b < vh_bins
                        out["vh"][o, j, sp[i], b] += np.uint64(1)
                for a in range(S):
                    for b in range(S):
                        out["cmsd"][o, lag, a, b] += U[a][0] * U[b][0] + U[a][1] * U[b][1] + U[a][2] * U[b][2]
                        out["cmsd_abs"][o, lag, a, b] += Uabs[a][0] * Uabs[b][0] + Uabs[a][1] * Uabs[b][1] + Uabs[a][2] * Uabs[b][2]
                        out["jacf"][o, lag, a, b] += J1[a][0] * J0[b][0] + J1[a][1] * J0[b][1] + J1[a][2] * J0[b][2]
                        out["jacf_abs"][o, lag, a, b] += J1abs[a][0] * J0abs[b][0] + J1abs[a][1] * J0abs[b][1] + J1abs[a][2] * J0abs[b][2]
                out["cnt"][o, lag] += 1
    out["msd4_abs"] = out["msd4"].copy()
    return out
