"""Transport observables without a device: the NumPy restatement (tests/md_transport_ref.py) on closed forms, ``MDObservables`` on
hand-made raw arrays (conductivities, Haven ratio, the unit constant, van Hove normalisation), every refusal of ``MDObservers`` and
the layout of the two new C structs."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

import md_transport_ref as ref
from conftest import REPO

from chgnet_amd import _lib
from chgnet_amd.observables import MDObservables, MDObservers


# ---- the restatement on closed forms ----------------------------------------------------------------------------------------------

def test_species_drifting_as_one_give_n2_u2_t2_and_alpha2_of_minus_two_fifths():
    rng = np.random.default_rng(0)
    n, T, L, dt = 7, 8, 5, 0.7
    m = rng.uniform(1.0, 50.0, n)
    sp = np.array([0, 1, 0, 1, 1, 0, 1], np.int32)
    n_per = np.bincount(sp)
    drift = rng.normal(0, 0.3, (2, 3))                     # one constant velocity per species
    v = drift[sp]
    r0 = rng.uniform(0, 8, (n, 3))
    pos = np.stack([r0 + v * (k * dt) for k in range(T)])
    mom = np.stack([v * m[:, None]] * T)
    cells = np.tile(np.eye(3) * 9.0, (T, 1, 1, 1))
    c = ref.transport(pos, mom, cells, np.zeros((T, 1), np.int32), np.array([0, n]), sp, m, 2, L, subtract_com=False)
    assert np.array_equal(c["cnt"][0], [T - lag for lag in range(L)]) and c["samples"][0] == T
    assert c["vol_sum"][0] == pytest.approx(T * 729.0, rel=1e-13)
    for lag in range(L):
        t, cnt = lag * dt, T - lag
        for a in range(2):
            for b in range(2):
                assert c["cmsd"][0, lag, a, b] == pytest.approx(cnt * n_per[a] * n_per[b] * (drift[a] @ drift[b]) * t * t, rel=1e-11, abs=1e-13)
                assert c["jacf"][0, lag, a, b] == pytest.approx(cnt * n_per[a] * n_per[b] * (drift[a] @ drift[b]), rel=1e-11)
            assert c["msd4"][0, lag, a] == pytest.approx(cnt * n_per[a] * (drift[a] @ drift[a]) ** 2 * t ** 4, rel=1e-11, abs=1e-13)
    assert np.array_equal(c["msd4_abs"], c["msd4"]) and np.all(c["cmsd_abs"] >= np.abs(c["cmsd"])) and np.all(c["jacf_abs"] >= np.abs(c["jacf"]))
    # every atom of a species has moved equally far: <r^4> = <r^2>^2, so alpha_2 = 3/5 - 1
    msd = np.stack([[(T - lag) * n_per[a] * (drift[a] @ drift[a]) * (lag * dt) ** 2 for a in range(2)] for lag in range(L)])
    obs = MDObservables([3, 8], n_per, dt, msd, np.zeros((L, 2)), c["cnt"][0], msd4_sum=c["msd4"][0])
    for z in (3, 8):
        a2 = obs.non_gaussian_parameter(z)
        assert np.isnan(a2[0]) and np.allclose(a2[1:], -0.4, rtol=1e-11)


def test_isotropic_gaussian_displacements_give_alpha2_of_zero_within_sampling_error():
    # alpha_2 = 3 A / (5 B^2) - 1 with A, B the sample means of r^4, r^2.  For r^2 = sigma^2 chi^2_3: E r^2 = 3, E r^4 = 15, E r^6 = 105,
    # E r^8 = 945 (sigma = 1), so Var r^4 = 720, Var r^2 = 6, Cov = 60; the gradient at the means is (1/15, -2/3) and the delta method
    # gives Var alpha_2 = (720 / 225 + 6 * 4 / 9 - 2 * 60 * 2 / 45) / n = 8 / (15 n).  Five standard deviations.
    rng = np.random.default_rng(1)
    n, sigma = 4000, 0.4
    r0 = rng.uniform(0, 10, (n, 3))
    pos = np.stack([r0, r0 + rng.normal(0, sigma, (n, 3))])
    sp = np.zeros(n, np.int32)
    cells = np.tile(np.eye(3) * 10.0, (2, 1, 1, 1))
    c = ref.transport(pos, np.zeros_like(pos), cells, np.zeros((2, 1), np.int32), np.array([0, n]), sp, np.ones(n), 1, 2, subtract_com=False)
    msd = np.array([[0.0], [((pos[1] - pos[0]) ** 2).sum()]])
    obs = MDObservables([3], [n], 1.0, msd, np.zeros((2, 1)), c["cnt"][0], msd4_sum=c["msd4"][0])
    a2 = obs.non_gaussian_parameter(3)[1]
    print(f"alpha_2 = {a2:.4f}, one standard deviation {np.sqrt(8 / (15 * n)):.4f}")
    assert abs(a2) < 5 * np.sqrt(8 / (15 * n))


def test_the_histogram_counts_displacements_and_its_edge_guard_refuses_an_edge():
    n, bins, rmax = 4, 8, 2.0
    r0 = np.zeros((n, 3))
    step = np.array([[0.1, 0, 0], [0, 0.3, 0], [0, 0, 1.9], [2.5, 0, 0]])          # bins 0, 1, 7 and beyond rmax
    pos = np.stack([r0, r0 + step, r0 + 2 * step])
    sp = np.array([0, 1, 0, 1], np.int32)
    kw = {"momenta": np.zeros_like(pos), "cells": np.tile(np.eye(3) * 5.0, (3, 1, 1, 1)), "status": np.zeros((3, 1), np.int32),
          "atom_off": np.array([0, n]), "species": sp, "masses": np.ones(n), "n_species": 2, "n_lags": 3, "subtract_com": False}
    c = ref.transport(pos, vh_bins=bins, vh_rmax=rmax, vh_lags=2, vh_stride=2, **kw)
    assert c["vh"][0, 0].sum(axis=1).tolist() == [6, 6]                          # lag 0: 3 origins x 2 atoms per species, all in bin 0
    assert c["vh"][0, 0, :, 0].tolist() == [6, 6]
    lag2 = np.zeros((2, bins), np.uint64)                                        # lag 2: 0.2, 0.6 and twice beyond rmax (3.8, 5.0)
    lag2[0, 0], lag2[1, 2] = 1, 1
    assert np.array_equal(c["vh"][0, 1], lag2) and not c["vh_doubt"].any()
    with pytest.raises(AssertionError, match="bin edge"):                        # lag 1: 0.25 * 2 is an edge of 8 bins to 2.0
        ref.transport(np.stack([r0, r0 + np.array([0.5, 0, 0])]), vh_bins=bins, vh_rmax=rmax, vh_lags=2, vh_stride=1,
                      **{**kw, "momenta": np.zeros((2, n, 3)), "cells": kw["cells"][:2], "status": kw["status"][:2], "n_lags": 2})
    soft = ref.transport(np.stack([r0, r0 + np.array([0.5, 0, 0])]), vh_bins=bins, vh_rmax=rmax, vh_lags=2, vh_stride=1, guard=False,
                         **{**kw, "momenta": np.zeros((2, n, 3)), "cells": kw["cells"][:2], "status": kw["status"][:2], "n_lags": 2})
    assert soft["vh_doubt"][0, 1].sum(axis=1).tolist() == [2, 2] and soft["vh_doubt"][0, 1, 0, 1:3].all()


# ---- MDObservables on raw arrays --------------------------------------------------------------------------------------------------

def _walkers():
    """Raw sums of independent walkers of two species: a linear MSD, and collective sums whose cross terms are exactly zero."""
    L, dt = 40, 5.0
    n_per = np.array([6, 10])
    D = np.array([2e-4, 5e-5])                                                    # A^2/fs
    cnt = np.arange(L, 0, -1) * 2
    t = np.arange(L) * dt
    msd_sum = (0.03 + 6 * D[None, :] * t[:, None]) * cnt[:, None] * n_per[None, :]
    cmsd = np.zeros((L, 2, 2))
    cmsd[:, 0, 0], cmsd[:, 1, 1] = msd_sum[:, 0], msd_sum[:, 1]                   # sum_i |u_i|^2 and nothing else
    return L, dt, n_per, D, cnt, msd_sum, cmsd


def test_independent_unit_charge_walkers_have_a_haven_ratio_of_one():
    L, dt, n_per, D, cnt, msd_sum, cmsd = _walkers()
    samples, volume, T = 80, 1234.5, 700.0
    obs = MDObservables([3, 11], n_per, dt, msd_sum, np.zeros((L, 2)), cnt, cmsd_sum=cmsd, jacf_sum=np.zeros((L, 2, 2)),
                        transport_samples=samples, transport_vol_sum=samples * volume)
    q, fit = {3: 1.0, 11: 1.0}, (20.0, 150.0)
    sigma, ne = obs.ionic_conductivity(q, T, fit), obs.nernst_einstein_conductivity(q, T, fit)
    assert sigma == pytest.approx(ne, rel=1e-12) and obs.haven_ratio(q, T, fit) == pytest.approx(1.0, rel=1e-12)
    # the unit, derived here in SI: sigma = e^2 sum_a n_a 6 D_a / (6 V kB T) with D in m^2/s, V in m^3, kB in J/K gives S/m
    e, kB_J = 1.6021766208e-19, 1.38064852e-23
    si = e ** 2 * float((n_per * D).sum()) * (1e-20 / 1e-15) / (volume * 1e-30 * kB_J * T)
    assert sigma == pytest.approx(si / 100.0, rel=1e-11)                          # S/m -> S/cm
    from chgnet_amd import observables
    from chgnet_amd.dynamics import KB
    assert observables._E2_PER_A_FS_EV_IN_S_PER_CM == pytest.approx(1.6021766208e4, rel=1e-15) and observables._KB == KB
    # a species without a charge counts as 0; a positive cross term (atoms moving together) lowers the Haven ratio
    assert obs.ionic_conductivity({3: 1.0}, T, fit) == pytest.approx(si / 100.0 * n_per[0] * D[0] / (n_per * D).sum(), rel=1e-11)
    together = cmsd.copy()
    together[:, 0, 1] = together[:, 1, 0] = 0.25 * np.sqrt(cmsd[:, 0, 0] * cmsd[:, 1, 1])
    moved = MDObservables([3, 11], n_per, dt, msd_sum, np.zeros((L, 2)), cnt, cmsd_sum=together, transport_samples=samples,
                          transport_vol_sum=samples * volume)
    assert moved.haven_ratio(q, T, fit) < 0.9
    assert np.allclose(moved.collective_msd(3, 11), together[:, 0, 1] / cnt)
    with pytest.raises(ValueError, match="not among"):
        obs.ionic_conductivity({8: -2.0}, T, fit)
    with pytest.raises(ValueError, match="fewer than two lags"):
        obs.ionic_conductivity(q, T, (21.0, 24.0))
    with pytest.raises(ValueError, match="collective=True"):
        MDObservables([3, 11], n_per, dt, msd_sum, np.zeros((L, 2)), cnt).ionic_conductivity(q, T, fit)


def test_current_correlation_is_per_origin_in_angstrom_per_fs_and_not_symmetrised():
    from chgnet_amd.dynamics import FS
    L = 3
    cnt = np.array([4, 3, 0])
    jacf = np.arange(L * 4, dtype=np.float64).reshape(L, 2, 2) + 1.0
    obs = MDObservables([3, 8], [2, 2], 2.0, np.zeros((L, 2)), np.zeros((L, 2)), cnt, jacf_sum=jacf, cmsd_sum=np.zeros((L, 2, 2)))
    c01, c10 = obs.current_correlation(3, 8), obs.current_correlation(8, 3)
    assert np.allclose(c01[:2], jacf[:2, 0, 1] / cnt[:2] * FS ** 2) and np.allclose(c10[:2], jacf[:2, 1, 0] / cnt[:2] * FS ** 2)
    assert np.isnan(c01[2]) and np.isnan(obs.collective_msd(3, 3)[2]) and not np.allclose(c01[:2], c10[:2])


def test_van_hove_self_integrates_to_the_counted_fraction():
    rng = np.random.default_rng(4)
    L, lags, stride, bins, rmax = 7, 3, 3, 16, 4.0
    n_per = np.array([5, 9])
    cnt = np.array([9, 8, 7, 6, 5, 4, 0])                                         # lag 6 (the third histogram) was never reached
    hist = np.zeros((lags, 2, bins), np.uint64)
    inside = [[1.0, 1.0], [0.8, 0.6], [0.0, 0.0]]                                 # fraction of the displacements below rmax
    for j in range(lags):
        for s in range(2):
            total = int(round(inside[j][s] * cnt[j * stride] * n_per[s]))
            hist[j, s] = np.bincount(rng.integers(0, bins, total), minlength=bins)
    obs = MDObservables([3, 8], n_per, 2.0, np.zeros((L, 2)), np.zeros((L, 2)), cnt, vanhove_hist=hist, vanhove_rmax=rmax,
                        vanhove_stride=stride)
    assert np.allclose(obs.vanhove_r, (np.arange(bins) + 0.5) * rmax / bins) and obs.vanhove_lag_times_fs.tolist() == [0.0, 6.0, 12.0]
    edges = np.arange(bins + 1) * rmax / bins
    shell = 4 / 3 * np.pi * np.diff(edges ** 3)
    for s, z in enumerate((3, 8)):
        g = obs.van_hove_self(z)
        assert g.shape == (lags, bins) and np.isnan(g[2]).all()
        for j in range(2):
            counted = int(hist[j, s].sum()) / (cnt[j * stride] * n_per[s])                # what was put in, after rounding to whole counts
            assert abs(counted - inside[j][s]) < 0.02 and (g[j] * shell).sum() == pytest.approx(counted, rel=1e-12)
        assert g[1, 3] == pytest.approx(hist[1, s, 3] / (cnt[3] * n_per[s] * shell[3]), rel=1e-13)
    with pytest.raises(ValueError, match="vanhove_bins"):
        MDObservables([3], [1], 1.0).van_hove_self(3)
    with pytest.raises(ValueError, match="vanhove_hist"):
        MDObservables([3, 8], n_per, 2.0, np.zeros((L, 2)), np.zeros((L, 2)), cnt, vanhove_hist=hist, vanhove_rmax=rmax, vanhove_stride=4)


# ---- MDObservers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw, match", [
    ({"collective": True}, "msd_lags"),
    ({"rdf_bins": 10, "rdf_rmax": 5.0, "collective": True}, "collective needs msd_lags"),
    ({"rdf_bins": 10, "rdf_rmax": 5.0, "non_gaussian": True}, "non_gaussian needs msd_lags"),
    ({"rdf_bins": 10, "rdf_rmax": 5.0, "vanhove_bins": 8, "vanhove_rmax": 2.0}, "vanhove_bins needs msd_lags"),
    ({"msd_lags": 8, "vanhove_bins": -1}, "vanhove_bins"),
    ({"msd_lags": 8, "vanhove_bins": 2.5, "vanhove_rmax": 2.0}, "integer"),
    ({"msd_lags": 8, "vanhove_bins": 4097, "vanhove_rmax": 2.0}, "van Hove cells"),
    ({"msd_lags": 8, "vanhove_bins": 16}, "vanhove_rmax"),
    ({"msd_lags": 8, "vanhove_bins": 16, "vanhove_rmax": 0.0}, "vanhove_rmax"),
    ({"msd_lags": 8, "vanhove_bins": 16, "vanhove_rmax": float("inf")}, "vanhove_rmax"),
    ({"msd_lags": 8, "vanhove_rmax": 2.0}, "need vanhove_bins"),
    ({"msd_lags": 8, "vanhove_lags": 2}, "need vanhove_bins"),
    ({"msd_lags": 8, "vanhove_stride": 2}, "need vanhove_bins"),
    ({"msd_lags": 8, "vanhove_bins": 16, "vanhove_rmax": 2.0, "vanhove_stride": 0}, "vanhove_stride"),
    ({"msd_lags": 8, "vanhove_bins": 16, "vanhove_rmax": 2.0, "vanhove_stride": True}, "integer"),
    ({"msd_lags": 8, "vanhove_bins": 16, "vanhove_rmax": 2.0, "vanhove_lags": 0}, "vanhove_lags"),
    ({"msd_lags": 8, "vanhove_bins": 16, "vanhove_rmax": 2.0, "vanhove_lags": 5, "vanhove_stride": 2}, "not among"),
    ({"msd_lags": 8, "vanhove_bins": 16, "vanhove_rmax": 2.0, "vanhove_lags": 9}, "not among"),
    ({}, "nothing to observe"),
])
def test_observers_refuse_bad_transport_arguments(kw, match):
    with pytest.raises(ValueError, match=match):
        MDObservers(**kw)


def test_transport_params_and_their_limit():
    plain = MDObservers(sample_interval=2, msd_lags=8, rdf_rmax=6.0, rdf_bins=200)
    assert plain.transport_params(3) is None
    p = plain.params(3)                                                           # unchanged by the new keywords
    assert (p.sample_interval, p.n_lags, p.subtract_com, p.n_species, p.rdf_bins, p.rdf_rmax) == (2, 8, 1, 3, 200, 6.0)
    ob = MDObservers(msd_lags=64, collective=True, vanhove_bins=64, vanhove_rmax=4.0, vanhove_stride=16)
    assert ob.vanhove_lags == 4                                                   # as many as fit: lags 0, 16, 32, 48
    t = ob.transport_params(3)
    assert (t.collective, t.non_gaussian, t.vh_bins, t.vh_lags, t.vh_stride, t.vh_rmax) == (1, 0, 64, 4, 16, 4.0)
    t = MDObservers(msd_lags=4, non_gaussian=True).transport_params(2)
    assert (t.collective, t.non_gaussian, t.vh_bins, t.vh_lags) == (0, 1, 0, 0)
    assert MDObservers(msd_lags=4, vanhove_bins=512, vanhove_rmax=2.0).transport_params(8).vh_bins == 512      # the limit itself
    with pytest.raises(ValueError, match="van Hove cells"):
        MDObservers(msd_lags=4, vanhove_bins=513, vanhove_rmax=2.0).transport_params(8)
    species, index = ob.species_map([25, 3, 8, 8, 3])                             # unchanged too
    assert species.tolist() == [3, 8, 25] and index.tolist() == [2, 0, 1, 1, 0]


def test_transport_structs_mirror_the_c_header(tmp_path):
    fields = {"chg_md_transport_params": _lib.MdTransportParams, "chg_md_transport_host": _lib.MdTransportHost}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "chgnet_hip.h"', "int main(void) {"]
    for cname, cls in fields.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", f"-I{os.path.join(REPO, 'include')}", str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in fields.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert len(got) == 2 + 7 + 6
