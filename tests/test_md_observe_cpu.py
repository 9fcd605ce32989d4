"""MD observables without a device: the NumPy restatement (tests/md_observe_ref.py) on closed forms, ``MDObservables`` on raw arrays,
and every refusal of ``MDObservers``."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

import md_observe_ref as ref
from conftest import REPO

from chgnet_amd import _lib
from chgnet_amd.observables import MDObservables, MDObservers


# ---- the restatement on closed forms ----------------------------------------------------------------------------------------------

def test_ballistic_atoms_give_v2_t2_and_a_constant_vacf():
    rng = np.random.default_rng(0)
    n, T, L, dt = 6, 9, 5, 0.7
    m = rng.uniform(1.0, 50.0, n)
    sp = np.array([0, 1, 0, 1, 1, 0], np.int32)
    r0, v = rng.uniform(0, 8, (n, 3)), rng.normal(0, 0.3, (n, 3))
    pos = np.stack([r0 + v * (k * dt) for k in range(T)])
    mom = np.stack([v * m[:, None]] * T)
    c = ref.correlations(pos, mom, np.zeros((T, 1), np.int32), np.array([0, n]), sp, m, 2, L, subtract_com=False)
    assert np.array_equal(c["cnt"][0], [T - lag for lag in range(L)])
    for s in range(2):
        v2 = (v[sp == s] ** 2).sum()
        for lag in range(L):
            assert c["msd"][0, lag, s] == pytest.approx(v2 * (lag * dt) ** 2 * (T - lag), rel=1e-12, abs=1e-13)
            assert c["vacf"][0, lag, s] == pytest.approx(v2 * (T - lag), rel=1e-12)
    # in the centre-of-mass frame the velocities are v - V: still ballistic
    V = (m[:, None] * v).sum(0) / m.sum()
    c = ref.correlations(pos, mom, np.zeros((T, 1), np.int32), np.array([0, n]), sp, m, 2, L, subtract_com=True)
    assert c["msd"][0, 3, 0] == pytest.approx((((v - V)[sp == 0]) ** 2).sum() * (3 * dt) ** 2 * (T - 3), rel=1e-11)


def _simple_cubic(a: float, bins: int, rmax: float):
    cell = np.eye(3) * (2 * a)
    r = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)], np.float64) * a + 0.123
    return ref.pair_histogram_one(r, cell, np.zeros(8, np.int32), 1, bins, rmax)[0, 0], r, cell


def test_simple_cubic_lattice_has_shells_of_6_12_8():
    a, bins, rmax = 2.0, 40, 3.7
    hist, r, _ = _simple_cubic(a, bins, rmax)
    width = rmax / bins
    expect = np.zeros(bins, np.uint64)
    for d, z in ((a, 6), (np.sqrt(2) * a, 12), (np.sqrt(3) * a, 8)):
        expect[int(d / width)] += 8 * z
    assert np.array_equal(hist, expect)


def test_the_edge_guard_refuses_a_distance_on_a_bin_edge():
    with pytest.raises(AssertionError, match="bin edge"):
        _simple_cubic(2.0, 40, 4.0)        # 2.0 A sits on the edge of bin 20


def test_ordered_pairs_are_symmetric_and_wrapping_changes_nothing():
    rng = np.random.default_rng(3)
    cell = np.array([[5.1, 0.3, -0.2], [0.8, 5.6, 0.4], [-0.5, 1.1, 6.2]])
    sp = np.array([0, 0, 1, 2, 1, 0, 2], np.int32)
    r = rng.random((7, 3)) @ cell
    h = ref.pair_histogram_one(r, cell, sp, 3, 32, 6.0)
    for a in range(3):
        for b in range(3):
            assert np.array_equal(h[a, b], h[b, a])
    shifted = r + np.array([[3, -2, 1]] * 3 + [[0, 0, 0]] * 4) @ cell      # unwrapped positions: the same crystal
    assert np.array_equal(ref.pair_histogram_one(shifted, cell, sp, 3, 32, 6.0), h)
    assert np.array_equal(ref.pair_histogram_one(shifted, cell, sp, 3, 32, 6.0, wrap=True), h)


@pytest.fixture(scope="module")
def ideal_gas():
    """Uniform random points of two species in a cubic box: raw sums of 3 samples."""
    rng = np.random.default_rng(5)
    n, a, bins, rmax, T = 60, 9.0, 12, 4.5, 3
    sp = (np.arange(n) % 3 == 0).astype(np.int32)          # 20 of species 1, 40 of species 0
    pos = rng.random((T, n, 3)) * a
    cells = np.tile(np.eye(3) * a, (T, 1, 1, 1))
    out = ref.pair_histogram(pos, cells, np.zeros((T, 1), np.int32), np.array([0, n]), sp, 2, bins, rmax)
    return out, sp, bins, rmax, a


def test_uniform_random_points_give_g_of_one_within_counting_error(ideal_gas):
    out, sp, bins, rmax, a = ideal_gas
    assert out["rdf_samples"][0] == 3 and out["vol_sum"][0] == pytest.approx(3 * a ** 3)
    obs = MDObservables([3, 8], np.bincount(sp), 1.0, rdf_hist=out["rdf"][0], rdf_samples=3, vol_sum=out["vol_sum"][0], rdf_rmax=rmax)
    assert np.allclose(obs.r, (np.arange(bins) + 0.5) * rmax / bins)
    for za, zb in ((3, 3), (3, 8), (8, 3), (8, 8)):
        g = obs.rdf(za, zb)
        counts = out["rdf"][0][obs._s(za), obs._s(zb)].astype(np.float64)
        # Poisson counting error of every bin (like pairs are counted twice: the error of the count doubles with it), 5 sigma
        sigma = np.sqrt(np.maximum(counts, 1.0) * (2.0 if za == zb else 1.0)) / np.maximum(counts, 1.0)
        far = obs.r > 1.0
        assert np.all(np.abs(g[far] - 1.0) < 5 * sigma[far] * g[far].clip(1.0)), (za, zb, g)
        # the pair count N_a (N_b - [a == b]) makes the whole-range mean 1 for like and unlike pairs at this small N
        shell = np.diff((np.arange(bins + 1) * rmax / bins) ** 3)
        assert np.average(g, weights=shell) == pytest.approx(1.0, abs=5 * np.sqrt((2.0 if za == zb else 1.0) / counts.sum()))


# ---- MDObservables on raw arrays --------------------------------------------------------------------------------------------------

def test_normalisation_per_atom_and_time_origin():
    L, n_per = 4, np.array([2, 5])
    cnt = np.array([7, 6, 5, 0])
    msd = np.arange(8, dtype=np.float64).reshape(L, 2)
    vacf = 1.0 + np.arange(8, dtype=np.float64).reshape(L, 2)
    obs = MDObservables([3, 25], n_per, 4.0, msd, vacf, cnt)
    assert np.array_equal(obs.lag_times_fs, [0.0, 4.0, 8.0, 12.0])
    assert np.allclose(obs.msd(25)[:3], msd[:3, 1] / (cnt[:3] * 5)) and np.isnan(obs.msd(25)[3])
    from chgnet_amd.dynamics import FS
    assert np.allclose(obs.vacf(3)[:3], vacf[:3, 0] / (cnt[:3] * 2) * FS ** 2)
    assert obs.vacf(3, normalized=True)[0] == 1.0
    assert obs.msd_sum is not None and np.array_equal(obs.cnt, cnt)      # the raw arrays stay available
    with pytest.raises(ValueError, match="not among"):
        obs.msd(8)


def test_coordination_number_integrates_to_the_lattice_shells():
    a, bins, rmax = 2.0, 40, 3.7
    hist, _, cell = _simple_cubic(a, bins, rmax)
    obs = MDObservables([26], [8], 1.0, rdf_hist=hist[None, None], rdf_samples=1, vol_sum=abs(np.linalg.det(cell)), rdf_rmax=rmax)
    assert obs.coordination_number(26, 26, 2.4) == 6
    assert obs.coordination_number(26, 26, 3.0) == 18
    assert obs.coordination_number(26, 26, 3.7) == 26
    g = obs.rdf(26, 26)
    k = int(a / (rmax / bins))
    edges = np.arange(bins + 1) * rmax / bins
    shell = 4 / 3 * np.pi * (edges[k + 1] ** 3 - edges[k] ** 3)
    assert g[k] == pytest.approx(8 * 6 / (1 * 8 * 7 / (2 * a) ** 3 * shell), rel=1e-12)
    with pytest.raises(ValueError, match="r_cut"):
        obs.coordination_number(26, 26, 4.0)


def test_diffusion_coefficient_recovers_a_linear_msd():
    # D = 1e-5 cm^2/s: MSD = 6 D t.  1e-5 cm^2/s = 1e-5 * 1e16 A^2 / 1e15 fs = 1e-4 A^2/fs, so MSD = 6e-4 A^2/fs * t
    L, n, dt = 50, 4, 10.0
    cnt = np.arange(L, 0, -1) * 3
    t = np.arange(L) * dt
    msd_sum = (0.02 + 6e-4 * t) * cnt * n
    obs = MDObservables([3], [n], dt, msd_sum[:, None], np.zeros((L, 1)), cnt)
    assert obs.diffusion_coefficient(3, fit=(100.0, 400.0)) == pytest.approx(1e-5, rel=1e-10)
    with pytest.raises(ValueError, match="fewer than two lags"):
        obs.diffusion_coefficient(3, fit=(101.0, 109.0))
    with pytest.raises(ValueError, match="fewer than two lags"):
        obs.diffusion_coefficient(3, fit=(95.0, 105.0))


# ---- MDObservers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw, match", [
    ({"sample_interval": 0, "msd_lags": 4}, "sample_interval"),
    ({"sample_interval": 1.5, "msd_lags": 4}, "integer"),
    ({"msd_lags": -1}, "msd_lags"),
    ({"msd_lags": 4097}, "msd_lags"),
    ({"msd_lags": True}, "integer"),
    ({"rdf_bins": -3, "rdf_rmax": 5.0}, "rdf_bins"),
    ({"rdf_bins": 16385, "rdf_rmax": 5.0}, "histogram cells"),
    ({"rdf_bins": 10}, "rdf_rmax"),
    ({"rdf_bins": 10, "rdf_rmax": 0.0}, "rdf_rmax"),
    ({"rdf_bins": 10, "rdf_rmax": float("nan")}, "rdf_rmax"),
    ({"msd_lags": 4, "rdf_rmax": 5.0}, "needs rdf_bins"),
    ({}, "nothing to observe"),
])
def test_observers_refuse_bad_arguments(kw, match):
    with pytest.raises(ValueError, match=match):
        MDObservers(**kw)


def test_species_map_and_its_limits():
    ob = MDObservers(sample_interval=2, msd_lags=8, rdf_rmax=6.0, rdf_bins=200)
    species, index = ob.species_map([25, 3, 8, 8, 3])
    assert species.tolist() == [3, 8, 25] and index.tolist() == [2, 0, 1, 1, 0] and index.dtype == np.int32
    p = ob.params(3)
    assert (p.sample_interval, p.n_lags, p.subtract_com, p.n_species, p.rdf_bins, p.rdf_rmax) == (2, 8, 1, 3, 200, 6.0)
    with pytest.raises(ValueError, match="9 species"):
        ob.species_map(np.arange(1, 10))
    with pytest.raises(ValueError, match="histogram cells"):
        MDObservers(rdf_rmax=6.0, rdf_bins=2000).species_map([3, 8, 25])
    with pytest.raises(ValueError, match="MDObservers"):
        from chgnet_amd.dynamics import MolecularDynamics
        MolecularDynamics(None, ensemble="nve", observers="msd")


def test_observer_structs_mirror_the_c_header(tmp_path):
    fields = {"chg_md_observe_params": _lib.MdObserveParams, "chg_md_observables_host": _lib.MdObservablesHost}
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
