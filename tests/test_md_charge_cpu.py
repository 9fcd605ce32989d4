"""Charge-state observers without a device: the NumPy restatement (tests/md_charge_ref.py) on hand cases with known answers, its edge
guard, ``MDObservables`` on the restatement's raw sums, every refusal of the new ``MDObservers`` keywords and the layout of the two new
C structs."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import md_charge_ref as ref

from chgnet_amd import _lib
from chgnet_amd.observables import ChargeStateSums, MDObservables, MDObservers

CELL = np.eye(3) * 9.0


def _run(mag, species, n_bounds, bounds, L=0, S=None, status=None, pos=None, **kw):
    mag = np.asarray(mag, np.float32)
    T, n = mag.shape
    S = int(max(species)) + 1 if S is None else S
    pos = np.zeros((T, n, 3)) if pos is None else pos
    status = np.zeros((T, 1), np.int32) if status is None else status
    return ref.charge_states(mag, pos, np.tile(CELL, (T, 1, 1, 1)), status, np.array([0, n]), np.asarray(species), S, L, n_bounds,
                             np.asarray(bounds, np.float64), **kw)


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------

def test_two_atoms_alternating_between_two_states():
    lo, hi = 3.0, 4.0
    T, L = 6, 3
    mag = [[lo, hi] if k % 2 == 0 else [hi, lo] for k in range(T)]          # atom 0: 0 1 0 1 0 1, atom 1: 1 0 1 0 1 0
    c = _run(mag, [0, 0], [1], [[3.5, 0, 0]], L=L)
    assert c["pop"][0, 0].tolist() == [6, 6, 0, 0]
    assert c["trans"][0, 0].tolist() == [[0, 5, 0, 0], [5, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]     # every step flips both atoms
    assert c["occ"].tolist() == [[3, 3, 0, 0], [3, 3, 0, 0]]
    assert c["cnt"][0].tolist() == [6, 5, 4]
    # lag 0: always the same state; lag 1: never; lag 2: always -- one atom in each state per time origin
    assert c["same"][0, :, 0, :2].tolist() == [[6, 6], [0, 0], [4, 4]]
    assert c["mcorr"][0, :, 0].tolist() == [6 * (lo * lo + hi * hi), 5 * 2 * lo * hi, 4 * (lo * lo + hi * hi)]
    assert c["samples"][0] == T and c["skipped"][0] == 0 and c["vol_sum"][0] == pytest.approx(T * 729.0)


def test_constant_moments_give_n_m2_cnt():
    n, T, L, m = 5, 7, 4, np.float32(2.75)
    c = _run(np.full((T, n), m), [0] * n, [0], [[0, 0, 0]], L=L, mag_bins=4, mag_max=4.0)
    cnt = np.array([T - lag for lag in range(L)])
    assert np.array_equal(c["cnt"][0], cnt)
    assert np.array_equal(c["mcorr"][0, :, 0], n * float(m) ** 2 * cnt) and np.array_equal(c["mcorr_abs"], c["mcorr"])
    assert c["msum"][0, 0] == n * T * float(m) and c["msq"][0, 0] == n * T * float(m) ** 2
    assert c["mhist"][0, 0].tolist() == [0, 0, n * T, 0]
    assert c["pop"][0, 0].tolist() == [n * T, 0, 0, 0] and c["same"][0, :, 0, 0].tolist() == (n * cnt).tolist()


def test_a_moment_on_a_boundary_goes_to_the_upper_state_and_mag_max_is_not_counted():
    b, top = float(np.float32(3.5)), float(np.float32(5.0))
    mag = [[b, top, np.nextafter(np.float32(b), np.float32(0)), 1.1]]
    with pytest.raises(AssertionError, match="boundary"):
        _run(mag, [0, 0, 0, 0], [1], [[b, 0, 0]], mag_bins=10, mag_max=top)                  # the guard refuses the tie ...
    c = _run(mag, [0, 0, 0, 0], [1], [[b, 0, 0]], mag_bins=10, mag_max=top, allow={(0, 0), (0, 1), (0, 2)})   # ... unless it is named
    assert c["occ"].tolist() == [[0, 1, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]]
    assert c["pop"][0, 0].tolist() == [2, 2, 0, 0]
    assert c["mhist"][0, 0].sum() == 3 and c["mhist"][0, 0, 7] == 1 and c["mhist"][0, 0, 6] == 1 and c["mhist"][0, 0, 2] == 1   # 5.0 left out
    assert c["msum"][0, 0] == pytest.approx(b + top + float(mag[0][2]) + float(np.float32(1.1)))                 # but it is in every other sum


def test_a_nan_moment_is_skipped_in_its_sample_and_in_its_lag_pairs():
    T, L = 4, 3
    mag = np.full((T, 2), 2.0, np.float32)
    mag[:, 1] = 4.0
    mag[1, 0] = np.nan
    c = _run(mag, [0, 0], [1], [[3.0, 0, 0]], L=L, mag_bins=5, mag_max=7.0)
    assert c["skipped"][0] == 1 and c["samples"][0] == T
    assert c["pop"][0, 0].tolist() == [3, 4, 0, 0] and c["occ"].tolist() == [[3, 0, 0, 0], [0, 4, 0, 0]]
    assert c["trans"][0, 0, 0, 0] == 1 and c["trans"][0, 0, 1, 1] == 3          # atom 0: only 2 -> 3 has both ends
    assert c["same"][0, :, 0, 0].tolist() == [3, 1, 1] and c["same"][0, :, 0, 1].tolist() == [4, 3, 2]    # atom 0: (0,0) (2,2) (3,3) | (3,2) | (2,0)
    assert c["mcorr"][0, :, 0].tolist() == [3 * 4.0 + 4 * 16.0, 1 * 4.0 + 3 * 16.0, 1 * 4.0 + 2 * 16.0]
    assert c["msum"][0, 0] == 3 * 2.0 + 4 * 4.0 and np.isfinite(c["msq"]).all() and c["mhist"][0, 0].sum() == 7
    assert c["cnt"][0].tolist() == [4, 3, 2]                                    # the lag counts are those of the plain observers


def test_a_stopped_replica_is_left_alone_and_negative_moments_are_state_zero():
    T = 4
    status = np.zeros((T, 1), np.int32)
    status[2:] = 1
    c = _run(np.full((T, 1), -0.5), [0], [1], [[1.0, 0, 0]], L=2, status=status, mag_bins=4, mag_max=2.0)
    assert c["samples"][0] == 2 and c["pop"][0, 0].tolist() == [2, 0, 0, 0] and c["mhist"].sum() == 0 and c["cnt"][0].tolist() == [2, 1]


def test_the_state_resolved_pair_histogram_counts_images_and_skips_other_centres():
    # a centre (species 0, state 1) and one neighbour (species 1) 1.2 A away in a cubic 3.1 A cell, rmax 3.5: the neighbour and its
    # images, the centre's own images at 3.1 A, nothing for the neighbour as a centre
    cell = np.eye(3) * 3.1
    pos = np.array([[[0.1, 0.2, 0.3], [1.3, 0.2, 0.3]]])
    c = ref.charge_states(np.array([[4.0, 1.0]], np.float32), pos, cell[None, None], np.zeros((1, 1), np.int32), np.array([0, 2]),
                          np.array([0, 1]), 2, 0, [1, 0], np.array([[3.0, 0, 0], [0, 0, 0]]), center=0, srdf_bins=7, srdf_rmax=3.5)
    h = c["shist"][0]
    assert h[0].sum() == 0 and h[2:].sum() == 0
    assert h[1, 0].tolist() == [0, 0, 0, 0, 0, 0, 6]                            # six images of itself at 3.1
    d = sorted(np.linalg.norm(np.array([1.2, 0, 0]) + 3.1 * np.array(s)) for s in np.ndindex(3, 3, 3) for s in [np.array(s) - 1])
    assert h[1, 1].sum() == sum(x < 3.5 for x in d) == 6 and h[1, 1, 2] == 1 and h[1, 1, 3] == 1 and h[1, 1, 6] == 4    # 1.2, 1.9, then 3.32 x 4
    with pytest.raises(AssertionError, match="bin edge"):
        ref.charge_states(np.array([[4.0, 1.0]], np.float32), pos, cell[None, None], np.zeros((1, 1), np.int32), np.array([0, 2]),
                          np.array([0, 1]), 2, 0, [1, 0], np.array([[3.0, 0, 0], [0, 0, 0]]), center=0, srdf_bins=2, srdf_rmax=6.2)


# ---- MDObservables on the raw sums ------------------------------------------------------------------------------------------------

def test_observables_arithmetic_on_the_alternating_pair():
    T, L, dt = 6, 3, 4.0
    mag = [[3.25, 4.25] if k % 2 == 0 else [4.25, 3.25] for k in range(T)]
    c = _run(mag, [0, 0], [1], [[3.5, 0, 0]], L=L, mag_bins=10, mag_max=5.0)
    sums = ChargeStateSums(c, 0, slice(0, 2), [1], [[3.5, 0, 0]], 5.0, -1, 0.0)
    obs = MDObservables([25], [2], dt, np.zeros((L, 1)), np.zeros((L, 1)), c["cnt"][0], charge=sums)
    assert obs.n_states(25) == 2 and obs.state_populations(25).tolist() == [0.5, 0.5]
    assert obs.mean_magmom(25) == pytest.approx(3.75) and obs.magmom_std(25) == pytest.approx(0.5)
    assert obs.transition_counts(25).tolist() == [[0, 5], [5, 0]]
    assert obs.transition_rate(25, 0, 1) == pytest.approx(1.0 / (dt * 1e-3)) and obs.transition_rate(25, 0, 0) == 0.0
    assert obs.state_persistence(25, 0).tolist() == [1.0, 0.0, 1.0]
    assert np.allclose(obs.magmom_correlation(25), [14.3125, 13.8125, 14.3125])
    assert obs.site_occupancy().tolist() == [[0.5, 0.5, 0, 0], [0.5, 0.5, 0, 0]]
    h = obs.magmom_histogram(25)
    assert h.sum() * 0.5 == pytest.approx(1.0) and h[6] == h[8] == pytest.approx(1.0) and obs.magmom_bin_centres[6] == pytest.approx(3.25)
    with pytest.raises(ValueError, match="state-resolved"):
        obs.state_rdf(0, 25)
    plain = MDObservables([25], [2], dt, np.zeros((L, 1)), np.zeros((L, 1)), c["cnt"][0])
    with pytest.raises(ValueError, match="no charge states"):
        plain.state_populations(25)


def test_state_rdf_of_an_ideal_lattice_is_normalised_by_population_and_mean_volume():
    cell = np.eye(3) * 3.1
    pos = np.array([[[0.1, 0.2, 0.3], [1.3, 0.2, 0.3]]])
    c = ref.charge_states(np.array([[4.0, 1.0]], np.float32), pos, cell[None, None], np.zeros((1, 1), np.int32), np.array([0, 2]),
                          np.array([0, 1]), 2, 0, [1, 0], np.array([[3.0, 0, 0], [0, 0, 0]]), center=0, srdf_bins=7, srdf_rmax=3.5)
    sums = ChargeStateSums(c, 0, slice(0, 2), [1, 0], [[3.0, 0, 0], [0, 0, 0]], 0.0, 0, 3.5)
    obs = MDObservables([25, 8], [1, 1], 1.0, charge=sums)
    g = obs.state_rdf(1, 8)
    edges = np.arange(8) * 0.5
    shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    assert np.allclose(g, c["shist"][0, 1, 1] / (1 * (1 / 3.1 ** 3) * shell)) and g[2] > 0 and obs.state_rdf_r[2] == pytest.approx(1.25)
    with pytest.raises(ValueError, match="no centre atom"):
        obs.state_rdf(0, 8)


# ---- Python validation --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw, text", [
    ({"magmom_states": {"Mn": [4.2, 3.4]}}, "ascending"),
    ({"magmom_states": {"Mn": [3.4, 3.4]}}, "ascending"),
    ({"magmom_states": {"Mn": [1.0, 2.0, 3.0, 4.0]}}, "at most 3"),
    ({"magmom_states": {"Xx": [1.0]}}, "unknown element"),
    ({"magmom_states": {25: [1.0], "Mn": [2.0]}}, "twice"),
    ({"magmom_states": {"Mn": [-1.0]}}, ">= 0"),
    ({"magmom_states": {"Mn": [float("nan")]}}, "finite"),
    ({"magmom_bins": 8}, "magmom_max"),
    ({"magmom_max": 5.0}, "needs magmom_bins"),
    ({"magmom_bins": -1, "magmom_max": 5.0}, ">= 0"),
    ({"magmom_bins": 4097, "magmom_max": 5.0}, "exceeds"),
    ({"magmom_bins": 1.5}, "integer"),
    ({"state_rdf_bins": 8, "state_rdf_rmax": 4.0}, "state_rdf_center"),
    ({"state_rdf_bins": 8, "state_rdf_center": "Mn"}, "state_rdf_rmax"),
    ({"state_rdf_bins": 8, "state_rdf_center": "Mn", "state_rdf_rmax": float("inf")}, "state_rdf_rmax"),
    ({"state_rdf_center": "Mn"}, "need state_rdf_bins"),
    ({"state_rdf_bins": 4097, "state_rdf_center": "Mn", "state_rdf_rmax": 4.0}, "exceeds"),
])
def test_bad_keywords_are_refused_with_a_message(kw, text):
    with pytest.raises(ValueError, match=text):
        MDObservers(msd_lags=2, **kw)


def test_species_are_checked_when_the_batch_is_known():
    ob = MDObservers(msd_lags=2, magmom_states={"Mn": [3.4, 4.2], 8: [0.1]}, magmom_bins=16, magmom_max=5.0, state_rdf_center="Mn",
                     state_rdf_bins=32, state_rdf_rmax=4.0)
    assert ob.charge_states and ob.magmom_states == {25: [3.4, 4.2], 8: [0.1]}
    p, bounds = ob.charge_params([3, 8, 25])
    assert list(p.n_bounds)[:3] == [0, 1, 2] and p.center_species == 2 and p.mag_bins == 16 and p.srdf_bins == 32
    assert bounds.tolist() == [[0, 0, 0], [0.1, 0, 0], [3.4, 4.2, 0]] and p.mag_max == 5.0 and p.srdf_rmax == 4.0
    with pytest.raises(ValueError, match="not among the species"):
        ob.charge_params([3, 8])                                                 # Mn named, not in the run
    with pytest.raises(ValueError, match="state_rdf_center"):
        MDObservers(msd_lags=2, state_rdf_center="Fe", state_rdf_bins=8, state_rdf_rmax=4.0).charge_params([3, 8, 25])
    with pytest.raises(ValueError, match="fewer bins"):
        MDObservers(msd_lags=2, magmom_bins=2048, magmom_max=5.0).charge_params([3, 8, 25])
    with pytest.raises(ValueError, match="fewer bins"):
        MDObservers(msd_lags=2, state_rdf_center=8, state_rdf_bins=2048, state_rdf_rmax=4.0).charge_params([3, 8, 25])
    old = MDObservers(msd_lags=2, collective=True)
    assert not old.charge_states and old.charge_params([3, 8, 25]) is None      # the old keywords ask for nothing new


def test_struct_layouts_and_exported_symbols():
    assert ctypes.sizeof(_lib.MdChargeParams) == 8 * 4 + 4 * 4 + 2 * 8 and _lib.MdChargeParams.mag_max.offset == 48
    assert ctypes.sizeof(_lib.MdChargeHost) == 12 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in _lib.MdChargeHost._fields_] == ["mhist", "msum", "msq", "pop", "trans", "occ", "mcorr", "same", "shist", "samples",
                                                          "skipped", "vol_sum"]
    for name in ("chg_md_set_magmoms", "chg_md_download_magmoms", "chg_md_set_charge_states", "chg_md_download_charge_states",
                 "chg_test_md_charge_states"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert (_lib.MD_CHG_STATES, _lib.MD_CHG_BOUNDS, ref.Q) == (4, 3, 4)
