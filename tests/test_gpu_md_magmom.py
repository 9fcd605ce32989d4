"""Charge-informed MD on the MI355X: the charge-state kernels alone on caller-given snapshots against the NumPy restatement
(tests/md_charge_ref.py), bit-wise determinism, the limits and refusals of the C interface, the moments in the frames of real runs
against ``predict_structure`` at the frames' own geometry, and real runs whose own frames are the truth of what they accumulated.

Tolerance of the float sums: ``1e-12 * sum|terms|`` with the sum of absolute values from the restatement, the ``REL`` of
tests/test_gpu_md_transport.py: a bound on the float64 reordering of at most 300 terms per cell and sample, not a measured figure.
Counts are integers and must be equal.

Tolerance of the moments in the frames (test 4): not fixed in advance.  The engine's float32 atomic sums are not bit-reproducible
(DESIGN.md 7b), so two ``predict_structure`` calls on one structure differ; the test measures that difference on every frame, allows
four times the largest one for the run's own evaluation (graph built from the integrator's staged coordinates, not from an uploaded
structure) and prints both figures.  One MI355X run of this file: DESIGN.md "MD observables -> Charge states"."""

from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import pytest

import md_charge_ref as ref
from conftest import GOLDEN, load_case
from md_hard_cells import BINS, HARD, RMAX, hard_batch

pytestmark = pytest.mark.gpu

REL = 1e-12
EINVAL = -1
Q = ref.Q
INT_SUMS = ("mhist", "pop", "trans", "occ", "same", "shist", "samples", "skipped")
FLOAT_SUMS = ("msum", "msq", "mcorr")


def _charge(eng, observe: dict, charge: dict, bounds, aoff, species, masses, positions, momenta, cells, status, magmoms):
    """chg_test_md_charge_states -> (rc, plain sums, charge-state sums)."""
    from chgnet_amd import _lib
    from chgnet_amd.observables import empty_arrays, empty_charge_arrays

    B, T, N = len(aoff) - 1, len(positions), int(aoff[-1])
    p = _lib.MdObserveParams(**{"sample_interval": 1, "n_lags": 0, "subtract_com": 1, "n_species": 1, "rdf_bins": 0, "reserved": 0,
                                "rdf_rmax": 0.0, **observe})
    charge = dict(charge)
    n_bounds = charge.pop("n_bounds", [])
    c = _lib.MdChargeParams(**{"mag_bins": 0, "center_species": -1, "srdf_bins": 0, "reserved": 0, "mag_max": 0.0, "srdf_rmax": 0.0, **charge})
    for s, nb in enumerate(n_bounds):
        c.n_bounds[s] = nb
    S = max(p.n_species, 1)
    hb = np.zeros((8, 3))
    hb[:len(bounds)] = bounds
    d = empty_arrays(B, max(p.n_lags, 0), S, max(p.rdf_bins, 0))
    dc = empty_charge_arrays(B, N, max(p.n_lags, 0), S, max(c.mag_bins, 0), max(c.srdf_bins, 0))
    out, cout = _lib.fill_out(_lib.MdObservablesHost(), d), _lib.fill_out(_lib.MdChargeHost(), dc)
    dp = ctypes.POINTER(ctypes.c_double)
    arr = [np.ascontiguousarray(x, np.float64) for x in (masses, positions, momenta, cells)]
    ints = [np.ascontiguousarray(x, np.int32) for x in (aoff, species, status)]
    mag = np.ascontiguousarray(magmoms, np.float32)
    rc = eng.lib.chg_test_md_charge_states(eng.handle, ctypes.byref(p), ctypes.byref(c), hb.ctypes.data_as(dp), B,
                                           ints[0].ctypes.data_as(_lib.c_int_p), ints[1].ctypes.data_as(_lib.c_int_p),
                                           arr[0].ctypes.data_as(dp), T, arr[1].ctypes.data_as(dp), arr[2].ctypes.data_as(dp),
                                           arr[3].ctypes.data_as(dp), ints[2].ctypes.data_as(_lib.c_int_p), mag.ctypes.data_as(_lib.c_float_p),
                                           ctypes.byref(out), ctypes.byref(cout))
    return rc, d, dc


def _assert_float_sums(got: dict, want: dict, where=""):
    for name in FLOAT_SUMS:
        err, bound = np.abs(got[name] - want[name]), REL * want[name + "_abs"]
        print(f"{where} {name}: max |device - restatement| / sum|terms| = {np.max(err / np.maximum(want[name + '_abs'], 1e-300)):.2e}")
        assert np.all(err <= bound), (where, name, float(np.max(err - bound)))


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------------------
SIZES = [1, 5, 17, 300, 40]            # 300: more than one pass of a 256-thread workgroup; 1: a replica of a single atom
STOPPED, STOP_AT = 1, 3                # replica 1 is non-finite from sample 3 on
WALK_SEED = 3                          # chosen on the CPU: the restatement's edge guard passes for the moments and the distances
T_WALK, S_WALK, L_WALK = 11, 3, 4      # the ring of 4 wraps twice
N_BOUNDS = [0, 2, 3]
BOUNDS = np.array([[0.0, 0.0, 0.0], [1.5, 3.0, 0.0], [1.0, 2.5, 3.5]])
CENTER = 2                             # absent from replica 2
CHARGE = {"n_bounds": N_BOUNDS, "mag_bins": 16, "mag_max": 4.5, "center_species": CENTER, "srdf_bins": 32, "srdf_rmax": 6.0}
TRICLINIC = np.array([[4.0, 0.0, 0.0], [0.5, 4.0, 0.0], [0.3, -0.4, 4.0]])      # heights below srdf_rmax: several lattice shifts count


@functools.lru_cache(maxsize=None)
def _walk():
    """11 snapshots of five replicas, S = 3 (species 2 absent from replica 2), moments that wander across the boundaries, and three
    deliberate values: one moment exactly on a boundary, one exactly at mag_max, one NaN."""
    rng = np.random.default_rng(WALK_SEED)
    T, S = T_WALK, S_WALK
    aoff = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    N = int(aoff[-1])
    species = rng.integers(0, S, N).astype(np.int32)
    species[aoff[2]:aoff[3]] = rng.integers(0, 2, SIZES[2])
    masses = rng.uniform(1.0, 200.0, N)
    pos = np.empty((T, N, 3))
    pos[0] = rng.uniform(0.0, 4.0, (N, 3))
    mag = np.empty((T, N), np.float32)
    mag[0] = rng.uniform(0.0, 5.0, N)
    for k in range(1, T):
        pos[k] = pos[k - 1] + rng.normal(0, 0.15, (N, 3))
        mag[k] = np.abs(mag[k - 1] + rng.normal(0, 0.5, N)).astype(np.float32)
    mom = np.zeros((T, N, 3))
    cells = np.tile(TRICLINIC, (T, len(SIZES), 1, 1))
    status = np.zeros((T, len(SIZES)), np.int32)
    status[STOP_AT:, STOPPED] = 1
    big = np.arange(aoff[3], aoff[4])
    on_bound = int(big[species[big] == 1][0])        # species 1, boundary 1.5: belongs to the upper state
    at_max = int(big[species[big] == 2][0])          # species 2 and a centre: state 3, not in the moment histogram
    nan_atom = int(big[species[big] == 2][1])        # a centre that is skipped at sample 5 and in the lag pairs that touch it
    mag[2, on_bound] = np.float32(1.5)
    mag[4, at_max] = np.float32(4.5)
    mag[5, nan_atom] = np.nan
    ties = frozenset({(2, on_bound), (4, at_max)})
    return aoff, species, masses, pos, mom, cells, status, mag, ties, (on_bound, at_max, nan_atom)


@functools.lru_cache(maxsize=None)
def _want(samples: int = T_WALK) -> dict:
    """The restatement, computed once (its edge guard asserts inside; the two ties are on its allow-list)."""
    aoff, species, masses, pos, mom, cells, status, mag, ties, _ = _walk()
    return ref.charge_states(mag[:samples], pos[:samples], cells[:samples], status[:samples], aoff, species, S_WALK, L_WALK, N_BOUNDS, BOUNDS,
                             mag_bins=CHARGE["mag_bins"], mag_max=CHARGE["mag_max"], center=CENTER, srdf_bins=CHARGE["srdf_bins"],
                             srdf_rmax=CHARGE["srdf_rmax"], allow=ties)


def _run_walk(eng, samples: int = T_WALK, charge: dict = CHARGE):
    aoff, species, masses, pos, mom, cells, status, mag, _, _ = _walk()
    rc, plain, got = _charge(eng, {"n_lags": L_WALK, "n_species": S_WALK}, charge, BOUNDS, aoff, species, masses, pos[:samples], mom[:samples],
                             cells[:samples], status[:samples], mag[:samples])
    assert rc == 0, eng.lib.chg_last_error(eng.handle)
    return plain, got


def test_charge_state_kernels_match_the_restatement(hip_engine):
    aoff, species, _, _, _, _, _, mag, _, (on_bound, at_max, nan_atom) = _walk()
    want = _want()
    plain, got = _run_walk(hip_engine)
    _assert_float_sums(got, want, "walk")
    for name in INT_SUMS:
        assert np.array_equal(got[name], want[name]), name                                            # integers: exactly
    assert np.array_equal(plain["cnt"], want["cnt"])
    assert plain["cnt"][0].tolist() == [11, 10, 9, 8] and plain["cnt"][STOPPED].tolist() == [3, 2, 1, 0]   # ring wrapped twice; stopped for good
    assert got["samples"].tolist() == [11, 3, 11, 11, 11] and got["skipped"].tolist() == [0, 0, 0, 1, 0]
    assert np.allclose(got["vol_sum"], want["vol_sum"], rtol=1e-14, atol=0)
    # the deliberate values
    assert got["occ"][on_bound].sum() == T_WALK and got["occ"][nan_atom].sum() == T_WALK - 1
    assert want["occ"][at_max, 3] >= 1 and ref.state_of(float(mag[2, on_bound]), BOUNDS[1, :2]) == 1
    assert got["mhist"].sum() < got["pop"].sum()                                                     # moments at or beyond mag_max: not binned
    # species 0 has no boundary: one state; the species absent from replica 2 owns nothing; no centre there either
    assert np.all(got["pop"][:, 0, 1:] == 0) and np.all(got["pop"][:, 1, 3] == 0) and got["pop"][3, 2, 3] > 0
    for name in ("mhist", "pop", "trans", "msum", "msq"):
        assert np.all(got[name][2, 2] == 0), name
    assert np.all(got["mcorr"][2, :, 2] == 0) and np.all(got["same"][2, :, 2] == 0) and got["shist"][2].sum() == 0
    assert got["shist"][3].sum() > 100000 and np.count_nonzero(got["shist"][3]) > 300                 # several shifts count; spread out
    assert got["trans"][3].sum() == want["pop"][3].sum() - SIZES[3] - 1 and np.count_nonzero(got["trans"][3, 2]) > 8
    assert np.array_equal(got["same"][:, 0], got["pop"])                                              # lag 0: every counted atom is where it is
    # a single atom
    s0 = species[0]
    assert got["pop"][0, s0].sum() == T_WALK and got["occ"][0].sum() == T_WALK
    # the stopped replica's cells are those of a run that ended at its last sample
    _, early = _run_walk(hip_engine, samples=STOP_AT)
    sl = slice(aoff[STOPPED], aoff[STOPPED + 1])
    for name in INT_SUMS + FLOAT_SUMS + ("vol_sum",):
        if name == "occ":
            assert np.array_equal(got[name][sl], early[name][sl]), name
        else:
            assert np.array_equal(got[name][STOPPED], early[name][STOPPED]), name
    assert got["samples"][STOPPED] == STOP_AT


# ---- 1b. the state-resolved pair histogram on the hard cells: the plain one, split by the state of the centre ---------------------------
HARD_CENTER = 1                        # the species present in eight of the nine hard cells
HARD_BOUNDS = [1.0, 2.0]               # case (b): three states


@pytest.mark.parametrize("n_bounds", [pytest.param(0, id="one_state"), pytest.param(2, id="three_states")])
def test_state_resolved_pair_histogram_is_the_plain_one_on_hard_cells(hip_engine, n_bounds):
    """k_md_chg_srdf and k_md_obs_rdf run the same image pass (kernels_md_sample.h) and differ only in the histogram row of a pair, so on
    the nine hard cells -- two snapshots each, the one-atom cell and the replica stopped before the second snapshot included -- the
    state-resolved counts of a centre species, summed over its states, are the plain counts of that species to the last integer.  The
    plain counts themselves are held to the float64 restatement, as in tests/test_gpu_md_observe.py."""
    aoff, species, S, pos, cells, status, want = hard_batch()
    assert sum(np.any(species[aoff[o]:aoff[o + 1]] == HARD_CENTER) for o in range(len(HARD))) >= 2
    mag = np.random.default_rng(5).uniform(0.0, 3.0, (2, int(aoff[-1]))).astype(np.float32)   # all finite, spread over the three states
    bounds = np.zeros((S, 3))
    bounds[HARD_CENTER, :2] = HARD_BOUNDS
    nb = [n_bounds if s == HARD_CENTER else 0 for s in range(S)]
    rc, plain, got = _charge(hip_engine, {"n_species": S, "rdf_bins": BINS, "rdf_rmax": RMAX},
                             {"n_bounds": nb, "center_species": HARD_CENTER, "srdf_bins": BINS, "srdf_rmax": RMAX}, bounds, aoff, species,
                             np.ones(aoff[-1]), pos, np.zeros_like(pos), cells, status, mag)
    assert rc == 0, hip_engine.lib.chg_last_error(hip_engine.handle)
    for o, name in enumerate(HARD):
        assert np.array_equal(plain["rdf"][o], want["rdf"][o]), name                                  # the reference: the restatement
    assert np.array_equal(plain["rdf_samples"], want["rdf_samples"]) and got["samples"].tolist() == want["rdf_samples"].tolist()
    shist, rdf = got["shist"], plain["rdf"]
    assert shist.shape == (len(HARD), Q, S, BINS) and rdf[:, HARD_CENTER].sum() > 1000
    if n_bounds == 0:
        assert np.array_equal(shist[:, 0], rdf[:, HARD_CENTER]) and np.all(shist[:, 1:] == 0)
    else:
        assert np.array_equal(shist.sum(axis=1), rdf[:, HARD_CENTER])
        assert np.all(got["pop"][:, HARD_CENTER, :3].sum(axis=0) > 0) and np.all(shist[:, :3].sum(axis=(0, 2, 3)) > 0) and np.all(shist[:, 3] == 0)
    assert shist[HARD.index("thin_cube16")].sum() == 0                                                # one atom of another species: no centre


# ---- 2. determinism -----------------------------------------------------------------------------------------------------------------
def test_two_runs_of_the_same_input_give_the_same_bits(hip_engine):
    first_plain, first = _run_walk(hip_engine)
    again_plain, again = _run_walk(hip_engine)
    for name in first:
        assert np.array_equal(first[name], again[name], equal_nan=True), name
    for name in first_plain:
        assert np.array_equal(first_plain[name], again_plain[name]), name
    assert first["mcorr"].sum() > 0 and first["shist"].sum() > 0 and first["trans"].sum() > 0


# ---- 3. limits and refusals -------------------------------------------------------------------------------------------------------------
def _refused(eng, rc, text):
    assert rc == EINVAL
    assert text in eng.lib.chg_last_error(eng.handle).decode()


def _structure(name, rattle=0.02, seed=0):
    from chgnet_amd.graph.structure import Lattice, Structure

    _, d = load_case(name)
    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"])
    cart = s.frac_coords @ s.lattice.matrix + rattle * np.random.default_rng(seed).normal(size=(len(s), 3))
    return Structure(s.lattice, s.atomic_numbers, cart @ np.linalg.inv(s.lattice.matrix))


@pytest.fixture(scope="module")
def calc(trained_like_weights):
    from chgnet_amd import CHGNet
    from chgnet_amd.calculator import CHGNetCalculator

    return CHGNetCalculator(model=CHGNet(state_dict=trained_like_weights))


def test_limits_and_refusals(hip_engine, calc):
    from chgnet_amd import _lib
    from chgnet_amd.dynamics import MolecularDynamics, _DeviceRun
    from chgnet_amd.observables import MDObservers, empty_charge_arrays

    n = 9
    aoff = np.array([0, n], np.int32)
    species = np.array([0, 1, 2, 3, 4, 5, 6, 7, 7], np.int32)
    rng = np.random.default_rng(0)
    pos = np.cumsum(rng.normal(0, 0.2, (3, n, 3)), axis=0) + rng.uniform(0, 5, (n, 3))
    mag = rng.uniform(0.1, 0.9, (3, n)).astype(np.float32)
    snap = (aoff, species, np.ones(n), pos, np.zeros_like(pos), np.tile(np.eye(3) * 5.0, (3, 1, 1, 1)), np.zeros((3, 1), np.int32), mag)
    ring = {"n_lags": 3, "n_species": 8}
    b8 = np.tile([0.5, 1.0, 2.0], (8, 1))
    srdf = {"center_species": 7, "srdf_rmax": 3.0}
    rc, _, got = _charge(hip_engine, ring, {**srdf, "srdf_bins": 512}, b8, *snap)              # Q * S * srdf_bins = 16384: the LDS limit itself
    assert rc == 0, hip_engine.lib.chg_last_error(hip_engine.handle)
    assert got["shist"][0, 0].sum() > 0 and got["shist"][0, 1:].sum() == 0 and got["pop"][0, :, 0].tolist() == [3, 3, 3, 3, 3, 3, 3, 6]
    rc, _, got = _charge(hip_engine, ring, {"mag_bins": 512, "mag_max": 1.0}, b8, *snap)      # S * mag_bins = 4096: the limit of the moment histogram
    assert rc == 0 and got["mhist"].sum() == 3 * n
    one = [1, 0, 0, 0, 0, 0, 0, 0]
    for c, b, text in (({**srdf, "srdf_bins": 513}, b8, "4 * n_species * srdf_bins must be <= 16384"),
                       ({"mag_bins": 513, "mag_max": 1.0}, b8, "n_species * mag_bins must be <= 4096"),
                       ({}, b8, "nothing requested"),
                       ({"n_bounds": [0] * 8}, b8, "nothing requested"),
                       ({"mag_bins": -1, "mag_max": 1.0}, b8, "mag_bins must be >= 0"),
                       ({"srdf_bins": -1}, b8, "srdf_bins must be >= 0"),
                       ({"mag_bins": 8}, b8, "mag_max must be > 0 and finite"),
                       ({"mag_bins": 8, "mag_max": float("nan")}, b8, "mag_max must be > 0 and finite"),
                       ({"n_bounds": [4, 0, 0, 0, 0, 0, 0, 0]}, b8, "n_bounds must be 0..3"),
                       ({"n_bounds": [0, 0, 0, 0, 0, 0, 0, -1]}, b8, "n_bounds must be 0..3"),
                       ({"n_bounds": [2] + [0] * 7}, np.tile([1.0, 0.5, 2.0], (8, 1)), "finite, >= 0 and ascending"),
                       ({"n_bounds": [2] + [0] * 7}, np.tile([1.0, 1.0, 2.0], (8, 1)), "finite, >= 0 and ascending"),
                       ({"n_bounds": one}, np.tile([-0.5, 1.0, 2.0], (8, 1)), "finite, >= 0 and ascending"),
                       ({"n_bounds": one}, np.tile([float("nan"), 1.0, 2.0], (8, 1)), "finite, >= 0 and ascending"),
                       ({"n_bounds": one}, np.tile([float("inf"), 1.0, 2.0], (8, 1)), "finite, >= 0 and ascending"),
                       ({"srdf_bins": 8, "srdf_rmax": 3.0}, b8, "center_species must be 0 .. n_species - 1"),
                       ({"srdf_bins": 8, "srdf_rmax": 3.0, "center_species": 8}, b8, "center_species must be 0 .. n_species - 1"),
                       ({"srdf_bins": 8, "center_species": 7}, b8, "srdf_rmax must be > 0 and finite"),
                       ({"srdf_bins": 8, "center_species": 7, "srdf_rmax": float("inf")}, b8, "srdf_rmax must be > 0 and finite")):
        rc, _, _ = _charge(hip_engine, ring, c, b, *snap)
        _refused(hip_engine, rc, text)
    rc, _, got = _charge(hip_engine, {"n_species": 8, "rdf_bins": 8, "rdf_rmax": 3.0}, {"n_bounds": one}, b8, *snap)   # observers without a ring
    assert rc == 0 and got["pop"][0, 0].tolist() == [int((mag[:, 0] < 0.5).sum()), int((mag[:, 0] >= 0.5).sum()), 0, 0]
    assert got["trans"][0, 0].sum() == 2 and got["mcorr"].size == 0

    md = MolecularDynamics(_structure("limno2"), model=calc, ensemble="nve", starting_temperature=300, loginterval=1, seed=1)
    run = _DeviceRun(md.calculator, [md._structure], md._masses, md._momenta, md.kind, md.cfg, seeds=[md.thermostat_seed], fixed=[md._fixed])
    eng = run.eng                                                                # a handle that has not run yet
    ob = MDObservers(msd_lags=2, magmom_states={25: [0.9]})
    cp, cb = ob.charge_params([3, 8, 25])
    dp = ctypes.POINTER(ctypes.c_double)
    fp = _lib.c_float_p
    set_charge = lambda: eng.lib.chg_md_set_charge_states(eng.handle, run.handle, ctypes.byref(cp), cb.ctypes.data_as(dp))   # noqa: E731
    _refused(eng, set_charge(), "need observers")
    out = _lib.MdChargeHost()
    _refused(eng, eng.lib.chg_md_download_charge_states(eng.handle, run.handle, ctypes.byref(out)), "no charge-state observers")
    last = np.full(run.N, -1.0, np.float32)
    _refused(eng, eng.lib.chg_md_download_magmoms(eng.handle, run.handle, last.ctypes.data_as(fp), None, 0), "chg_md_set_magmoms")
    p = ob.params(3)
    index = np.searchsorted([3, 8, 25], np.asarray(md._structure.atomic_numbers)).astype(np.int32)
    assert eng.lib.chg_md_set_observers(eng.handle, run.handle, ctypes.byref(p), index.ctypes.data_as(_lib.c_int_p)) == 0
    _refused(eng, eng.lib.chg_md_download_charge_states(eng.handle, run.handle, ctypes.byref(out)), "no charge-state observers")
    assert set_charge() == 0 and set_charge() == 0                               # valid before the first run, twice too
    assert eng.lib.chg_md_set_observers(eng.handle, run.handle, ctypes.byref(p), index.ctypes.data_as(_lib.c_int_p)) == 0
    _refused(eng, eng.lib.chg_md_download_charge_states(eng.handle, run.handle, ctypes.byref(out)), "no charge-state observers")   # dropped
    assert set_charge() == 0
    assert eng.lib.chg_md_download_magmoms(eng.handle, run.handle, last.ctypes.data_as(fp), None, 0) == 0 and np.all(last == 0)   # implied
    assert eng.lib.chg_md_set_magmoms(eng.handle, run.handle, 1) == 0
    assert eng.lib.chg_md_run(eng.handle, run.handle, 1) == 0, eng.lib.chg_last_error(eng.handle)
    _refused(eng, set_charge(), "already started")
    _refused(eng, eng.lib.chg_md_set_magmoms(eng.handle, run.handle, 1), "already started")
    frames = np.zeros((2, run.N), np.float32)
    assert eng.lib.chg_md_download_magmoms(eng.handle, run.handle, last.ctypes.data_as(fp), frames.ctypes.data_as(fp), 2) == 0
    assert np.all(last > 0) and np.array_equal(last, frames[1]) and not np.array_equal(frames[0], frames[1])
    d = empty_charge_arrays(1, run.N, 2, 3, 0, 0)
    assert eng.lib.chg_md_download_charge_states(eng.handle, run.handle, ctypes.byref(_lib.fill_out(out, d))) == 0
    assert d["samples"].tolist() == [2] and d["pop"][0].sum() == 2 * run.N and d["pop"][0, 2, :2].sum() == 4
    run.free()
    md.close()


# ---- 4. the moments in the frames ---------------------------------------------------------------------------------------------------------
def _predict_m(model, z, pos, cell):
    from chgnet_amd.graph.structure import Lattice, Structure

    return np.asarray(model.predict_structure(Structure(Lattice(cell), z, pos @ np.linalg.inv(cell)), task="efsm")["m"], np.float32).reshape(-1)


@pytest.mark.parametrize("kw", [pytest.param({"ensemble": "nve"}, id="nve"),
                                pytest.param({"ensemble": "nvt", "thermostat": "Nose-Hoover-Chain", "temperature": 1000}, id="nvt_nhc")])
def test_every_frame_holds_the_moments_of_its_own_geometry(calc, kw, tmp_path):
    import pickle

    from chgnet_amd.dynamics import MolecularDynamics

    path = str(tmp_path / "md.pkl")
    md = MolecularDynamics(_structure("limno2"), model=calc, starting_temperature=1000, timestep=2.0, loginterval=2, seed=11, log_magmoms=True,
                           trajectory=path, **kw)
    md.run(3)
    md.run(5)
    traj = md.traj
    assert traj.steps == [0, 2, 4, 6, 8] and len(traj.magmoms) == 5
    z = np.asarray(md._structure.atomic_numbers)
    noise = err = 0.0
    for k in range(len(traj)):
        assert traj.magmoms[k].dtype == np.float32 and traj.magmoms[k].shape == (len(z),)
        first = _predict_m(calc.model, z, traj.atom_positions[k], traj.cells[k])
        second = _predict_m(calc.model, z, traj.atom_positions[k], traj.cells[k])
        noise = max(noise, float(np.max(np.abs(first - second))))
        err = max(err, float(np.max(np.abs(traj.magmoms[k] - first))))
    print(f"{kw['ensemble']}: max |frame moment - predict_structure| = {err:.3e}; max difference of two predict_structure calls = {noise:.3e}; "
          f"allowed 4 x = {4 * noise:.3e}")
    assert err <= 4 * noise
    assert np.array_equal(md.magmoms, traj.magmoms[-1])                          # the last completed step IS the last frame here
    assert not np.array_equal(traj.magmoms[0], traj.magmoms[-1]) and np.all(traj.magmoms[0] > 0)
    with open(path, "rb") as fh:
        saved = pickle.load(fh)
    assert len(saved["magmoms"]) == 5 and np.array_equal(saved["magmoms"][3], traj.magmoms[3])
    md.close()


def test_without_log_magmoms_nothing_changes(calc, monkeypatch):
    from chgnet_amd.dynamics import MolecularDynamics

    eng = calc.model.engine
    real, calls = eng.lib.chg_md_set_magmoms, []

    def counted(*args):
        calls.append(args)
        return real(*args)

    monkeypatch.setattr(eng.lib, "chg_md_set_magmoms", counted)
    md = MolecularDynamics(_structure("limno2"), model=calc, ensemble="nve", starting_temperature=300, loginterval=1, seed=1)
    traj = md.run(2)
    assert traj.magmoms == [] and md.magmoms is None and len(traj) == 3 and calls == []
    md.close()
    md = MolecularDynamics(_structure("limno2"), model=calc, ensemble="nve", starting_temperature=300, loginterval=1, seed=1, log_magmoms=True)
    assert len(md.run(2).magmoms) == 3 and len(calls) == 1
    md.close()


# ---- 5. a run accumulates what its own frames give ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_moments(name: str, seed: int) -> np.ndarray:
    """The float64 CPU model's moments of the rattled cell the run starts from."""
    import torch

    from chgnet_amd.graph.converter import CrystalGraphConverter
    from oracle.chgnet_oracle import OracleCHGNet

    weights = dict(np.load(os.path.join(GOLDEN, "weights_trained_like.npz")))
    graph = CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3)(_structure(name, seed=seed))
    return np.asarray(OracleCHGNet(weights, dtype=torch.float64).predict_graph(graph, task="m")["m"], np.float64).reshape(-1)


def _split(moments) -> float:
    """A boundary half way between the smallest and the largest of the moments: both sides are populated at step 0."""
    lo, hi = float(np.min(moments)), float(np.max(moments))
    assert hi - lo > 1e-3, "the oracle's moments of the rattled cell do not differ enough to tell two states apart"
    return 0.5 * (lo + hi)


def _restate(traj, species_index, S, steps, ob, cp, bounds):
    """The charge-state sums of one replica recomputed from its own frames at ``steps`` (edge guard off: doubtful values are marked)."""
    at = [traj.steps.index(s) for s in steps]
    pos = np.stack([traj.atom_positions[k] for k in at])
    cells = np.stack([traj.cells[k] for k in at])[:, None]
    mag = np.stack([traj.magmoms[k] for k in at])
    n, status = pos.shape[1], np.zeros((len(at), 1), np.int32)
    return ref.charge_states(mag, pos, cells, status, np.array([0, n]), species_index, S, ob.msd_lags, list(cp.n_bounds)[:S], bounds,
                             mag_bins=ob.magmom_bins, mag_max=ob.magmom_max, center=cp.center_species, srdf_bins=ob.state_rdf_bins,
                             srdf_rmax=ob.state_rdf_rmax, guard=False)


def _assert_replica(obs, want, where):
    c = obs.charge
    assert not want["doubt_atoms"].any(), f"{where}: a float32 moment lies within {ref.MAG_GUARD} of a boundary"
    got = {"msum": c.msum[None], "msq": c.msq[None], "mcorr": c.mcorr[None]}
    _assert_float_sums(got, want, where)
    for name, mine in (("pop", c.pop), ("trans", c.trans), ("same", c.same)):
        assert np.array_equal(mine, want[name][0]), (where, name)
    assert np.array_equal(c.occ, want["occ"]), where
    for name, mine in (("mhist", c.mhist), ("shist", c.shist)):
        doubt = want[name + "_doubt"][0]
        if doubt.any():
            print(f"{where}: edge guard, {int(doubt.sum())} bins of {name} left out")
        assert doubt.sum() <= 8, (where, name)
        assert np.array_equal(mine[~doubt], want[name][0][~doubt]), (where, name)
    assert c.samples == want["samples"][0] and c.skipped == want["skipped"][0] == 0
    assert c.vol_sum == pytest.approx(want["vol_sum"][0], rel=1e-14)
    assert np.array_equal(obs.cnt, want["cnt"][0]), where


@pytest.mark.parametrize("kw", [pytest.param({"ensemble": "nve"}, id="nve"),
                                pytest.param({"ensemble": "nvt", "thermostat": "Nose-Hoover-Chain", "temperature": 1000}, id="nvt_nhc")])
def test_a_run_accumulates_what_its_own_frames_give(calc, kw):
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.observables import MDObservers

    z = np.asarray(_structure("limno2").atomic_numbers)
    m0 = _oracle_moments("limno2", 0)
    ob = MDObservers(sample_interval=2, msd_lags=4, magmom_states={"Mn": [_split(m0[z == 25])], 8: [_split(m0[z == 8])]}, magmom_bins=64,
                     magmom_max=2.0, state_rdf_center="Mn", state_rdf_bins=48, state_rdf_rmax=5.0)
    md = MolecularDynamics(_structure("limno2"), model=calc, starting_temperature=1000, timestep=2.0, loginterval=2, seed=11, observers=ob,
                           log_magmoms=True, **kw)
    md.run(3)
    md.run(5)
    obs = md.observables
    assert md.traj.steps == [0, 2, 4, 6, 8] and obs.species.tolist() == [3, 8, 25]
    cp, bounds = md._run.charge
    want = _restate(md.traj, md._run.species_index, 3, [0, 2, 4, 6, 8], ob, cp, bounds)
    assert want["cnt"][0].tolist() == [5, 4, 3, 2] and obs.charge.samples == 5
    _assert_replica(obs, want, kw["ensemble"])
    # Mn populates two states (its boundary lies between the oracle's two Mn moments of the starting cell)
    assert np.count_nonzero(obs.charge.pop[2]) >= 2 and np.all(obs.state_populations(25) > 0) and obs.n_states(25) == 2
    # what a user reads off
    assert obs.state_populations(25).sum() == pytest.approx(1.0) and obs.n_states(3) == 1 and obs.state_populations(3).tolist() == [1.0]
    assert 0.5 < obs.mean_magmom(25) < 1.5 and 0 < obs.magmom_std(25) < 0.5
    assert obs.transition_counts(25).sum() == 2 * 4 and np.isfinite(obs.transition_rate(25, 0, 0))
    assert obs.state_persistence(25, 0)[0] == 1.0 and np.all(obs.magmom_correlation(25) > 0)
    assert np.allclose(np.nansum(obs.site_occupancy(), axis=1), 1.0) and obs.site_occupancy().shape == (8, Q)
    assert obs.magmom_histogram(25).sum() * (2.0 / 64) == pytest.approx(1.0)
    q_on = int(np.flatnonzero(obs.charge.pop[2])[0])
    g = obs.state_rdf(q_on, 8)
    assert g.shape == (48,) and np.all(g[:10] == 0) and g.max() > 1.0           # no oxygen within 1 A of Mn, a first shell further out
    md.close()


def test_run_batch_gives_every_replica_the_sums_of_its_own_frames(calc):
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.observables import MDObservers

    structs = [_structure("limno2", seed=1), _structure("noangle", seed=2)]      # Li Mn O and Cl Cs: one species map of five
    kinds = [3, 8, 17, 25, 55]
    m1, z1 = _oracle_moments("limno2", 1), np.asarray(structs[0].atomic_numbers)
    m2 = _oracle_moments("noangle", 2)
    cs_cl = 0.5 * float(m2[0] + m2[1])                                           # between the Cs and the Cl moment
    ob = MDObservers(sample_interval=1, msd_lags=3, magmom_states={25: [_split(m1[z1 == 25])], 8: [_split(m1[z1 == 8])], 55: [cs_cl], 17: [cs_cl]},
                     magmom_bins=32, magmom_max=1.2, state_rdf_center=25, state_rdf_bins=24, state_rdf_rmax=4.0)
    kw = {"model": calc, "ensemble": "nvt", "thermostat": "Berendsen", "temperature": 800, "starting_temperature": 800, "timestep": 2.0,
          "loginterval": 1}
    out = MolecularDynamics.run_batch(structs, 4, seeds=[3, 4], observers=ob, log_magmoms=True, **kw)
    cp, bounds = ob.charge_params(kinds)
    for s, res in zip(structs, out):
        obs = res["observables"]
        assert obs.species.tolist() == kinds
        z = np.asarray(s.atomic_numbers)
        index = np.searchsorted(kinds, z).astype(np.int32)
        want = _restate(res["trajectory"], index, 5, [0, 1, 2, 3, 4], ob, cp, bounds)
        assert want["cnt"][0].tolist() == [5, 4, 3]
        _assert_replica(obs, want, f"{len(z)} atoms")
        assert np.array_equal(res["magmoms"], res["trajectory"].magmoms[-1])
        absent = [k for k in range(5) if kinds[k] not in z]
        assert absent and np.all(obs.charge.pop[absent] == 0) and np.all(obs.charge.mcorr[:, absent] == 0)
        if 25 in z:
            assert np.count_nonzero(obs.charge.pop[3]) >= 2 and obs.charge.shist.sum() > 0
        else:
            assert obs.charge.shist.sum() == 0                                   # no centre atom in this replica
            assert obs.charge.pop[4, 1] == 5 and obs.charge.pop[2, 0] == 5       # Cs above, Cl below their common boundary


# ---- 6. the old keywords --------------------------------------------------------------------------------------------------------------------
def _parent_kernels_on_frames(eng, ob, S, species_index, masses, traj, steps) -> dict:
    """chg_test_md_observe -- the plain observers alone -- on the frames a run sampled."""
    from chgnet_amd import _lib
    from chgnet_amd.observables import empty_arrays

    at = [traj.steps.index(s) for s in steps]
    pos = np.ascontiguousarray(np.stack([traj.atom_positions[k] for k in at]), np.float64)
    mom = np.ascontiguousarray(np.stack([traj.momenta[k] for k in at]), np.float64)
    cells = np.ascontiguousarray(np.stack([traj.cells[k] for k in at])[:, None], np.float64)
    n = pos.shape[1]
    p = ob.params(S)
    d = empty_arrays(1, ob.msd_lags, S, ob.rdf_bins)
    out = _lib.fill_out(_lib.MdObservablesHost(), d)
    dp = ctypes.POINTER(ctypes.c_double)
    aoff, sp, status = np.array([0, n], np.int32), np.ascontiguousarray(species_index, np.int32), np.zeros((len(at), 1), np.int32)
    m = np.ascontiguousarray(masses, np.float64)
    rc = eng.lib.chg_test_md_observe(eng.handle, ctypes.byref(p), 1, aoff.ctypes.data_as(_lib.c_int_p), sp.ctypes.data_as(_lib.c_int_p),
                                     m.ctypes.data_as(dp), len(at), pos.ctypes.data_as(dp), mom.ctypes.data_as(dp), cells.ctypes.data_as(dp),
                                     status.ctypes.data_as(_lib.c_int_p), ctypes.byref(out))
    assert rc == 0, eng.lib.chg_last_error(eng.handle)
    return d


def test_old_keywords_never_reach_the_new_entry_points_and_charge_states_leave_the_plain_sums_alone(calc, monkeypatch):
    """Two runs from one seed are not the same trajectory on this engine (DESIGN.md 7b "Reproducibility"), so what the charge states must
    not change is checked where it can be checked exactly: the plain sums of the run WITH charge states must be bit for bit what the
    plain observers' kernels alone -- chg_test_md_observe -- give on the frames that run sampled."""
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.observables import MDObservers

    eng = calc.model.engine
    calls = {"chg_md_set_charge_states": [], "chg_md_set_magmoms": []}
    for name, log in calls.items():
        real = getattr(eng.lib, name)
        monkeypatch.setattr(eng.lib, name, lambda *args, _real=real, _log=log: (_log.append(args), _real(*args))[1])
    old = {"sample_interval": 2, "msd_lags": 4, "rdf_rmax": 6.0, "rdf_bins": 64, "collective": True}
    new = {"magmom_states": {"Mn": [0.95]}, "magmom_bins": 16, "magmom_max": 2.0, "state_rdf_center": "Mn", "state_rdf_bins": 16, "state_rdf_rmax": 4.0}
    runs = {}
    for name, extra in (("plain", {}), ("charge", new)):
        ob = MDObservers(**old, **extra)
        md = MolecularDynamics(_structure("limno2"), model=calc, ensemble="nvt", thermostat="Nose-Hoover-Chain", temperature=1000,
                               starting_temperature=1000, timestep=2.0, loginterval=1, seed=11, observers=ob)
        md.run(8)
        obs = md.observables
        alone = _parent_kernels_on_frames(eng, ob, 3, md._run.species_index, md._masses, md.traj, [0, 2, 4, 6, 8])
        assert md.traj.magmoms == []                                             # charge states alone log no moments
        md.close()
        assert len(calls["chg_md_set_charge_states"]) == (1 if name == "charge" else 0), name     # the old keywords never reach the new entry point
        assert calls["chg_md_set_magmoms"] == []                                  # implied inside the library, never called from Python
        for key, mine in (("msd", obs.msd_sum), ("vacf", obs.vacf_sum), ("cnt", obs.cnt), ("rdf", obs.rdf_hist)):
            assert np.array_equal(mine, alone[key][0]), (name, key)               # bit for bit, with and without charge states
        assert obs.rdf_samples == alone["rdf_samples"][0] == 5 and obs.vol_sum == alone["vol_sum"][0]
        runs[name] = obs
    a, b = runs["plain"], runs["charge"]
    assert a.charge is None and b.charge is not None and b.charge.samples == 5 and b.charge.pop[2].sum() == 10
    assert b.charge.vol_sum == b.vol_sum and np.array_equal(a.cnt, b.cnt) and a.cmsd_sum is not None and b.cmsd_sum is not None
