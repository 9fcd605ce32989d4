"""MD observables on the MI355X against the float64 restatement (tests/md_observe_ref.py): the kernels alone on caller-given
snapshots (ring wrap, species absent from a replica, a stopped replica, one atom, more atoms than one pass of a workgroup), the pair
histogram exactly on hard cells, the sampling point of a real run (its own frames are the truth: split runs, the two-evaluation NPT
loop, the private frame slot), run_batch, and the refusals.

Tolerance of the sums: ``1e-12 * sum|terms|`` with the sum of absolute values from the restatement -- a bound on the float64
reordering of at most 300 x 7 terms (2100 x 2^-53 = 2.3e-13), not a measured figure.  Histograms are integers and must be equal."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import md_observe_ref as ref
from conftest import load_case
from md_hard_cells import BINS, HARD, RMAX, hard_batch as _hard

pytestmark = pytest.mark.gpu

REL = 1e-12


def _observe(eng, params: dict, aoff, species, masses, positions, momenta, cells, status):
    """chg_test_md_observe -> (rc, raw arrays)."""
    from chgnet_amd import _lib
    from chgnet_amd.observables import empty_arrays

    B, T = len(aoff) - 1, len(positions)
    p = _lib.MdObserveParams(**{"sample_interval": 1, "n_lags": 0, "subtract_com": 1, "n_species": 1, "rdf_bins": 0, "reserved": 0,
                                "rdf_rmax": 0.0, **params})
    d = empty_arrays(B, max(p.n_lags, 0), max(p.n_species, 1), max(p.rdf_bins, 0))
    out = _lib.fill_out(_lib.MdObservablesHost(), d)
    dp = ctypes.POINTER(ctypes.c_double)
    arr = [np.ascontiguousarray(x, np.float64) for x in (masses, positions, momenta, cells)]
    ints = [np.ascontiguousarray(x, np.int32) for x in (aoff, species, status)]
    rc = eng.lib.chg_test_md_observe(eng.handle, ctypes.byref(p), B, ints[0].ctypes.data_as(_lib.c_int_p), ints[1].ctypes.data_as(_lib.c_int_p),
                                     arr[0].ctypes.data_as(dp), T, arr[1].ctypes.data_as(dp), arr[2].ctypes.data_as(dp),
                                     arr[3].ctypes.data_as(dp), ints[2].ctypes.data_as(_lib.c_int_p), ctypes.byref(out))
    return rc, d


def _assert_sums(got: dict, want: dict, where=""):
    assert np.array_equal(got["cnt"], want["cnt"]), where
    for name in ("msd", "vacf"):
        err, bound = np.abs(got[name] - want[name]), REL * want[name + "_abs"]
        print(f"{where} {name}: max |device - restatement| / sum|terms| = {np.max(err / np.maximum(want[name + '_abs'], 1e-300)):.2e}")
        assert np.all(err <= bound), (where, name, float(np.max(err - bound)))


# ---- 1. the kernels alone: ring, species, status ------------------------------------------------------------------------------------
SIZES = [1, 5, 17, 300, 40]            # 300: more than one pass of a 256-thread workgroup; 1: nothing moves in its own frame
STOPPED, STOP_AT = 1, 3                # replica 1 is non-finite from sample 3 on


@functools.lru_cache(maxsize=None)
def _walk():
    """7 snapshots of five replicas, S = 3 (species 2 absent from replica 2), and the restatement for both frames of reference."""
    rng = np.random.default_rng(7)
    T, S, L = 7, 3, 4
    aoff = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    N = int(aoff[-1])
    species = rng.integers(0, S, N).astype(np.int32)
    species[aoff[2]:aoff[3]] = rng.integers(0, 2, SIZES[2])
    masses = rng.uniform(1.0, 200.0, N)
    pos = np.empty((T, N, 3))
    pos[0] = rng.uniform(-3.0, 12.0, (N, 3))
    for k in range(1, T):
        pos[k] = pos[k - 1] + rng.normal(0, 0.3, (N, 3)) + np.array([0.05, -0.02, 0.01])      # a walk on a common drift
    mom = rng.normal(0, 0.3, (T, N, 3)) * np.sqrt(masses)[None, :, None]
    cells = np.tile(np.eye(3) * 10.0, (T, len(SIZES), 1, 1))
    status = np.zeros((T, len(SIZES)), np.int32)
    status[STOP_AT:, STOPPED] = 1
    want = {sub: ref.correlations(pos, mom, status, aoff, species, masses, S, L, sub) for sub in (False, True)}
    return aoff, species, masses, pos, mom, cells, status, S, L, want


@pytest.mark.parametrize("subtract_com", [False, True])
def test_msd_and_vacf_kernels_match_the_restatement(hip_engine, subtract_com):
    aoff, species, masses, pos, mom, cells, status, S, L, want = _walk()
    rc, got = _observe(hip_engine, {"n_lags": L, "n_species": S, "subtract_com": int(subtract_com)}, aoff, species, masses, pos, mom, cells, status)
    assert rc == 0, hip_engine.lib.chg_last_error(hip_engine.handle)
    w = want[subtract_com]
    _assert_sums(got, w, f"subtract_com={subtract_com}")
    assert w["cnt"][0].tolist() == [7, 6, 5, 4] and w["cnt"][STOPPED].tolist() == [3, 2, 1, 0]      # ring wrapped; stopped for good
    assert np.all(got["msd"][2, :, 2] == 0) and np.all(got["vacf"][2, :, 2] == 0)                   # the absent species
    if subtract_com:
        assert np.all(got["msd"][0] == 0.0)                                                         # one atom: it IS the centre of mass
    else:
        assert got["msd"][0, 1, species[0]] > 0.1


# ---- 2. the pair histogram on hard cells: exact ------------------------------------------------------------------------------------
def test_pair_histogram_is_exact_on_hard_cells(hip_engine):
    aoff, species, S, pos, cells, status, want = _hard()
    rc, got = _observe(hip_engine, {"n_species": S, "rdf_bins": BINS, "rdf_rmax": RMAX}, aoff, species, np.ones(aoff[-1]), pos,
                       np.zeros_like(pos), cells, status)
    assert rc == 0, hip_engine.lib.chg_last_error(hip_engine.handle)
    for o, name in enumerate(HARD):
        assert np.array_equal(got["rdf"][o], want["rdf"][o]), name
    assert np.array_equal(got["rdf_samples"], want["rdf_samples"]) and want["rdf_samples"].tolist().count(1) == 1
    assert np.allclose(got["vol_sum"], want["vol_sum"], rtol=1e-14, atol=0)
    assert want["rdf"][HARD.index("thin_cube16")].sum() > 100                    # one atom: nothing but its own images
    assert want["rdf"].sum() > 5000


# ---- 3. end to end: the sampling point -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def calc(trained_like_weights):
    from chgnet_amd import CHGNet
    from chgnet_amd.calculator import CHGNetCalculator

    return CHGNetCalculator(model=CHGNet(state_dict=trained_like_weights))


def _structure(name, rattle=0.02, seed=0):
    from chgnet_amd.graph.structure import Lattice, Structure

    _, d = load_case(name)
    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"])
    cart = s.frac_coords @ s.lattice.matrix + rattle * np.random.default_rng(seed).normal(size=(len(s), 3))
    return Structure(s.lattice, s.atomic_numbers, cart @ np.linalg.inv(s.lattice.matrix))


def _restate(traj, masses, species_index, S, steps, L, bins, rmax, subtract_com=True):
    """The observables of one replica recomputed from its own frames at ``steps``."""
    at = [traj.steps.index(s) for s in steps]
    pos = np.stack([traj.atom_positions[k] for k in at])
    mom = np.stack([traj.momenta[k] for k in at])
    cells = np.stack([traj.cells[k] for k in at])[:, None]
    n, status = pos.shape[1], np.zeros((len(at), 1), np.int32)
    out = ref.correlations(pos, mom, status, np.array([0, n]), species_index, masses, S, L, subtract_com) if L else {}
    if bins:
        try:
            out.update(ref.pair_histogram(pos, cells, status, np.array([0, n]), species_index, S, bins, rmax))
        except AssertionError as exc:           # a frame put a distance within 1e-9 A of a bin edge: the histogram has no exact truth
            assert "bin edge" in str(exc)
            print("edge guard:", exc)
    return out


def _assert_replica(obs, want, where):
    _assert_sums({"msd": obs.msd_sum[None], "vacf": obs.vacf_sum[None], "cnt": obs.cnt[None]}, want, where)
    if "rdf" in want:
        assert np.array_equal(obs.rdf_hist, want["rdf"][0]), where
        assert obs.rdf_samples == want["rdf_samples"][0]
        assert obs.vol_sum == pytest.approx(want["vol_sum"][0], rel=1e-14)


NPT = {"ensemble": "npt", "bulk_modulus": 100.0, "taup": 50.0}
SAMPLED = [
    pytest.param({"ensemble": "nvt", "thermostat": "Nose-Hoover-Chain"}, id="nvt_nhc"),
    # the two-evaluation Berendsen NPT loop, in both of its forms (ensemble="npt" has no thermostat called plain "Berendsen")
    pytest.param({**NPT, "thermostat": "Berendsen_inhomogeneous"}, id="npt_berendsen_inhomogeneous"),
    pytest.param({**NPT, "thermostat": "npt_berendsen"}, id="npt_berendsen"),
]


@pytest.mark.parametrize("kw", SAMPLED)
def test_a_run_samples_completed_steps_across_split_runs(calc, kw):
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.observables import MDObservers

    ob = MDObservers(sample_interval=2, msd_lags=4, rdf_rmax=6.0, rdf_bins=64)
    md = MolecularDynamics(_structure("limno2"), model=calc, temperature=1000, starting_temperature=1000, timestep=2.0, loginterval=1,
                           seed=11, observers=ob, **kw)
    md.run(3)
    md.run(5)
    obs = md.observables
    assert md.traj.steps == list(range(9)) and obs.species.tolist() == [3, 8, 25]
    assert obs.sample_dt_fs == 4.0 and obs.lag_times_fs.tolist() == [0.0, 4.0, 8.0, 12.0]
    run = md._run
    want = _restate(md.traj, md._masses, run.species_index, 3, [0, 2, 4, 6, 8], 4, 64, 6.0)
    assert want["cnt"][0].tolist() == [5, 4, 3, 2]
    _assert_replica(obs, want, kw["thermostat"])
    if kw["ensemble"] == "npt":                 # the cell moved, so vol_sum is no multiple of one volume
        vols = [abs(np.linalg.det(c)) for c in md.traj.cells]
        assert max(vols) - min(vols) > 1e-6 * vols[0]
    assert np.all(np.isfinite(obs.msd(3))) and obs.msd(3)[0] == 0.0 and obs.msd(3)[1] > 0.0
    assert obs.vacf(8, normalized=True)[0] == 1.0
    assert np.isfinite(obs.rdf(3, 8)).all() and obs.coordination_number(25, 8, 3.0) > 0
    md.close()


def test_a_sample_between_two_frames_goes_through_the_private_slot(calc):
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.observables import MDObservers

    ob = MDObservers(sample_interval=2, msd_lags=3, rdf_rmax=6.0, rdf_bins=64)
    md = MolecularDynamics(_structure("limno2"), model=calc, ensemble="nvt", thermostat="Nose-Hoover-Chain", temperature=1000,
                           starting_temperature=1000, timestep=2.0, loginterval=4, seed=12, observers=ob)
    md.run(4)
    obs = md.observables
    assert md.traj.steps == [0, 4]                                               # step 2 was sampled and not logged
    assert obs.cnt.tolist() == [3, 2, 1] and obs.rdf_samples == 3
    want = _restate(md.traj, md._masses, md._run.species_index, 3, [0, 4], 2, 0, 0.0)
    for name, mine in (("msd", obs.msd_sum), ("vacf", obs.vacf_sum)):
        assert np.all(np.abs(mine[2] - want[name][0, 1]) <= REL * want[name + "_abs"][0, 1]), name
    assert np.all(obs.msd_sum[2] > 0) and np.all(obs.msd_sum[1] > 0)
    md.close()


# ---- 4. run_batch ------------------------------------------------------------------------------------------------------------------
def test_run_batch_observes_every_replica_on_its_own(calc):
    from chgnet_amd.dynamics import ATOMIC_MASSES, MolecularDynamics
    from chgnet_amd.observables import MDObservers

    structs = [_structure("limno2", seed=1), _structure("noangle", seed=2)]      # Li Mn O and Cl Cs: one species map of five
    kw = {"model": calc, "ensemble": "nvt", "thermostat": "Berendsen", "temperature": 800, "starting_temperature": 800, "timestep": 2.0,
          "loginterval": 1}
    out = MolecularDynamics.run_batch(structs, 4, seeds=[3, 4], observers=MDObservers(msd_lags=3, rdf_rmax=6.0, rdf_bins=32), **kw)
    kinds = [3, 8, 17, 25, 55]
    for s, res in zip(structs, out):
        obs = res["observables"]
        assert obs.species.tolist() == kinds
        z = np.asarray(s.atomic_numbers)
        index = np.searchsorted(kinds, z).astype(np.int32)
        assert obs.n_per_species.tolist() == np.bincount(index, minlength=5).tolist()
        want = _restate(res["trajectory"], ATOMIC_MASSES[z], index, 5, [0, 1, 2, 3, 4], 3, 32, 6.0)
        assert want["cnt"][0].tolist() == [5, 4, 3]
        _assert_replica(obs, want, f"{len(z)} atoms")
    plain = MolecularDynamics.run_batch(structs, 1, seeds=[3, 4], **kw)
    assert all("observables" not in res for res in plain)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def _refused(eng, rc, text):
    assert rc == -1                                                              # CHG_EINVAL
    assert text in eng.lib.chg_last_error(eng.handle).decode()


def test_refusals(hip_engine, calc):
    from chgnet_amd import _lib
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.observables import MDObservers

    aoff, n = np.array([0, 3], np.int32), 3
    snap = (np.ones(n), np.zeros((1, n, 3)), np.zeros((1, n, 3)), np.eye(3)[None, None] * 5.0, np.zeros((1, 1), np.int32))
    rc, _ = _observe(hip_engine, {"n_lags": 2, "n_species": 2}, aoff, [0, 2, 1], *snap)
    _refused(hip_engine, rc, "species index 2 of atom 1")
    rc, _ = _observe(hip_engine, {"n_species": 8, "rdf_bins": 257, "rdf_rmax": 5.0}, aoff, [0, 1, 7], *snap)
    _refused(hip_engine, rc, "16384")
    rc, _ = _observe(hip_engine, {"n_lags": 4097}, aoff, [0, 0, 0], *snap)
    _refused(hip_engine, rc, "n_lags must be 0..4096")
    rc, _ = _observe(hip_engine, {"n_lags": 2, "sample_interval": 0}, aoff, [0, 0, 0], *snap)
    _refused(hip_engine, rc, "sample_interval")
    rc, _ = _observe(hip_engine, {"n_species": 8, "rdf_bins": 256, "rdf_rmax": 5.0}, aoff, [0, 1, 7], *snap)      # the limit itself: 64 KB of LDS
    assert rc == 0, hip_engine.lib.chg_last_error(hip_engine.handle)

    md = MolecularDynamics(_structure("limno2"), model=calc, ensemble="nve", starting_temperature=300, loginterval=1, seed=1)
    md.run(1)
    eng, run = md._run.eng, md._run
    ob = MDObservers(msd_lags=2)
    p = ob.params(1)
    rc = eng.lib.chg_md_set_observers(eng.handle, run.handle, ctypes.byref(p), np.zeros(run.N, np.int32).ctypes.data_as(_lib.c_int_p))
    _refused(eng, rc, "already started")
    out = _lib.MdObservablesHost()
    _refused(eng, eng.lib.chg_md_download_observables(eng.handle, run.handle, ctypes.byref(out)), "no observers")
    with pytest.raises(ValueError, match="no observers"):
        md.observables
    md.close()
