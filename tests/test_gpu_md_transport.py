"""Transport observables on the MI355X against the float64 restatement (tests/md_transport_ref.py): the kernels alone on caller-given
snapshots (ring wrap, a species absent from a replica, a stopped replica, one atom, more atoms than one pass of a workgroup), bit-wise
determinism, the limits and refusals of the C interface, and real runs whose own frames are the truth.

Tolerance of the float sums: ``1e-12 * sum|terms|`` with the sum of absolute values from the restatement, the bound the plain
observers' test uses for the MSD and VACF: a bound on the float64 reordering of at most 300 x 7 terms (2100 x 2^-53 = 2.3e-13), not a
measured figure.  Histograms and sample counts are integers and must be equal."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import md_observe_ref as plain_ref
import md_transport_ref as ref
from conftest import load_case

pytestmark = pytest.mark.gpu

REL = 1e-12
EINVAL = -1


def _transport(eng, observe: dict, transport: dict, aoff, species, masses, positions, momenta, cells, status):
    """chg_test_md_transport -> (rc, plain sums, transport sums)."""
    from chgnet_amd import _lib
    from chgnet_amd.observables import empty_arrays, empty_transport_arrays

    B, T = len(aoff) - 1, len(positions)
    p = _lib.MdObserveParams(**{"sample_interval": 1, "n_lags": 0, "subtract_com": 1, "n_species": 1, "rdf_bins": 0, "reserved": 0,
                                "rdf_rmax": 0.0, **observe})
    t = _lib.MdTransportParams(**{"collective": 0, "non_gaussian": 0, "vh_bins": 0, "vh_lags": 0, "vh_stride": 1, "reserved": 0,
                                  "vh_rmax": 0.0, **transport})
    d = empty_arrays(B, max(p.n_lags, 0), max(p.n_species, 1), max(p.rdf_bins, 0))
    dt = empty_transport_arrays(B, max(p.n_lags, 0), max(p.n_species, 1), max(t.vh_lags, 0), max(t.vh_bins, 0))
    out, tout = _lib.fill_out(_lib.MdObservablesHost(), d), _lib.fill_out(_lib.MdTransportHost(), dt)
    dp = ctypes.POINTER(ctypes.c_double)
    arr = [np.ascontiguousarray(x, np.float64) for x in (masses, positions, momenta, cells)]
    ints = [np.ascontiguousarray(x, np.int32) for x in (aoff, species, status)]
    rc = eng.lib.chg_test_md_transport(eng.handle, ctypes.byref(p), ctypes.byref(t), B, ints[0].ctypes.data_as(_lib.c_int_p),
                                       ints[1].ctypes.data_as(_lib.c_int_p), arr[0].ctypes.data_as(dp), T, arr[1].ctypes.data_as(dp),
                                       arr[2].ctypes.data_as(dp), arr[3].ctypes.data_as(dp), ints[2].ctypes.data_as(_lib.c_int_p),
                                       ctypes.byref(out), ctypes.byref(tout))
    return rc, d, dt


def _assert_sums(got: dict, want: dict, where=""):
    for name in ("msd4", "cmsd", "jacf"):
        err, bound = np.abs(got[name] - want[name]), REL * want[name + "_abs"]
        print(f"{where} {name}: max |device - restatement| / sum|terms| = {np.max(err / np.maximum(want[name + '_abs'], 1e-300)):.2e}")
        assert np.all(err <= bound), (where, name, float(np.max(err - bound)))


# ---- 1. the kernels alone: ring, species, status ------------------------------------------------------------------------------------
SIZES = [1, 5, 17, 300, 40]            # 300: more than one pass of a 256-thread workgroup; 1: it is its own centre of mass
STOPPED, STOP_AT = 1, 3                # replica 1 is non-finite from sample 3 on
WALK_SEED = 7                          # chosen on the CPU: the restatement's edge guard passes for both histograms and both frames of reference
VH = {"stride2": {"vh_bins": 32, "vh_rmax": 2.0, "vh_stride": 2, "vh_lags": 2},
      "stride1": {"vh_bins": 32, "vh_rmax": 2.0, "vh_stride": 1, "vh_lags": 3}}
T_WALK, S_WALK, L_WALK = 7, 3, 4       # the ring of 4 wraps


@functools.lru_cache(maxsize=None)
def _walk():
    """7 snapshots of five replicas, S = 3 (species 2 absent from replica 2): the walk of the plain observers' test."""
    rng = np.random.default_rng(WALK_SEED)
    T, S = T_WALK, S_WALK
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
    return aoff, species, masses, pos, mom, cells, status


@functools.lru_cache(maxsize=None)
def _want(subtract_com: bool, vh: str) -> dict:
    """The restatement, computed once per case (its edge guard asserts inside)."""
    aoff, species, masses, pos, mom, cells, status = _walk()
    return ref.transport(pos, mom, cells, status, aoff, species, masses, S_WALK, L_WALK, subtract_com, **VH[vh])


def _run_walk(eng, subtract_com: bool, vh: str, samples: int = T_WALK):
    aoff, species, masses, pos, mom, cells, status = _walk()
    rc, plain, got = _transport(eng, {"n_lags": L_WALK, "n_species": S_WALK, "subtract_com": int(subtract_com)},
                                {"collective": 1, "non_gaussian": 1, **VH[vh]}, aoff, species, masses, pos[:samples], mom[:samples],
                                cells[:samples], status[:samples])
    assert rc == 0, eng.lib.chg_last_error(eng.handle)
    return plain, got


@pytest.mark.parametrize("vh", list(VH))
@pytest.mark.parametrize("subtract_com", [False, True])
def test_transport_kernels_match_the_restatement(hip_engine, subtract_com, vh):
    aoff, species, *_ = _walk()
    want = _want(subtract_com, vh)
    plain, got = _run_walk(hip_engine, subtract_com, vh)
    _assert_sums(got, want, f"subtract_com={subtract_com} {vh}")
    assert np.array_equal(got["vh"], want["vh"])                                                    # integers: exactly
    assert np.array_equal(got["samples"], want["samples"]) and got["samples"].tolist() == [7, 3, 7, 7, 7]
    assert np.array_equal(plain["cnt"], want["cnt"])
    assert plain["cnt"][0].tolist() == [7, 6, 5, 4] and plain["cnt"][STOPPED].tolist() == [3, 2, 1, 0]   # ring wrapped; stopped for good
    assert np.allclose(got["vol_sum"], want["vol_sum"], rtol=1e-14, atol=0)
    # the species absent from replica 2 owns nothing
    assert np.all(got["msd4"][2, :, 2] == 0) and np.all(got["vh"][2, :, 2] == 0)
    for name in ("cmsd", "jacf"):
        assert np.all(got[name][2, :, 2, :] == 0) and np.all(got[name][2, :, :, 2] == 0), name
    assert np.array_equal(got["cmsd"], got["cmsd"].transpose(0, 1, 3, 2))                           # symmetric bit for bit
    assert not np.array_equal(got["jacf"], got["jacf"].transpose(0, 1, 3, 2))                       # J_a(k) . J_b(k - l) is not
    lag0 = got["vh"][:, 0].sum(axis=(1, 2))
    assert lag0.tolist() == [n * k for n, k in zip(SIZES, got["samples"])] and np.all(got["vh"][:, 0, :, 1:] == 0)   # lag 0: all in bin 0
    assert want["vh"][3, 1].sum() > 1000 and np.count_nonzero(want["vh"][3, 1]) > 10                # the histogram is spread out
    if subtract_com:
        assert np.all(got["msd4"][0] == 0.0) and np.all(got["cmsd"][0] == 0.0)                      # one atom: it IS the centre of mass
        assert got["vh"][0].sum() == got["vh"][0, :, species[0], 0].sum() > 0                       # and all of it is in bin 0
    else:
        assert got["msd4"][0, 1, species[0]] > 1e-4
    # the stopped replica's cells are those of a run that ended at its last sample
    _, early = _run_walk(hip_engine, subtract_com, vh, samples=STOP_AT)
    for name in ("msd4", "cmsd", "jacf", "vh", "samples", "vol_sum"):
        assert np.array_equal(got[name][STOPPED], early[name][STOPPED]), name
    assert got["samples"][STOPPED] == STOP_AT


# ---- 2. determinism -----------------------------------------------------------------------------------------------------------------
def test_two_runs_of_the_same_input_give_the_same_bits(hip_engine):
    first_plain, first = _run_walk(hip_engine, True, "stride1")
    again_plain, again = _run_walk(hip_engine, True, "stride1")
    for name in first:
        assert np.array_equal(first[name], again[name]), name
    for name in first_plain:
        assert np.array_equal(first_plain[name], again_plain[name]), name
    assert np.abs(first["cmsd"]).sum() > 0 and np.abs(first["jacf"]).sum() > 0 and first["msd4"].sum() > 0


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
    from chgnet_amd.observables import MDObservers, empty_transport_arrays

    n = 9
    aoff = np.array([0, n], np.int32)
    species = np.array([0, 1, 2, 3, 4, 5, 6, 7, 7], np.int32)
    rng = np.random.default_rng(0)
    pos = np.cumsum(rng.normal(0, 0.2, (3, n, 3)), axis=0)
    snap = (aoff, species, np.ones(n), pos, np.zeros_like(pos), np.tile(np.eye(3) * 5.0, (3, 1, 1, 1)), np.zeros((3, 1), np.int32))
    ring = {"n_lags": 3, "n_species": 8}
    vh = {"vh_rmax": 2.0, "vh_lags": 2, "vh_stride": 1}
    rc, _, got = _transport(hip_engine, ring, {**vh, "vh_bins": 512}, *snap)                   # S * vh_bins = 4096: the LDS limit itself
    assert rc == 0, hip_engine.lib.chg_last_error(hip_engine.handle)
    assert got["vh"][0, 0, :, 0].tolist() == [3, 3, 3, 3, 3, 3, 3, 6] and got["vh"][0, 0].sum() == 3 * n
    inside = int((np.linalg.norm(pos[1:] - pos[:-1], axis=2) < 2.0).sum())
    assert got["vh"][0, 1].sum() == inside > 0 and got["vh"][0, 1, 7, 511] == 0
    assert np.all(got["msd4"] == 0) and np.all(got["cmsd"] == 0)                               # not requested: left alone
    for t, text in (({**vh, "vh_bins": 513}, "n_species * vh_bins must be <= 4096"),
                    ({}, "nothing requested"),
                    ({"vh_bins": -1}, "vh_bins must be >= 0"),
                    ({**vh, "vh_bins": 8, "vh_rmax": 0.0}, "vh_rmax must be > 0 and finite"),
                    ({**vh, "vh_bins": 8, "vh_rmax": float("nan")}, "vh_rmax must be > 0 and finite"),
                    ({**vh, "vh_bins": 8, "vh_rmax": float("inf")}, "vh_rmax must be > 0 and finite"),
                    ({**vh, "vh_bins": 8, "vh_stride": 0}, "vh_stride must be >= 1"),
                    ({**vh, "vh_bins": 8, "vh_lags": 0}, "vh_lags must be >= 1"),
                    ({**vh, "vh_bins": 8, "vh_lags": 4}, "(vh_lags - 1) * vh_stride must be < n_lags"),
                    ({**vh, "vh_bins": 8, "vh_lags": 2, "vh_stride": 3}, "(vh_lags - 1) * vh_stride must be < n_lags")):
        rc, _, _ = _transport(hip_engine, ring, t, *snap)
        _refused(hip_engine, rc, text)
    rc, _, _ = _transport(hip_engine, {"n_species": 8, "rdf_bins": 8, "rdf_rmax": 3.0}, {"collective": 1}, *snap)      # observers, but no ring
    _refused(hip_engine, rc, "n_lags > 0")
    rc, _, got = _transport(hip_engine, ring, {**vh, "vh_bins": 8, "vh_lags": 3}, *snap)       # (3 - 1) * 1 < 3: the last lag of the ring
    assert rc == 0 and got["vh"][0, 2].sum() > 0

    md = MolecularDynamics(_structure("limno2"), model=calc, ensemble="nve", starting_temperature=300, loginterval=1, seed=1)
    run = _DeviceRun(md.calculator, [md._structure], md._masses, md._momenta, md.kind, md.cfg, seeds=[md.thermostat_seed], fixed=[md._fixed])
    eng = run.eng                                                                # a handle that has not run yet
    tp = MDObservers(msd_lags=2, collective=True).transport_params(1)
    _refused(eng, eng.lib.chg_md_set_transport(eng.handle, run.handle, ctypes.byref(tp)), "needs observers")
    out = _lib.MdTransportHost()
    _refused(eng, eng.lib.chg_md_download_transport(eng.handle, run.handle, ctypes.byref(out)), "no transport")
    p = MDObservers(msd_lags=2).params(1)
    assert eng.lib.chg_md_set_observers(eng.handle, run.handle, ctypes.byref(p), np.zeros(run.N, np.int32).ctypes.data_as(_lib.c_int_p)) == 0
    _refused(eng, eng.lib.chg_md_download_transport(eng.handle, run.handle, ctypes.byref(out)), "no transport")      # observers without transport
    assert eng.lib.chg_md_set_transport(eng.handle, run.handle, ctypes.byref(tp)) == 0           # valid before the first run, twice too
    assert eng.lib.chg_md_set_transport(eng.handle, run.handle, ctypes.byref(tp)) == 0
    assert eng.lib.chg_md_run(eng.handle, run.handle, 1) == 0, eng.lib.chg_last_error(eng.handle)
    _refused(eng, eng.lib.chg_md_set_transport(eng.handle, run.handle, ctypes.byref(tp)), "already started")
    d = empty_transport_arrays(1, 2, 1, 0, 0)
    assert eng.lib.chg_md_download_transport(eng.handle, run.handle, ctypes.byref(_lib.fill_out(out, d))) == 0
    assert d["samples"].tolist() == [2] and d["cmsd"][0, 0, 0, 0] == 0.0 and d["cmsd"][0, 1, 0, 0] > 0.0
    run.free()
    md.close()


# ---- 4. end to end: the frames of a run are the truth ---------------------------------------------------------------------------------
E2E = {"sample_interval": 2, "msd_lags": 4, "collective": True, "non_gaussian": True, "vanhove_bins": 32, "vanhove_rmax": 0.4, "vanhove_stride": 2}


def _restate(traj, masses, species_index, S, steps, ob):
    """The transport sums of one replica recomputed from its own frames at ``steps`` (edge guard off: doubtful bins are marked)."""
    at = [traj.steps.index(s) for s in steps]
    pos = np.stack([traj.atom_positions[k] for k in at])
    mom = np.stack([traj.momenta[k] for k in at])
    cells = np.stack([traj.cells[k] for k in at])[:, None]
    n, status = pos.shape[1], np.zeros((len(at), 1), np.int32)
    want = ref.transport(pos, mom, cells, status, np.array([0, n]), species_index, masses, S, ob.msd_lags, ob.subtract_com,
                         vh_bins=ob.vanhove_bins, vh_rmax=ob.vanhove_rmax, vh_lags=ob.vanhove_lags, vh_stride=ob.vanhove_stride, guard=False)
    want.update(plain_ref.correlations(pos, mom, status, np.array([0, n]), species_index, masses, S, ob.msd_lags, ob.subtract_com))
    return want


def _assert_replica(obs, want, where):
    got = {"msd4": obs.msd4_sum[None], "cmsd": obs.cmsd_sum[None], "jacf": obs.jacf_sum[None]}
    _assert_sums(got, want, where)
    assert np.array_equal(obs.cnt, want["cnt"][0]), where
    for name, mine in (("msd", obs.msd_sum), ("vacf", obs.vacf_sum)):
        assert np.all(np.abs(mine - want[name][0]) <= REL * want[name + "_abs"][0]), (where, name)
    doubt = want["vh_doubt"][0]
    assert np.all(doubt.sum(axis=2) <= 2), where               # a frame within 1e-9 A of an edge costs at most 2 bins per lag and species
    if doubt.any():
        print(f"{where}: edge guard, {int(doubt.sum())} bins left out")
    assert np.array_equal(obs.vanhove_hist[~doubt], want["vh"][0][~doubt]), where
    assert obs.transport_samples == want["samples"][0]
    assert obs.transport_vol_sum == pytest.approx(want["vol_sum"][0], rel=1e-14)


@pytest.mark.parametrize("kw", [pytest.param({"ensemble": "nve"}, id="nve"),
                                pytest.param({"ensemble": "nvt", "thermostat": "Nose-Hoover-Chain", "temperature": 1000}, id="nvt_nhc")])
def test_a_run_accumulates_what_its_own_frames_give(calc, kw):
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.observables import MDObservers

    ob = MDObservers(**E2E)
    assert ob.vanhove_lags == 2
    md = MolecularDynamics(_structure("limno2"), model=calc, starting_temperature=1000, timestep=2.0, loginterval=1, seed=11, observers=ob, **kw)
    md.run(3)
    md.run(5)
    obs = md.observables
    assert md.traj.steps == list(range(9)) and obs.species.tolist() == [3, 8, 25]
    want = _restate(md.traj, md._masses, md._run.species_index, 3, [0, 2, 4, 6, 8], ob)
    assert want["cnt"][0].tolist() == [5, 4, 3, 2] and obs.transport_samples == 5
    _assert_replica(obs, want, kw["ensemble"])
    # what a user reads off: all of it finite where the lag was reached
    assert np.isnan(obs.non_gaussian_parameter(3)[0]) and np.all(np.isfinite(obs.non_gaussian_parameter(3)[1:]))
    assert np.all(obs.collective_msd(3, 3)[1:] > 0) and np.array_equal(obs.collective_msd(3, 8), obs.collective_msd(8, 3))
    assert obs.current_correlation(3, 3)[0] > 0
    assert np.isfinite(obs.ionic_conductivity({3: 1.0, 25: 3.0, 8: -2.0}, 1000.0, (0.0, 12.0)))
    assert np.isfinite(obs.haven_ratio({3: 1.0}, 1000.0, (0.0, 12.0)))
    g = obs.van_hove_self(3)
    assert g.shape == (2, 32) and np.all(g[0, 1:] == 0) and g[0, 0] > 0 and g[1, 1:].sum() > 0 and obs.vanhove_lag_times_fs.tolist() == [0.0, 8.0]
    assert obs.mean_volume == pytest.approx(abs(np.linalg.det(md.traj.cells[0])), rel=1e-12)
    md.close()


def test_run_batch_gives_every_replica_the_sums_of_its_own_frames(calc):
    from chgnet_amd.dynamics import ATOMIC_MASSES, MolecularDynamics
    from chgnet_amd.observables import MDObservers

    structs = [_structure("limno2", seed=1), _structure("noangle", seed=2)]      # Li Mn O and Cl Cs: one species map of five
    kw = {"model": calc, "ensemble": "nvt", "thermostat": "Berendsen", "temperature": 800, "starting_temperature": 800, "timestep": 2.0,
          "loginterval": 1}
    ob = MDObservers(**{**E2E, "sample_interval": 1, "msd_lags": 3})
    out = MolecularDynamics.run_batch(structs, 4, seeds=[3, 4], observers=ob, **kw)
    kinds = [3, 8, 17, 25, 55]
    for s, res in zip(structs, out):
        obs = res["observables"]
        assert obs.species.tolist() == kinds
        z = np.asarray(s.atomic_numbers)
        index = np.searchsorted(kinds, z).astype(np.int32)
        want = _restate(res["trajectory"], ATOMIC_MASSES[z], index, 5, [0, 1, 2, 3, 4], ob)
        assert want["cnt"][0].tolist() == [5, 4, 3]
        _assert_replica(obs, want, f"{len(z)} atoms")
        absent = [k for k in range(5) if kinds[k] not in z]
        assert absent and np.all(obs.cmsd_sum[:, absent, :] == 0) and np.all(obs.vanhove_hist[:, absent] == 0)


def _parent_kernels_on_frames(eng, ob, S, species_index, masses, traj, steps) -> dict:
    """chg_test_md_observe -- the plain observers alone, no transport -- on the frames a run sampled."""
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


def test_old_keywords_never_reach_the_transport_entry_point_and_transport_leaves_the_plain_sums_alone(calc, monkeypatch):
    """Two runs from one seed are not the same trajectory on this engine: its float32 forces are summed with atomics and differ in the
    last bits from run to run (DESIGN.md 7b "Reproducibility"), so the plain sums of two runs differ in the seventh digit
    whether transport is on or not (one MI355X run of the figures printed below: msd_sum 3.5e-7 and vacf_sum 9.5e-7 plain against
    plain, 4.8e-7 and 3.4e-6 plain against transport).  What
    transport must not change is therefore checked where it can be checked exactly: the plain sums of the run WITH transport must be
    bit for bit what the plain observers' kernels alone -- chg_test_md_observe, no transport -- give on the frames that run sampled."""
    from chgnet_amd.dynamics import MolecularDynamics
    from chgnet_amd.observables import MDObservers

    eng = calc.model.engine
    real, calls = eng.lib.chg_md_set_transport, []

    def counted(*args):
        calls.append(args)
        return real(*args)

    monkeypatch.setattr(eng.lib, "chg_md_set_transport", counted)
    old = {"sample_interval": 2, "msd_lags": 4, "rdf_rmax": 6.0, "rdf_bins": 64}
    new = {k: v for k, v in E2E.items() if k not in old}
    runs = {}
    for name, extra in (("plain", {}), ("plain again", {}), ("transport", new)):
        ob = MDObservers(**old, **extra)
        md = MolecularDynamics(_structure("limno2"), model=calc, ensemble="nvt", thermostat="Nose-Hoover-Chain", temperature=1000,
                               starting_temperature=1000, timestep=2.0, loginterval=1, seed=11, observers=ob)
        md.run(8)
        obs = md.observables
        alone = _parent_kernels_on_frames(eng, ob, 3, md._run.species_index, md._masses, md.traj, [0, 2, 4, 6, 8])
        md.close()
        assert len(calls) == (1 if name == "transport" else 0), name              # the old keywords never reach the new entry point
        for key, mine in (("msd", obs.msd_sum), ("vacf", obs.vacf_sum), ("cnt", obs.cnt), ("rdf", obs.rdf_hist)):
            assert np.array_equal(mine, alone[key][0]), (name, key)               # bit for bit, with and without transport
        assert obs.rdf_samples == alone["rdf_samples"][0] == 5 and obs.vol_sum == alone["vol_sum"][0]
        runs[name] = obs
    a, b = runs["plain"], runs["transport"]
    assert a.msd4_sum is None and a.cmsd_sum is None and a.vanhove_hist is None and b.cmsd_sum is not None
    assert b.vol_sum == b.transport_vol_sum and np.array_equal(a.cnt, b.cnt)
    for other in ("plain again", "transport"):
        c = runs[other]
        print(f"plain against {other}: max relative difference of msd_sum "
              f"{np.max(np.abs(a.msd_sum[1:] - c.msd_sum[1:]) / np.abs(a.msd_sum[1:])):.2e}, of vacf_sum "
              f"{np.max(np.abs(a.vacf_sum - c.vacf_sum) / np.abs(a.vacf_sum)):.2e}")
