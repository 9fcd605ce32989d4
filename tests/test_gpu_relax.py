"""Batched relaxation on the MI355X: the step kernel against the float64 restatement (tests/relax_ref.py), StructOptimizer.relax
against the restatement driven by predict_structure, convergence / max-steps stops, relax_batch == relax per structure, and a
1024-structure batch."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from conftest import load_case
from relax_ref import FIRE, GPA, Relaxation, pack_state, relax_host, unpack_state

pytestmark = pytest.mark.gpu


def _params(relax_cell=1, fmax=0.1, max_steps=500):
    from chgnet_amd import _lib

    return _lib.RelaxParams(fmax=fmax, max_steps=max_steps, relax_cell=relax_cell, dt=FIRE["dt"], maxstep=FIRE["maxstep"], dtmax=FIRE["dtmax"],
                            finc=FIRE["finc"], fdec=FIRE["fdec"], astart=FIRE["astart"], fa=FIRE["fa"], nmin=FIRE["nmin"], exp_cell_factor=0.0,
                            r_atom=6.0, r_bond=3.0, numerical_tol=1e-8, stress_weight=GPA)


@pytest.fixture(scope="module")
def model(trained_like_weights):
    from chgnet_amd import CHGNet

    return CHGNet(state_dict=trained_like_weights)


def _structure(name, supercell=(1, 1, 1), rattle=0.0, strain=0.0, seed=0):
    from chgnet_amd.graph.structure import Lattice, Structure

    _, d = load_case(name)
    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]).make_supercell(supercell)
    rng = np.random.default_rng(seed)
    lat = s.lattice.matrix @ (np.eye(3) + strain * rng.normal(size=(3, 3)))
    cart = s.frac_coords @ s.lattice.matrix + rattle * rng.normal(size=(len(s), 3))
    return Structure(Lattice(lat), s.atomic_numbers, cart @ np.linalg.inv(lat))


# ---- 1. the step kernel on its own ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relax_cell", [1, 0])
def test_step_kernel_matches_restatement(hip_engine, relax_cell):
    from chgnet_amd import _lib

    rng = np.random.default_rng(7 + relax_cell)
    sizes = [5, 8, 17, 300, 3, 11, 40]      # 300: rows beyond one pass of the workgroup
    kinds = ["downhill", "uphill", "clamp", "first", "converged", "max_steps", "nonfinite"]
    max_steps = 50
    rel, forces, stresses = [], [], []
    for n, kind in zip(sizes, kinds):
        L0 = np.diag(rng.uniform(4, 9, 3)) + rng.normal(0, 0.6, (3, 3))
        r = Relaxation(rng.random((n, 3)), L0, relax_cell=bool(relax_cell), fmax=0.1, steps=max_steps)
        if relax_cell:
            r.q[n:] = r.c * rng.normal(0, 0.25, (3, 3))        # F far from I
        r.q[:n] += rng.normal(0, 0.3, (n, 3))
        r.steps, r.nsteps = int(rng.integers(1, 30)), int(rng.integers(0, 12))
        r.dt, r.a = rng.uniform(0.05, 0.5), rng.uniform(0.02, 0.1)
        f = rng.normal(0, 0.6, (n, 3)).astype(np.float32)
        s = rng.normal(0, 2.0, (3, 3))
        s = ((s + s.T) / 2).astype(np.float32)
        if kind == "clamp":
            f *= 40
        if kind == "first":
            r.steps, r.nsteps = 0, 0
        if kind == "converged":
            f = (f * 1e-3).astype(np.float32)
            s = (s * 1e-4).astype(np.float32)
        if kind == "max_steps":
            r.steps = max_steps
        if kind == "nonfinite":
            f[n // 2, 1] = np.nan
        rows = n + 3 if relax_cell else n
        g = r.generalized_forces(f.astype(np.float64), s.astype(np.float64) * GPA)
        sign = -1.0 if kind == "uphill" else 1.0
        r.v[:rows] = sign * np.nan_to_num(g) * rng.uniform(0.2, 2.0) + rng.normal(0, 0.01, (rows, 3))
        rel.append(r)
        forces.append(f)
        stresses.append(s)
    atom_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    q, v, sd, si = pack_state(rel, atom_off)
    energy = rng.normal(-5, 1, len(sizes)).astype(np.float32)
    force = np.ascontiguousarray(np.concatenate(forces), np.float32)
    stress = np.ascontiguousarray(np.stack(stresses), np.float32)
    magmom = rng.random(atom_off[-1]).astype(np.float32)
    frac_next = np.zeros((atom_off[-1], 3))
    lat_next = np.zeros((len(sizes), 3, 3))
    p = _params(relax_cell, 0.1, max_steps)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    hip_engine._check(hip_engine.lib.chg_test_relax_step(hip_engine.handle, ctypes.byref(p), len(sizes), atom_off.ctypes.data_as(_lib.c_int_p),
                                                         dp(q), dp(v), dp(sd), si.ctypes.data_as(_lib.c_int_p), fp(energy), fp(force),
                                                         fp(stress), fp(magmom), dp(frac_next), dp(lat_next)))
    want_status = {"downhill": 0, "uphill": 0, "clamp": 0, "first": 0, "converged": 1, "max_steps": 2, "nonfinite": 3}
    got = [Relaxation.__new__(Relaxation) for _ in rel]
    for gr, r in zip(got, rel):
        gr.n = r.n
    unpack_state(got, atom_off, q, v, sd, si)
    for o, (r, kind) in enumerate(zip(rel, kinds)):
        q0, v0, dt0, a0 = r.q.copy(), r.v.copy(), r.dt, r.a
        r.advance(forces[o].astype(np.float64), stresses[o].astype(np.float64) * GPA, True)
        gr = got[o]
        assert r.status == want_status[kind] == gr.status, (kind, r.status, gr.status)
        assert (r.steps, r.nsteps) == (gr.steps, gr.nsteps), kind
        tol = lambda ref: 2e-12 * (np.abs(ref).max() + 1.0)  # noqa: E731
        assert np.abs(gr.q - r.q).max() <= tol(r.q), kind
        assert np.abs(gr.v - r.v).max() <= tol(r.v), kind
        assert abs(gr.dt - r.dt) <= 1e-15 * r.dt and abs(gr.a - r.a) <= 1e-15 * r.a, kind
        if r.status != 0:                       # stopped: not moved
            assert np.array_equal(gr.q, q0) and np.array_equal(gr.v, v0) and (gr.dt, gr.a) == (dt0, a0), kind
            continue
        if kind == "clamp":
            moved = np.sqrt(((r.q - q0) ** 2).sum())
            assert moved == pytest.approx(FIRE["maxstep"], rel=1e-12)
        if kind == "uphill":
            assert r.nsteps == 0 and r.dt == pytest.approx(dt0 * FIRE["fdec"])
        sl = slice(atom_off[o], atom_off[o + 1])
        assert np.abs(frac_next[sl] - r.frac()).max() <= 2e-12 * (np.abs(r.frac()).max() + 1)
        lat = r.lattice()
        assert np.abs(lat_next[o] - lat).max() <= 2e-12 * np.abs(lat).max(), kind
        if not relax_cell:
            assert np.array_equal(lat_next[o], r.L0)


# ---- 2. StructOptimizer.relax against the host loop -----------------------------------------------------------------------------
def _host_predict(model):
    from chgnet_amd.graph.structure import Lattice, Structure

    def predict(z):
        def f(frac, lat):
            pred = model.predict_structure(Structure(Lattice(lat), z, frac), task="efsm")
            return pred["f"], pred["s"]
        return f
    return predict


@pytest.mark.parametrize("relax_cell", [True, False])
@pytest.mark.parametrize("case", [("limno2", (1, 1, 1)), ("li9co7o16", (1, 1, 1))])
def test_relax_matches_host_loop(model, relax_cell, case):
    from chgnet_amd.relax import StructOptimizer

    s = _structure(case[0], case[1], rattle=0.08, strain=0.03, seed=11)
    opt = StructOptimizer(model=model)
    res = opt.relax(s, fmax=1e-4, steps=30, relax_cell=relax_cell, loginterval=1, verbose=False)
    traj = res["trajectory"]
    r, frames = relax_host(s, _host_predict(model)(s.atomic_numbers), fmax=1e-4, steps=30, relax_cell=relax_cell)
    assert len(frames) == 31 and len(traj) == 32       # 31 evaluations + the final frame once more
    for k, (frac, lat) in enumerate(frames):
        assert np.abs(traj.cells[k] - lat).max() < 1e-5, k
        assert np.abs(traj.atom_positions[k] - frac @ lat).max() < 1e-5, k
        if not relax_cell:
            assert np.array_equal(traj.cells[k], s.lattice.matrix)
    fin = res["final_structure"]
    assert np.abs(fin.lattice.matrix - r.lattice()).max() < 1e-5
    assert len(fin.site_properties["magmom"]) == len(s)
    assert np.all(np.isfinite(traj.energies)) and traj.stresses[0].shape == (6,)


# ---- 3. convergence and max-steps stops -----------------------------------------------------------------------------------------
def test_convergence_step_matches_and_final_forces_below_fmax(model):
    from chgnet_amd.graph.structure import Lattice, Structure
    from chgnet_amd.relax import StructOptimizer

    s = _structure("limno2", rattle=0.06, strain=0.02, seed=5)
    pred = _host_predict(model)(s.atomic_numbers)
    gmax = []

    def recording(frac, lat):
        f, st = pred(frac, lat)
        gmax.append((f, st))
        return f, st

    r, frames = relax_host(s, recording, fmax=0.0, steps=15)
    # max generalized force per evaluation, replayed through the restatement
    rr = Relaxation(s.frac_coords, s.lattice.matrix, fmax=0.0, steps=15)
    g_at = []
    for f, st in gmax:
        g = rr.generalized_forces(np.asarray(f, np.float64), np.asarray(st, np.float64) * GPA)
        g_at.append(float(np.sqrt((g ** 2).sum(1).max())))
        rr.advance(np.asarray(f, np.float64), np.asarray(st, np.float64) * GPA)
    k = int(np.argmin(g_at[1:])) + 1
    fmax = g_at[k] + 0.5 * (min(g_at[:k]) - g_at[k])
    host, _ = relax_host(s, pred, fmax=fmax, steps=100)
    res = StructOptimizer(model=model).relax_batch([s], fmax=fmax, steps=100)[0]
    assert host.status == 1 and host.steps == k
    assert res["status"] == "CONVERGED" and res["converged"] and res["n_steps"] == k
    fin = res["final_structure"]
    p = model.predict_structure(Structure(Lattice(fin.lattice.matrix), fin.atomic_numbers, fin.frac_coords))
    g = host.generalized_forces(np.asarray(p["f"], np.float64), np.asarray(p["s"], np.float64) * GPA)
    assert np.sqrt((g ** 2).sum(1).max()) < fmax
    res3 = StructOptimizer(model=model).relax_batch([s], fmax=1e-6, steps=3)[0]
    assert res3["status"] == "MAX_STEPS" and res3["n_steps"] == 3


# ---- 4. relax_batch == relax per structure (compaction) -------------------------------------------------------------------------
def test_batch_equals_single(model):
    from chgnet_amd.relax import StructOptimizer

    structs = [_structure("limno2", rattle=0.05, strain=0.02, seed=1), _structure("li9co7o16", rattle=0.03, strain=0.01, seed=2),
               _structure("limno2", (2, 1, 1), rattle=0.1, strain=0.04, seed=3), _structure("li9co7o16", (2, 2, 2), rattle=0.02, seed=4),
               _structure("limno2", (2, 2, 1), rattle=0.02, strain=0.005, seed=5), _structure("li9co7o16", (2, 1, 1), rattle=0.06, strain=0.03, seed=6)]
    opt = StructOptimizer(model=model)
    for fmax in (0.15, 0.3, 0.6, 1.2, 2.5):    # the loosest of these that lets the structures stop at different steps
        kw = dict(fmax=fmax, steps=25)
        singles = [opt.relax_batch([s], **kw)[0] for s in structs]
        if len({r["n_steps"] for r in singles}) >= 3:
            break
    assert len({r["n_steps"] for r in singles}) >= 3          # different stop steps: the batch shrinks as it runs
    batch = opt.relax_batch(structs, **kw)
    # the engine's fp32 forces are not bit-reproducible run to run (atomic accumulation order): positions agree to ~1e-5 A, not bitwise
    for b, s1, s in zip(batch, singles, structs):
        assert (b["n_steps"], b["status"]) == (s1["n_steps"], s1["status"])
        pb = b["final_structure"].frac_coords @ b["final_structure"].lattice.matrix
        ps = s1["final_structure"].frac_coords @ s1["final_structure"].lattice.matrix
        assert np.abs(pb - ps).max() < 2e-5
        assert np.abs(b["final_structure"].lattice.matrix - s1["final_structure"].lattice.matrix).max() < 2e-5
    one = opt.relax(structs[0], verbose=False, **kw)          # relax: the same optimizer, one evaluation per call
    f1, fs = one["final_structure"], singles[0]["final_structure"]
    assert np.abs(f1.frac_coords @ f1.lattice.matrix - fs.frac_coords @ fs.lattice.matrix).max() < 2e-5


# ---- 5. a large batch -----------------------------------------------------------------------------------------------------------
def test_large_batch_five_steps(model):
    from chgnet_amd import _lib

    structs = [_structure("limno2", (5, 1, 1), rattle=0.05, strain=0.02, seed=100 + i) for i in range(1024)]
    eng = model.engine
    prep = eng.prepare_structures(structs)
    host = prep.host()
    p = _params(1, 0.1, 5)
    h = ctypes.c_void_p()
    eng._check(eng.lib.chg_relax_create(eng.handle, ctypes.byref(host), ctypes.byref(p), ctypes.byref(h)))
    try:
        n_active, history = ctypes.c_int32(), []
        for _ in range(8):
            eng._check(eng.lib.chg_relax_run(eng.handle, h, 1, ctypes.byref(n_active)))
            history.append(n_active.value)
            if n_active.value == 0:
                break
        N, B = int(prep.atom_off[-1]), 1024
        out = {"frac": np.empty((N, 3)), "lattice": np.empty((B, 3, 3)), "energy": np.empty(B, np.float32), "force": np.empty((N, 3), np.float32),
               "stress": np.empty((B, 9), np.float32), "magmom": np.empty(N, np.float32), "n_steps": np.empty(B, np.int32),
               "status": np.empty(B, np.int32)}
        eng._check(eng.lib.chg_relax_download(eng.handle, h, ctypes.byref(_lib.fill_out(_lib.RelaxOutHost(), out))))
    finally:
        eng.lib.chg_relax_free(eng.handle, h)
    assert history[-1] == 0 and len(history) == 6 and all(a >= b for a, b in zip(history, history[1:]))
    for k in ("frac", "lattice", "energy", "force", "stress", "magmom"):
        assert np.all(np.isfinite(out[k])), k
    assert set(np.unique(out["status"])) <= {1, 2}
    assert np.all(out["n_steps"][out["status"] == 2] == 5) and np.all(out["n_steps"] <= 5)


# ---- 6. isolated atoms -------------------------------------------------------------------------------------------------------------
def test_isolated_atoms_reported_once_per_structure(model, capsys):
    """A batch with one structure holding isolated atoms: the converter's message once on stderr under "warn", ValueError under "error"."""
    from chgnet_amd.graph.structure import Lattice, Structure
    from chgnet_amd.relax import StructOptimizer

    lone = Structure(Lattice(np.eye(3) * 20.0), ["H", "O"], [[0, 0, 0], [0.5, 0.5, 0.5]])
    structs = [_structure("limno2", rattle=0.05, seed=1), lone, _structure("li9co7o16", rattle=0.03, seed=2)]
    try:
        capsys.readouterr()
        StructOptimizer(model=model, on_isolated_atoms="warn").relax_batch(structs, steps=3)
        assert capsys.readouterr().err.count("has 2 isolated atom") == 1
        with pytest.raises(ValueError, match="has 2 isolated atom"):
            StructOptimizer(model=model, on_isolated_atoms="error").relax_batch(structs, steps=3)
    finally:
        model.graph_converter.set_isolated_atom_response("warn")
