"""L-BFGS relaxation, CPU side: the float64 restatement (tests/lbfgs_ref.py) against a dense BFGS inverse Hessian, the secant
equation, the first step, the history ring, evaluation counts against FIRE on a toy family, argument validation of
StructOptimizer(optimizer_class="LBFGS") and the C-ABI additions."""

from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from lbfgs_ref import LBFGS, LbfgsRelaxation, lbfgs_step, pack_state, ring_slots, two_loop, unpack_state
from relax_ref import FIRE, Relaxation, fire_step


def _spd(rng, dof, lo, hi):
    qmat, _ = np.linalg.qr(rng.normal(size=(dof, dof)))
    return (qmat * np.geomspace(lo, hi, dof)) @ qmat.T


def _run_quadratic(K, x, steps, p=LBFGS):
    """L-BFGS on E = x K x / 2 from x: yields (x, g, history) before every step."""
    s, y, rho, r0, g0 = [], [], [], None, None
    for k in range(steps):
        g = -K @ x
        dr, _ = lbfgs_step(x, g, k == 0, r0, g0, s, y, rho, p)
        yield x, g, (s, y, rho), dr
        r0, g0, x = x, g, x + dr


# ---- the two-loop recursion ------------------------------------------------------------------------------------------------------
def test_two_loop_direction_equals_dense_bfgs():
    """30-dof convex quadratic, 8 steps: the two-loop direction == H g, H built by the dense BFGS update
    H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T from H = I / alpha, and H y_last = s_last after every update."""
    rng = np.random.default_rng(0)
    dof, alpha = 30, LBFGS["alpha"]
    K = _spd(rng, dof, 5.0, 150.0)
    H, eye, seen = np.eye(dof) / alpha, np.eye(dof), 0
    for x, g, (s, y, rho), _ in _run_quadratic(K, rng.normal(0, 0.3, dof), 8):
        if len(s) > seen:
            si, yi, ri = s[-1], y[-1], rho[-1]
            H = (eye - ri * np.outer(si, yi)) @ H @ (eye - ri * np.outer(yi, si)) + ri * np.outer(si, si)
            seen = len(s)
            assert np.abs(H @ yi - si).max() <= 1e-12 * np.abs(si).max()           # secant equation, dense
            # ... and through the recursion: two_loop(v) = H v
            assert np.abs(two_loop(yi, s, y, rho, alpha) - si).max() <= 1e-12 * np.abs(si).max()
        want, got = H @ g, two_loop(g, s, y, rho, alpha)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert seen == 7


def test_first_step_is_scaled_force_with_per_row_clamp():
    g = np.array([[3.0, -4.0, 0.0], [0.7, 0.0, 0.0], [0.0, 0.0, -7.0]])
    dr, appended = lbfgs_step(np.zeros(9), g.ravel(), True, None, None, [], [], [])
    assert not appended
    assert np.allclose(dr.reshape(3, 3), g / 70.0, rtol=1e-15)                   # longest row 0.1 < maxstep: no clamp
    dr, _ = lbfgs_step(np.zeros(9), 40 * g.ravel(), True, None, None, [], [], [])
    rows = np.sqrt((dr.reshape(3, 3) ** 2).sum(1))
    assert rows.max() == pytest.approx(LBFGS["maxstep"], rel=1e-14) and np.argmax(rows) == 2
    assert np.allclose(dr.reshape(3, 3), 40 * g / 70.0 * (0.2 / (40 * 7.0 / 70.0)), rtol=1e-14)
    # the clamp is per row, not on the norm: two rows of 0.15 (norm 0.21 > maxstep) stay as they are
    g2 = np.array([[0.15 * 70, 0, 0], [0, 0.15 * 70, 0]])
    dr, _ = lbfgs_step(np.zeros(6), g2.ravel(), True, None, None, [], [], [])
    assert np.allclose(dr.reshape(2, 3), g2 / 70.0, rtol=1e-15)
    # damping scales the clamped step
    dr, _ = lbfgs_step(np.zeros(9), 40 * g.ravel(), True, None, None, [], [], [], {**LBFGS, "damping": 0.5})
    assert np.sqrt((dr.reshape(3, 3) ** 2).sum(1)).max() == pytest.approx(0.1, rel=1e-14)


def test_ring_holds_the_last_memory_triples_in_order():
    rng = np.random.default_rng(1)
    K = _spd(rng, 12, 5.0, 100.0)
    p = {**LBFGS, "memory": 4}
    xs, gs, hist = [], [], None
    for x, g, hist, _ in _run_quadratic(K, rng.normal(0, 0.3, 12), 10, p):
        xs.append(x)
        gs.append(g)
    s, y, rho = hist
    assert len(s) == len(y) == len(rho) == 4
    for i, k in enumerate(range(5, 9)):                                          # triples 5..8 of the 9 appended, oldest first
        assert np.array_equal(s[i], xs[k + 1] - xs[k]) and np.array_equal(y[i], gs[k] - gs[k + 1])
        assert rho[i] == 1.0 / float(np.dot(y[i], s[i]))


def test_pack_unpack_round_trip_through_the_ring_layout():
    """The flat layout of chg_test_lbfgs_step: the k-th triple appended sits in slot k % slots."""
    rng = np.random.default_rng(2)
    rel = []
    for n, appended, cell in ((2, 0, True), (5, 3, True), (3, 9, False)):
        r = LbfgsRelaxation(rng.random((n, 3)), np.eye(3) * 5, relax_cell=cell, p={**LBFGS, "memory": 4})
        m = min(appended, 4)
        r.s, r.y = [rng.normal(size=3 * r.rows) for _ in range(m)], [rng.normal(size=3 * r.rows) for _ in range(m)]
        r.rho, r.appended, r.steps = list(rng.normal(size=m)), appended, appended + 1
        r.r0[:r.rows], r.g0[:r.rows] = rng.normal(size=(r.rows, 3)), rng.normal(size=(r.rows, 3))
        rel.append(r)
    atom_off = np.array([0, 2, 7, 10], np.int32)
    state = pack_state(rel, atom_off, 4)
    S, rho = state[3], state[5]
    assert S.shape == (4, 10 + 9, 3) and rho.shape == (3, 4)
    # structure 2 appended 9 triples: the newest (number 8) is in slot 0, the oldest held (number 5) in slot 1
    assert np.array_equal(S[0, 13:16].ravel(), rel[2].s[3]) and np.array_equal(S[1, 13:16].ravel(), rel[2].s[0])
    got = [LbfgsRelaxation.__new__(LbfgsRelaxation) for _ in rel]
    for gr, r in zip(got, rel):
        gr.n, gr.relax_cell = r.n, r.relax_cell
    unpack_state(got, atom_off, 4, *state)
    for gr, r in zip(got, rel):
        assert (gr.appended, gr.steps, gr.status) == (r.appended, r.steps, r.status)
        assert np.array_equal(gr.r0, r.r0) and np.array_equal(gr.g0, r.g0) and gr.rho == [float(x) for x in r.rho]
        assert all(np.array_equal(a, b) for a, b in zip(gr.s + gr.y, r.s + r.y))
    assert ring_slots(100, 5) == 5 and ring_slots(4, 500) == 4 and ring_slots(100, 0) == 1


def test_triple_with_zero_curvature_is_skipped():
    x0, g0 = np.array([0.1, 0.0, 0.0]), np.array([1.0, 2.0, 3.0])
    s, y, rho = [], [], []
    dr, appended = lbfgs_step(x0 + 0.01, g0, False, x0, g0, s, y, rho)           # g == g0: y = 0, y . s = 0
    assert not appended and s == [] and np.allclose(dr, g0 / 70.0, rtol=1e-15)
    # negative curvature is kept, as ASE keeps it
    dr, appended = lbfgs_step(x0 + 0.01, g0 + 0.5, False, x0, g0, s, y, rho)
    assert appended and rho[0] < 0
    # through the Relaxation: the appended counter does not move on a skipped triple
    r = LbfgsRelaxation(np.full((2, 3), 0.5), np.eye(3) * 5, relax_cell=False, fmax=1e-3)
    f = np.array([[0.3, 0.0, 0.0], [0.0, -0.2, 0.0]])
    for _ in range(3):
        r.advance(f, np.zeros((3, 3)))
    assert r.steps == 3 and r.appended == 0 and r.rho == []


# ---- against FIRE ----------------------------------------------------------------------------------------------------------------
def _toy(seed, rows=43, cond=100.0):
    """An anharmonic well around x*: E = d K d / 2 + c sum d^4 / 4 with d = x - x*, K of the given condition number."""
    rng = np.random.default_rng(seed)
    K = _spd(rng, 3 * rows, 1.0, cond)
    x_star = rng.normal(0, 1.0, 3 * rows)
    x0 = x_star + rng.normal(0, 0.15, 3 * rows)
    return (lambda x: -(K @ (x - x_star)) - 20.0 * (x - x_star) ** 3), x0


def _evaluations(step, force, x, fmax=0.05, limit=400):
    for k in range(limit):
        g = force(x)
        if (g.reshape(-1, 3) ** 2).sum(1).max() < fmax ** 2:
            return k + 1
        x = x + step(x, g, k == 0)
    return limit + 1


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_fewer_evaluations_than_fire_on_the_toy_family(seed):
    force, x0 = _toy(seed)
    st = {"v": np.zeros_like(x0), "dt": FIRE["dt"], "a": FIRE["astart"], "n": 0}

    def fire(x, g, first):
        dr, st["v"], st["dt"], st["a"], st["n"] = fire_step(g, st["v"], first, st["dt"], st["a"], st["n"])
        return dr

    hist = {"s": [], "y": [], "rho": [], "r0": None, "g0": None}

    def lbfgs(x, g, first):
        dr, _ = lbfgs_step(x, g, first, hist["r0"], hist["g0"], hist["s"], hist["y"], hist["rho"])
        hist["r0"], hist["g0"] = x, g
        return dr

    n_fire, n_lbfgs = _evaluations(fire, force, x0), _evaluations(lbfgs, force, x0)
    print(f"seed {seed}: FIRE {n_fire} evaluations, L-BFGS {n_lbfgs}")
    assert n_lbfgs < n_fire <= 400


def test_restatement_stop_rules_match_fire_restatement():
    frac0, L = np.full((4, 3), 0.5), np.eye(3) * 5.0
    rng = np.random.default_rng(1)
    r = LbfgsRelaxation(frac0 + rng.normal(0, 0.02, (4, 3)), L, relax_cell=False, fmax=1e-3, steps=500)
    while r.status == 0:
        r.advance(-0.8 * (r.positions() - frac0 @ L), np.zeros((3, 3)))
    assert r.status == 1 and 0 < r.steps < 20
    assert LbfgsRelaxation(frac0, L, relax_cell=False, fmax=1e-3).advance(np.zeros((4, 3)), np.zeros((3, 3))) == 1
    assert LbfgsRelaxation(frac0, L, relax_cell=False, fmax=1e-3, steps=0).advance(np.ones((4, 3)), np.zeros((3, 3))) == 2
    assert LbfgsRelaxation(frac0, L, relax_cell=False).advance(np.full((4, 3), np.nan), np.zeros((3, 3))) == 3
    # the generalized forces are Relaxation's
    a, b = LbfgsRelaxation(frac0, L), Relaxation(frac0, L)
    a.q[4:] = b.q[4:] = 0.1 * rng.normal(size=(3, 3))
    f, sig = rng.normal(size=(4, 3)), 0.01 * np.eye(3)
    assert np.array_equal(a.generalized_forces(f, sig), b.generalized_forces(f, sig))


# ---- StructOptimizer argument validation (no GPU: the engine is never created) -------------------------------------------------
@pytest.fixture()
def optimizer():
    from chgnet_amd import CHGNet
    from chgnet_amd.relax import StructOptimizer

    return StructOptimizer(model=CHGNet(), optimizer_class="LBFGS")


def test_lbfgs_optimizer_is_accepted_by_name_and_by_class(optimizer):
    from chgnet_amd import CHGNet
    from chgnet_amd.relax import OPTIMIZERS, StructOptimizer

    class LBFGS:  # noqa: N801  stands in for ase.optimize.LBFGS
        pass

    assert optimizer.optimizer_class == "LBFGS"
    assert StructOptimizer(model=CHGNet(), optimizer_class=LBFGS).optimizer_class == "LBFGS"
    assert StructOptimizer(model=CHGNet()).optimizer_class == "FIRE" and OPTIMIZERS[0] == "FIRE"     # the default stays
    for name in ("BFGS", "LBFGSLineSearch", "lbfgs"):
        with pytest.raises(ValueError, match=r"Optimizer instance not found. Select from \['FIRE'\].*'LBFGS'"):
            StructOptimizer(model=CHGNet(), optimizer_class=name)


def test_lbfgs_keywords_are_validated(optimizer):
    from chgnet_amd import CHGNet
    from chgnet_amd.graph.structure import Lattice, Structure
    from chgnet_amd.relax import StructOptimizer

    s = Structure(Lattice(np.eye(3) * 4), [3], [[0, 0, 0]])
    with pytest.raises(ValueError, match="use_line_search"):
        optimizer.relax(s, use_line_search=True)
    with pytest.raises(ValueError, match="use_line_search"):
        optimizer.relax_batch([s], use_line_search=True)
    for fire_only in ("dt", "dtmax", "Nmin", "finc", "fdec", "astart", "fa", "downhill_check"):
        with pytest.raises(TypeError, match="unexpected keyword"):
            optimizer.relax(s, **{fire_only: 1})
    with pytest.raises(TypeError, match="unexpected keyword"):
        optimizer.relax_batch([s], memmory=5)
    for bad in ({"memory": 0}, {"memory": -3}, {"maxstep": 0.0}, {"maxstep": -0.2}, {"damping": 0.0}, {"alpha": 0.0}, {"alpha": -70.0},
                {"alpha": float("nan")}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            optimizer.relax(s, **bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            optimizer.relax_batch([s], **bad)
    # what both optimizers share is still checked
    with pytest.raises(ValueError, match="Invalid ase_filter="):
        optimizer.relax(s, ase_filter="ExpCellFilter")
    with pytest.raises(ValueError, match="non-negative"):
        optimizer.relax(s, fmax=-1.0, memory=5)
    # FIRE does not take L-BFGS keywords
    fire = StructOptimizer(model=CHGNet())
    for lbfgs_only in ("memory", "alpha", "damping", "use_line_search"):
        with pytest.raises(TypeError, match="unexpected keyword"):
            fire.relax(s, **{lbfgs_only: 1})
    p = optimizer._params(0.05, 200, True, "FrechetCellFilter", {"memory": 7, "alpha": 50.0})
    assert p["lbfgs"] == {"maxstep": 0.2, "memory": 7, "damping": 1.0, "alpha": 50.0} and p["steps"] == 200
    assert "lbfgs" not in fire._params(0.05, 200, True, "FrechetCellFilter", {})


# ---- C-ABI -----------------------------------------------------------------------------------------------------------------------
def test_abi_gains_the_lbfgs_entry_points_without_a_bump():
    from chgnet_amd import _lib

    with open(os.path.join(REPO, "include", "chgnet_hip.h")) as fh:
        header = fh.read()
    assert int(re.search(r"#define\s+CHG_ABI_VERSION\s+(\d+)", header).group(1)) == 5 == _lib.ABI_VERSION
    lib = _lib.load()
    assert int(lib.chg_abi_version()) == 5
    for name in ("chg_relax_create_lbfgs", "chg_test_lbfgs_step"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(rf"\b{name}\s*\(", header)
    # null arguments are refused before anything touches a device
    assert lib.chg_relax_create_lbfgs(None, None, None, None, None) != 0


def test_lbfgs_params_mirror_the_c_header(tmp_path):
    from chgnet_amd import _lib

    fields = {"chg_lbfgs_params": _lib.LbfgsParams, "chg_relax_params": _lib.RelaxParams}
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
    assert [f for f, _ in _lib.LbfgsParams._fields_] == ["maxstep", "damping", "alpha", "memory", "reserved"]
    assert ctypes.sizeof(_lib.LbfgsParams) == 32
