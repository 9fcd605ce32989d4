"""The device graph builder (csrc/kernels_graph.h, engine_graph.hip) against the brute-force neighbour oracle
(tests/neighbor_ref.py) on the hard cell shapes of tests/graph_hard_cases.py: every search route, the exact and the single-pass
build, the 1,024-row limit of the in-LDS sort, the sort-key guard -- and what the float32 geometry kernels make of skewed cell
descriptions, measured against the float64 oracle with the reference-equivalent float32 oracle as the yardstick.

Every test is a single pass over fixed inputs."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

import graph_hard_cases as hard
import neighbor_ref
from device_graph import fetch_device_graph
from test_gpu_parity import TOL, _split
from test_gpu_round2 import TOL_TL

pytestmark = pytest.mark.gpu

ROUTES = {"all_pairs": ("all_pairs", 0), "cells": ("cells", 0), "auto64": ("auto", 64)}
GRAPH_KEYS = ("center", "neighbor", "image", "directed2undirected", "undirected2directed", "bond_graph")


def _batches():
    """cutoff pair -> case names in build order: an isolated-atoms-only structure first, last and between the structures below
    64 atoms and those from 64 atoms up (which ``auto`` with ``cell_min_atoms = 64`` bins).  The sort-limit cases have their own test."""
    by_cut: dict = {}
    for name, s, cuts in hard.cases():
        if name == "isolated" or name.startswith("sort_"):
            continue
        for cut in cuts:
            by_cut.setdefault(cut, []).append((name, len(s)))
    return {cut: ["isolated", *[n for n, k in lst if k < 64], "isolated", *[n for n, k in lst if k >= 64], "isolated"]
            for cut, lst in by_cut.items()}


def _check(engine, batch, names, r_atom, r_bond, tag):
    got = fetch_device_graph(engine, batch)
    want = [hard.oracle_graph(n, r_atom, r_bond) for n in names]
    for b, (name, g, w) in enumerate(zip(names, got, want)):
        assert np.all(g["owner"] == b), (tag, name, "e_owner")
        expect = {"center": w["atom_graph"][:, 0], "neighbor": w["atom_graph"][:, 1], "image": w["image"],
                  "directed2undirected": w["directed2undirected"], "undirected2directed": w["undirected2directed"],
                  "bond_graph": w["bond_graph"]}
        for key in GRAPH_KEYS:
            assert np.array_equal(g[key], expect[key]), (tag, name, r_atom, r_bond, key)
    assert batch.packed.n_isolated == sum(w["n_isolated"] for w in want), (tag, "n_isolated")
    assert batch.packed.n_directed == sum(len(w["atom_graph"]) for w in want), (tag, "n_directed")
    assert batch.packed.n_angles == sum(len(w["bond_graph"]) for w in want), (tag, "n_angles")


def _structs(names):
    return [hard.case(n)[0] for n in names]


def _reset_speculation(engine):
    """A build with cutoffs nobody else uses: the next build of any other cutoff pair takes the exact, three-round-trip pass."""
    engine.build_batch(_structs(["isolated"]), 7.7, 1.1).free()


# ---- a. every search route against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_builds_the_oracles_graph_in_one_batch_per_cutoff(hip_engine, route):
    try:
        hip_engine.set_graph_search(*ROUTES[route])
        for (r_atom, r_bond), names in _batches().items():
            structs = _structs(names)
            _reset_speculation(hip_engine)
            s0, o0 = hip_engine.build_stats()
            c0, f0 = hip_engine.cell_stats()
            batch = hip_engine.build_batch(structs, r_atom, r_bond)
            assert hip_engine.build_stats() == (s0, o0)                       # the exact pass
            _check(hip_engine, batch, names, r_atom, r_bond, (route, "exact"))
            batch.free()
            batch = hip_engine.build_batch(structs, r_atom, r_bond)
            assert hip_engine.build_stats() == (s0 + 1, o0)                   # ... and the single-pass build that follows it
            _check(hip_engine, batch, names, r_atom, r_bond, (route, "single pass"))
            batch.free()
            if route == "cells":
                assert hip_engine.cell_stats() == (c0 + 2, f0)                # no centre of these batches exceeds the in-LDS sort
            if route == "all_pairs":
                assert hip_engine.cell_stats() == (c0, f0)
    finally:
        hip_engine.set_graph_search("auto", 2048)


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_builds_the_oracles_graph_case_by_case(hip_engine, route):
    try:
        hip_engine.set_graph_search(*ROUTES[route])
        for name, s, cuts in hard.cases():
            if name.startswith("sort_"):
                continue
            for r_atom, r_bond in cuts:
                batch = hip_engine.build_batch([s], r_atom, r_bond)
                _check(hip_engine, batch, [name], r_atom, r_bond, (route, "B = 1"))
                batch.free()
    finally:
        hip_engine.set_graph_search("auto", 2048)


# ---- b. the 1,024-row limit of the in-LDS sort ----------------------------------------------------------------------------------
def test_sort_limit_1024_rows_build_through_the_cell_list_1025_stand_down(hip_engine):
    try:
        hip_engine.set_graph_search("cells")
        for K, used_cells in ((1024, True), (1025, False)):
            name = f"sort_{K}"
            s, ((r_atom, r_bond),) = hard.case(name)
            assert np.bincount(hard.oracle_rows(name, r_atom)[0].center).max() == K
            _reset_speculation(hip_engine)
            c0, f0 = hip_engine.cell_stats()
            batch = hip_engine.build_batch([s], r_atom, r_bond)
            assert hip_engine.cell_stats() == ((c0 + 1, f0) if used_cells else (c0, f0 + 1)), K
            _check(hip_engine, batch, [name], r_atom, r_bond, ("cells", K))
            batch.free()
    finally:
        hip_engine.set_graph_search("auto", 2048)


# ---- c. the guard of the sort key ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["coord_p4000", "coord_m4000", "coord_far1e6"])
def test_coordinates_beyond_the_sort_key_guard_go_all_pairs_silently(hip_engine, name):
    try:
        hip_engine.set_graph_search("cells")
        s, cuts = hard.case(name)
        for r_atom, r_bond in cuts:
            c0, f0 = hip_engine.cell_stats()
            batch = hip_engine.build_batch([s], r_atom, r_bond)
            assert hip_engine.cell_stats() == (c0, f0)
            _check(hip_engine, batch, [name], r_atom, r_bond, ("cells", "guard"))
            batch.free()
    finally:
        hip_engine.set_graph_search("auto", 2048)


# ---- d. physics on the unimodular and sheared cases -------------------------------------------------------------------------------
def _oracle_input(s, og, dtype):
    return SimpleNamespace(atomic_number=np.asarray(s.atomic_numbers), atom_frac_coord=s.frac_coords.astype(dtype),
                           lattice=s.lattice.matrix.astype(dtype), atom_graph=og["atom_graph"], neighbor_image=og["image"].astype(dtype),
                           directed2undirected=og["directed2undirected"], undirected2directed=og["undirected2directed"],
                           bond_graph=og["bond_graph"])


def _graph_of(s, r_atom=6.0, r_bond=3.0):
    rows, _ = neighbor_ref.brute_neighbors(s.frac_coords, s.lattice.matrix, r_atom)
    return {"atom_graph": np.stack([rows.center, rows.neighbor], 1), "image": rows.image,
            **neighbor_ref.line_graph_ref(len(s), rows, r_bond)}


def _judge(got, r64, r32, tol, label):
    """The project's yardstick (test_trained_like_weights_batched_and_ragged): engine error against float64 below
    max(2 x tolerance, 20 x the float32 oracle's own error on the same input).  Prints both errors, returns the misses."""
    misses, cells = [], []
    for key in ("e", "f", "s", "m"):
        err = float(np.abs(np.asarray(got[key], np.float64) - r64[key]).max())
        ref_err = float(np.abs(np.asarray(r32[key], np.float64) - r64[key]).max())
        cells.append(f"{key} {err:.2e} / {ref_err:.2e}")
        if not (np.isfinite(err) and err < max(2 * tol[key], 20 * ref_err)):
            misses.append(f"{label}:{key} engine {err:.3e} vs reference-fp32 {ref_err:.3e}")
    print(f"{label:28s} engine / fp32 oracle vs fp64:  " + "   ".join(cells))
    return misses


@pytest.fixture(scope="module")
def engine_tl(trained_like_weights):
    from chgnet_amd.engine import Engine
    from chgnet_amd.pack import pack_weights

    eng = Engine(pack_weights(trained_like_weights), 0)
    yield eng
    eng.close()


@pytest.mark.parametrize("which", ["golden", "trained_like"])
def test_skewed_descriptions_predict_what_the_identity_description_predicts(hip_engine, engine_tl, golden_weights, trained_like_weights, which):
    """E / F / S / M from the device-built batch of every description against the float64 oracle on the IDENTITY description's
    oracle-built graph (forces, magmoms and stress are Cartesian: no transformation between descriptions)."""
    import torch
    from oracle.chgnet_oracle import OracleCHGNet

    engine, weights, tol = (hip_engine, golden_weights, TOL) if which == "golden" else (engine_tl, trained_like_weights, TOL_TL)
    truth_of = hard.physics_cases()
    names = list(truth_of)
    torch.set_num_threads(8)
    o64, o32 = OracleCHGNet(weights, dtype=torch.float64), OracleCHGNet(weights)
    identities = sorted(set(truth_of.values()))
    r64 = dict(zip(identities, o64.predict_graph([_oracle_input(hard.case(n)[0], hard.oracle_graph(n, 6.0, 3.0), np.float64) for n in identities],
                                                 "efsm", batch_size=64)))
    r32 = o32.predict_graph([_oracle_input(hard.case(n)[0], hard.oracle_graph(n, 6.0, 3.0), np.float32) for n in names], "efsm", batch_size=64)
    batch = engine.build_batch(_structs(names), 6.0, 3.0)
    _check(engine, batch, names, 6.0, 3.0, ("physics", which))
    engine.predict(batch, "efsm")
    outs = _split(engine.download(batch, "efsm"), batch.packed)
    batch.free()
    misses = []
    for name, got, ref32 in zip(names, outs, r32):
        misses += _judge(got, r64[truth_of[name]], ref32, tol, f"{which}:{name}")
    assert not misses, "; ".join(misses)


# ---- e. the loops: the stepper's own rebuild path on a shape it has never seen ------------------------------------------------------
@pytest.fixture(scope="module")
def model_tl(trained_like_weights):
    from chgnet_amd import CHGNet

    return CHGNet(state_dict=trained_like_weights)


def _final_structure_against_the_oracle(model, weights, final, label):
    import torch
    from chgnet_amd import Structure
    from chgnet_amd.graph.structure import Lattice
    from oracle.chgnet_oracle import OracleCHGNet

    s = Structure(Lattice(np.asarray(final.lattice.matrix, np.float64)), np.asarray(final.atomic_numbers), np.asarray(final.frac_coords, np.float64))
    assert np.isfinite(s.frac_coords).all() and np.isfinite(s.lattice.matrix).all()
    og = _graph_of(s)
    got = model.predict_structure(s, task="efsm")
    torch.set_num_threads(8)
    r64 = OracleCHGNet(weights, dtype=torch.float64).predict_graph(_oracle_input(s, og, np.float64), "efsm")
    r32 = OracleCHGNet(weights).predict_graph(_oracle_input(s, og, np.float32), "efsm")
    misses = _judge(got, r64, r32, TOL_TL, label)
    assert not misses, "; ".join(misses)


def test_relaxation_with_the_cell_filter_from_a_skewed_description(model_tl, trained_like_weights):
    from chgnet_amd.relax import StructOptimizer

    start, _ = hard.case("tri8_m130")
    res = StructOptimizer(model=model_tl).relax(start, fmax=1e-4, steps=5, relax_cell=True, verbose=False)
    final = res["final_structure"]
    assert np.abs(final.lattice.matrix - start.lattice.matrix).max() > 1e-6          # the cell did move
    _final_structure_against_the_oracle(model_tl, trained_like_weights, final, "relax:tri8_m130")


def test_npt_dynamics_from_a_skewed_description(model_tl, trained_like_weights):
    from chgnet_amd.dynamics import MolecularDynamics

    start, _ = hard.case("tri8_m130")
    md = MolecularDynamics(start, model=model_tl, ensemble="npt", thermostat="Berendsen_inhomogeneous", temperature=300.0,
                           starting_temperature=300.0, pressure=5.0, bulk_modulus=100.0, taup=200.0, timestep=1.0, loginterval=1, seed=7)
    try:
        md.run(5)
        final = md.atoms
        assert np.abs(final.lattice.matrix - start.lattice.matrix).max() > 1e-9 and np.abs(final.frac_coords - start.frac_coords).max() > 1e-6
        _final_structure_against_the_oracle(model_tl, trained_like_weights, final, "npt:tri8_m130")
    finally:
        md.close()
