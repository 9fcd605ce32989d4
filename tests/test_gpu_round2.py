"""GPU tests added in round 2: edge-order independence, memory contract, ``CHGNet.forward``, the full-size
batch against the oracle fixture, and the device graph builder against the reference's compiled C builder."""

from __future__ import annotations

import os

import numpy as np
import pytest

from conftest import GOLDEN, load_case
from test_gpu_parity import TOL, _oracle, _predict, _split, _structures_for_graph_tests

pytestmark = pytest.mark.gpu


def _permute_directed_edges(g, perm):
    """The same graph with its directed edges listed in another order (new position i holds old edge perm[i])."""
    from chgnet_amd.graph.crystalgraph import CrystalGraph

    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    bg = g.bond_graph.copy()
    if len(bg):
        bg[:, 2] = inv[bg[:, 2]]
        bg[:, 4] = inv[bg[:, 4]]
    return CrystalGraph(atomic_number=g.atomic_number, atom_frac_coord=g.atom_frac_coord, atom_graph=g.atom_graph[perm],
                        atom_graph_cutoff=6, neighbor_image=g.neighbor_image[perm], directed2undirected=g.directed2undirected[perm],
                        undirected2directed=inv[g.undirected2directed].astype(np.int32), bond_graph=bg, bond_graph_cutoff=3,
                        lattice=g.lattice)


@pytest.mark.parametrize("name", ["limno2", "s16tri", "s40"])
def test_edge_order_does_not_matter(hip_engine, name):
    """predict_graph takes hand-built graphs in ANY edge order (the reference's index_add_ does); the force
    kernel's segmented scan must not merge two separate runs of one centre atom ([A, B, A])."""
    g, d = load_case(name)
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(g.atom_graph))
    # interleaved: centre-major blocks dealt round-robin, so equal centres recur inside one wave
    order = np.argsort(np.arange(len(g.atom_graph)) % 7, kind="stable")
    for p in (perm, order):
        batch, res = _predict(hip_engine, [_permute_directed_edges(g, p), g])
        a, b = _split(res, batch.packed)
        batch.free()
        for key in ("e", "f", "s", "m"):
            assert np.abs(a[key] - d["out_" + key]).max() < TOL[key], (name, key)
            assert np.abs(a[key] - b[key]).max() < TOL[key], (name, key)


def test_memory_limit_splits_chunks_and_keeps_results(hip_engine, golden_weights):
    """batch_size / device-memory contract: an arena above the engine's limit is refused with CHG_ENOMEM, the
    host halves the chunk and retries; results are those of the unrestricted run."""
    import bench
    from chgnet_amd.engine import EngineOutOfMemory
    from chgnet_amd.model import CHGNet

    structs = bench.workload_structures(48, 100)
    model = CHGNet(state_dict=golden_weights)
    model._engine = hip_engine
    free, total = hip_engine.memory_info()
    assert 0 < free <= total
    want = model.predict_structure(structs, task="efs", batch_size=48)
    full = hip_engine.build_batch(structs)
    need = hip_engine.bytes_required(48, full.packed.n_atoms, full.packed.n_directed, full.packed.n_angles, full.packed.n_bnodes)
    assert 0 < need <= full.device_bytes            # the arena may be a (larger) pooled one
    full.free()
    builds = []
    orig = hip_engine.build_prepared
    hip_engine.build_prepared = lambda prep, *a, **k: (builds.append(prep.n_struct), orig(prep, *a, **k))[1]
    try:
        hip_engine.set_memory_limit(need // 3)
        got = model.predict_structure(structs, task="efs", batch_size=48)
        assert builds[0] == 48 and len(builds) > 3 and max(builds[1:]) <= 24
        for a, b in zip(got, want):
            for key in ("e", "f", "s"):
                assert np.abs(a[key] - b[key]).max() < 2e-6, key
        # batch_size is a hard cap when the atom floor is switched off (the reference's meaning)
        builds.clear()
        hip_engine.set_memory_limit(0)
        model.predict_structure(structs, task="e", batch_size=5, min_atoms_per_batch=0)
        assert builds == [5] * 9 + [3]
        # a single structure that does not fit raises, and the engine stays usable
        hip_engine.set_memory_limit(1 << 20)
        with pytest.raises(EngineOutOfMemory, match="limit"):
            model.predict_structure(structs[0], task="e")
        with pytest.raises(EngineOutOfMemory):
            model.predict_graph(load_case("limno2")[0], task="e")
    finally:
        hip_engine.set_memory_limit(0)
        hip_engine.build_prepared = orig
        model._engine = None
    hip_engine.build_batch(structs[:2]).free()                         # still usable after the refusals


def test_forward_returns_the_reference_batch_dictionary(hip_engine, golden_weights):
    """CHGNet.forward (model.py:330-387): key set, container types, shapes and values of the batch dict."""
    from chgnet_amd.model import CHGNet

    d = np.load(os.path.join(GOLDEN, "batch_mixed.npz"))
    order = [str(x) for x in d["order"]]
    graphs = [load_case(n)[0] for n in order]
    model = CHGNet(state_dict=golden_weights)
    model._engine = hip_engine
    try:
        out = model.forward(graphs)                                   # default task "e"
        assert set(out) == {"atoms_per_graph", "e"} and out["e"].shape == (len(graphs),) and out["e"].dtype == np.float32
        assert out["atoms_per_graph"].tolist() == [len(g.atomic_number) for g in graphs] and out["atoms_per_graph"].dtype == np.int64
        out = model(graphs, task="efsm", return_site_energies=True, return_atom_feas=True, return_crystal_feas=True)
        assert set(out) == {"atoms_per_graph", "e", "f", "s", "m", "site_energies", "atom_fea", "crystal_fea"}
        for key in ("f", "s", "m", "site_energies", "atom_fea"):
            assert isinstance(out[key], list) and len(out[key]) == len(graphs), key
        assert out["crystal_fea"].shape == (len(graphs), 64)
        for i, n in enumerate(order):
            na = len(graphs[i].atomic_number)
            assert out["f"][i].shape == (na, 3) and out["s"][i].shape == (3, 3) and out["m"][i].shape == (na,)
            assert out["site_energies"][i].shape == (na,) and out["atom_fea"][i].shape == (na, 64)
            assert abs(out["e"][i] - d[f"{n}_e"]) < TOL["e"]
            for key in ("f", "s", "m", "site_energies", "atom_fea"):
                ref = d[f"{n}_{key}"]
                assert (np.abs(out[key][i] - ref).max() if ref.size else 0.0) < TOL[key], (n, key)
            assert np.abs(out["crystal_fea"][i] - d[f"{n}_crystal_fea"]).max() < TOL["crystal_fea"]
        single = model.predict_structure([_structures_for_graph_tests()[0]], task="e")
        assert isinstance(single, dict)                               # one-element list -> bare dict, like the reference
    finally:
        model.release_forward_state()
        model._engine = None


def test_full_size_batch_every_structure_against_the_oracle(hip_engine, golden_weights):
    """BASELINE configs[1] at full size: ALL 1024 structures against the oracle's fixture
    (tests/golden/make_bench_fixture.py: E, |F|, tr S, force on atom 0) and 64 of them against the live oracle."""
    import bench

    fx = np.load(os.path.join(GOLDEN, "bench_c2_oracle.npz"))
    graphs = bench.build_workload(1024, 0)
    assert np.array_equal(fx["n_directed"], [len(g.atom_graph) for g in graphs])      # same workload as the fixture
    assert np.array_equal(fx["n_angles"], [len(g.bond_graph) for g in graphs])
    batch, res = _predict(hip_engine, graphs, task="efs")
    outs = _split(res, batch.packed)
    batch.free()
    e = np.array([o["e"] for o in outs])
    assert np.abs(e - fx["e"]).max() < TOL["e"]
    fn = np.array([np.sqrt((o["f"].astype(np.float64) ** 2).sum()) for o in outs])
    assert np.abs(fn - fx["f_norm"]).max() < 40 ** 0.5 * 3 ** 0.5 * TOL["f"]
    st = np.array([np.trace(o["s"].astype(np.float64)) for o in outs])
    assert np.abs(st - fx["s_trace"]).max() < 3 * TOL["s"]
    f0 = np.array([o["f"][0] for o in outs])
    assert np.abs(f0 - fx["f_atom0"]).max() < TOL["f"]
    sample = list(range(0, 1024, 16))
    refs = _oracle(golden_weights, [graphs[i] for i in sample], task="efs")
    for i, r in zip(sample, refs):
        assert abs(outs[i]["e"] - r["e"]) < TOL["e"]
        assert np.abs(outs[i]["f"] - r["f"]).max() < TOL["f"]
        assert np.abs(outs[i]["s"] - r["s"]).max() < TOL["s"]


def test_device_graph_build_against_the_compiled_reference(hip_engine):
    """The device builder vs the reference's own C builder (create_graph.c compiled in place) DIRECTLY: the neighbour list
    found on the device is the one the reference's create_graph + line-graph code was fed (tests/golden/ref_graph_c.json,
    make_ref_graph_golden.py), and every index array must come out as the reference built it."""
    import json

    from chgnet_amd.graph.converter import build_graph_arrays
    from device_graph import fetch_device_graph
    from golden.make_golden_helpers import array_digest

    with open(os.path.join(GOLDEN, "ref_graph_c.json")) as fh:
        fx = json.load(fh)
    structs = _structures_for_graph_tests()
    for j, (r_atom, r_bond) in enumerate(((6.0, 3.0), (5.0, 3.0), (4.0, 4.0))):
        batch = hip_engine.build_batch(structs, r_atom, r_bond)
        per_struct = fetch_device_graph(hip_engine, batch)          # packed indices made local to each structure
        batch.free()
        for b, (s, g) in enumerate(zip(structs, per_struct)):
            if len(g["center"]) == 0:
                continue                                               # isolated atoms only: nothing to index
            host = build_graph_arrays(np.asarray(s.frac_coords, np.float64), np.asarray(s.lattice.matrix, np.float64), r_atom, r_bond)
            assert np.array_equal(host["atom_graph"], np.stack([g["center"], g["neighbor"]], 1)) and np.array_equal(host["image"], g["image"])
            ref = fx[f"gpu_{b}_{j}"]
            fed = {"center": g["center"], "neighbor": g["neighbor"], "image": g["image"], "distance": host["distance"]}
            for key, v in fed.items():                                 # the list the reference was fed
                assert array_digest(v) == ref[key], (b, key)
            assert array_digest(g["directed2undirected"]) == ref["directed2undirected"], (b, "d2u")
            assert array_digest(g["undirected2directed"]) == ref["undirected2directed"], (b, "u2d")
            assert array_digest(g["bond_graph"]) == ref["bond_graph"], (b, "bond_graph")


# ---------------------------------------------------------------------------------------------------
# second weight set: the magnitudes of a trained checkpoint (tests/golden/weights_trained_like.npz)
# ---------------------------------------------------------------------------------------------------
# |E| 5-6 eV/atom, |F| up to 4.6 eV/A, |stress| up to 29 GPa, gates driven into saturation.  The reference's own
# fp32-vs-fp64 error at this scale is E 4e-7, F 1.2e-5, S 1e-4; the north star asks 1e-4 eV and 1e-3 eV/A.
TOL_TL = {"e": 5e-6, "f": 5e-5, "s": 5e-4, "m": 2e-5, "site_energies": 3e-5, "atom_fea": 1e-4, "crystal_fea": 6e-4}


@pytest.fixture(scope="module")
def engine_tl(trained_like_weights):
    from chgnet_amd.engine import Engine
    from chgnet_amd.pack import pack_weights

    eng = Engine(pack_weights(trained_like_weights), 0)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", ["limno2", "s40", "s16tri", "noangle", "li9co7o16"])
def test_trained_like_weights_match_reference_golden(engine_tl, name):
    g, d = load_case(name)
    batch, res = _predict(engine_tl, [g])
    out = _split(res, batch.packed)[0]
    batch.free()
    for key, tol in TOL_TL.items():
        ref = d["tl_out_" + key]
        err = float(np.abs(out[key] - ref).max()) if ref.size else 0.0
        assert np.isfinite(out[key]).all() and err < tol, f"{name}:{key} max|d|={err:.3e} tol={tol:.1e}"


def test_trained_like_weights_batched_and_ragged(engine_tl, trained_like_weights):
    """The mixed batch of the reference (batch_mixed.npz, tl_ keys) and a ragged 10-100-atom batch against the oracle
    (fp64 as truth, the reference-equivalent fp32 oracle as the yardstick)."""
    import bench
    import torch
    from chgnet_amd import CrystalGraphConverter
    from oracle.chgnet_oracle import OracleCHGNet

    d = np.load(os.path.join(GOLDEN, "batch_mixed.npz"))
    order = [str(x) for x in d["order"]]
    batch, res = _predict(engine_tl, [load_case(n)[0] for n in order])
    for n, o in zip(order, _split(res, batch.packed)):
        for key, tol in TOL_TL.items():
            ref = d[f"tl_{n}_{key}"]
            assert (float(np.abs(o[key] - ref).max()) if ref.size else 0.0) < tol, (n, key)
    batch.free()
    conv = CrystalGraphConverter(on_isolated_atoms="ignore")
    graphs = [conv(bench.sweep_structure(i)) for i in range(10)]
    batch, res = _predict(engine_tl, graphs)
    outs = _split(res, batch.packed)
    batch.free()
    torch.set_num_threads(8)
    kw = dict(return_site_energies=True, return_atom_feas=True, return_crystal_feas=True, batch_size=64)
    o64 = OracleCHGNet(trained_like_weights, dtype=torch.float64).predict_graph(graphs, "efsm", **kw)
    o32 = OracleCHGNet(trained_like_weights).predict_graph(graphs, "efsm", **kw)
    worst = {}
    for got, r64, r32 in zip(outs, o64, o32):
        for key in ("e", "f", "s", "m"):
            ref_err = float(np.abs(np.asarray(r32[key], np.float64) - r64[key]).max())
            err = float(np.abs(got[key] - r64[key]).max())
            worst[key] = max(worst.get(key, 0.0), err)
            assert err < max(2 * TOL_TL[key], 20 * ref_err), f"{key}: engine {err:.3e} vs reference-fp32 {ref_err:.3e}"
    assert worst["e"] < 1e-4 and worst["f"] < 1e-3        # the north star's bars, at realistic magnitudes


def test_single_pass_graph_build_is_bit_exact_and_falls_back_on_overflow(hip_engine):
    """Later builds size their scratch from the previous build and read the counts once (one round trip instead of
    three): same arrays bit for bit; a denser structure than predicted trips the device-side overflow flag and
    the exact pass takes over."""
    import bench
    from chgnet_amd import CrystalGraphConverter, Structure
    from chgnet_amd.graph.structure import Lattice
    from chgnet_amd.pack import pack_batch
    from test_gpu_parity import INT_ARRAYS

    structs = bench.workload_structures(24, 7)
    conv = CrystalGraphConverter()
    want = pack_batch([conv(s) for s in structs])
    hip_engine.build_batch(structs).free()                     # primes the per-atom counts for these cutoffs
    s0, o0 = hip_engine.build_stats()
    batch = hip_engine.build_batch(structs)
    s1, o1 = hip_engine.build_stats()
    assert (s1, o1) == (s0 + 1, o0)                            # went through the single-pass path
    for attr in ("n_directed", "n_undirected", "n_angles", "n_bnodes"):
        assert getattr(batch.packed, attr) == getattr(want, attr), attr
    for name, count in INT_ARRAYS.items():
        assert np.array_equal(hip_engine.debug_fetch_i32(batch, name, getattr(want, count)), want.arrays[name]), name
    hip_engine.predict(batch, "efs")
    r1 = hip_engine.download(batch, "efs")
    batch.free()
    up = hip_engine.upload(want)
    hip_engine.predict(up, "efs")
    r2 = hip_engine.download(up, "efs")
    up.free()
    for key in ("e", "f", "s"):
        assert np.abs(r1[key] - r2[key]).max() < 2e-6, key
    # a sparse gas primes tiny capacities; the dense cells that follow overflow them and are rebuilt exactly
    sparse = [Structure(Lattice(np.eye(3) * 9.0), ["H", "O"], [[0, 0, 0], [0.3, 0.3, 0.3]]) for _ in range(24 * 20)]
    hip_engine.build_batch(sparse).free()
    batch = hip_engine.build_batch(structs)
    s2, o2 = hip_engine.build_stats()
    assert o2 == o1 + 1 and s2 == s1 + 1                       # (the sparse batch itself went single-pass) overflow detected, exact pass used
    for name, count in INT_ARRAYS.items():
        assert np.array_equal(hip_engine.debug_fetch_i32(batch, name, getattr(want, count)), want.arrays[name]), name
    batch.free()


def test_device_graph_build_2048_atom_cell(hip_engine):
    """A 2,048-atom cell: the device builder (one wave per centre over all atoms of the structure) against the host's
    cell-list builder, every index array bit for bit."""
    import bench
    from chgnet_amd import CrystalGraphConverter
    from chgnet_amd.pack import pack_batch
    from test_gpu_parity import INT_ARRAYS

    big = bench.limno2((4, 4, 2)).perturb(0.03, np.random.default_rng(9)).make_supercell([2, 2, 2])
    assert len(big) == 2048
    want = pack_batch([CrystalGraphConverter()(big)])
    batch = hip_engine.build_batch([big])
    for attr in ("n_directed", "n_undirected", "n_angles", "n_bnodes"):
        assert getattr(batch.packed, attr) == getattr(want, attr), attr
    for name, count in INT_ARRAYS.items():
        assert np.array_equal(hip_engine.debug_fetch_i32(batch, name, getattr(want, count)), want.arrays[name]), name
    hip_engine.predict(batch, "ef")
    res = hip_engine.download(batch, "ef")
    batch.free()
    assert np.isfinite(res["e"]).all() and np.abs(res["f"].sum(0)).max() < 5e-3


def test_device_cell_list_search_is_bit_exact(hip_engine):
    """The device cell list (chg_engine_set_graph_search): forced on for the small, oddly shaped fixture cells (a single
    bin reached through many images, unwrapped and negative coordinates, an isolated pair) and chosen by size for a
    mixed batch with a 2,048-atom cell -- the arrays equal the host builder's bit for bit, as with all pairs, and the
    build time of the large cell drops."""
    import time

    import bench
    from chgnet_amd import CrystalGraphConverter, Structure
    from chgnet_amd.pack import pack_batch
    from test_gpu_parity import INT_ARRAYS

    def same(batch, want):
        for attr in ("n_struct", "n_atoms", "n_directed", "n_undirected", "n_angles", "n_bnodes"):
            assert getattr(batch.packed, attr) == getattr(want, attr), attr
        for name, count in INT_ARRAYS.items():
            assert np.array_equal(hip_engine.debug_fetch_i32(batch, name, getattr(want, count)), want.arrays[name]), name
        assert np.array_equal(hip_engine.debug_fetch(batch, "e_image", (want.n_directed, 3)), want.e_image)

    try:
        structs = _structures_for_graph_tests()
        shifted = Structure(structs[0].lattice, structs[0].atomic_numbers, structs[0].frac_coords + np.array([3.0, -2.0, 0.999999999]))
        structs = [*structs, shifted]
        conv = CrystalGraphConverter(on_isolated_atoms="ignore")
        hip_engine.set_graph_search("cells")
        for r_atom, r_bond in ((6.0, 3.0), (4.0, 4.0)):
            cv = CrystalGraphConverter(atom_graph_cutoff=r_atom, bond_graph_cutoff=r_bond, on_isolated_atoms="ignore")
            want = pack_batch([cv(s) for s in structs])
            c0, f0 = hip_engine.cell_stats()
            batch = hip_engine.build_batch(structs, r_atom, r_bond)
            assert hip_engine.cell_stats() == (c0 + 1, f0)
            same(batch, want)
            batch.free()
        # by size: the 2,048-atom cell is binned, its small companions go through all pairs, in one batch
        big = bench.limno2((4, 4, 2)).perturb(0.03, np.random.default_rng(9)).make_supercell([2, 2, 2])
        mixed = [structs[0], big, structs[1]]
        want = pack_batch([conv(s) for s in mixed])
        hip_engine.set_graph_search("auto", 512)
        c0, f0 = hip_engine.cell_stats()
        batch = hip_engine.build_batch(mixed)
        assert hip_engine.cell_stats() == (c0 + 1, f0)
        same(batch, want)
        hip_engine.predict(batch, "ef")
        r_cells = hip_engine.download(batch, "ef")
        batch.free()
        hip_engine.set_graph_search("all_pairs")
        batch = hip_engine.build_batch(mixed)
        assert hip_engine.cell_stats() == (c0 + 1, f0)
        same(batch, want)
        hip_engine.predict(batch, "ef")
        r_all = hip_engine.download(batch, "ef")
        batch.free()
        assert np.array_equal(r_cells["e"], r_all["e"])
        # more than 1,024 rows per centre (14 A cutoff): the in-LDS sort stands down, all pairs takes over
        dense = bench.limno2((3, 2, 2))
        cv8 = CrystalGraphConverter(atom_graph_cutoff=14, bond_graph_cutoff=3)
        want = pack_batch([cv8(dense)])
        assert want.n_directed / want.n_atoms > 1024
        hip_engine.set_graph_search("cells")
        c0, f0 = hip_engine.cell_stats()
        batch = hip_engine.build_batch([dense], 14.0, 3.0)
        assert hip_engine.cell_stats() == (c0, f0 + 1)
        same(batch, want)
        batch.free()
        # timing: all pairs grows with the square of the cell, the cell list with the atoms (both after a priming build)
        for cell in ((5, 5, 5), (10, 10, 10), (16, 16, 12)):
            huge = bench.limno2(cell).perturb(0.02, np.random.default_rng(3))
            times = {}
            for mode in ("all_pairs", "cells"):
                hip_engine.set_graph_search(mode)
                hip_engine.build_batch([huge]).free()
                hip_engine.synchronize()
                t0 = time.perf_counter()
                b = hip_engine.build_batch([huge])
                hip_engine.synchronize()
                times[mode] = time.perf_counter() - t0
                times[mode + "_edges"] = b.packed.n_directed
                b.free()
            print(f"device graph build, {len(huge)} atoms: all pairs {times['all_pairs'] * 1e3:.1f} ms, cell list {times['cells'] * 1e3:.1f} ms")
            assert times["all_pairs_edges"] == times["cells_edges"]
        assert times["cells"] < times["all_pairs"]
    finally:
        hip_engine.set_graph_search("auto", 2048)       # the engine's default (all pairs wins up to ~1,000 atoms: engine_internal.h)


def test_pipelined_chunks_give_the_single_chunk_results(hip_engine, golden_weights):
    """Several chunks through the overlapped loop (next chunk prepared / packed during the sweep) == one chunk."""
    import bench
    from chgnet_amd import CrystalGraphConverter
    from chgnet_amd.model import CHGNet

    model = CHGNet(state_dict=golden_weights)
    structs = bench.workload_structures(10, 123) + _structures_for_graph_tests()[:3]
    one = model.predict_structure(structs, task="efsm", return_crystal_feas=True)
    many = model.predict_structure(structs, task="efsm", return_crystal_feas=True, batch_size=3, min_atoms_per_batch=0)
    graphs = [CrystalGraphConverter()(s) for s in structs]
    many_g = model.predict_graph(graphs, task="efsm", return_crystal_feas=True, batch_size=4, min_atoms_per_batch=0)
    assert len(one) == len(many) == len(many_g) == len(structs)
    for a, b, c in zip(one, many, many_g):
        for key in ("e", "f", "s", "m", "crystal_fea"):
            tol = 2e-5 if key == "crystal_fea" else 2e-6   # crystal_fea: atomics-ordered sums of ~50-sized features
            assert np.abs(a[key] - b[key]).max() < tol and np.abs(a[key] - c[key]).max() < tol, key


def test_rccl_communicator_through_the_c_abi():
    """chg_comm_*: RCCL opened by the engine library itself (no torch.distributed).  One GPU here, so the group has one
    rank: unique id, communicator, all-gather, all-reduce and barrier run through RCCL and return the input; the sharded
    sweep and the gradient all-reduce accept the communicator."""
    from chgnet_amd.distributed import RcclComm, all_gather_energies
    from chgnet_amd.trainer import allreduce_gradients

    comm = RcclComm(rank=0, world=1, device=0)
    try:
        x = np.arange(1000, dtype=np.float32) * 0.5 - 3.0
        assert np.array_equal(comm.all_gather(x), x)
        assert np.array_equal(comm.all_reduce_sum(x.reshape(10, 100)), x.reshape(10, 100))
        big = np.random.default_rng(0).normal(size=412_525).astype(np.float32)      # the parameter gradient
        assert np.array_equal(comm.all_reduce_sum(big), big)
        comm.barrier()
        e = all_gather_energies(np.array([1.0, 2.0, 3.0], np.float32), [[2, 0, 1]], 3, comm=comm)
        assert np.array_equal(e, np.array([2.0, 3.0, 1.0], np.float32))
        g = {"a": np.ones((2, 3), np.float32), "b": np.full(4, 2.0, np.float32)}
        out = allreduce_gradients(g, comm=comm)
        assert np.array_equal(out["a"], g["a"]) and np.array_equal(out["b"], g["b"])
    finally:
        comm.close()
