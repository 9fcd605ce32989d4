"""CPU side of tests/test_gpu_second_order_paths.py: the fixture claims its route matrix relies on (the headline batch is past the
launch sequence of MD-size batches and past the zsave threshold; predict_hessian's default batching of the 256-atom cell is past the
blocked-tile limit), the route query is part of the C-ABI, and the central differences of the new fixtures are converged."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest

import second_order_fixtures as sf
from conftest import GOLDEN, REPO


def test_headline_batch_takes_the_large_batch_route_with_zsave():
    from chgnet_amd.model import _plan_chunks
    from chgnet_amd.pack import pack_batch

    import angle_fixtures as af

    conv = af.converter()
    head = [conv(s) for s in sf.headline_structures()]
    pb = pack_batch(head)
    assert pb.n_atoms > 32768 and pb.n_atoms + 1 > 8192            # not tiny_batch; past the blocked tiles and TEAM
    assert pb.n_angles > 1 << 19                                      # zsave (engine_predict.hip carve)
    # CHGNet.hessian_vector_product(_with_strain)'s default chunking keeps the whole headline in one batch
    assert _plan_chunks([len(g.atomic_number) for g in head], 16, 40960) == [(0, len(head))]
    assert max(sf.HEAD_SAMPLE) < len(head) and max(sf.GRAD_SAMPLE) < len(head)


def test_predict_hessian_batches_the_256_atom_cell_past_the_blocked_tile_limit():
    from chgnet_amd import CHGNet
    from chgnet_amd.model import random_state_dict

    model = CHGNet(state_dict=random_state_dict({}, seed=0))
    md = model.graph_converter(sf.md_cell())
    n = len(md.atomic_number)
    assert n == 256 and max(sf.HESS_COLS) < 3 * n
    seen = []

    def fake(graphs, dirs, batch_size, min_atoms, strains=None):
        seen.append(sum(len(g.atomic_number) for g in graphs))
        z = [np.zeros((len(g.atomic_number), 3), np.float32) for g in graphs]
        return z if strains is None else [(x, np.zeros((3, 3), np.float32)) for x in z]

    model._hvp_graphs = fake
    model.predict_hessian(md, symmetrize=False)
    assert sum(seen) == 3 * n * n and min(seen) > 8191 and max(seen) <= 16384, seen
    assert model._engine is None


def test_route_query_is_declared():
    text = open(os.path.join(REPO, "include", "chgnet_hip.h")).read()
    assert '"route": five' in text
    src = open(os.path.join(REPO, "chgnet_amd", "csrc", "engine.hip")).read()
    assert re.search(r'strcmp\(name, "route"\)', src)


@pytest.mark.parametrize("weights", ["weights_seed0.npz", "weights_trained_like.npz"])
def test_finite_differences_of_the_new_fixtures_are_converged(weights):
    """The GPU matrix's references at 1e-5 A agree with 2e-5 A well inside its 3e-4 bar, on a structure of every fixture group, a
    malformed angle set, a headline structure and the 256-atom cell (H u and the strain products along (u, 0) and (0, W))."""
    import torch

    import angle_fixtures as af
    from elastic_ref import fd_hvp_strain
    from oracle.chgnet_oracle import OracleCHGNet

    torch.set_num_threads(8)
    o = OracleCHGNet(dict(np.load(os.path.join(GOLDEN, weights))), dtype=torch.float64)
    conv = af.converter()
    groups = af.structure_groups()
    graphs = [conv(groups[name][-1]) for name in sf.GROUPS if name != "md"]
    graphs += [af.malformed_graphs()["b"][0], conv(sf.headline_structures()[sf.HEAD_SAMPLE[1]]), conv(sf.md_cell())]
    rng = np.random.default_rng(5)
    for g in graphs:
        n = len(g.atomic_number)
        u, w = rng.normal(size=(n, 3)), rng.normal(size=(3, 3))
        dirs, strains = [u, np.zeros((n, 3))], [np.zeros((3, 3)), w]
        r1, r2 = fd_hvp_strain(o, [g, g], dirs, strains, 1e-5), fd_hvp_strain(o, [g, g], dirs, strains, 2e-5)
        for part in (0, 1):       # hx, hs; the scale of each block is the structure's (a perfect lattice has no internal strain)
            scale = max(float(np.abs(r[part]).max()) for r in r1)
            err = max(float(np.abs(a[part] - b[part]).max()) for a, b in zip(r1, r2))
            assert err <= 3e-5 * scale, (n, part, err / scale)
