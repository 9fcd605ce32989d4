"""Inputs of the released-0.2.0-architecture route matrix (tests/test_gpu_v020_paths.py, pinned on the CPU by
tests/test_v020_fixtures_cpu.py): the generators of tests/angle_fixtures.py at the architecture's 5 A / 3 A cutoffs, grouped into
single device batches, with seeded cotangents and directions.  Everything is generated, nothing is read from outside the repository.

What only this architecture enters (chgnet_amd/csrc): the constant shift of the bonds outside the bond graph (q_bias / q_shift),
switched per BATCH by A > 0 like the reference (model.py:459); non-null mlp_out biases in the row programs; their gradients
(bond_shift_wgrad, colsum over all Eu bonds); the two-hidden-layer head; zero-padded frequencies; envelope exponent 5."""

from __future__ import annotations

import functools
import zlib

import numpy as np

import angle_fixtures as af

R_ATOM, R_BOND = 5.0, 3.0
SHELL_KS = (2, 13, 14, 15, 16, 32)              # both sides of the 13 / 14 / 15 private-row limits, the edge of WIN_LIST
WEIGHTS = ("v020", "v020_trained_like")
LONG_SEED = 2020
LONG_LIMIT = 65536                              # rows past which the training reductions loop over their capped grids
# groups whose angle sets are not the canonical n (n - 1) blocks of the centre-major index
NONCANONICAL = {"shell_33", "tie"}
PREDICT_GROUPS = ("shell", "shell_33", "tie", "low", "noangle", "noangle_2", "md")
GRAD_GROUPS = ("shell", "shell_33", "low", "noangle", "noangle_2")
PRODUCT_GROUPS = ("shell", "low", "tie")
INDEX_GROUPS = ("tie", "shell_33")
MLP_OUT_BIASES = tuple(f"{kind}.{i}.mlp_out.layers.1.bias" for kind, n in (("atom_conv_layers", 4), ("bond_conv_layers", 3)) for i in range(n))
BOND_BIASES = MLP_OUT_BIASES[4:]


def converter():
    return af.converter(R_ATOM, R_BOND)


@functools.lru_cache(maxsize=None)
def structure_groups() -> dict:
    """name -> list of structures; each group is ONE batch (the shift is a property of the batch)."""
    pair, trimer, chain = af.low_coordination_cells()[:3]
    return {
        "shell": [af.shell_cluster(k) for k in SHELL_KS],
        "shell_33": [af.shell_cluster(33)],
        "tie": af.tie_cells(),
        "low": [pair, trimer, chain],           # the zero-angle pair rides in a batch that has angles: it receives the shift
        "noangle": [pair],                      # A == 0: q_bias off for the whole batch, BondConv never runs
        "noangle_2": [pair, pair],
        "md": af.md_cells()[:1],
    }


@functools.lru_cache(maxsize=None)
def long_structures() -> tuple:
    """The shortest prefix of bench.workload_structures(., LONG_SEED) (40-atom cells) whose batch at 5 / 3 has more than LONG_LIMIT
    directed edges AND angles, with an angle count that is no multiple of 32."""
    import bench

    structs = bench.workload_structures(96, LONG_SEED)
    conv = converter()
    ed = a = 0
    for n, s in enumerate(structs, 1):
        g = conv(s)
        ed += len(np.asarray(g.atom_graph).reshape(-1, 2))
        a += len(np.asarray(g.bond_graph).reshape(-1, 5))
        if ed > LONG_LIMIT and a > LONG_LIMIT and a % 32 != 0:
            return tuple(structs[:n])
    raise AssertionError("no such prefix")


def _rng(key: str):
    return np.random.default_rng(zlib.crc32(("v020/" + key).encode()))


def cotangents(name: str, sizes) -> dict:
    """Seeded e / m / f / s cotangents of one batch (``sizes``: atoms per structure), float32."""
    rng = _rng("cot/" + name)
    n_s, n_a = len(sizes), int(np.sum(sizes))
    return {"e": rng.normal(1, 0.2, n_s).astype(np.float32), "m": rng.normal(size=n_a).astype(np.float32),
            "f": rng.normal(size=(n_a, 3)).astype(np.float32), "s": rng.normal(size=(n_s, 3, 3)).astype(np.float32)}


def directions(name: str, sizes) -> dict:
    """u [N,3] and a general strain W [B,3,3], seeded (the style of tests/second_order_fixtures.directions)."""
    rng = _rng("dir/" + name)
    return {"u": rng.normal(size=(int(np.sum(sizes)), 3)).astype(np.float32),
            "W": rng.normal(size=(len(sizes), 3, 3)).astype(np.float32)}


def sizes_of(structs) -> list:
    return [len(s) for s in structs]
