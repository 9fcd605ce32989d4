"""Inputs of the second-order route matrix (tests/test_gpu_second_order_paths.py, pinned on the CPU by
tests/test_second_order_fixtures_cpu.py): the headline-shaped batch, the 256-atom cell at predict_hessian's default batching, seeded
directions and strains, and the moved geometries of the chg_batch_update_geometry cases.  Everything is generated, nothing is read
from outside the repository."""

from __future__ import annotations

import copy
import zlib

import numpy as np

GROUPS = ("shell_le32", "shell_33", "shell_40", "tie", "dense", "low", "md")
HEAD_N = 1024                                   # bench.py's headline: 1,024 LiMnO2 5 x 1 x 1 cells, 40,960 atoms in one batch
HEAD_SEED = 0
HEAD_SAMPLE = (0, 205, 410, 614, 819, 1023)     # structures the oracle checks
GRAD_SAMPLE = (1, 341, 682, 1022)               # structures with nonzero fine-tuning cotangents
HESS_COLS = tuple(int(c) for c in np.linspace(0, 767, 12).round())   # sampled columns of the 256-atom cell's Hessian
MOVE_SIGMA = 0.02                               # A: displacement of the update_geometry cases


def headline_structures():
    import bench

    return bench.workload_structures(HEAD_N, HEAD_SEED)


def md_cell():
    """The thermalised 256-atom Li9Co7O16 cell of tests/angle_fixtures.md_cells."""
    import angle_fixtures as af

    return af.md_cells()[0]


def _rng(key: str):
    return np.random.default_rng(zlib.crc32(key.encode()))


def directions(key: str, sizes) -> dict:
    """Seeded inputs of one batch (``sizes``: atoms per structure): u, v [N,3]; a general strain W [B,3,3]; a translation t (one
    vector per structure, repeated on its atoms) [N,3]; an antisymmetric strain R [B,3,3]."""
    rng = _rng(key)
    sizes = np.asarray(sizes, np.int64)
    n, b = int(sizes.sum()), len(sizes)
    r = rng.normal(size=(b, 3, 3))
    return {"u": rng.normal(size=(n, 3)).astype(np.float32),
            "W": rng.normal(size=(b, 3, 3)).astype(np.float32),
            "v": rng.normal(size=(n, 3)).astype(np.float32),
            "t": np.repeat(rng.normal(size=(b, 3)), sizes, axis=0).astype(np.float32),
            "R": (r - r.transpose(0, 2, 1)).astype(np.float32)}


def moved(graphs, key: str) -> list:
    """Copies of ``graphs`` with every atom displaced by ~MOVE_SIGMA A (same graph; float32 fractional coordinates, as a batch holds
    them)."""
    rng = _rng("move/" + key)
    out = []
    for g in graphs:
        lat = np.asarray(g.lattice, np.float64).reshape(3, 3)
        d = rng.normal(0, MOVE_SIGMA, (len(g.atomic_number), 3))
        h = copy.copy(g)
        h.atom_frac_coord = (np.asarray(g.atom_frac_coord, np.float64) + d @ np.linalg.inv(lat)).astype(np.float32)
        out.append(h)
    return out


def head_cotangents(sizes) -> dict:
    """Fine-tuning cotangents of the headline batch: random on the GRAD_SAMPLE structures, zero everywhere else."""
    rng = _rng("head/cot")
    sizes = np.asarray(sizes, np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    n, b = int(off[-1]), len(sizes)
    e, m, f, s = np.zeros(b, np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros((b, 3, 3), np.float32)
    for i in GRAD_SAMPLE:
        sl = slice(off[i], off[i + 1])
        e[i] = rng.normal(1, 0.2)
        m[sl] = rng.normal(size=sizes[i])
        f[sl] = rng.normal(size=(sizes[i], 3))
        s[i] = rng.normal(size=(3, 3))
    return {"e": e, "m": m, "f": f, "s": s}
