"""The hard-cell batch of the pair-histogram tests (tests/test_gpu_md_observe.py, tests/test_gpu_md_magmom.py): two rattled snapshots of
every hard cell of tests/graph_hard_cases.py as one batch, with the float64 restatement's histograms (tests/md_observe_ref.py)."""

from __future__ import annotations

import functools

import numpy as np

import graph_hard_cases
import md_observe_ref as ref

HARD = ("shear_30", "shear_150", "shear_mixed", "thin_needle", "thin_slab", "thin_cube16", "left_handed", "coord_p3999", "tri8_1000")
FAR = ("coord_p3999", "tri8_1000")     # the restatement wraps these with np.round
RATTLE_SEED = 2                         # chosen on the CPU: the restatement's edge guard passes on every input below
BINS, RMAX = 64, 6.0


@functools.lru_cache(maxsize=None)
def hard_batch():
    """Two rattled snapshots of every hard cell as one batch, and the restatement's histograms (its edge guard asserts inside)."""
    rng = np.random.default_rng(RATTLE_SEED)
    zs, carts, cells = [], [], []
    for name in HARD:
        if name == "tri8_1000":                      # unwrapped positions: atoms displaced by up to 1000 lattice vectors
            s = graph_hard_cases.tri8()
            frac = s.frac_coords + rng.integers(-1000, 1001, (len(s), 3))
        else:
            s, _ = graph_hard_cases.case(name)
            frac = np.asarray(s.frac_coords, np.float64)
        L = np.asarray(s.lattice.matrix, np.float64)
        r0 = frac @ L + rng.normal(0, 0.03, (len(s), 3))
        carts.append(np.stack([r0, r0 + rng.normal(0, 0.05, (len(s), 3))]))
        cells.append(L)
        zs.append(np.asarray(s.atomic_numbers))
    sizes = [len(z) for z in zs]
    assert 1 in sizes and max(sizes) > 16
    assert RMAX > 2 * ref.heights(cells[HARD.index("thin_slab")]).min()          # several self-images inside rmax
    aoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    kinds, species = np.unique(np.concatenate(zs), return_inverse=True)
    species = species.astype(np.int32)
    pos = np.concatenate(carts, axis=1)
    cell_t = np.tile(np.stack(cells), (2, 1, 1, 1))
    status = np.zeros((2, len(HARD)), np.int32)
    status[1, HARD.index("shear_150")] = 1                                       # stopped before the second snapshot
    want = {"rdf": [], "rdf_samples": [], "vol_sum": []}
    for o, name in enumerate(HARD):
        one = ref.pair_histogram(pos[:, aoff[o]:aoff[o + 1]], cell_t[:, o:o + 1], status[:, o:o + 1], np.array([0, sizes[o]]),
                                 species[aoff[o]:aoff[o + 1]], len(kinds), BINS, RMAX, wrap=name in FAR)
        for k in want:
            want[k].append(one[k][0])
    return aoff, species, len(kinds), pos, cell_t, status, {k: np.stack(v) for k, v in want.items()}
