"""Outputs of the reference's own compiled C graph builder, for the graph-builder tests that compare against it.

    python tests/golden/make_ref_graph_golden.py      # needs the reference checkout (oracle/_refimport.py REFERENCE_ROOT)

Feeds neighbour lists to ``oracle/_ref/libref_graph.so`` (the reference's create_graph.c, compiled from where it lies by
``oracle/ref_graph.py``) and records every input list and what the reference built from it in ``ref_graph_c.json``:

  cpu_<case>_<cutoffs>_<shuffled>     tests/test_graph_builder.py::test_builder_matches_the_references_compiled_c_algorithm:
                                      the structures of ``_cases_for_native_reference``, our builder's neighbour list as
                                      found and shuffled within each centre (numpy default_rng(3), in this loop order)
  gpu_<structure>_<cutoffs>           tests/test_gpu_round2.py::test_device_graph_build_against_the_compiled_reference:
                                      the structures of ``_structures_for_graph_tests``, our builder's neighbour list

Each array is kept as its length and SHA-256 (make_golden_helpers.array_digest), not as its values: the tests need exact
equality only, and the index arrays of these cases would take megabytes.  Inputs: center, neighbor, image, distance;
outputs: atom_graph, directed2undirected, undirected2directed, bond_graph.  CUTOFFS is the (r_atom, r_bond) list both
tests iterate.
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from chgnet_amd.graph.converter import build_graph_arrays  # noqa: E402
from make_golden_helpers import array_digest  # noqa: E402
from oracle import ref_graph  # noqa: E402

CUTOFFS = ((6.0, 3.0), (5.0, 3.0), (4.0, 4.0))
IN_KEYS = ("center", "neighbor", "image", "distance")
OUT_KEYS = ("atom_graph", "directed2undirected", "undirected2directed", "bond_graph")


def neighbour_list(s, r_atom, r_bond) -> dict:
    a = build_graph_arrays(s.frac_coords, s.lattice.matrix, r_atom, r_bond)
    return {"center": a["atom_graph"][:, 0].astype(np.int64), "neighbor": a["atom_graph"][:, 1].astype(np.int64),
            "image": a["image"].astype(np.int64), "distance": a["distance"]}


def record(n_atoms: int, nl: dict, r_bond: float) -> dict:
    ref = ref_graph.reference_graph(n_atoms, nl["center"], nl["neighbor"], nl["image"], nl["distance"], r_bond)
    return {**{k: array_digest(nl[k]) for k in IN_KEYS}, **{k: array_digest(ref[k]) for k in OUT_KEYS}}


def main() -> None:
    from test_gpu_parity import _structures_for_graph_tests
    from test_graph_builder import _cases_for_native_reference

    if ref_graph.build() is None:
        raise SystemExit("the reference's C graph builder cannot be built here")
    out = {}
    rng = np.random.default_rng(3)
    for i, s in enumerate(_cases_for_native_reference()):
        for j, (r_atom, r_bond) in enumerate(CUTOFFS):
            nl = neighbour_list(s, r_atom, r_bond)
            for shuffle in (0, 1):
                if shuffle and len(nl["center"]):
                    perm = np.concatenate([rng.permutation(np.flatnonzero(nl["center"] == c)) for c in range(len(s))])
                    nl = {k: v[perm] for k, v in nl.items()}
                out[f"cpu_{i}_{j}_{shuffle}"] = record(len(s), nl, r_bond)
    for b, s in enumerate(_structures_for_graph_tests()):
        for j, (r_atom, r_bond) in enumerate(CUTOFFS):
            out[f"gpu_{b}_{j}"] = record(len(s), neighbour_list(s, r_atom, r_bond), r_bond)
    with open(os.path.join(HERE, "ref_graph_c.json"), "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
