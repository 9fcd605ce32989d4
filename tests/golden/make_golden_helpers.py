"""Shared by the fixture generators and the tests that read their fixtures: what the reference converter touches on a
pymatgen Structure (chgnet/graph/converter.py:120-134, 162, 187), served from one of our structures plus a neighbour list;
and the compact record of an array a fixture keeps instead of the array itself."""

from __future__ import annotations

import hashlib

import numpy as np


def array_digest(a) -> dict:
    """Length and SHA-256 of an array's values, flattened row-major (integers as int64, floats as float64): two arrays have the
    same record exactly when they hold the same values in the same order, whatever their integer width or shape."""
    a = np.asarray(a)
    a = np.ascontiguousarray(a.reshape(-1), np.float64 if a.dtype.kind == "f" else np.int64)
    return {"n": int(a.size), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


class DuckStructure:
    def __init__(self, s, nl: dict) -> None:
        self._s, self._nl = s, nl
        self.frac_coords = s.frac_coords
        self.lattice = s.lattice
        self.sites = s.sites
        self.composition = s.composition

    def __len__(self):
        return len(self._s)

    def __iter__(self):
        return iter(self._s)

    def get_neighbor_list(self, r, sites=None, numerical_tol=1e-8):  # noqa: ARG002
        nl = self._nl
        return nl["center"], nl["neighbor"], nl["image"], nl["distance"]
