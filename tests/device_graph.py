"""Fetch the graph of a device-built batch and undo the packing offsets, structure by structure (GPU tests only)."""

from __future__ import annotations

import numpy as np


def fetch_device_graph(engine, batch) -> list[dict]:
    """One dict per structure of a ``build_batch`` result, every index local to the structure: ``center``, ``neighbor``,
    ``image`` (int64), ``directed2undirected``, ``undirected2directed``, ``bond_graph`` [A,5] (through the compact bond-node
    numbering: ``bn_und[a_b1c]``)."""
    pb = batch.packed
    f = lambda name, n: engine.debug_fetch_i32(batch, name, n)  # noqa: E731
    ec, en, d2u, eo = (f(k, pb.n_directed) for k in ("e_center", "e_nbr", "e_d2u", "e_owner"))
    img = engine.debug_fetch(batch, "e_image", (pb.n_directed, 3)).astype(np.int64)
    u2d = f("u_u2d", pb.n_undirected)
    bn = f("bn_und", pb.n_bnodes)
    a_ctr, a_b1c, a_b2c, a_d1, a_d2 = (f(k, pb.n_angles) for k in ("a_ctr", "a_b1c", "a_b2c", "a_d1", "a_d2"))
    a_off = pb.atom_off
    e_off = np.searchsorted(eo, np.arange(pb.n_struct + 1))
    a_owner = np.searchsorted(a_off, a_ctr, side="right") - 1 if pb.n_angles else np.zeros(0, np.int64)
    u_off = e_off // 2
    out = []
    for b in range(pb.n_struct):
        sl = slice(e_off[b], e_off[b + 1])
        rows = np.flatnonzero(a_owner == b)
        bg = np.stack([a_ctr[rows] - a_off[b], bn[a_b1c[rows]] - u_off[b], a_d1[rows] - e_off[b], bn[a_b2c[rows]] - u_off[b],
                       a_d2[rows] - e_off[b]], 1) if len(rows) else np.zeros((0, 5), np.int32)
        out.append({"center": ec[sl] - a_off[b], "neighbor": en[sl] - a_off[b], "image": img[sl], "owner": eo[sl],
                    "directed2undirected": d2u[sl] - u_off[b], "undirected2directed": u2d[u_off[b]:u_off[b + 1]] - e_off[b],
                    "bond_graph": bg})
    return out
