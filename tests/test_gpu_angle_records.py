"""The index records of the per-atom angle adjoints (csrc/kernels_angle_w.h: WinIndex::rows, one 16-byte record per row of the
centre-major order -- angle, first bond, second bond, rank of the second bond at the centre -- and WinIndex::atoms, one record per
scheduled atom) on the smallest batches on which they can go wrong, in both address modes, through both producers of the row
records: k_win_rows (uploaded graphs) and k_win_pack (graphs built on the device, whose order the builder emits).

Batches:
  golden   the five golden structures as one batch
  low      one cell with atoms that have 0, 1 and 2 bonds inside the bond-graph cutoff: no row, no row, one tile with two valid rows
  high     shell clusters whose centre has 15 and 24 short bonds: second-bond ranks past the 13 / 14 private rows (direct atomics),
           15 x 14 = 210 and 24 x 23 = 552 rows -- neither a multiple of the 16-row tile
  last0    a batch whose last atom has no angles;  first0  a batch whose first atom has none

Every batch runs with the per-atom kernels forced (the switches of tests/test_gpu_addr_modes.py) in 32-bit and in 64-bit address
mode, and once through the row-order adjoint of the same build.  The knobs are read once per process: one child per configuration."""

from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import REPO, load_case

pytestmark = pytest.mark.gpu

GOLDEN_CASES = ["limno2", "noangle", "s16tri", "s40", "li9co7o16"]
GOLDEN_TOL = {"e": 5e-6, "f": 1e-5, "s": 1e-4}          # the golden tolerances (tests/test_gpu_addr_modes.py)
MODE_TOL = {"e": 2e-6, "f": 4e-5, "s": 4e-4}            # two launch sequences of one build (tests/test_gpu_addr_modes.py)
BUFFERS = ("Gang", "GR", "GS", "Gwbgc")
BUF_REL = 2e-5                                          # relative to the buffer's largest entry (tests/test_gpu_addr_modes.py)
PER_ATOM = {"CHGNET_WIN_MIN_ATOMS_PER_WAVE": "0", "CHGNET_TINY_FUSE": "0", "CHGNET_TEAM_MIN_ANGLES": "-1", "CHGNET_BLK_MAX_ANGLES": "0"}
CONFIGS = {
    "a32": {**PER_ATOM, "CHGNET_ADDR_MODE": "32"},
    "a64": {**PER_ATOM, "CHGNET_ADDR_MODE": "64"},
    "row_order": {"CHGNET_TINY_FUSE": "0", "CHGNET_TEAM_MIN_ANGLES": "-1", "CHGNET_BLK_MAX_ANGLES": "0"},
}
KNOBS = ("CHGNET_ADDR_MODE", "CHGNET_ADDR32_MAX_BYTES", "CHGNET_TINY_FUSE", "CHGNET_TEAM_MIN_ANGLES", "CHGNET_BLK_MAX_ANGLES",
         "CHGNET_WIN_MIN_ATOMS_PER_WAVE", "CHGNET_PER_ATOM_FWD", "CHGNET_ZSAVE")


def _golden_structure(name: str):
    from chgnet_amd import Structure
    from chgnet_amd.graph.structure import Lattice

    d = load_case(name)[1]
    return Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"])


def _sparse_cell(order):
    """O - Co - O in a line 2 A apart and a Li 4.5 A from the Co (no bond inside 3 A), in a 14 A cube: short-bond counts 1, 2, 1, 0."""
    import angle_fixtures as af

    atoms = {"Oa": ("O", [5.0, 7.0, 7.0]), "Co": ("Co", [7.0, 7.0, 7.0]), "Ob": ("O", [9.0, 7.0, 7.0]), "Li": ("Li", [7.0, 11.5, 7.0])}
    return af._from_cart(np.eye(3) * 14.0, [atoms[k][0] for k in order], [atoms[k][1] for k in order])


def structure_batches() -> dict:
    """name -> structures (the batches that run through the device builder AND the host converter)."""
    import angle_fixtures as af

    return {
        "low": [_sparse_cell(("Oa", "Co", "Ob", "Li"))],
        "high": [af.shell_cluster(15), af.shell_cluster(24)],
        "last0": [_golden_structure("limno2"), _sparse_cell(("Co", "Oa", "Ob", "Li"))],
        "first0": [_sparse_cell(("Li", "Oa", "Ob", "Co")), _golden_structure("limno2")],
    }


_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import angle_fixtures as af
import test_gpu_angle_records as T
from conftest import load_case
from chgnet_amd.engine import Engine
from chgnet_amd.pack import pack_weights
W = dict(np.load(sys.argv[1] + "/tests/golden/weights_seed0.npz"))
eng = Engine(pack_weights(W), 0)
out = {}
def run(tag, b):
    pb = b.packed
    eng.predict(b, "efs")
    for k, v in eng.download(b, "efs").items():
        out[f"{tag}/{k}"] = v
    N, A, Eb = pb.n_atoms, pb.n_angles, pb.n_bnodes
    for name, shape in (("Gang", (A, 64)), ("GR", (Eb, 256)), ("GS", (N, 128)), ("Gwbgc", (Eb, 64))):
        out[f"{tag}/{name}"] = eng.debug_fetch(b, name, shape)
    out[f"{tag}/route"] = eng.debug_fetch_i32(b, "route", 6)
    out[f"{tag}/flag"] = eng.debug_fetch_i32(b, "win_flag", 4)
    out[f"{tag}/atom_off"] = np.asarray(pb.atom_off)
    b.free()
run("golden/upload", eng.upload([load_case(n)[0] for n in T.GOLDEN_CASES]))
conv = af.converter()
for name, structs in T.structure_batches().items():
    run(name + "/upload", eng.upload([conv(s) for s in structs]))
    run(name + "/device", eng.build_batch(structs, af.R_ATOM, af.R_BOND))
eng.close()
np.savez(sys.argv[2], **out)
'''

TAGS = ["golden/upload"] + [f"{name}/{origin}" for name in ("low", "high", "last0", "first0") for origin in ("upload", "device")]


@pytest.fixture(scope="module")
def runs():
    """One child per configuration, one after another; the first that fails ends the fixture before the next is started."""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for cfg, extra in CONFIGS.items():
            env = dict(os.environ)
            for k in KNOBS:
                env.pop(k, None)
            env.update(extra)
            path = os.path.join(tmp, cfg + ".npz")
            r = subprocess.run([sys.executable, "-c", _CHILD, REPO, path], env=env, timeout=300, capture_output=True, text=True)
            assert r.returncode == 0, f"configuration {cfg}: exit status {r.returncode}\n{r.stderr[-4000:]}"
            res[cfg] = dict(np.load(path))
    return res


@pytest.fixture(scope="module")
def oracle64(golden_weights):
    """float64 oracle of every batch (computed once; the device-built graph equals the converter's bit for bit)."""
    import torch

    import angle_fixtures as af
    from oracle.chgnet_oracle import OracleCHGNet

    torch.set_num_threads(8)
    o = OracleCHGNet(golden_weights, dtype=torch.float64)
    conv = af.converter()
    ref = {"golden": o.predict_graph([load_case(n)[0] for n in GOLDEN_CASES], "efs", batch_size=64)}
    for name, structs in structure_batches().items():
        ref[name] = o.predict_graph([conv(s) for s in structs], "efs", batch_size=64)
    return ref


def test_the_fixtures_have_the_shapes_the_records_branch_on():
    """Short-bond counts of the hand-made cells and of the shell centres, from the host converter's graphs (no GPU work)."""
    import angle_fixtures as af

    conv = af.converter()
    b = structure_batches()
    assert list(af.short_bond_counts(conv(b["low"][0]))) == [0, 2, 0, 0]       # (an atom with one short bond heads no angle row)
    assert len(np.asarray(conv(b["low"][0]).bond_graph).reshape(-1, 5)) == 2   # one tile, two valid rows
    for s, k in zip(b["high"], (15, 24)):
        n = af.short_bond_counts(conv(s))
        assert n[0] == k and k > 14 and (k * (k - 1)) % 16 != 0
    assert af.short_bond_counts(conv(b["last0"][1]))[-1] == 0 and af.short_bond_counts(conv(b["last0"][0]))[0] >= 2
    assert af.short_bond_counts(conv(b["first0"][0]))[0] == 0 and af.short_bond_counts(conv(b["first0"][1]))[-1] >= 2


def test_routes(runs):
    for tag in TAGS:
        for mode, a32 in (("a32", 1), ("a64", 0)):
            r = runs[mode]
            assert int(r[f"{tag}/flag"][0]) == 1 and int(r[f"{tag}/route"][3]) == 1, (mode, tag)      # the per-atom kernels ran
            assert int(r[f"{tag}/route"][0]) == 0 and int(r[f"{tag}/route"][4]) == 0, (mode, tag)      # large-batch sequence, not TEAM
            assert int(r[f"{tag}/route"][5]) == a32, (mode, tag)
        r = runs["row_order"]
        assert int(r[f"{tag}/route"][3]) == 0 and int(r[f"{tag}/route"][4]) == 0, tag                   # row order: no index in use


@pytest.mark.parametrize("mode", ["a32", "a64"])
def test_per_atom_adjoints_equal_the_row_order_adjoint(runs, mode):
    got, ref = runs[mode], runs["row_order"]
    msgs = []
    for tag in TAGS:
        for k, tol in MODE_TOL.items():
            x, y = got[f"{tag}/{k}"], ref[f"{tag}/{k}"]
            err = float(np.abs(x - y).max())
            print(f"{mode} {tag}/{k}: max|d| = {err:.3e} (tol {tol:.1e})")
            if not (np.isfinite(x).all() and err <= tol):
                msgs.append(f"{tag}/{k}: {err:.3e} > {tol:.1e}")
        for name in BUFFERS:
            x, y = got[f"{tag}/{name}"], ref[f"{tag}/{name}"]
            scale = float(np.abs(y).max())
            err = float(np.abs(x - y).max())
            print(f"{mode} {tag}/{name}: max|d| = {err:.3e}, max|ref| = {scale:.3e} (tol {BUF_REL:.0e} x max|ref|)")
            if not (np.isfinite(x).all() and scale > 0 and err <= BUF_REL * scale):
                msgs.append(f"{tag}/{name}: {err:.3e} > {BUF_REL:.0e} x {scale:.3e}")
    assert not msgs, "; ".join(msgs)


@pytest.mark.parametrize("mode", ["a32", "a64"])
def test_per_atom_adjoints_against_the_float64_oracle(runs, oracle64, mode):
    r = runs[mode]
    msgs = []
    for tag in TAGS:
        ref = oracle64[tag.split("/")[0]]
        off = r[f"{tag}/atom_off"]
        for i, want in enumerate(ref):
            got = {"e": r[f"{tag}/e"][i], "f": r[f"{tag}/f"][off[i]:off[i + 1]], "s": r[f"{tag}/s"][i]}
            for k, tol in GOLDEN_TOL.items():
                err = float(np.abs(np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64)).max())
                print(f"{mode} {tag}[{i}]/{k}: max|d| = {err:.3e} (tol {tol:.1e})")
                if not (np.isfinite(got[k]).all() and err < tol):
                    msgs.append(f"{tag}[{i}]/{k}: {err:.3e}")
    assert not msgs, "; ".join(msgs)
