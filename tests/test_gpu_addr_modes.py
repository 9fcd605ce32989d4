"""The two address modes of the large-batch tile kernels (csrc/mfma_tile.h grow: 32-bit row offsets against the uniform table base when
every table span of the batch is below 4 GiB, 64-bit offsets otherwise; picked per batch by engine_predict.hip addr32_mode) and the
operand split on the mixed-precision FMA (csrc/mfma_split.h split8).

The mode and its threshold are read once per process (CHGNET_ADDR_MODE, CHGNET_ADDR32_MAX_BYTES), so every configuration runs in a
fresh child: forced 32, forced 64, and the automatic choice with the threshold below the batch's largest table.  Small batches go
through the large-batch kernels with CHGNET_WIN_MIN_ATOMS_PER_WAVE=0 and the launch sequence of the large batches, as in the parity
tests.  Inputs: the five golden structures as one batch and one thermalised 256-atom Li9Co7O16 cell (two tiles per wave and more,
atoms with up to 18 short bonds: the direct-atomics fallback of the per-atom adjoints)."""

from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import REPO, load_case

pytestmark = pytest.mark.gpu

CASES = ["limno2", "noangle", "s16tri", "s40", "li9co7o16"]
GOLDEN_TOL = {"e": 5e-6, "f": 1e-5, "s": 1e-4}                     # the golden tolerances (tests/test_gpu_round4.py TOL)
MODE_TOL = {"e": 2e-6, "f": 4e-5, "s": 4e-4}                       # old-against-new launch sequence (tests/test_gpu_round6.py)
# The adjoint buffers the tile kernels leave behind, relative to the buffer's largest entry: the bound tests/test_gpu_round6.py puts on
# gradients that reach the same point through two launch sequences (test_fine_tuning_gradient_of_a_device_built_batch_equals_the_
# uploaded_one: max|a - b| <= 2e-5 max|b|).  Both modes run the same arithmetic on the same addresses; only the order in which the fp32
# atomics of different waves land differs.
BUFFERS = ("Gb", "Gang", "GP", "GR", "Gu")
BUF_REL = 2e-5

_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from conftest import load_case
from chgnet_amd import CrystalGraphConverter, Structure
from chgnet_amd.graph.structure import Lattice
from chgnet_amd.engine import Engine
from chgnet_amd.pack import pack_weights
W = dict(np.load(sys.argv[1] + "/tests/golden/weights_seed0.npz"))
eng = Engine(pack_weights(W), 0)
out = {}
def run(tag, graphs):
    b = eng.upload(graphs)
    pb = b.packed
    eng.predict(b, "efs")
    for k, v in eng.download(b, "efs").items():
        out[f"{tag}/{k}"] = v
    N, Ed, A, Eb = pb.n_atoms, pb.n_directed, pb.n_angles, pb.n_bnodes
    for name, shape in (("Gb", (Ed // 2, 64)), ("Gang", (A, 64)), ("GP", (N, 256)), ("GR", (Eb, 256)), ("Gu", (Ed, 4))):
        out[f"{tag}/{name}"] = eng.debug_fetch(b, name, shape)
    out[f"{tag}/route"] = eng.debug_fetch_i32(b, "route", 6)
    out[f"{tag}/flag"] = eng.debug_fetch_i32(b, "win_flag", 4)
    out[f"{tag}/atom_off"] = np.asarray(pb.atom_off)
    b.free()
run("golden", [load_case(n)[0] for n in sys.argv[3].split(",")])
_, d = load_case("li9co7o16")
s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]).make_supercell((2, 2, 2))
rng = np.random.default_rng(3)
s = Structure(s.lattice, s.atomic_numbers, s.frac_coords + rng.normal(0, 0.01, s.frac_coords.shape))
run("md256", [CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3)(s)])
eng.close()
np.savez(sys.argv[2], **out)
'''


def _child(env_extra: dict, tmp: str, name: str) -> dict:
    env = dict(os.environ)
    for k in ("CHGNET_ADDR_MODE", "CHGNET_ADDR32_MAX_BYTES", "CHGNET_TINY_FUSE", "CHGNET_TEAM_MIN_ANGLES", "CHGNET_BLK_MAX_ANGLES"):
        env.pop(k, None)
    # the large-batch kernels on small batches: per-atom kernels, the launch sequence of the large batches, no TEAM / blocked tiles
    env.update({"CHGNET_WIN_MIN_ATOMS_PER_WAVE": "0", "CHGNET_TINY_FUSE": "0", "CHGNET_TEAM_MIN_ANGLES": "-1", "CHGNET_BLK_MAX_ANGLES": "0"})
    env.update(env_extra)
    path = os.path.join(tmp, name + ".npz")
    subprocess.run([sys.executable, "-c", _CHILD, REPO, path, ",".join(CASES)], check=True, env=env, timeout=300)
    return dict(np.load(path))


@pytest.fixture(scope="module")
def runs():
    with tempfile.TemporaryDirectory() as tmp:
        return {"a32": _child({"CHGNET_ADDR_MODE": "32"}, tmp, "a32"),
                "a64": _child({"CHGNET_ADDR_MODE": "64"}, tmp, "a64"),
                "threshold": _child({"CHGNET_ADDR32_MAX_BYTES": "4096"}, tmp, "threshold")}     # below every table of both batches


@pytest.fixture(scope="module")
def md256_oracle(golden_weights):
    """The fp32 oracle on the 256-atom cell (computed once: the graph is the child's, bit for bit -- same seed, same builder)."""
    import torch

    from chgnet_amd import CrystalGraphConverter, Structure
    from chgnet_amd.graph.structure import Lattice
    from oracle.chgnet_oracle import OracleCHGNet

    _, d = load_case("li9co7o16")
    s = Structure(Lattice(d["lattice_f64"]), d["atomic_number"], d["frac_coord_f64"]).make_supercell((2, 2, 2))
    rng = np.random.default_rng(3)
    s = Structure(s.lattice, s.atomic_numbers, s.frac_coords + rng.normal(0, 0.01, s.frac_coords.shape))
    g = CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3)(s)
    torch.set_num_threads(8)
    return OracleCHGNet(golden_weights).predict_graph(g, "efs")


def _diffs(a: dict, b: dict, tag: str) -> list[str]:
    msgs = []
    for k, tol in MODE_TOL.items():
        err = float(np.abs(a[f"{tag}/{k}"] - b[f"{tag}/{k}"]).max())
        print(f"{tag}/{k}: max|d| = {err:.3e} (tol {tol:.1e})")
        if not (np.isfinite(a[f"{tag}/{k}"]).all() and err <= tol):
            msgs.append(f"{tag}/{k}: {err:.3e} > {tol:.1e}")
    for name in BUFFERS:
        x, y = a[f"{tag}/{name}"], b[f"{tag}/{name}"]
        scale = float(np.abs(y).max())
        err = float(np.abs(x - y).max())
        print(f"{tag}/{name}: max|d| = {err:.3e}, max|ref| = {scale:.3e} (tol {BUF_REL:.0e} x max|ref|)")
        if not (np.isfinite(x).all() and scale > 0 and err <= BUF_REL * scale):
            msgs.append(f"{tag}/{name}: {err:.3e} > {BUF_REL:.0e} x {scale:.3e}")
    return msgs


def test_forced_modes_take_their_route_and_agree(runs):
    for tag in ("golden", "md256"):
        assert int(runs["a32"][f"{tag}/route"][5]) == 1 and int(runs["a64"][f"{tag}/route"][5]) == 0
        for r in runs.values():
            assert int(r[f"{tag}/flag"][0]) == 1 and int(r[f"{tag}/route"][3]) == 1      # the per-atom kernels ran
            assert int(r[f"{tag}/route"][0]) == 0 and int(r[f"{tag}/route"][4]) == 0      # not the MD-size launch sequence, not TEAM
    msgs = _diffs(runs["a32"], runs["a64"], "golden") + _diffs(runs["a32"], runs["a64"], "md256")
    assert not msgs, "; ".join(msgs)


def test_threshold_below_the_largest_table_picks_64_bit_offsets(runs):
    for tag in ("golden", "md256"):
        assert int(runs["threshold"][f"{tag}/route"][5]) == 0, "a table above CHGNET_ADDR32_MAX_BYTES must send the batch to 64-bit offsets"
    msgs = _diffs(runs["threshold"], runs["a32"], "golden") + _diffs(runs["threshold"], runs["a32"], "md256")
    assert not msgs, "; ".join(msgs)


@pytest.mark.parametrize("mode", ["a32", "a64"])
def test_each_mode_matches_the_goldens_and_the_oracle(runs, md256_oracle, mode):
    r = runs[mode]
    off = r["golden/atom_off"]
    msgs = []
    for i, name in enumerate(CASES):
        d = load_case(name)[1]
        got = {"e": r["golden/e"][i], "f": r["golden/f"][off[i]:off[i + 1]], "s": r["golden/s"][i]}
        for k, tol in GOLDEN_TOL.items():
            err = float(np.abs(got[k] - d["out_" + k]).max())
            print(f"{mode} {name}/{k}: max|d| = {err:.3e} (tol {tol:.1e})")
            if not err < tol:
                msgs.append(f"{name}/{k}: {err:.3e}")
    ref = md256_oracle
    for k, got, want in (("e", r["md256/e"][0], ref["e"]), ("f", r["md256/f"], ref["f"]), ("s", r["md256/s"][0], ref["s"])):
        err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
        print(f"{mode} md256/{k}: max|d| = {err:.3e} (tol {GOLDEN_TOL[k]:.1e})")
        if not err < GOLDEN_TOL[k]:
            msgs.append(f"md256/{k}: {err:.3e}")
    assert not msgs, "; ".join(msgs)


@pytest.mark.parametrize("f", [64, 128])
def test_split_contraction_on_one_tile_of_rows(hip_engine, f):
    """chg_test_split_gemm (gemm_split / gemm_rm with the operand split on v_fma_mixlo_f16 / v_fma_mixhi_f16) on 16 x 64 and 16 x 128
    rows, all four forms, inside the bounds of tests/test_gpu_round4.py::test_split_contraction_against_float64: every output within
    3e-7 of sum |w| |x| of its row (5e-7 for a row with one non-zero entry), 99.9 % of them within 1.5e-7, mean 3e-8, a row of zeros
    exactly zero."""
    for mode in (0, 1, 2, 3):
        rng = np.random.default_rng(100 * mode + f)
        rows = 16
        adjoint = bool(mode & 1)
        kin = f if adjoint else 64
        mags = 10.0 ** rng.uniform(-7 if adjoint else -4, 4, size=(rows, 1))
        x = (mags * rng.normal(size=(rows, kin))).astype(np.float32)
        x[5] = 0.0
        x[6, 1:] = 0.0
        w = (rng.normal(size=(f, 64)) * 10.0 ** rng.uniform(-2, 0.5, size=(f, 1))).astype(np.float32)
        y = hip_engine.test_split_gemm(x, w, mode)
        x64, w64 = x.astype(np.float64), w.astype(np.float64)
        ref = x64 @ w64 if adjoint else x64 @ w64.T
        bound = np.abs(x64) @ np.abs(w64) if adjoint else np.abs(x64) @ np.abs(w64).T
        assert y.shape == ref.shape and np.isfinite(y).all()
        rel = np.abs(y - ref) / np.maximum(bound, 1e-300)
        dense = np.ones(rows, bool)
        dense[6] = False
        print(f"mode {mode} f {f}: max {rel[dense].max():.2e} q99.9 {np.quantile(rel[dense], 0.999):.2e} mean {rel[dense].mean():.2e} one-entry row {rel[6].max():.2e}")
        assert rel[dense].max() <= 3e-7, (mode, f, float(rel[dense].max()))
        assert np.quantile(rel[dense], 0.999) <= 1.5e-7 and rel[dense].mean() <= 3e-8
        assert rel[6].max() <= 5e-7
        assert np.array_equal(y[5], np.zeros_like(y[5]))
