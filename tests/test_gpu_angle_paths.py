"""Every family of angle kernels (BondConv / AngleUpdate) against the float64 oracle at the coordination numbers, cutoff ties and
graph shapes where the kernels branch (tests/angle_fixtures.py), through the device builder and the host converter + upload.

Families and how a batch reaches them (chgnet_amd/csrc/engine_predict.hip launch_angle, decide_windows, prepare_windows): blocked
tiles (k_angle_bwd_blk; index from the builder or k_blk_from_q), team (k_angle_bwd_w<.., true>), per-atom windows (k_angle_bwd_w,
k_angleupd_fwd_a) and row order (k_angle), which is also the fallback whenever the index kernels clear win.flag[0].  The knobs are
read once per process, so every configuration runs in a child process of its own; the children run one after another and the
first one that fails stops the rest."""

from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

KNOBS = ("CHGNET_BLK_MAX_ANGLES", "CHGNET_TEAM_MIN_ANGLES", "CHGNET_WIN_MIN_ATOMS_PER_WAVE", "CHGNET_PER_ATOM_FWD",
         "CHGNET_TINY_FUSE", "CHGNET_TINY_CHAIN", "CHGNET_ZSAVE")
PER_ATOM = {"CHGNET_BLK_MAX_ANGLES": "0", "CHGNET_TEAM_MIN_ANGLES": "-1", "CHGNET_WIN_MIN_ATOMS_PER_WAVE": "0"}
CONFIGS = {
    "default": {},                                                           # blocked tiles (the suite may switch them off)
    "team": {"CHGNET_BLK_MAX_ANGLES": "0", "CHGNET_TEAM_MIN_ANGLES": "0"},
    "per_atom": PER_ATOM,
    "per_atom_rowfwd": {**PER_ATOM, "CHGNET_PER_ATOM_FWD": "0"},
    "row_order": {"CHGNET_BLK_MAX_ANGLES": "0", "CHGNET_TEAM_MIN_ANGLES": "-1"},
}
WEIGHTS = ("seed0", "trained_like")
# groups whose angle sets are not the canonical n (n - 1) blocks of the centre-major index: an atom with more than WIN_LIST = 32
# short bonds, or a bond exactly at the bond cutoff
NONCANONICAL = {"shell_33", "shell_40", "shell_mixed", "tie", "dense"}
GRAD_GROUPS = ("shell_le32", "tie", "shell_40")
GRAD_CONFIGS = ("default", "row_order")
LARGE_SAMPLE = (0, 1, 52, 104, 157, 208, 209)           # structures of the 210-cell batch the oracle checks

_CHILD = r'''
import sys
import numpy as np
repo, out_path, cot_path, cfg = sys.argv[1:5]
sys.path.insert(0, repo); sys.path.insert(0, repo + "/tests")
import angle_fixtures as af
from chgnet_amd.engine import Engine
from chgnet_amd.model import CHGNet
from chgnet_amd.pack import pack_weights
from test_gpu_parity import INT_ARRAYS
GRAD_GROUPS, GRAD_CONFIGS = %r, %r

conv = af.converter()
groups = af.structure_groups()
malformed = af.malformed_graphs()
cots = dict(np.load(cot_path))
out = {}

def fetch(eng, b, name, n):
    try:
        return int(eng.debug_fetch_i32(b, name, n)[0])
    except RuntimeError:              # no such buffer in this batch (no blocked tiles): -1
        return -1

def run(eng, b, tag):
    eng.predict(b, "efsm")
    for k, v in eng.download(b, "efsm", site_energies=True).items():
        out[tag + "/" + k] = v
    out[tag + "/route"] = np.array([fetch(eng, b, "blk_tiles", 1), fetch(eng, b, "win_flag", 4), fetch(eng, b, "wide_range", 1)])
    b.free()

for wname in %r:
    W = dict(np.load(repo + "/tests/golden/weights_" + wname + ".npz"))
    eng = Engine(pack_weights(W), 0)
    for name, structs in groups.items():
        b = eng.build_batch(structs, af.R_ATOM, af.R_BOND)
        if name in ("tie", "dense") and wname == "seed0":       # the device builder's index arrays (compared with the host's)
            out["idx/" + name + "/counts"] = np.array([b.packed.n_directed, b.packed.n_angles, b.packed.n_bnodes])
            for arr, count in INT_ARRAYS.items():
                out["idx/" + name + "/" + arr] = eng.debug_fetch_i32(b, arr, getattr(b.packed, count))
        run(eng, b, wname + "/" + name + "/device")
        run(eng, eng.upload([conv(s) for s in structs]), wname + "/" + name + "/upload")
    run(eng, eng.build_batch(af.large_batch(), af.R_ATOM, af.R_BOND), wname + "/large/device")
    for kind, gs in malformed.items():
        run(eng, eng.upload(gs), wname + "/malformed_" + kind + "/upload")
    if cfg in GRAD_CONFIGS:       # fine-tuning gradient: chg_backward starts from the first-order adjoints of these paths
        model = CHGNet(state_dict=W)
        model._engine = eng
        for name in GRAD_GROUPS:
            c = [cots[name + "/" + k] for k in ("e", "m", "f", "s")]
            for origin in ("device", "upload"):
                if origin == "device":
                    b = eng.build_batch(groups[name], af.R_ATOM, af.R_BOND)
                    model.forward(b.packed, task="efsm", device_batch=b)
                else:
                    model.forward([conv(s) for s in groups[name]], task="efsm")
                for k, v in model.backward(*c).items():
                    out["grad/" + wname + "/" + name + "/" + origin + "/" + k] = v
                model.release_forward_state()
        model._engine = None
    eng.close()
np.savez(out_path, **out)
''' % (GRAD_GROUPS, GRAD_CONFIGS, WEIGHTS)


def _run_configs(tmp: str, cot_path: str) -> dict:
    """One child per configuration, in order; the first failure (exit status, signal or time-out) ends the test before the next
    child is started."""
    res = {}
    for cfg, extra in CONFIGS.items():
        env = dict(os.environ)
        for k in KNOBS:
            if not (cfg == "default" and k == "CHGNET_BLK_MAX_ANGLES"):
                env.pop(k, None)
        env.update(extra)
        path = os.path.join(tmp, cfg + ".npz")
        r = subprocess.run([sys.executable, "-c", _CHILD, REPO, path, cot_path, cfg], env=env, timeout=600, capture_output=True, text=True)
        assert r.returncode == 0, f"configuration {cfg}: exit status {r.returncode}\n{r.stderr[-4000:]}"
        res[cfg] = dict(np.load(path))
    return res


def _cotangents(groups) -> dict:
    rng = np.random.default_rng(41)
    out = {}
    for name in GRAD_GROUPS:
        n_s, n_a = len(groups[name]), sum(len(s) for s in groups[name])
        out[name + "/e"] = rng.normal(1, 0.2, n_s).astype(np.float32)
        out[name + "/m"] = rng.normal(size=n_a).astype(np.float32)
        out[name + "/f"] = rng.normal(size=(n_a, 3)).astype(np.float32)
        out[name + "/s"] = rng.normal(size=(n_s, 3, 3)).astype(np.float32)
    return out


def _expected_flag(cfg: str, group: str, origin: str, blk_on: bool):
    """win_flag[0] the index kernels must leave (None: no index is built, or its flag does not decide the route)."""
    if group == "large":
        return 1                                  # every configuration: per-atom windows, index from k_win_* (prepare_windows)
    if group.startswith("malformed_"):
        if cfg == "default":
            return 0 if blk_on else None          # k_blk_from_q / k_win_*: all four defects send the batch to the row-order kernel
        if cfg == "row_order":
            return None
        # the per-atom index keys rows by position: a repeated pair (b) or a foreign second bond (d) is valid input for it, and
        # the oracle comparison decides
        return 0 if group[-1] in ("a", "c") else None
    if cfg == "row_order" or (cfg == "default" and (not blk_on or origin == "device")):
        return None                               # (device-built, default: the builder writes the blocked tiles, or none at all)
    return 0 if group in NONCANONICAL else 1


def _route_name(cfg: str, name: str, origin: str, tiles: int, flag: int, blk_on: bool) -> tuple[str, str]:
    """(win_flag[0] where an index was built, else "-"; the kernels that did the angle adjoints)."""
    if cfg == "default" and not blk_on:
        return "-", "default (blocked tiles off)"
    if tiles > 0:
        if origin == "device":
            return "-", "blocked tiles"                       # (the builder's index: no flag)
        return str(flag), "blocked tiles" if flag == 1 else "blocked tiles -> row order"
    per_atom = "per-atom, row-order fwd" if cfg == "per_atom_rowfwd" else "per-atom"
    if name == "large":
        base = per_atom                                       # N + 1 > 8192: neither blocked tiles nor team
    elif cfg == "team":
        base = "team"
    elif cfg.startswith("per_atom"):
        base = per_atom
    else:
        return "-", "row order"
    return str(flag), base if flag == 1 else base + " -> row order"


def _oracle(weights, graphs):
    import torch

    from oracle.chgnet_oracle import OracleCHGNet

    kw = dict(return_site_energies=True, batch_size=64)
    return (OracleCHGNet(weights, dtype=torch.float64).predict_graph(graphs, "efsm", **kw),
            OracleCHGNet(weights).predict_graph(graphs, "efsm", **kw))


def test_every_angle_path_against_the_float64_oracle():
    """Five configurations (blocked tiles, team, per-atom, per-atom with the row-order forward, row order) x device-built and
    uploaded graphs x both weight sets: shell clusters with 2 ... 40 short bonds at the centre (both sides of NS, FA_NSL and
    WIN_LIST, every blocked-tile shape), bonds exactly at the bond cutoff, 42 short bonds per atom, 0-2 angles per atom, the 256- and
    512-atom MD cells, an 8,400-atom device-built batch (per-atom index from k_win_*) and four malformed uploaded angle sets.
    E / F / S / M and site energies against OracleCHGNet(float64) within max(TOL x scale, 20 x the fp32 oracle's own error); the route
    each batch took (blocked tiles, win.flag[0], wide-range sweep); the device builder's index arrays == the host converter's at the
    cutoff ties and the dense cell; CHGNet.backward == the float64 oracle's parameter gradients under blocked tiles and row order."""
    import torch

    import angle_fixtures as af
    from chgnet_amd.pack import pack_batch
    from oracle.chgnet_oracle import OracleCHGNet
    from test_gpu_parity import INT_ARRAYS, TOL
    from test_gpu_train import REL_TOL_B

    blk_on = os.environ.get("CHGNET_BLK_MAX_ANGLES") is None       # (the suite is also run with the blocked tiles switched off)
    groups = af.structure_groups()
    conv = af.converter()
    cots = _cotangents(groups)
    with tempfile.TemporaryDirectory() as tmp:
        cot_path = os.path.join(tmp, "cot.npz")
        np.savez(cot_path, **cots)
        res = _run_configs(tmp, cot_path)

    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    graphs = {name: [conv(s) for s in structs] for name, structs in groups.items()}
    large = af.large_batch()
    graphs["large"] = [conv(large[i]) for i in LARGE_SAMPLE]
    graphs.update({"malformed_" + k: v for k, v in af.malformed_graphs().items()})
    large_off = np.concatenate([[0], np.cumsum([len(s) for s in large])])
    msgs, table = [], []
    for wname in WEIGHTS:
        weights = dict(np.load(os.path.join(GOLDEN, f"weights_{wname}.npz")))
        for name, gs in graphs.items():
            o64, o32 = _oracle(weights, gs)
            if name == "large":
                idx, off = list(LARGE_SAMPLE), large_off
            else:
                idx, off = list(range(len(gs))), np.concatenate([[0], np.cumsum([len(g.atomic_number) for g in gs])])
            origins = ("device",) if name == "large" else ("upload",) if name.startswith("malformed_") else ("device", "upload")
            for cfg, got in res.items():
                for origin in origins:
                    tag = f"{wname}/{name}/{origin}"
                    tiles, flag, wide = (int(x) for x in got[tag + "/route"])
                    tiles = max(tiles, 0)
                    want_flag = _expected_flag(cfg, name, origin, blk_on)
                    if wname == WEIGHTS[0]:
                        table.append((name, origin, cfg, tiles, *_route_name(cfg, name, origin, tiles, flag, blk_on)))
                    if wide != 0:
                        msgs.append(f"{cfg} {tag}: ran on the wide-range sweep")
                    if want_flag is not None and flag != want_flag:
                        msgs.append(f"{cfg} {tag}: win_flag {flag}, expected {want_flag}")
                    if cfg == "default" and blk_on and name != "large":
                        want_tiles = not (origin == "device" and name in NONCANONICAL)
                        if (tiles > 0) != want_tiles:
                            msgs.append(f"{cfg} {tag}: {tiles} blocked tiles")
                    elif cfg != "default" and tiles != 0:
                        msgs.append(f"{cfg} {tag}: {tiles} blocked tiles with the blocked tiles off")
                    for i, r64, r32 in zip(idx, o64, o32):
                        sl = slice(off[i], off[i + 1])
                        for key in ("e", "f", "s", "m", "site_energies"):
                            v = got[f"{tag}/{key}"]
                            g = v[i] if key in ("e", "s") else v[sl]
                            ref = np.asarray(r64[key], np.float64)
                            if ref.size == 0:
                                continue
                            ref_err = float(np.abs(np.asarray(r32[key], np.float64) - ref).max())
                            err = float(np.abs(g - ref).max())
                            scale = max(1.0, float(np.abs(ref).max()))
                            if not np.isfinite(g).all() or not err < max(TOL[key] * scale, 20 * ref_err):
                                msgs.append(f"{cfg} {tag}[{i}] {key}: {err:.3e} vs fp32 oracle {ref_err:.3e} (scale {scale:.3g})")
        for name in GRAD_GROUPS:      # fine-tuning gradients
            want, want32 = ({}, {})
            for dt, dst in ((torch.float64, want), (torch.float32, want32)):
                t = {k: torch.tensor(np.asarray(cots[f"{name}/{k}"]), dtype=dt) for k in ("e", "m", "f", "s")}
                dst.update(OracleCHGNet(weights, dtype=dt).parameter_gradients(
                    graphs[name], lambda o: (o["e"] * t["e"]).sum() + (o["m"] * t["m"]).sum() + (o["f"] * t["f"]).sum() + (o["s"] * t["s"]).sum(),
                    task="efsm"))
            for cfg in GRAD_CONFIGS:
                for origin in ("device", "upload"):
                    for k, ref in want.items():
                        got = res[cfg][f"grad/{wname}/{name}/{origin}/{k}"]
                        if k.startswith(("angle_layers.2.", "composition_model")):
                            if np.any(got):
                                msgs.append(f"grad {cfg} {wname}/{name}/{origin} {k}: not zero")
                            continue
                        scale, err = float(np.abs(ref).max()), float(np.abs(got - ref).max())
                        # (floor: 3x the fp32 oracle's own error -- the exact fcc tie cell has collinear angles, where an fp32
                        # arccos is off by ~sqrt(eps): the Fourier frequencies' gradient of the fp32 oracle is 5e-4 off there)
                        ref_err = float(np.abs(want32[k] - ref).max())
                        if not np.isfinite(got).all() or not err <= max(REL_TOL_B * scale, 3 * ref_err):
                            msgs.append(f"grad {cfg} {wname}/{name}/{origin} {k}: {err:.3e} / {scale:.3e} (fp32 oracle {ref_err:.3e})")
    for name in ("tie", "dense"):     # the cutoff ties and the dense cell: the device builder's index arrays == the host converter's
        want = pack_batch(graphs[name])
        for cfg, got in res.items():
            if not np.array_equal(got[f"idx/{name}/counts"], [want.n_directed, want.n_angles, want.n_bnodes]):
                msgs.append(f"{cfg} idx/{name}: counts {got[f'idx/{name}/counts']}")
                continue
            for arr in INT_ARRAYS:
                if not np.array_equal(got[f"idx/{name}/{arr}"], want.arrays[arr]):
                    msgs.append(f"{cfg} idx/{name}/{arr} differs from the host converter's")
    print("\nroute per fixture group (weights_seed0; tiles = blk_tiles, flag = win_flag[0])")
    print(f"{'group':<20} {'origin':<7} {'configuration':<16} {'tiles':>6} {'flag':>5}  route")
    for row in table:
        print(f"{row[0]:<20} {row[1]:<7} {row[2]:<16} {row[3]:>6} {row[4]:>5}  {row[5]}")
    assert not msgs, f"{len(msgs)} failures:\n" + "\n".join(msgs[:80])
