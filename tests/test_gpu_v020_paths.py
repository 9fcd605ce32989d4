"""The released 0.2.0 architecture (9 + 9 basis functions zero-padded to 31, a 64-64 head, cutoffs 5 / 3, envelope exponent 5,
``mlp_out`` biases) against the float64 oracle on every kernel route.  What only this architecture enters sits inside
route-specific kernels and launch sequences: the constant shift of the bonds outside the bond graph (q_bias / q_shift in
k_atomconv_fwd, gemm_Q / gemm_Qnode, the chained row programs), switched per BATCH by A > 0; non-null ``mlp_out`` biases in
k_rows_chain / k_rows_gemm / k_rows_gemm_multi; their gradients (bond_shift_wgrad, colsum over all Eu bonds) after whichever angle
adjoint the batch took; the two-hidden-layer head in k_readout, its adjoint and the second-order readout; zero-padded frequencies
in the embedding kernels, fused and as separate launches.

Configurations: the five angle-adjoint families of tests/test_gpu_angle_paths.py, the large-batch launch sequence with 32-bit and
with 64-bit row offsets, the fused sequence without chained row GEMMs, the wide-range compile; the ``long`` batch (training
reductions past 65,536 rows) with k_xty3 and with k_xty.  The knobs are read once per process, so every configuration is one child
process and one parametrised test; children run one after another, each under its own time-out, and after the first child that
exits non-zero, dies on a signal or times out no further child is started (the remaining cases fail without running).  The children
run the engine only; the parent computes the float64 references (tests/v020_fixtures.py
batches, the oracle called with the ENGINE's batch: the shift is a property of the batch) once, while the first child runs."""

from __future__ import annotations

import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np
import pytest

import v020_fixtures as vf
from conftest import GOLDEN, REPO
from test_gpu_angle_paths import CONFIGS as ANGLE_CONFIGS
from test_gpu_angle_paths import KNOBS as ANGLE_KNOBS
from test_gpu_angle_paths import _expected_flag
from test_gpu_second_order_paths import CROSS_TOL, PRODUCTS, REL_TOL, REPLAY_TOL, _block_scale, _rel
from test_v020 import DEAD, V020_ARGS

pytestmark = pytest.mark.gpu

NO_FUSE = {"CHGNET_TINY_FUSE": "0"}
CONFIGS = {**ANGLE_CONFIGS, "no_fuse": NO_FUSE, "no_fuse_addr64": {**NO_FUSE, "CHGNET_ADDR_MODE": "64"},
           "no_chain": {"CHGNET_TINY_CHAIN": "0"}, "wide": {"CHGNET_WIDE_RANGE": "1"}}
LONG_CONFIGS = {"long": {}, "long_f32_mfma": {"CHGNET_XTY3": "0"}}
DEFAULT_LIKE = ("default", "no_fuse", "no_fuse_addr64", "no_chain", "wide", *LONG_CONFIGS)     # the angle knobs at their defaults
KNOBS = (*ANGLE_KNOBS, "CHGNET_ADDR_MODE", "CHGNET_ADDR32_MAX_BYTES", "CHGNET_WIDE_RANGE", "CHGNET_XTY3")
CHILD_TIMEOUT = 300                      # s: a limit, not an expectation (tests/test_gpu_angle_records.py)
GRAD_TOL_2 = 3.2e-4                      # a loss with force / stress terms (tests/test_v020.py, tests/test_gpu_train.py)
XTY_TOL = 2e-5                           # k_xty3 vs k_xty (tests/test_gpu_train.py: the three-piece bf16 contraction vs the f32 MFMA one)
LONG_CHUNK = 8                           # structures per oracle call of the long batch (every chunk has angles: the same shift)
ROUTE_FIELDS = ("tiny", "chained", "zsave", "win_built", "team", "a32", "blk_tiles", "win_flag", "wide", "N", "Ed", "A", "Eb")
OUT_KEYS = ("e", "f", "s", "m", "site_energies")
ORIGINS = ("device", "upload")
MOVE_KEY = "v020/low"
_FAILED: list = []                       # the configuration whose child failed: no further child is started


# ---- child: the engine only ------------------------------------------------------------------------------------------------------

def _route(eng, b) -> np.ndarray:
    def fetch(name, n):
        try:
            return eng.debug_fetch_i32(b, name, n)
        except RuntimeError:          # no such buffer in this batch (no blocked tiles): -1
            return np.full(n, -1, np.int32)

    pb = b.packed
    return np.array([*eng.debug_fetch_i32(b, "route", 6), fetch("blk_tiles", 1)[0], fetch("win_flag", 4)[0],
                     eng.debug_fetch_i32(b, "wide_range", 1)[0], pb.n_atoms, pb.n_directed, pb.n_angles, pb.n_bnodes], np.int64)


def _batch(eng, origin, structs, graphs):
    return eng.build_batch(structs, vf.R_ATOM, vf.R_BOND) if origin == "device" else eng.upload(graphs)


def _products(eng, b, d, out, tag):
    """E + F, then H u and the strain products along (u, W), (0, W), (u, 0)."""
    eng.predict(b, "ef")
    out[tag + "/route"] = _route(eng, b)
    out[tag + "/h"] = eng.hessian_vector(b, d["u"])
    zu, zw = np.zeros_like(d["u"]), np.zeros_like(d["W"])
    for kind, (u, w) in (("uw", (d["u"], d["W"])), ("0w", (zu, d["W"])), ("u0", (d["u"], zw))):
        out[f"{tag}/{kind}_x"], out[f"{tag}/{kind}_s"] = eng.hessian_vector_strain(b, u, w)


def _replay_and_geometry(eng, b, graphs, d, out, tag):
    """(after _products on ``b``) three predictions -- eager, captured, replayed -- then H u; chg_batch_update_geometry to moved
    positions, a prediction, H u; and H u of a fresh batch at the moved positions."""
    import second_order_fixtures as sf

    for _ in range(3):
        eng.predict(b, "ef")
    out[tag + "/replay_route"] = _route(eng, b)
    out[tag + "/replay_h"] = eng.hessian_vector(b, d["u"])
    mv = sf.moved(graphs, MOVE_KEY)
    b.update_geometry(frac=np.concatenate([g.atom_frac_coord for g in mv]))
    eng.predict(b, "ef")
    out[tag + "/geo_route"] = _route(eng, b)
    out[tag + "/geo_h"] = eng.hessian_vector(b, d["u"])
    fresh = eng.upload(mv)
    try:
        eng.predict(fresh, "ef")
        out[tag + "/fresh_h"] = eng.hessian_vector(fresh, d["u"])
    finally:
        fresh.free()


def child(out_path: str, cfg: str) -> None:
    from chgnet_amd.engine import Engine
    from chgnet_amd.model import CHGNet
    from chgnet_amd.pack import pack_batch, pack_weights
    from test_gpu_parity import INT_ARRAYS

    conv = vf.converter()
    out = {}
    if cfg in LONG_CONFIGS:
        structs = vf.long_structures()
        pb = pack_batch([conv(s) for s in structs])
        assert pb.n_directed > vf.LONG_LIMIT and pb.n_angles > vf.LONG_LIMIT and pb.n_angles % 32 != 0, (pb.n_directed, pb.n_angles)
        c = vf.cotangents("long", vf.sizes_of(structs))
    else:
        groups = vf.structure_groups()
        graphs = {name: [conv(s) for s in structs] for name, structs in groups.items()}
    for wname in vf.WEIGHTS:
        W = dict(np.load(os.path.join(GOLDEN, f"weights_{wname}.npz")))
        eng = Engine(pack_weights(W, V020_ARGS), 0)
        if cfg in LONG_CONFIGS:
            b = eng.upload(pb)
            try:
                eng.predict(b, "efsm")
                out[f"{wname}/long/route"] = _route(eng, b)
                out[f"{wname}/long/grad1"] = eng.backward(b, c["e"], c["m"])
                out[f"{wname}/long/grad2"] = eng.backward(b, c["e"], c["m"], c["f"], c["s"])
            finally:
                b.free()
            eng.close()
            continue
        model = CHGNet(state_dict=W, **V020_ARGS)
        model._engine = eng
        # 1. predictions, from both origins; 2. the device builder's index arrays at the non-canonical groups
        for name in vf.PREDICT_GROUPS:
            for origin in ORIGINS:
                tag = f"{wname}/{name}/{origin}"
                b = _batch(eng, origin, groups[name], graphs[name])
                try:
                    if origin == "device" and name in vf.INDEX_GROUPS and wname == vf.WEIGHTS[0]:
                        out[f"idx/{name}/counts"] = np.array([b.packed.n_directed, b.packed.n_angles, b.packed.n_bnodes])
                        for arr, count in INT_ARRAYS.items():
                            out[f"idx/{name}/{arr}"] = eng.debug_fetch_i32(b, arr, getattr(b.packed, count))
                    eng.predict(b, "efsm")
                    for k, v in eng.download(b, "efsm", site_energies=True).items():
                        out[f"{tag}/{k}"] = v
                    out[tag + "/route"] = _route(eng, b)
                finally:
                    b.free()
        # 3. parameter gradients: first order after an energy-only forward (chg_backward builds the Q tables: atomconv_q_table),
        # and the full e / m / f / s loss after task = "efsm"
        for name in vf.GRAD_GROUPS:
            c = vf.cotangents(name, vf.sizes_of(groups[name]))
            for origin in ORIGINS:
                for kind, task, cot in (("grad1", "e", (c["e"], c["m"])), ("grad2", "efsm", (c["e"], c["m"], c["f"], c["s"]))):
                    tag = f"{kind}/{wname}/{name}/{origin}"
                    if origin == "device":
                        b = eng.build_batch(groups[name], vf.R_ATOM, vf.R_BOND)
                        model.forward(b.packed, task=task, device_batch=b)
                    else:
                        model.forward(graphs[name], task=task)
                    try:
                        out[tag + "/route"] = _route(eng, model._fwd_batch)
                        for k, v in model.backward(*cot).items():
                            out[f"{tag}/{k}"] = v
                    finally:
                        model.release_forward_state()
        # 4. Hessian products; on ``low`` (upload) again after three predictions, after update_geometry and on a fresh batch
        for name in vf.PRODUCT_GROUPS:
            d = vf.directions(name, vf.sizes_of(groups[name]))
            for origin in ORIGINS:
                tag = f"prod/{wname}/{name}/{origin}"
                b = _batch(eng, origin, groups[name], graphs[name])
                try:
                    _products(eng, b, d, out, tag)
                    if name == "low" and origin == "upload":
                        _replay_and_geometry(eng, b, graphs[name], d, out, tag)
                finally:
                    b.free()
        model._engine = None
        eng.close()
    np.savez(out_path, **out)


_CHILD = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']; import test_gpu_v020_paths as t; t.child(*sys.argv[2:])"


def _run_child(cfg: str) -> dict:
    """One child under its own time-out; a non-zero exit status, a signal or the time-out fails the calling test here."""
    if _FAILED:
        pytest.fail(f"configuration {cfg}: not started, the child of configuration {_FAILED[0]} failed")
    env = dict(os.environ)
    for k in KNOBS:
        if not (cfg in DEFAULT_LIKE and k == "CHGNET_BLK_MAX_ANGLES"):       # (the suite is also run with the blocked tiles off)
            env.pop(k, None)
    env.update({**CONFIGS, **LONG_CONFIGS}[cfg])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, cfg + ".npz")
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, "-c", _CHILD, REPO, path, cfg], env=env, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            _FAILED.append(cfg)
            pytest.fail(f"configuration {cfg}: time-out after {CHILD_TIMEOUT} s")
        if r.returncode != 0:
            _FAILED.append(cfg)
        assert r.returncode == 0, f"configuration {cfg}: exit status {r.returncode}\n{r.stderr[-4000:]}"
        print(f"configuration {cfg}: child ran {time.time() - t0:.1f} s")
        return dict(np.load(path))


# ---- parent: float64 references, computed once -----------------------------------------------------------------------------------

def _oracle(w, dtype):
    from oracle.chgnet_oracle import OracleCHGNet

    return OracleCHGNet(w, atom_graph_cutoff=vf.R_ATOM, bond_graph_cutoff=vf.R_BOND, cutoff_coeff=5, dtype=dtype)


def _loss(cot, dt, keys):
    import torch

    t = {k: torch.tensor(np.asarray(cot[k]), dtype=dt) for k in keys}
    return lambda r: sum((r[k] * t[k]).sum() for k in keys)


def _grad_pair(w, graphs, cot, keys, task):
    """(float64, float32) oracle parameter gradients of the seeded loss on ONE oracle batch."""
    import torch

    return tuple(_oracle(w, dt).parameter_gradients(graphs, _loss(cot, dt, keys), task=task) for dt in (torch.float64, torch.float32))


def _split_cot(cot, off, lo, hi):
    return {"e": cot["e"][lo:hi], "s": cot["s"][lo:hi], "m": cot["m"][off[lo]:off[hi]], "f": cot["f"][off[lo]:off[hi]]}


def _strain_refs(o, graphs, d, off):
    """Per graph: the references of the products, from the two central differences along (u, 0) and (0, W); ONE oracle batch per
    central difference (2 x len(graphs) graphs)."""
    from elastic_ref import fd_hvp_strain

    us = [d["u"][off[i]:off[i + 1]] for i in range(len(graphs))]
    n = 2 * len(graphs)
    a = fd_hvp_strain(o, graphs, us, [np.zeros((3, 3))] * len(graphs), batch_size=n)
    c = fd_hvp_strain(o, graphs, [np.zeros_like(u) for u in us], list(d["W"]), batch_size=n)
    return [{"h": ax, "u0_x": ax, "u0_s": as_, "0w_x": cx, "0w_s": cs, "uw_x": ax + cx, "uw_s": as_ + cs} for (ax, as_), (cx, cs) in zip(a, c)]


def _references() -> dict:
    import torch

    import second_order_fixtures as sf
    from hessian_ref import fd_hvp

    conv = vf.converter()
    groups = vf.structure_groups()
    graphs = {name: [conv(s) for s in structs] for name, structs in groups.items()}
    ref = {"graphs": graphs}
    kw = dict(return_site_energies=True)
    for wname in vf.WEIGHTS:
        w = dict(np.load(os.path.join(GOLDEN, f"weights_{wname}.npz")))
        o64, o32 = _oracle(w, torch.float64), _oracle(w, torch.float32)
        r = ref[wname] = {"pred": {}, "grad1": {}, "grad2": {}, "prod": {}}
        for name in vf.PREDICT_GROUPS:                   # the oracle's batch is the engine's batch
            gs = graphs[name]
            r["pred"][name] = (o64.predict_graph(gs, "efsm", batch_size=len(gs), **kw), o32.predict_graph(gs, "efsm", batch_size=len(gs), **kw))
        for name in vf.GRAD_GROUPS:
            cot = vf.cotangents(name, vf.sizes_of(groups[name]))
            r["grad1"][name] = _grad_pair(w, graphs[name], cot, ("e", "m"), "em")
            r["grad2"][name] = _grad_pair(w, graphs[name], cot, ("e", "m", "f", "s"), "efsm")
        for name in vf.PRODUCT_GROUPS:
            sizes = vf.sizes_of(groups[name])
            off = np.concatenate([[0], np.cumsum(sizes)])
            r["prod"][name] = _strain_refs(o64, graphs[name], vf.directions(name, sizes), off)
        sizes = vf.sizes_of(groups["low"])
        off = np.concatenate([[0], np.cumsum(sizes)])
        d = vf.directions("low", sizes)
        mv = sf.moved(graphs["low"], MOVE_KEY)
        r["low_geo"] = fd_hvp(o64, mv, [d["u"][off[i]:off[i + 1]] for i in range(len(mv))], batch_size=2 * len(mv))
    return ref


def _long_references() -> dict:
    """The long batch: the loss is additive over structures and every structure has angles (the same shift in every chunk), so the
    gradient is the sum of the per-chunk oracle gradients, accumulated in float64 (also for the float32 oracle)."""
    conv = vf.converter()
    graphs = [conv(s) for s in vf.long_structures()]
    sizes = [len(g.atomic_number) for g in graphs]
    off = np.concatenate([[0], np.cumsum(sizes)])
    cot = vf.cotangents("long", sizes)
    ref = {}
    for wname in vf.WEIGHTS:
        w = dict(np.load(os.path.join(GOLDEN, f"weights_{wname}.npz")))
        ref[wname] = {}
        for kind, keys, task in (("grad1", ("e", "m"), "em"), ("grad2", ("e", "m", "f", "s"), "efsm")):
            total = [None, None]
            for lo in range(0, len(graphs), LONG_CHUNK):
                hi = min(len(graphs), lo + LONG_CHUNK)
                pair = _grad_pair(w, graphs[lo:hi], _split_cot(cot, off, lo, hi), keys, task)
                for j, g in enumerate(pair):
                    total[j] = {k: np.asarray(v, np.float64) + (total[j][k] if total[j] else 0.0) for k, v in g.items()}
            ref[wname][kind] = tuple(total)
    return ref


class _Refs:
    """References computed once per session, on a thread that starts with the first child of the module."""

    def __init__(self, fn):
        self.fn, self.thread, self.value, self.error = fn, None, None, None

    def start(self):
        if self.thread is None:
            self.thread = threading.Thread(target=self._run, daemon=True)
            self.thread.start()

    def _run(self):
        import torch

        try:
            torch.set_num_threads(max(1, min(8, (os.cpu_count() or 2) // 2)))       # (two such threads run side by side)
            self.value = self.fn()
        except BaseException as e:  # noqa: BLE001
            self.error = e

    def get(self) -> dict:
        self.start()
        self.thread.join()
        if self.error is not None:
            raise self.error
        return self.value


_REFS, _LONG_REFS = _Refs(_references), _Refs(_long_references)


# ---- checks ----------------------------------------------------------------------------------------------------------------------

def _fields(r) -> dict:
    return dict(zip(ROUTE_FIELDS, (int(x) for x in r)))


def _expected_route(cfg: str, name: str, origin: str, r, blk_on: bool) -> list:
    """What the route record of a batch must show under configuration ``cfg`` (after tests/test_gpu_second_order_paths.py)."""
    f = _fields(r)
    msgs = []
    n, ed, a, eb = f["N"], f["Ed"], f["A"], f["Eb"]
    tiny = cfg not in ("no_fuse", "no_fuse_addr64") and n <= 32768 and ed <= 1 << 18 and a <= 1 << 19
    want = {"tiny": tiny, "chained": tiny and cfg != "no_chain" and ed > 0 and a > 0 and eb > 0, "zsave": 0,
            "wide": cfg == "wide", "a32": cfg != "no_fuse_addr64"}
    tiles = max(f["blk_tiles"], 0)
    if a == 0:
        want.update(win_built=0, team=0)
    elif cfg == "team":
        want.update(win_built=0, team=1)
    elif cfg.startswith("per_atom"):
        want.update(win_built=1, team=0)
    elif cfg == "row_order" or tiles > 0:        # (blocked tiles: prepare_windows clears both)
        want.update(win_built=0, team=0)
    if cfg not in DEFAULT_LIKE and tiles:
        msgs.append(f"{tiles} blocked tiles with the blocked tiles off")
    if cfg in DEFAULT_LIKE and blk_on and (tiles > 0) != (a > 0 and not (origin == "device" and name in vf.NONCANONICAL)):
        msgs.append(f"{tiles} blocked tiles")
    if a > 0:
        flag = _expected_flag(cfg if cfg in ANGLE_CONFIGS else "default", name, origin, blk_on)
        if flag is not None and f["win_flag"] != flag:
            msgs.append(f"win_flag {f['win_flag']}, expected {flag}")
    for k, v in want.items():
        if f[k] != int(v):
            msgs.append(f"route {k} = {f[k]}, expected {int(v)}")
    return msgs


def _route_str(r, origin) -> str:
    f = _fields(r)
    seq = "chained" if f["chained"] else "fused" if f["tiny"] else "large"
    if f["A"] == 0:
        ang = "no angles"
    elif f["blk_tiles"] > 0 and origin == "device":
        ang = "blk(builder)"
    elif f["blk_tiles"] > 0:
        ang = "blk" if f["win_flag"] == 1 else "blk->row"
    elif f["team"]:
        ang = "team" if f["win_flag"] == 1 else "team->row"
    elif f["win_built"]:
        ang = "per-atom" if f["win_flag"] == 1 else "per-atom->row"
    else:
        ang = "row"
    return f"{seq}/{ang}" + ("" if f["a32"] else "/addr64") + ("/wide" if f["wide"] else "")


def _check_grads(msgs, label, got, want, want32, rel_tol, no_angles):
    assert len(want) == 141 and set(want) <= set(got)
    for k, r in want.items():
        g = np.asarray(got[k])
        if k.startswith(DEAD) or (no_angles and k in vf.BOND_BIASES):
            if np.any(g):
                msgs.append(f"{label} {k}: not exactly zero")
            continue
        scale, err = float(np.abs(r).max()), float(np.abs(g - r).max())
        ref_err = float(np.abs(np.asarray(want32[k], np.float64) - r).max())
        # (floor: 3x the fp32 oracle's own error, as in tests/test_gpu_angle_paths.py)
        if not np.isfinite(g).all() or not err <= max(rel_tol * scale, 3 * ref_err):
            msgs.append(f"{label} {k}: {err:.3e} / {scale:.3e} (fp32 oracle {ref_err:.3e})")


def _print_table(rows):
    print("\ngroup      origin  configuration    route                         F: engine / fp32 oracle    S: engine / fp32 oracle")
    for name, origin, cfg, route, ef, of, es, os_ in rows:
        print(f"{name:<10} {origin:<7} {cfg:<16} {route:<29} {ef:.2e} / {of:.2e}        {es:.2e} / {os_:.2e}")


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_v020_route_against_the_float64_oracle(cfg):
    """One configuration x both 0.2.0 weight sets x device-built and uploaded batches: E / F / S / M and site energies of every group
    within max(TOL x scale, 20 x the fp32 oracle's own error) of OracleCHGNet(float64) called with the engine's batch; the route each
    batch took; the device builder's index arrays at the non-canonical groups; all 141 gradient tensors, first order (after an
    energy-only forward: atomconv_q_table) and with force / stress terms, within max(3e-4 / 3.2e-4 x scale, 3 x fp32 oracle error),
    the BondConv bias gradients exactly zero without angles; H u and the strain products against central differences of the float64
    oracle, also after a captured-graph replay and after update_geometry."""
    from chgnet_amd.pack import pack_batch
    from test_gpu_parity import INT_ARRAYS, TOL
    from test_gpu_train import REL_TOL_B

    blk_on = os.environ.get("CHGNET_BLK_MAX_ANGLES") is None
    _REFS.start()
    _LONG_REFS.start()
    got = _run_child(cfg)
    ref = _REFS.get()
    graphs = ref["graphs"]
    msgs, rows = [], {}

    def check_route(case, name, origin, r):
        for m in _expected_route(cfg, name, origin, r, blk_on):
            msgs.append(f"{case}: {m}")
        return _route_str(r, origin)

    for wname in vf.WEIGHTS:
        R = ref[wname]
        for name in vf.PREDICT_GROUPS:
            gs = graphs[name]
            off = np.concatenate([[0], np.cumsum([len(g.atomic_number) for g in gs])])
            o64, o32 = R["pred"][name]
            for origin in ORIGINS:
                tag = f"{wname}/{name}/{origin}"
                rs = check_route(tag, name, origin, got[tag + "/route"])
                row = rows.setdefault((name, origin), [rs, 0.0, 0.0, 0.0, 0.0])
                for i, (r64, r32) in enumerate(zip(o64, o32)):
                    sl = slice(off[i], off[i + 1])
                    for key in OUT_KEYS:
                        v = got[f"{tag}/{key}"]
                        g = v[i] if key in ("e", "s") else v[sl]
                        r = np.asarray(r64[key], np.float64)
                        ref_err = float(np.abs(np.asarray(r32[key], np.float64) - r).max())
                        err = float(np.abs(g - r).max())
                        scale = max(1.0, float(np.abs(r).max()))
                        if key in ("f", "s"):
                            j = 1 if key == "f" else 3
                            row[j], row[j + 1] = max(row[j], err), max(row[j + 1], ref_err)
                        if not np.isfinite(g).all() or not err < max(TOL[key] * scale, 20 * ref_err):
                            msgs.append(f"{tag}[{i}] {key}: {err:.3e} vs fp32 oracle {ref_err:.3e} (scale {scale:.3g})")
        for kind, tol in (("grad1", REL_TOL_B), ("grad2", GRAD_TOL_2)):
            for name in vf.GRAD_GROUPS:
                want, want32 = R[kind][name]
                for origin in ORIGINS:
                    tag = f"{kind}/{wname}/{name}/{origin}"
                    check_route(tag, name, origin, got[tag + "/route"])
                    sub = {k[len(tag) + 1:]: v for k, v in got.items() if k.startswith(tag + "/")}
                    _check_grads(msgs, tag, sub, want, want32, tol, name.startswith("noangle"))
        for name in vf.PRODUCT_GROUPS:
            off = np.concatenate([[0], np.cumsum([len(g.atomic_number) for g in graphs[name]])])
            for origin in ORIGINS:
                tag = f"prod/{wname}/{name}/{origin}"
                check_route(tag, name, origin, got[tag + "/route"])
                for i, r in enumerate(R["prod"][name]):
                    for p in PRODUCTS:
                        v = got[f"{tag}/{p}"]
                        g = v[i] if p.endswith("_s") else v[off[i]:off[i + 1]]
                        err = _rel(g, r[p], _block_scale(r, p))
                        if not err <= REL_TOL:
                            msgs.append(f"{tag}[{i}] {p}: {err:.3e} of scale (bar {REL_TOL:g})")
        # ``low`` (upload): three predictions (eager, capture, replay), update_geometry, a fresh batch at the moved positions
        tag = f"prod/{wname}/low/upload"
        off = np.concatenate([[0], np.cumsum([len(g.atomic_number) for g in graphs["low"]])])
        check_route(tag + "/replay", "low", "upload", got[tag + "/replay_route"])
        check_route(tag + "/geometry", "low", "upload", got[tag + "/geo_route"])
        for i, r in enumerate(R["low_geo"]):
            sl = slice(off[i], off[i + 1])
            for what, err, bar in (("3 predictions vs 1", _rel(got[tag + "/replay_h"][sl], got[tag + "/h"][sl]), REPLAY_TOL),
                                   ("update_geometry vs a fresh batch", _rel(got[tag + "/geo_h"][sl], got[tag + "/fresh_h"][sl]), CROSS_TOL),
                                   ("update_geometry vs oracle", _rel(got[tag + "/geo_h"][sl], r), REL_TOL)):
                if not err <= bar:
                    msgs.append(f"{tag}[{i}] {what}: {err:.3e} of scale (bar {bar:g})")
    for name in vf.INDEX_GROUPS:          # the device builder's index arrays == the host converter's at 5 / 3
        want = pack_batch(graphs[name])
        if not np.array_equal(got[f"idx/{name}/counts"], [want.n_directed, want.n_angles, want.n_bnodes]):
            msgs.append(f"idx/{name}: counts {got[f'idx/{name}/counts']}")
            continue
        for arr in INT_ARRAYS:
            if not np.array_equal(got[f"idx/{name}/{arr}"], want.arrays[arr]):
                msgs.append(f"idx/{name}/{arr} differs from the host converter's")
    _print_table([(name, origin, cfg, *row) for (name, origin), row in rows.items()])
    per_group = {name: sum(f"/{name}/" in m or f"/{name}[" in m or f"/{name}:" in m for m in msgs) for name in vf.PREDICT_GROUPS}
    assert not msgs, f"{len(msgs)} failures (per group: {per_group}):\n" + "\n".join(msgs[:100])


@pytest.fixture(scope="module")
def long_runs():
    return {}


@pytest.mark.parametrize("cfg", list(LONG_CONFIGS))
def test_v020_long_batch_training_reductions_against_the_summed_float64_oracle(cfg, long_runs):
    """The shortest batch of 40-atom cells with more than 65,536 directed edges and angles (an angle count that is no multiple of 32):
    k_xty3 / k_xty at their size, k_colsum_nonnode and colsum looping over their capped grids, with bias gradients.  First-order and
    full gradients against the float64 oracle's per-chunk gradients summed in float64, at the bars of the route matrix; the second
    child (CHGNET_XTY3=0) also against the first, at 2e-5 of the blob's largest entry."""
    from chgnet_amd.pack import pack_weights, unpack_weight_grads
    from test_gpu_train import REL_TOL_B

    blk_on = os.environ.get("CHGNET_BLK_MAX_ANGLES") is None
    _LONG_REFS.start()
    got = long_runs[cfg] = _run_child(cfg)
    ref = _LONG_REFS.get()
    msgs = []
    for wname in vf.WEIGHTS:
        pw = pack_weights(dict(np.load(os.path.join(GOLDEN, f"weights_{wname}.npz"))), V020_ARGS)
        r = got[f"{wname}/long/route"]
        for m in _expected_route(cfg, "long", "upload", r, blk_on):
            msgs.append(f"{wname}/long: {m}")
        print(f"{cfg} {wname}: route {_route_str(r, 'upload')}, N = {int(r[9])}, Ed = {int(r[10])}, A = {int(r[11])}")
        for kind, tol in (("grad1", REL_TOL_B), ("grad2", GRAD_TOL_2)):
            want, want32 = ref[wname][kind]
            _check_grads(msgs, f"{kind}/{wname}/long", unpack_weight_grads(got[f"{wname}/long/{kind}"], pw), want, want32, tol, False)
            if cfg != "long" and "long" in long_runs:
                a, b = got[f"{wname}/long/{kind}"].astype(np.float64), long_runs["long"][f"{wname}/long/{kind}"].astype(np.float64)
                scale, err = float(np.abs(a).max()), float(np.abs(a - b).max())
                print(f"{kind} {wname}: k_xty3 vs k_xty {err / scale:.3e} of the largest entry (bar {XTY_TOL:g})")
                if not (scale > 0 and np.isfinite(b).all() and err <= XTY_TOL * scale):
                    msgs.append(f"{kind}/{wname}/long: k_xty3 vs k_xty {err / scale:.3e}")
    if cfg != "long":
        assert "long" in long_runs, "the default child of the long batch did not run"
    assert not msgs, f"{len(msgs)} failures:\n" + "\n".join(msgs[:100])
