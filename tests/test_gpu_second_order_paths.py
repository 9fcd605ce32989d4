"""Second-order results (chg_hessian_vector, chg_hessian_vector_strain, the second-order sweep of chg_backward) against the float64
oracle on every route a prediction can take.  The second-order sweep does not rebuild the first-order adjoints: it reads the GP_l /
GR_l / GS_l tables of every layer, Gwag, Gwbgc and the Q tables the force sweep of the last chg_predict left in the batch -- written
by whichever kernels that prediction ran: the launch sequence of MD-size batches (fused, chained row GEMMs) or of large ones, the
angle adjoints over blocked tiles, TEAM, per-atom windows or row order, and with or without the z rows kept by the forward angle
kernels (zsave).  Also after a captured-graph replay and after chg_batch_update_geometry.

Configurations as in tests/test_gpu_angle_paths.py (one child process each, one after another, the first failure stops the rest),
plus CHGNET_TINY_FUSE=0, CHGNET_TINY_CHAIN=0 and CHGNET_ZSAVE=0 (the headline batch only).  The children run the engine only; the
parent computes the float64 references (central differences on the fixed graph, tests/hessian_ref.py, tests/elastic_ref.py; the
oracle's parameter gradients) while they run, and compares.  Each run asserts the route it was meant to take (chg_debug_fetch_i32
"route", "blk_tiles", "win_flag") and that it stayed off the wide-range sweeps."""

from __future__ import annotations

import os
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

import second_order_fixtures as sf
from conftest import GOLDEN, REPO
from test_gpu_angle_paths import CONFIGS as ANGLE_CONFIGS
from test_gpu_angle_paths import GRAD_GROUPS, KNOBS, NONCANONICAL, WEIGHTS, _cotangents

pytestmark = pytest.mark.gpu

REL_TOL = 3e-4          # H u, hx, hs vs the oracle (tests/test_gpu_hessian.py, tests/test_gpu_elastic.py)
CROSS_TOL = 1e-5        # a configuration vs the default on the same batch, and a fresh batch vs update_geometry (batch vs single)
REPLAY_TOL = 1e-6       # three predictions (eager, capture, replay) vs one, then the same product
CONFIGS = {**ANGLE_CONFIGS, "no_fuse": {"CHGNET_TINY_FUSE": "0"}, "no_chain": {"CHGNET_TINY_CHAIN": "0"}, "no_zsave": {"CHGNET_ZSAVE": "0"}}
DEFAULT_LIKE = ("default", "no_fuse", "no_chain", "no_zsave")           # the angle knobs at their defaults
GRAD_CONFIGS = ("default", "team", "per_atom", "per_atom_rowfwd", "no_fuse")
HEAD_ONLY = ("no_zsave",)
ROUTE_FIELDS = ("tiny", "chained", "zsave", "win_built", "team", "blk_tiles", "win_flag", "wide", "N", "Ed", "A", "Eb")
PRODUCTS = ("h", "uw_x", "uw_s", "0w_x", "0w_s", "u0_x", "u0_s")


# ---- child: the engine only ------------------------------------------------------------------------------------------------------

def _route(eng, b) -> np.ndarray:
    def fetch(name, n):
        try:
            return eng.debug_fetch_i32(b, name, n)
        except RuntimeError:          # no such buffer in this batch (no blocked tiles): -1
            return np.full(n, -1, np.int32)

    pb = b.packed
    return np.array([*eng.debug_fetch_i32(b, "route", 5), fetch("blk_tiles", 1)[0], fetch("win_flag", 4)[0],
                     eng.debug_fetch_i32(b, "wide_range", 1)[0], pb.n_atoms, pb.n_directed, pb.n_angles, pb.n_bnodes], np.int64)


def _products(eng, b, d, out, tag):
    """E + F, then H u and the strain products along (u, W), (0, W), (u, 0)."""
    eng.predict(b, "ef")
    out[tag + "/route"] = _route(eng, b)
    out[tag + "/off"] = np.asarray(b.packed.atom_off, np.int64)
    out[tag + "/h"] = eng.hessian_vector(b, d["u"])
    zu, zw = np.zeros_like(d["u"]), np.zeros_like(d["W"])
    for kind, (u, w) in (("uw", (d["u"], d["W"])), ("0w", (zu, d["W"])), ("u0", (d["u"], zw))):
        out[f"{tag}/{kind}_x"], out[f"{tag}/{kind}_s"] = eng.hessian_vector_strain(b, u, w)


def _replay_and_geometry(eng, b, graphs, d, key, out, tag):
    """(after _products on ``b``) three predictions -- eager, captured, replayed -- then H u; chg_batch_update_geometry to moved
    positions, a prediction (a replay of the captured sweep), H u; and H u of a fresh batch at the moved positions."""
    from chgnet_amd.pack import pack_batch

    for _ in range(3):
        eng.predict(b, "ef")
    out[tag + "/replay_route"] = _route(eng, b)
    out[tag + "/replay_h"] = eng.hessian_vector(b, d["u"])
    mv = sf.moved(graphs, key)
    b.update_geometry(frac=np.concatenate([g.atom_frac_coord for g in mv]))
    eng.predict(b, "ef")
    out[tag + "/geo_route"] = _route(eng, b)
    out[tag + "/geo_h"] = eng.hessian_vector(b, d["u"])
    fresh = eng.upload(pack_batch(mv))
    try:
        eng.predict(fresh, "ef")
        out[tag + "/fresh_h"] = eng.hessian_vector(fresh, d["u"])
    finally:
        fresh.free()


def _recording(eng, routes):
    """Wrap the engine's product calls so that the model API's own batches report their route."""
    hv, hvs = eng.hessian_vector, eng.hessian_vector_strain

    def hessian_vector(b, u):
        routes.append(_route(eng, b))
        return hv(b, u)

    def hessian_vector_strain(b, u, w):
        routes.append(_route(eng, b))
        return hvs(b, u, w)

    eng.hessian_vector, eng.hessian_vector_strain = hessian_vector, hessian_vector_strain
    return lambda: (setattr(eng, "hessian_vector", hv), setattr(eng, "hessian_vector_strain", hvs))


def child(out_path: str, cot_path: str, cfg: str) -> None:
    import angle_fixtures as af
    from chgnet_amd.engine import Engine
    from chgnet_amd.model import CHGNet
    from chgnet_amd.pack import pack_weights

    conv = af.converter()
    groups = af.structure_groups()
    malformed = af.malformed_graphs()
    head = [conv(s) for s in sf.headline_structures()]
    head_sizes = [len(g.atomic_number) for g in head]
    hd = sf.directions("head", head_sizes)
    cots = dict(np.load(cot_path))
    out = {}
    for wname in WEIGHTS:
        W = dict(np.load(os.path.join(GOLDEN, f"weights_{wname}.npz")))
        eng = Engine(pack_weights(W), 0)
        model = CHGNet(state_dict=W)
        model._engine = eng
        if cfg not in HEAD_ONLY:
            for name in sf.GROUPS:
                gs = [conv(s) for s in groups[name]]
                d = sf.directions(name, [len(g.atomic_number) for g in gs])
                for origin in ("device", "upload"):
                    b = eng.build_batch(groups[name], af.R_ATOM, af.R_BOND) if origin == "device" else eng.upload(gs)
                    try:
                        _products(eng, b, d, out, f"{wname}/{name}/{origin}")
                        if name == "md" and origin == "upload":       # the fused launch sequence
                            _replay_and_geometry(eng, b, gs, d, name, out, f"{wname}/{name}/{origin}")
                    finally:
                        b.free()
            for kind, gs in malformed.items():
                d = sf.directions("malformed_" + kind, [len(g.atomic_number) for g in gs])
                b = eng.upload(gs)
                try:
                    _products(eng, b, d, out, f"{wname}/malformed_{kind}/upload")
                finally:
                    b.free()
            # the model API at its default batching: 64 replicas of the 256-atom cell per batch; the 6 Voigt strains in one
            routes = []
            restore = _recording(eng, routes)
            try:
                md = conv(sf.md_cell())
                out[f"{wname}/api_hess/cols"] = model.predict_hessian(md, symmetrize=False)[:, list(sf.HESS_COLS)]
                out[f"{wname}/api_hess/route"] = np.stack(routes)
                routes.clear()
                el = model.predict_elastic_tensor(md, relaxed_ion=False)
                out[f"{wname}/api_elastic/internal_strain"] = el["internal_strain"]
                out[f"{wname}/api_elastic/clamped_ion"] = el["clamped_ion"]
                out[f"{wname}/api_elastic/route"] = np.stack(routes)
                routes.clear()
            finally:
                restore()
            if cfg in GRAD_CONFIGS:        # fine-tuning: chg_backward's second-order sweep
                for name in GRAD_GROUPS:
                    c = [cots[name + "/" + k] for k in ("e", "m", "f", "s")]
                    for origin in ("device", "upload"):
                        if origin == "device":
                            b = eng.build_batch(groups[name], af.R_ATOM, af.R_BOND)
                            model.forward(b.packed, task="efsm", device_batch=b)
                        else:
                            model.forward([conv(s) for s in groups[name]], task="efsm")
                        out[f"grad/{wname}/{name}/{origin}/route"] = _route(eng, model._fwd_batch)
                        for k, v in model.backward(*c).items():
                            out[f"grad/{wname}/{name}/{origin}/{k}"] = v
                        model.release_forward_state()
        # the headline-shaped batch: H u, the strain products, the identities, replay and geometry update
        tag = f"{wname}/head/engine"
        b = eng.upload(head)
        try:
            _products(eng, b, hd, out, tag)
            out[tag + "/trans_h"] = eng.hessian_vector(b, hd["t"])
            out[tag + "/v_h"] = eng.hessian_vector(b, hd["v"])
            out[tag + "/rot_x"], out[tag + "/rot_s"] = eng.hessian_vector_strain(b, np.zeros_like(hd["u"]), hd["R"])
            _replay_and_geometry(eng, b, head, hd, "head", out, tag)
        finally:
            b.free()
        routes = []
        restore = _recording(eng, routes)
        try:
            hsz = np.cumsum([0] + head_sizes)
            us = [hd["u"][hsz[i]:hsz[i + 1]] for i in range(len(head))]
            out[f"{wname}/head/api/h"] = np.concatenate(model.hessian_vector_product(head, us))
            res = model.hessian_vector_product_with_strain(head, us, list(hd["W"]))
            out[f"{wname}/head/api/uw_x"] = np.concatenate([r[0] for r in res])
            out[f"{wname}/head/api/uw_s"] = np.stack([r[1] for r in res])
            out[f"{wname}/head/api/route"] = np.stack(routes)
        finally:
            restore()
        hc = sf.head_cotangents(head_sizes)
        model.forward(head, task="efsm")
        out[f"grad/{wname}/head/route"] = _route(eng, model._fwd_batch)
        for k, v in model.backward(hc["e"], hc["m"], hc["f"], hc["s"]).items():
            out[f"grad/{wname}/head/{k}"] = v
        model.release_forward_state()
        model._engine = None
        eng.close()
    np.savez(out_path, **out)


_CHILD = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']; import test_gpu_second_order_paths as t; t.child(*sys.argv[2:])"


def _run_configs(tmp: str, cot_path: str, res: dict, errors: list) -> None:
    """One child per configuration, in order; the first failure (exit status, signal or time-out) ends the chain before the next
    child is started."""
    import time

    for cfg, extra in CONFIGS.items():
        env = dict(os.environ)
        for k in KNOBS:
            if not (cfg in DEFAULT_LIKE and k == "CHGNET_BLK_MAX_ANGLES"):
                env.pop(k, None)
        env.update(extra)
        path = os.path.join(tmp, cfg + ".npz")
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, "-c", _CHILD, REPO, path, cot_path, cfg], env=env, timeout=600, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            errors.append(f"configuration {cfg}: time-out")
            return
        if r.returncode != 0:
            errors.append(f"configuration {cfg}: exit status {r.returncode}\n{r.stderr[-4000:]}")
            return
        res[cfg] = dict(np.load(path))
        print(f"configuration {cfg}: {time.time() - t0:.0f} s", flush=True)


# ---- parent: references and checks ---------------------------------------------------------------------------------------------

def _oracle(w, dtype=None):
    import torch

    from oracle.chgnet_oracle import OracleCHGNet

    return OracleCHGNet(w, dtype=dtype or torch.float64)


def _split(d, i, off):
    return {k: (v[off[i]:off[i + 1]] if k in ("u", "v", "t") else v[i]) for k, v in d.items()}


def _chunked(fd, o, graphs, *per_graph, atoms=800):
    """``fd(o, graphs, *per_graph)`` over consecutive chunks of at most ``atoms`` atoms (one central difference holds every graph
    twice, in float64, with the double-backward graph: the memory of the host)."""
    out, start = [], 0
    while start < len(graphs):
        stop, n = start, 0
        while stop < len(graphs) and (stop == start or n + len(graphs[stop].atomic_number) <= atoms):
            n += len(graphs[stop].atomic_number)
            stop += 1
        out += fd(o, graphs[start:stop], *(list(x[start:stop]) for x in per_graph))
        start = stop
    return out


def _strain_refs(o, graphs, ds):
    """Per graph: the references of the four products, from the two central differences along (u, 0) and (0, W) (the products are
    linear in (u, W))."""
    from elastic_ref import fd_hvp_strain

    zero = [np.zeros((3, 3))] * len(graphs)
    a = _chunked(fd_hvp_strain, o, graphs, [d["u"] for d in ds], zero)
    c = _chunked(fd_hvp_strain, o, graphs, [np.zeros_like(d["u"]) for d in ds], [d["W"] for d in ds])
    return [{"h": ax, "u0_x": ax, "u0_s": as_, "0w_x": cx, "0w_s": cs, "uw_x": ax + cx, "uw_s": as_ + cs}
            for (ax, as_), (cx, cs) in zip(a, c)]


def _references(wname, cots):
    """Everything the children's results are compared with, for one weight set."""
    import torch

    import angle_fixtures as af
    from elastic_ref import fd_hvp_strain, voigt_strains
    from hessian_ref import fd_hvp

    W = dict(np.load(os.path.join(GOLDEN, f"weights_{wname}.npz")))
    o = _oracle(W)
    conv = af.converter()
    groups = af.structure_groups()
    ref = {}
    sets = {name: [conv(s) for s in groups[name]] for name in sf.GROUPS}
    sets.update({"malformed_" + k: v for k, v in af.malformed_graphs().items()})
    for name, gs in sets.items():
        sizes = [len(g.atomic_number) for g in gs]
        off = np.concatenate([[0], np.cumsum(sizes)])
        d = sf.directions(name, sizes)
        ref[name] = _strain_refs(o, gs, [_split(d, i, off) for i in range(len(gs))])
    md_mv = sf.moved(sets["md"], "md")
    d = sf.directions("md", [len(g.atomic_number) for g in sets["md"]])
    off = np.concatenate([[0], np.cumsum([len(g.atomic_number) for g in sets["md"]])])
    ref["md/geo"] = _chunked(fd_hvp, o, md_mv, [d["u"][off[i]:off[i + 1]] for i in range(len(md_mv))])
    # the model API on the 256-atom cell
    md = conv(sf.md_cell())
    n = len(md.atomic_number)
    eye = np.eye(3 * n).reshape(3 * n, n, 3)
    ref["api_hess"] = np.stack([c.reshape(-1) for c in _chunked(fd_hvp, o, [md] * len(sf.HESS_COLS), [eye[c] for c in sf.HESS_COLS])], axis=1)
    wv = voigt_strains()
    cols = _chunked(fd_hvp_strain, o, [md] * 6, [np.zeros((n, 3))] * 6, list(wv))
    vol = abs(float(np.linalg.det(np.asarray(md.lattice, np.float64).reshape(3, 3))))
    c = np.einsum("iab,jab->ij", wv, np.stack([cs for _, cs in cols])) * (160.21766208 / vol)
    ref["api_elastic"] = {"internal_strain": np.stack([cx.reshape(-1) for cx, _ in cols], axis=1), "clamped_ion": 0.5 * (c + c.T)}
    # the headline batch: the sampled structures, at the original and the moved positions
    head = [conv(s) for s in sf.headline_structures()]
    sizes = [len(g.atomic_number) for g in head]
    off = np.concatenate([[0], np.cumsum(sizes)])
    hd = sf.directions("head", sizes)
    sample = [head[i] for i in sf.HEAD_SAMPLE]
    ref["head"] = _strain_refs(o, sample, [_split(hd, i, off) for i in sf.HEAD_SAMPLE])
    mv = sf.moved(head, "head")
    ref["head/geo"] = _chunked(fd_hvp, o, [mv[i] for i in sf.HEAD_SAMPLE], [hd["u"][off[i]:off[i + 1]] for i in sf.HEAD_SAMPLE])
    # fine-tuning gradients: the angle-path groups, and the four headline structures with nonzero cotangents
    grads = {}
    hc = sf.head_cotangents(sizes)
    jobs = {name: (sets[name], {k: cots[f"{name}/{k}"] for k in ("e", "m", "f", "s")}) for name in GRAD_GROUPS}
    jobs["head"] = ([head[i] for i in sf.GRAD_SAMPLE],
                    {"e": hc["e"][list(sf.GRAD_SAMPLE)], "s": hc["s"][list(sf.GRAD_SAMPLE)],
                     "m": np.concatenate([hc["m"][off[i]:off[i + 1]] for i in sf.GRAD_SAMPLE]),
                     "f": np.concatenate([hc["f"][off[i]:off[i + 1]] for i in sf.GRAD_SAMPLE])})
    for name, (gs, cot) in jobs.items():
        pair = []
        for dt in (torch.float64, torch.float32):
            t = {k: torch.tensor(np.asarray(v), dtype=dt) for k, v in cot.items()}
            pair.append(_oracle(W, dt).parameter_gradients(
                gs, lambda r: (r["e"] * t["e"]).sum() + (r["m"] * t["m"]).sum() + (r["f"] * t["f"]).sum() + (r["s"] * t["s"]).sum(),
                task="efsm"))
        grads[name] = pair
    ref["grad"] = grads
    return ref


def _rel(got, ref, floor=0.0) -> float:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    scale = max(float(np.abs(ref).max()) if ref.size else 0.0, floor)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


def _block_scale(r, p) -> float:
    """Scale of product ``p`` of one structure: the largest reference entry of its block (hx or hs) over the structure's products
    -- hx along (0, W) and hs along (u, 0) vanish on a perfect lattice (no internal strain), where their own maximum is noise."""
    keys = [k for k in PRODUCTS if k.endswith("_s") == p.endswith("_s")]
    return max(float(np.abs(r[k]).max()) for k in keys)


def _expected_route(cfg, name, origin, r, blk_on) -> list[str]:
    """What the route record ``r`` of a batch must show under configuration ``cfg``; the messages of the mismatches."""
    from test_gpu_angle_paths import _expected_flag

    f = dict(zip(ROUTE_FIELDS, (int(x) for x in r)))
    msgs = []
    n, ed, a, eb = f["N"], f["Ed"], f["A"], f["Eb"]
    tiny = cfg != "no_fuse" and n <= 32768 and ed <= 1 << 18 and a <= 1 << 19
    want = {"tiny": tiny, "chained": tiny and cfg != "no_chain" and ed > 0 and a > 0 and eb > 0, "wide": 0}
    tiles = max(f["blk_tiles"], 0)
    big = n + 1 > 8192
    if big:                                    # past the blocked tiles and TEAM: the per-atom windows in every configuration
        want.update(win_built=1, team=0)
    elif cfg == "team":
        want.update(win_built=0, team=int(a > 0))
    elif cfg.startswith("per_atom"):
        want.update(win_built=int(a > 0), team=0)
    elif cfg == "row_order":
        want.update(win_built=0, team=0)
    elif tiles > 0:                            # blocked tiles: prepare_windows clears both
        want.update(win_built=0, team=0)
    if cfg not in DEFAULT_LIKE and tiles:
        msgs.append(f"{tiles} blocked tiles with the blocked tiles off")
    if cfg in DEFAULT_LIKE and blk_on and not big and not name.startswith(("head", "api")):
        if (tiles > 0) != (not (origin == "device" and name in NONCANONICAL)):
            msgs.append(f"{tiles} blocked tiles")
    if not name.startswith(("head", "api")):
        flag = _expected_flag(cfg if cfg in ANGLE_CONFIGS else "default", name, origin, blk_on)
        if flag is not None and f["win_flag"] != flag:
            msgs.append(f"win_flag {f['win_flag']}, expected {flag}")
    if big and f["win_flag"] != 1:
        msgs.append(f"win_flag {f['win_flag']}: the per-atom index of a canonical graph was refused")
    want["zsave"] = int(cfg != "no_zsave" and a > 1 << 19 and (f["win_built"] or f["team"]))
    for k, v in want.items():
        if f[k] != int(v):
            msgs.append(f"route {k} = {f[k]}, expected {int(v)}")
    return msgs


def _route_str(r, origin="upload") -> str:
    f = dict(zip(ROUTE_FIELDS, (int(x) for x in r)))
    seq = "chained" if f["chained"] else "fused" if f["tiny"] else "large"
    if f["blk_tiles"] > 0 and origin == "device":
        ang = "blk(builder)"                   # the graph builder's index: no flag
    elif f["blk_tiles"] > 0:
        ang = "blk" if f["win_flag"] == 1 else "blk->row"
    elif f["team"]:
        ang = "team" if f["win_flag"] == 1 else "team->row"
    elif f["win_built"]:
        ang = "per-atom" if f["win_flag"] == 1 else "per-atom->row"
    else:
        ang = "row"
    return f"{seq}/{ang}" + ("/zsave" if f["zsave"] else "")


def test_second_order_results_on_every_route_against_the_float64_oracle():
    """Eight configurations x both weight sets: H u and the strain products (u, W), (0, W), (u, 0) of the angle-path fixture groups
    (device-built and uploaded) and the four malformed uploaded angle sets; the headline-shaped batch (40,960 atoms, > 2^19 angles:
    large launch sequence, per-atom windows with the index from k_win_*, zsave) through the engine and through the model API at its
    default chunking, with the translation / symmetry / rotation identities on every structure; predict_hessian and
    predict_elastic_tensor at their default batching; CHGNet.backward's second-order sweep; three predictions (eager, capture,
    replay) and chg_batch_update_geometry before a product."""
    import torch

    from test_gpu_train import REL_TOL_B

    import angle_fixtures as af

    blk_on = os.environ.get("CHGNET_BLK_MAX_ANGLES") is None
    cots = _cotangents(af.structure_groups())
    res, errors = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        cot_path = os.path.join(tmp, "cot.npz")
        np.savez(cot_path, **cots)
        runner = threading.Thread(target=_run_configs, args=(tmp, cot_path, res, errors))
        runner.start()
        try:
            torch.set_num_threads(max(1, min(12, (os.cpu_count() or 2) - 2)))
            refs = {wname: _references(wname, cots) for wname in WEIGHTS}
        finally:
            runner.join()
    assert not errors, errors[0]

    msgs, table, worst = [], {}, {}

    def note(cfg, case, route, err, bar, what):
        key = (cfg, case)
        table.setdefault(key, set()).add(route)
        worst[key] = max(worst.get(key, 0.0), err)
        if not err <= bar:
            msgs.append(f"{cfg} {case} {what}: {err:.3e} of scale (bar {bar:g})")

    def check_route(cfg, case, name, origin, r):
        for m in _expected_route(cfg, name, origin, r, blk_on):
            msgs.append(f"{cfg} {case}: {m}")
        return _route_str(r, origin)

    for cfg, got in res.items():
        for wname in WEIGHTS:
            ref = refs[wname]
            names = [] if cfg in HEAD_ONLY else list(sf.GROUPS) + ["malformed_" + k for k in af.MALFORMED_KINDS]
            for name in names:
                for origin in (("upload",) if name.startswith("malformed_") else ("device", "upload")):
                    tag = f"{wname}/{name}/{origin}"
                    case = f"{name}/{origin}"
                    rs = check_route(cfg, case, name, origin, got[tag + "/route"])
                    off = got[tag + "/off"]
                    for i, r in enumerate(ref[name]):
                        for p in PRODUCTS:
                            v = got[f"{tag}/{p}"]
                            g = v[i] if p.endswith("_s") else v[off[i]:off[i + 1]]
                            note(cfg, case, rs, _rel(g, r[p], _block_scale(r, p)), REL_TOL, f"[{i}] {p}")
            if cfg not in HEAD_ONLY:
                # replay and geometry update on the md cells (fused launch sequence)
                tag = f"{wname}/md/upload"
                off = got[tag + "/off"]
                rs = check_route(cfg, "md/replay", "md", "upload", got[tag + "/replay_route"])
                check_route(cfg, "md/geometry", "md", "upload", got[tag + "/geo_route"])
                note(cfg, "md/replay", rs, _rel(got[tag + "/replay_h"], got[tag + "/h"]), REPLAY_TOL, "3 predictions vs 1")
                for i, r in enumerate(ref["md/geo"]):
                    sl = slice(off[i], off[i + 1])
                    note(cfg, "md/geometry", rs, _rel(got[tag + "/geo_h"][sl], got[tag + "/fresh_h"][sl]), CROSS_TOL, f"[{i}] vs a fresh batch")
                    note(cfg, "md/geometry", rs, _rel(got[tag + "/geo_h"][sl], r), REL_TOL, f"[{i}] vs oracle")
                # the model API on the 256-atom cell
                rs = " ".join(sorted({check_route(cfg, "api/predict_hessian", "api", "upload", r) for r in got[f"{wname}/api_hess/route"]}))
                if min(int(r[8]) for r in got[f"{wname}/api_hess/route"]) <= 8191:
                    msgs.append(f"{cfg} api/predict_hessian: a batch within the blocked-tile limit")
                for j, c in enumerate(sf.HESS_COLS):
                    note(cfg, "api/predict_hessian", rs, _rel(got[f"{wname}/api_hess/cols"][:, j], ref["api_hess"][:, j]), REL_TOL, f"column {c}")
                rs = " ".join(sorted({check_route(cfg, "api/elastic", "api", "upload", r) for r in got[f"{wname}/api_elastic/route"]}))
                for k in ("internal_strain", "clamped_ion"):
                    note(cfg, "api/elastic", rs, _rel(got[f"{wname}/api_elastic/{k}"], ref["api_elastic"][k]), REL_TOL, k)
            # the headline batch
            tag = f"{wname}/head/engine"
            off = got[tag + "/off"]
            rs = check_route(cfg, "head/engine", "head", "upload", got[tag + "/route"])
            for j, i in enumerate(sf.HEAD_SAMPLE):
                for p in PRODUCTS:
                    v = got[f"{tag}/{p}"]
                    note(cfg, "head/engine", rs, _rel(v[i] if p.endswith("_s") else v[off[i]:off[i + 1]], ref["head"][j][p],
                                                      _block_scale(ref["head"][j], p)), REL_TOL, f"[{i}] {p}")
            rs_api = " ".join(sorted({check_route(cfg, "head/api", "head", "upload", r) for r in got[f"{wname}/head/api/route"]}))
            for j, i in enumerate(sf.HEAD_SAMPLE):
                sl = slice(off[i], off[i + 1])
                note(cfg, "head/api", rs_api, _rel(got[f"{wname}/head/api/h"][sl], ref["head"][j]["h"]), REL_TOL, f"[{i}] h")
                note(cfg, "head/api", rs_api, _rel(got[f"{wname}/head/api/uw_x"][sl], ref["head"][j]["uw_x"]), REL_TOL, f"[{i}] uw_x")
                note(cfg, "head/api", rs_api, _rel(got[f"{wname}/head/api/uw_s"][i], ref["head"][j]["uw_s"]), REL_TOL, f"[{i}] uw_s")
            # identities on every structure, relative to the structure's random-direction product
            h, hv, ht = (got[f"{tag}/{k}"].astype(np.float64) for k in ("h", "v_h", "trans_h"))
            hx0w, hrot = got[f"{tag}/0w_x"].astype(np.float64), got[f"{tag}/rot_x"].astype(np.float64)
            d = sf.directions("head", np.diff(off))
            for i in range(len(off) - 1):
                sl = slice(off[i], off[i + 1])
                scale = float(np.abs(h[sl]).max())
                note(cfg, "head/translation", rs, float(np.abs(ht[sl]).max()) / scale, REL_TOL, f"[{i}] |H t|")
                vhu, uhv = float((d["v"][sl] * h[sl]).sum()), float((d["u"][sl] * hv[sl]).sum())
                den = float(np.linalg.norm(d["v"][sl]) * np.linalg.norm(h[sl]) + np.linalg.norm(d["u"][sl]) * np.linalg.norm(hv[sl]))
                note(cfg, "head/symmetry", rs, abs(vhu - uhv) / den, REL_TOL, f"[{i}] v.Hu - u.Hv")
                note(cfg, "head/rotation", rs, float(np.abs(hrot[sl]).max()) / float(np.abs(hx0w[sl]).max()), REL_TOL, f"[{i}] |hx(0, R)|")
            # replay and geometry update on the headline batch
            rs = check_route(cfg, "head/replay", "head", "upload", got[tag + "/replay_route"])
            check_route(cfg, "head/geometry", "head", "upload", got[tag + "/geo_route"])
            note(cfg, "head/replay", rs, _rel(got[tag + "/replay_h"], got[tag + "/h"]), REPLAY_TOL, "3 predictions vs 1")
            note(cfg, "head/geometry", rs, max(_rel(got[tag + "/geo_h"][off[i]:off[i + 1]], got[tag + "/fresh_h"][off[i]:off[i + 1]])
                                               for i in range(len(off) - 1)), CROSS_TOL, "vs a fresh batch")
            for j, i in enumerate(sf.HEAD_SAMPLE):
                note(cfg, "head/geometry", rs, _rel(got[tag + "/geo_h"][off[i]:off[i + 1]], ref["head/geo"][j]), REL_TOL, f"[{i}] vs oracle")
            # fine-tuning gradients
            gcases = [("head", None)] + ([(n, o) for n in GRAD_GROUPS for o in ("device", "upload")] if cfg in GRAD_CONFIGS else [])
            for name, origin in gcases:
                gtag = f"grad/{wname}/{name}" + (f"/{origin}" if origin else "")
                case = f"grad/{name}" + (f"/{origin}" if origin else "")
                rs = check_route(cfg, case, name, origin or "upload", got[gtag + "/route"])
                want, want32 = ref["grad"][name]
                for k, r in want.items():
                    g = got[f"{gtag}/{k}"]
                    if k.startswith(("angle_layers.2.", "composition_model")):
                        if np.any(g):
                            msgs.append(f"{cfg} {case} {k}: not zero")
                        continue
                    # (floor: 3x the fp32 oracle's own error, as in tests/test_gpu_angle_paths.py: collinear angles of the fcc tie cell)
                    scale = float(np.abs(r).max())
                    bar = max(REL_TOL_B, 3 * float(np.abs(want32[k] - r).max()) / scale)
                    note(cfg, case, rs, _rel(g, r), bar, k)
    # every configuration vs the default on the same batch
    base = res.get("default", {})
    for cfg, got in res.items():
        if cfg == "default":
            continue
        for key, v in got.items():
            leaf = key.rsplit("/", 1)[-1]
            # (H t and hx(0, R) vanish: the identities above bound them against the structure's scale)
            if key not in base or "route" in leaf or leaf in ("off", "trans_h", "rot_x") or key.startswith("grad/"):
                continue
            parts = key.split("/")
            tag = "/".join(parts[:-1])
            off = got.get(tag + "/off", got.get(f"{parts[0]}/head/engine/off") if parts[1] == "head" else None)
            b0 = base[key].astype(np.float64)
            # scale of a product: its block (hx or hs) over the structure's products in the default run (as _block_scale)
            block = [base[f"{tag}/{k}"] for k in PRODUCTS if f"{tag}/{k}" in base and k.endswith("_s") == leaf.endswith("_s")]
            if leaf not in PRODUCTS:
                block = [b0]
            if off is not None and v.shape[0] == off[-1]:
                err = max(_rel(v[off[i]:off[i + 1]], b0[off[i]:off[i + 1]], max(float(np.abs(x[off[i]:off[i + 1]]).max()) for x in block))
                          for i in range(len(off) - 1) if off[i + 1] > off[i])
            elif v.ndim == 3:
                err = max(_rel(v[i], b0[i], max(float(np.abs(x[i]).max()) for x in block)) for i in range(v.shape[0]))
            else:
                err = _rel(v, b0)
            note(cfg, "vs default/" + "/".join(parts[1:3]), "-", err, CROSS_TOL, key)
        for key, v in got.items():
            if key.startswith("grad/") and key in base and not key.endswith("/route") and np.any(base[key]):
                note(cfg, "vs default/grad", "-", _rel(v, base[key]), CROSS_TOL, key)

    print("\nsecond-order route matrix: configuration, case, route(s), worst relative error")
    for (cfg, case), routes in table.items():
        print(f"{cfg:<16} {case:<28} {' '.join(sorted(routes)):<40} {worst[(cfg, case)]:.2e}")
    assert not msgs, f"{len(msgs)} failures:\n" + "\n".join(msgs[:100])
