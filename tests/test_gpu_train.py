"""Fine-tuning backward on the GPU (SURVEY 8f-3 stage A): chg_backward -- the gradient of
sum_b c_b * e_b with respect to all 136 parameter tensors -- against torch.autograd through the CPU oracle
(what loss.backward() computes in the reference's train step, trainer.py:399-411), fp64 as ground truth.

Tolerance: per tensor, max|engine - oracle_fp64| <= 1e-4 * max|oracle_fp64| (fp32 engine; the oracle's own
fp32 autograd differs from its fp64 by ~1e-6..1e-5 relative on these tensors)."""

from __future__ import annotations

import numpy as np
import pytest

from conftest import load_case

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4
DEAD = ("angle_layers.2.", "site_wise", "composition_model")     # no path to the energy (model.py:442-496, 484-487, 179-182)


def _compare(got: dict, want: dict, context: str):
    msgs = []
    assert set(got) == set(want)
    for k, ref in want.items():
        g = got[k]
        assert g.shape == ref.shape and g.dtype == np.float32, k
        if k.startswith(DEAD):
            if np.any(g) or np.any(ref):
                msgs.append(f"{k}: expected an all-zero gradient")
            continue
        scale = float(np.abs(ref).max())
        err = float(np.abs(g - ref).max())
        if not np.isfinite(g).all() or err > REL_TOL * scale:
            msgs.append(f"{k}: max|d|={err:.3e} scale={scale:.3e} rel={err / max(scale, 1e-300):.2e}")
    assert not msgs, context + ": " + "; ".join(msgs)


def _oracle_grads(weights, graphs, cot, **kw):
    import torch

    from oracle.chgnet_oracle import OracleCHGNet

    torch.set_num_threads(8)
    c = torch.tensor(np.asarray(cot, np.float64))
    return OracleCHGNet(weights, dtype=torch.float64, **kw).parameter_gradients(graphs, lambda o: (o["e"] * c).sum())


def test_packed_weight_gradients_vs_pipeline_model(hip_engine, packed_weights):
    """Localisation test: every entry of the gradient blob (packed names: ac0.w_cn, bc1.w2g, ...) against the
    float64 numpy model of the kernel pipeline (oracle/staged_ref.py, itself == autograd to 1e-10 on CPU)."""
    from oracle.staged_ref import StagedModel

    graphs = [load_case(n)[0] for n in ("limno2", "noangle", "s16tri")]
    cot = np.array([0.3, -1.2, 0.7], np.float32)
    batch = hip_engine.upload(graphs)
    hip_engine.predict(batch, "e")
    blob = hip_engine.backward(batch, cot)
    want = StagedModel(packed_weights).run(batch.packed, e_cot=cot.astype(np.float64))["wgrad"]
    batch.free()
    msgs = []
    for name, ref in want.items():
        off, shape = packed_weights.offsets[name]
        got = blob[off:off + int(np.prod(shape))].reshape(shape)
        scale, err = float(np.abs(ref).max()), float(np.abs(got - ref).max())
        if name.startswith("bc") and name.endswith("b_out"):
            continue                                   # BondConv mlp_out bias: 0.2.0 only, not differentiated (raises in CHGNet.backward)
        if not err <= REL_TOL * scale:
            msgs.append(f"{name}: max|d|={err:.3e} scale={scale:.3e}")
    assert not msgs, "; ".join(msgs)
    # derived blob entries (transposed copies, q_bias) and the frozen AtomRef carry no gradient
    for name, (off, shape) in packed_weights.offsets.items():
        if name not in want:
            assert not np.any(blob[off:off + int(np.prod(shape))]), name


def test_parameter_gradients_of_the_energy_loss_vs_autograd(hip_engine, golden_weights):
    from chgnet_amd.model import CHGNet

    graphs = [load_case(n)[0] for n in ("limno2", "noangle", "s16tri", "s40", "li9co7o16")]
    rng = np.random.default_rng(5)
    cot = rng.normal(size=len(graphs)).astype(np.float32)
    model = CHGNet(state_dict=golden_weights)
    model._engine = hip_engine
    try:
        out = model.forward(graphs, task="efs")
        assert np.isfinite(out["e"]).all()
        got = model.backward(cot)
        _compare(got, _oracle_grads(golden_weights, graphs, cot), "mixed batch, random cotangent")
        got1 = model.backward()                                   # default cotangent: ones
        _compare(got1, _oracle_grads(golden_weights, graphs, np.ones(len(graphs))), "mixed batch, ones")
        again = model.backward(cot)                               # repeatable: the sweep re-zeroes its workspace
        for k in got:
            assert np.allclose(again[k], got[k], rtol=0, atol=2e-5 * max(1e-30, float(np.abs(got[k]).max()))), k
        # a batch without any angle skips BondConv / AngleUpdate: their gradients are zero, the rest still matches
        g0 = [load_case("noangle")[0]]
        model.forward(g0, task="e")
        got0 = model.backward(np.array([2.0], np.float32))
        want0 = _oracle_grads(golden_weights, g0, [2.0])
        for k in want0:
            if k.startswith(("bond_conv_layers", "angle_layers", "angle_embedding", "angle_basis", "bond_weights_bg",
                             "bond_basis_expansion.rbf_expansion_bg")):
                assert not np.any(want0[k]) and not np.any(got0[k]), k
        _compare(got0, want0, "zero-angle batch")
    finally:
        model.release_forward_state()
        model._engine = None
    with pytest.raises(RuntimeError, match="preceding forward"):
        model.backward()


def test_parameter_gradients_extensive_model_without_atomref():
    """is_intensive=False, no composition model, 3 interaction blocks: the cotangent is not divided by the atom count."""
    from chgnet_amd.model import CHGNet, random_state_dict

    args = dict(n_conv=3, is_intensive=False, composition_model=None)
    sd = random_state_dict({"n_conv": 3, **args}, seed=21)
    rng = np.random.default_rng(22)
    for k, v in sd.items():
        if ".bn" in k or k.startswith("readout_norm") or k.endswith("frequencies"):
            sd[k] = (v + 0.1 * rng.normal(size=v.shape)).astype(np.float32)
    sd.pop("composition_model.fc.weight", None)
    model = CHGNet(state_dict=sd, **args)
    graphs = [load_case(n)[0] for n in ("limno2", "s16tri")]
    cot = np.array([0.5, -0.25], np.float32)
    try:
        model.forward(graphs, task="e")
        got = model.backward(cot)
    finally:
        model.release_forward_state()
    want = _oracle_grads(sd, graphs, cot, is_intensive=False)
    dead = ("angle_layers.1.", "site_wise")
    msgs = []
    for k, ref in want.items():
        if k.startswith(dead):
            assert not np.any(got[k]), k
            continue
        scale, err = float(np.abs(ref).max()), float(np.abs(got[k] - ref).max())
        if not err <= REL_TOL * scale:
            msgs.append(f"{k}: {err:.3e} / {scale:.3e}")
    assert not msgs, "; ".join(msgs)


def test_backward_error_paths(hip_engine):
    g = load_case("limno2")[0]
    batch = hip_engine.upload([g])
    try:
        with pytest.raises(RuntimeError, match="chg_predict on this batch first"):
            hip_engine.backward(batch)
        hip_engine.predict(batch, "e")
        with pytest.raises(ValueError, match="e_grad has 2 entries"):
            hip_engine.backward(batch, np.ones(2, np.float32))
        with pytest.raises(ValueError, match="m_grad has 3 entries"):
            hip_engine.backward(batch, None, np.ones(3, np.float32))
    finally:
        batch.free()


def test_energy_and_magmom_loss_gradients_vs_autograd(hip_engine, golden_weights):
    """d( sum_b c_b e_b + sum_i g_i m_i ) / d(parameters): the magmom head m = |h . w + b| (model.py:484-487) adds a
    first-order path into the atom features before the last AtomConv and gives site_wise.{weight,bias} a gradient."""
    import torch
    from chgnet_amd.model import CHGNet

    graphs = [load_case(n)[0] for n in ("limno2", "noangle", "s16tri")]
    n_atoms = sum(len(g.atomic_number) for g in graphs)
    rng = np.random.default_rng(8)
    ce, gm = rng.normal(size=len(graphs)).astype(np.float32), rng.normal(size=n_atoms).astype(np.float32)
    model = CHGNet(state_dict=golden_weights)
    model._engine = hip_engine
    try:
        model.forward(graphs, task="em")
        got = model.backward(ce, gm)
    finally:
        model.release_forward_state()
        model._engine = None
    from oracle.chgnet_oracle import OracleCHGNet

    torch.set_num_threads(8)
    tce, tgm = torch.tensor(ce.astype(np.float64)), torch.tensor(gm.astype(np.float64))
    want = OracleCHGNet(golden_weights, dtype=torch.float64).parameter_gradients(
        graphs, lambda o: (o["e"] * tce).sum() + (o["m"] * tgm).sum(), task="em")
    msgs = []
    for k, ref in want.items():
        if k.startswith(("angle_layers.2.", "composition_model")):
            assert not np.any(got[k]), k
            continue
        scale, err = float(np.abs(ref).max()), float(np.abs(got[k] - ref).max())
        assert scale > 0, k
        if not err <= REL_TOL * scale:
            msgs.append(f"{k}: {err:.3e} / {scale:.3e}")
    assert not msgs, "; ".join(msgs)


def test_train_step_lowers_the_loss_and_updates_the_engine(golden_weights):
    """A few Adam steps of the energy + magmom loss on synthetic labels (trainer.py:386-411 for the terms the device
    differentiates): the loss goes down, predictions move, the engine really runs on the updated weights."""
    import bench
    from chgnet_amd import CrystalGraphConverter
    from chgnet_amd.model import CHGNet
    from chgnet_amd.trainer import TrainStep

    conv = CrystalGraphConverter()
    graphs = [conv(s) for s in bench.workload_structures(24, 300)]
    model = CHGNet(state_dict=golden_weights)
    before = model.predict_graph(graphs, task="em")
    # labels a small, coherent shift away from the current predictions (with torch.optim.Adam at this learning rate the
    # CPU oracle brings the same loss from 3.5e-3 to 1.8e-4 in 10 steps)
    targets = {"e": np.array([p["e"] for p in before]) + 0.05, "m": [p["m"] + 0.1 for p in before]}
    step = TrainStep(model, targets="em", learning_rate=2e-4)
    try:
        losses = [step(graphs, targets)["loss"] for _ in range(10)]
    finally:
        model.release_forward_state()
    assert np.isfinite(losses).all() and abs(losses[0] - 3.5e-3) < 2e-4 and losses[-1] < 0.3 * losses[0], losses
    after = model.predict_graph(graphs, task="em")
    assert max(abs(a["e"] - b["e"]) for a, b in zip(after, before)) > 1e-4            # the engine sees the new weights
    fresh = CHGNet(state_dict=model.state_dict()).predict_graph(graphs[:3], task="em")  # ... and they are the state_dict's
    for a, b in zip(after[:3], fresh):
        assert abs(a["e"] - b["e"]) < 2e-6 and np.abs(a["m"] - b["m"]).max() < 2e-6


# ---------------------------------------------------------------------------------------------------------
# stage B: force / stress terms (second-order sweep)
# ---------------------------------------------------------------------------------------------------------
REL_TOL_B = 3e-4     # fp32, second derivatives: the fp32 torch double-backward of the oracle itself is ~1e-5..1e-4 off its fp64


def _cots(rng, pb):
    return (rng.normal(size=pb.n_struct).astype(np.float32), rng.normal(size=(pb.n_atoms, 3)).astype(np.float32),
            rng.normal(size=(pb.n_struct, 3, 3)).astype(np.float32))


def _packed_vs_model(blob, want, pw, msgs, whole_tol=None):
    """Every packed entry of a gradient blob against the float64 sweep model (bc*.b_out: no entry of StagedTrainer's); optionally the
    whole blob against max|ref| over all entries as well."""
    whole_err = whole_scale = 0.0
    for name, ref in want.items():
        if name.startswith("bc") and name.endswith("b_out"):
            continue
        off, shape = pw.offsets[name]
        got = blob[off:off + int(np.prod(shape))].reshape(shape)
        scale, err = float(np.abs(ref).max()), float(np.abs(got - ref).max())
        whole_err, whole_scale = max(whole_err, err), max(whole_scale, scale)
        if not np.isfinite(got).all() or not err <= REL_TOL_B * scale + 1e-12:
            msgs.append(f"{name}: max|d|={err:.3e} scale={scale:.3e}")
    if whole_tol is not None and not whole_err <= whole_tol * whole_scale:
        msgs.append(f"whole blob: max|d|={whole_err:.3e} scale={whole_scale:.3e}")


@pytest.mark.parametrize("terms", ["efs", "f", "s"])
def test_second_order_packed_gradients_vs_pipeline_model(hip_engine, packed_weights, terms):
    """Localisation test for the force / stress terms: every packed entry of the gradient blob against the float64 model of
    the tangent + two-adjoint sweep (oracle/staged_train.py, == torch double-backward to 2e-9 on the CPU)."""
    from oracle.staged_train import StagedTrainer

    graphs = [load_case(n)[0] for n in ("limno2", "noangle", "s16tri")]
    batch = hip_engine.upload(graphs)
    pb = batch.packed
    gE, gF, gS = _cots(np.random.default_rng(17), pb)
    cE, cF, cS = (gE if "e" in terms else None), (gF if "f" in terms else None), (gS if "s" in terms else None)
    hip_engine.predict(batch, "efs")
    blob = hip_engine.backward(batch, cE if cE is not None else np.zeros(pb.n_struct, np.float32), None, cF, cS)
    want = StagedTrainer(packed_weights).run(pb, gE=cE, gF=cF, gS=cS)["wgrad"]
    batch.free()
    msgs = []
    _packed_vs_model(blob, want, packed_weights, msgs)
    assert not msgs, f"[{terms}] " + "; ".join(msgs)


@pytest.mark.parametrize("which", ["seed0", "trained_like"])
def test_force_and_stress_loss_gradients_vs_double_backward(hip_engine, golden_weights, trained_like_weights, which):
    """d( sum ce e + sum gm m + sum gF.F + sum gS:S ) / d(all parameters) against torch double-backward through the fp64 oracle
    (the reference's create_graph=True path) on the five golden structures; also at trained-checkpoint magnitudes
    (saturating gates exercise the second derivatives of the activations)."""
    import torch
    from chgnet_amd.engine import Engine
    from chgnet_amd.model import CHGNet
    from chgnet_amd.pack import pack_weights
    from oracle.chgnet_oracle import OracleCHGNet

    if which == "trained_like":
        golden_weights = trained_like_weights
        hip_engine = Engine(pack_weights(golden_weights), 0)

    graphs = [load_case(n)[0] for n in ("limno2", "noangle", "s16tri", "s40", "li9co7o16")]
    n_atoms = sum(len(g.atomic_number) for g in graphs)
    rng = np.random.default_rng(23)
    ce, gm = rng.normal(size=len(graphs)).astype(np.float32), rng.normal(size=n_atoms).astype(np.float32)
    gf, gs = rng.normal(size=(n_atoms, 3)).astype(np.float32), rng.normal(size=(len(graphs), 3, 3)).astype(np.float32)
    model = CHGNet(state_dict=golden_weights)
    model._engine = hip_engine
    try:
        model.forward(graphs, task="efsm")
        got = model.backward(ce, gm, gf, gs)
    finally:
        model.release_forward_state()
        model._engine = None
        if which == "trained_like":
            hip_engine.close()
    torch.set_num_threads(8)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    want = OracleCHGNet(golden_weights, dtype=torch.float64).parameter_gradients(
        graphs, lambda o: (o["e"] * t(ce)).sum() + (o["m"] * t(gm)).sum() + (o["f"] * t(gf)).sum() + (o["s"] * t(gs)).sum(), task="efsm")
    msgs = []
    for k, ref in want.items():
        if k.startswith(("angle_layers.2.", "composition_model")):
            assert not np.any(got[k]), k
            continue
        scale, err = float(np.abs(ref).max()), float(np.abs(got[k] - ref).max())
        if not np.isfinite(got[k]).all() or not err <= REL_TOL_B * scale:
            msgs.append(f"{k}: {err:.3e} / {scale:.3e} = {err / max(scale, 1e-300):.1e}")
    assert not msgs, "; ".join(msgs)


@pytest.mark.parametrize("fname,which", [("grad_five_seed0.npz", "seed0"), ("grad_five_trained_like.npz", "trained_like"),
                                         ("grad_mixed_seed0.npz", "seed0")])
def test_loss_gradients_vs_the_reference_backward_fixtures(hip_engine, golden_weights, trained_like_weights, fname, which):
    """The same loss against gradients the UNMODIFIED reference produced with loss.backward() in train mode
    (tests/golden/make_grad_golden.py; model.py:517-535, trainer.py:399-411): reference-held numbers, fp32 on the CPU.
    Tolerance: the fixture itself is fp32 (its distance to the float64 oracle is up to 2e-5 relative), so 3e-4 + that."""
    import os

    from chgnet_amd.engine import Engine
    from chgnet_amd.model import CHGNet
    from chgnet_amd.pack import pack_weights
    from conftest import GOLDEN

    d = np.load(os.path.join(GOLDEN, fname))
    want = {k[len("grad/"):]: d[k] for k in d.files if k.startswith("grad/")}
    weights = golden_weights if which == "seed0" else trained_like_weights
    eng = hip_engine if which == "seed0" else Engine(pack_weights(weights), 0)
    graphs = [load_case(str(n))[0] for n in d["order"]]
    model = CHGNet(state_dict=weights)
    model._engine = eng
    try:
        model.forward(graphs, task="efsm")
        got = model.backward(d["cot_e"], d["cot_m"], d["cot_f"], d["cot_s"])
    finally:
        model.release_forward_state()
        model._engine = None
        if which != "seed0":
            eng.close()
    msgs = []
    for k, ref in want.items():
        if k.startswith(("angle_layers.2.", "composition_model", "site_wise")) and not np.any(ref):
            assert not np.any(got[k]), k
            continue
        scale, err = float(np.abs(ref).max()), float(np.abs(got[k] - ref).max())
        if not np.isfinite(got[k]).all() or not err <= 3.2e-4 * scale:
            msgs.append(f"{k}: {err:.3e} / {scale:.3e} = {err / max(scale, 1e-300):.1e}")
    assert not msgs, "; ".join(msgs)


def test_train_step_with_force_and_stress_terms(golden_weights):
    """All four terms of CombinedLoss through the device: energy, force, stress, magmom labels a small coherent shift away
    from the current predictions; Adam steps bring the loss down and the engine runs on the updated weights."""
    import bench
    from chgnet_amd import CrystalGraphConverter
    from chgnet_amd.model import CHGNet
    from chgnet_amd.trainer import TrainStep

    conv = CrystalGraphConverter()
    graphs = [conv(s) for s in bench.workload_structures(16, 500)]
    model = CHGNet(state_dict=golden_weights)
    before = model.predict_graph(graphs, task="efsm")
    targets = {"e": np.array([p["e"] for p in before]) + 0.05, "f": [p["f"] * 1.5 for p in before],
               "s": [p["s"] + 0.1 * np.eye(3, dtype=np.float32) for p in before], "m": [p["m"] + 0.1 for p in before]}
    step = TrainStep(model, targets="efsm", learning_rate=2e-4)
    try:
        losses = [step(graphs, targets)["loss"] for _ in range(10)]
    finally:
        model.release_forward_state()
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0], losses


def test_second_order_gradients_on_edge_case_batches(hip_engine, golden_weights):
    """Stage B on batches that skip whole branches of the sweep: no angle at all (BondConv / AngleUpdate never run) and a
    structure of isolated atoms next to a normal one."""
    import torch
    from chgnet_amd import CrystalGraphConverter, Structure
    from chgnet_amd.graph.structure import Lattice
    from chgnet_amd.model import CHGNet
    from oracle.chgnet_oracle import OracleCHGNet

    conv = CrystalGraphConverter(on_isolated_atoms="ignore")
    lone = conv(Structure(Lattice(np.eye(3) * 20.0), ["H", "O"], [[0, 0, 0], [0.5, 0.5, 0.5]]))
    cases = {"zero-angle batch": [load_case("noangle")[0]], "isolated atoms + normal": [lone, load_case("limno2")[0]]}
    torch.set_num_threads(8)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    model = CHGNet(state_dict=golden_weights)
    model._engine = hip_engine
    try:
        for label, graphs in cases.items():
            n_atoms = sum(len(g.atomic_number) for g in graphs)
            rng = np.random.default_rng(31)
            ce = rng.normal(size=len(graphs)).astype(np.float32)
            gf, gs = rng.normal(size=(n_atoms, 3)).astype(np.float32), rng.normal(size=(len(graphs), 3, 3)).astype(np.float32)
            model.forward(graphs, task="efs")
            got = model.backward(ce, None, gf, gs)
            want = OracleCHGNet(golden_weights, dtype=torch.float64).parameter_gradients(
                graphs, lambda o: (o["e"] * t(ce)).sum() + (o["f"] * t(gf)).sum() + (o["s"] * t(gs)).sum(), task="efs")
            for k, ref in want.items():
                scale = float(np.abs(ref).max())
                assert np.isfinite(got[k]).all(), (label, k)
                if scale == 0:
                    assert float(np.abs(got[k]).max()) < 1e-9, (label, k)
                else:
                    assert float(np.abs(got[k] - ref).max()) <= REL_TOL_B * scale, (label, k, float(np.abs(got[k] - ref).max()), scale)
    finally:
        model.release_forward_state()
        model._engine = None


def test_gradients_are_additive_over_structures_at_scale(hip_engine):
    """Size-independent property at a size no CPU oracle reaches: with per-structure cotangents the parameter gradient of
    a batch is the sum of the gradients of its parts (512 structures = 256 + 256), first- and second-order sweeps alike."""
    import bench

    structs = bench.workload_structures(512, 2000)
    rng = np.random.default_rng(77)

    def grads(sl, second_order):
        batch = hip_engine.build_batch(structs[sl])
        pb = batch.packed
        a0 = sl.start * 40
        hip_engine.predict(batch, "efs")
        kw = dict(f_grad=gF[a0:a0 + pb.n_atoms], s_grad=gS[sl]) if second_order else {}
        g = hip_engine.backward(batch, ce[sl], gm[a0:a0 + pb.n_atoms], **kw)
        batch.free()
        return g.astype(np.float64)

    ce, gm = rng.normal(size=512).astype(np.float32), rng.normal(size=512 * 40).astype(np.float32)
    gF, gS = rng.normal(size=(512 * 40, 3)).astype(np.float32), rng.normal(size=(512, 3, 3)).astype(np.float32)
    for second_order in (False, True):
        whole = grads(slice(0, 512), second_order)
        parts = grads(slice(0, 256), second_order) + grads(slice(256, 512), second_order)
        scale = np.abs(whole).max()
        assert np.isfinite(whole).all() and scale > 0
        # fp32 sums over ~2M rows in a different order: compare against the largest entry
        assert np.abs(whole - parts).max() < 2e-4 * scale, (second_order, float(np.abs(whole - parts).max()), float(scale))


def test_stress_term_after_a_cell_update_uses_the_new_volume(hip_engine):
    """chg_batch_update_geometry(lattice) refreshes the host copy of the cell volumes that scales the stress cotangent: a
    backward on a resident batch whose cell was rescaled by 0.5 % (graph topology unchanged) equals the backward on a batch
    uploaded with the new cell."""
    import bench

    from chgnet_amd.pack import PackedBatch, pack_batch

    pb = pack_batch(bench.build_workload(4, 4100))
    scale = 1.005
    rng = np.random.default_rng(5)
    gs = rng.normal(size=(4, 3, 3)).astype(np.float32)
    ce = rng.normal(size=4).astype(np.float32)
    resident = hip_engine.upload(pb)
    try:
        resident.update_geometry(lattice=np.asarray(pb.arrays["lattice"], np.float32).reshape(-1, 3, 3) * scale)
        hip_engine.predict(resident, "efs")
        got = hip_engine.backward(resident, ce, s_grad=gs)
        arr = dict(pb.arrays)
        arr["lattice"] = np.ascontiguousarray(np.asarray(arr["lattice"]) * scale)
        fresh = hip_engine.upload(PackedBatch(pb.n_struct, pb.n_atoms, pb.n_directed, pb.n_undirected, pb.n_angles, pb.n_bnodes, arr))
        try:
            hip_engine.predict(fresh, "efs")
            want = hip_engine.backward(fresh, ce, s_grad=gs)
        finally:
            fresh.free()
    finally:
        resident.free()
    ref = float(np.abs(want).max())
    assert ref > 0 and np.abs(got - want).max() <= 1e-4 * ref, float(np.abs(got - want).max() / ref)


def test_fused_second_order_sweep_on_a_large_batch_vs_the_float64_sweep_model(hip_engine, packed_weights):
    """kernels_train2_tile.h on a batch large enough for full tiles, ragged tails and long runs (24 structures, 960 atoms, 82,776
    directed edges, 96,280 angles) against the float64 model of the same sweep (oracle/staged_train.py, == torch double-backward to
    2e-9 on the CPU); the magmom cotangent, a first-order term, is checked against double-backward elsewhere."""
    import bench
    from chgnet_amd.pack import pack_batch
    from oracle.staged_train import StagedTrainer

    pb = pack_batch(bench.build_workload(24, 5200))
    rng = np.random.default_rng(11)
    ce = rng.normal(size=24).astype(np.float32); gm = rng.normal(size=pb.n_atoms).astype(np.float32)
    gf = rng.normal(size=(pb.n_atoms, 3)).astype(np.float32); gs = rng.normal(size=(24, 3, 3)).astype(np.float32)
    b = hip_engine.upload(pb)
    try:
        hip_engine.predict(b, "e")     # energy-only: chg_backward has to run the force sweep itself before the second-order sweep
        g1 = hip_engine.backward(b, ce, gm, f_grad=gf, s_grad=gs).astype(np.float64)
        hip_engine.predict(b, "efsm")
        g2 = hip_engine.backward(b, ce, gm, f_grad=gf, s_grad=gs).astype(np.float64)
        hip_engine.backward(b, ce, gm)  # a first-order sweep in between reuses the force sweep's buffers with other seeds
        g3 = hip_engine.backward(b, ce, gm, f_grad=gf, s_grad=gs).astype(np.float64)
        blob = hip_engine.backward(b, ce, None, f_grad=gf, s_grad=gs)
    finally:
        b.free()
    scale = np.abs(g2).max()
    assert scale > 0 and np.isfinite(g1).all() and np.isfinite(g3).all()
    # after an energy-only prediction == after a full one (the sweep's first-order inputs are rebuilt)
    assert np.abs(g1 - g2).max() <= 1e-5 * scale
    assert np.abs(g3 - g2).max() <= 1e-5 * scale      # ... and after a first-order chg_backward in between
    msgs = []
    _packed_vs_model(blob, StagedTrainer(packed_weights).run(pb, gE=ce, gF=gf, gS=gs)["wgrad"], packed_weights, msgs, whole_tol=1e-4)
    assert not msgs, "; ".join(msgs)


def test_frequency_gradients_on_a_ragged_batch_vs_the_float64_sweep_model(trained_like_weights):
    """kernels_train2_freq.h (16-row tiles, MFMA adjoints) on 40 + 3 structures (1,776 atoms, 184,094 angles: ragged last tiles)
    against the float64 model of the sweep.  Compared per ``frequencies`` tensor, each against its own magnitude -- next to the
    weight gradients of the same blob they are small."""
    import bench
    from chgnet_amd import CrystalGraphConverter
    from chgnet_amd.engine import Engine
    from chgnet_amd.pack import pack_batch, pack_weights
    from oracle.staged_train import StagedTrainer

    pw = pack_weights(trained_like_weights)
    conv = CrystalGraphConverter(atom_graph_cutoff=6, bond_graph_cutoff=3)
    pb = pack_batch(bench.build_workload(40, 7100) + [conv(bench.sweep_structure(i)) for i in range(3)])
    rng = np.random.default_rng(12)
    n = pb.n_struct
    gf = rng.normal(size=(pb.n_atoms, 3)).astype(np.float32); gs = rng.normal(size=(n, 3, 3)).astype(np.float32)
    ce = rng.normal(size=n).astype(np.float32)
    eng = Engine(pw, 0)
    try:
        b = eng.upload(pb)
        eng.predict(b, "efs")
        blob = eng.backward(b, ce, None, f_grad=gf, s_grad=gs)
        b.free()
    finally:
        eng.close()
    want = {k: v for k, v in StagedTrainer(pw).run(pb, gE=ce, gF=gf, gS=gs)["wgrad"].items() if k.startswith("freq_")}
    assert len(want) == 3, sorted(want)
    for k, ref in want.items():
        off, shape = pw.offsets[k]
        got = blob[off:off + int(np.prod(shape))].reshape(shape)
        scale = float(np.abs(ref).max())
        assert scale > 0 and np.isfinite(got).all(), k
        assert float(np.abs(got - ref).max()) <= 2e-4 * scale, (k, float(np.abs(got - ref).max()) / scale)


def test_three_piece_bf16_weight_gradient_contraction_equals_the_f32_mfma_one():
    """k_xty3 (long row operands: fp32 cut exactly into three bf16 pieces, six bf16 MFMAs per product) against k_xty (f32 MFMA,
    CHGNET_XTY3=0, chosen once per process: a child process each): first- and second-order gradient blobs agree to fp32
    reassociation on a batch whose angle / edge operands take the new kernel (> 65,536 rows, ragged last stage)."""
    import os
    import subprocess
    import sys
    import tempfile

    code = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import bench
from chgnet_amd.engine import Engine
from chgnet_amd.pack import pack_batch, pack_weights
W = dict(np.load(sys.argv[1] + "/tests/golden/weights_trained_like.npz"))
pb = pack_batch(bench.build_workload(27, 6100))
assert pb.n_angles > 65536 and pb.n_directed > 65536 and pb.n_angles % 32 != 0
rng = np.random.default_rng(13)
ce = rng.normal(size=27).astype(np.float32); gm = rng.normal(size=pb.n_atoms).astype(np.float32)
gf = rng.normal(size=(pb.n_atoms, 3)).astype(np.float32); gs = rng.normal(size=(27, 3, 3)).astype(np.float32)
eng = Engine(pack_weights(W), 0)
b = eng.upload(pb)
eng.predict(b, "efsm")
g1 = eng.backward(b, ce, gm)
g2 = eng.backward(b, ce, gm, f_grad=gf, s_grad=gs)
np.save(sys.argv[2], np.stack([g1, g2]))
'''
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for mode in ("bf16x3", "f32"):
            env = dict(os.environ)
            env.pop("CHGNET_XTY3", None)
            if mode == "f32":
                env["CHGNET_XTY3"] = "0"
            path = os.path.join(tmp, mode + ".npy")
            subprocess.run([sys.executable, "-c", code, repo, path], check=True, env=env, timeout=600)
            out[mode] = np.load(path).astype(np.float64)
    for k, label in ((0, "first order"), (1, "second order")):
        scale = np.abs(out["f32"][k]).max()
        err = np.abs(out["bf16x3"][k] - out["f32"][k]).max()
        assert scale > 0 and np.isfinite(out["bf16x3"][k]).all() and err <= 2e-5 * scale, (label, float(err / scale))


def test_a_missing_energy_cotangent_next_to_other_terms_means_no_energy_term(hip_engine):
    """``backward(batch)`` is the gradient of the summed energies; ``backward(batch, f_grad=...)`` is the force term alone."""
    graphs = [load_case(n)[0] for n in ("limno2", "s16tri")]
    rng = np.random.default_rng(9)
    batch = hip_engine.upload(graphs)
    try:
        gf = rng.normal(size=(batch.packed.n_atoms, 3)).astype(np.float32)
        hip_engine.predict(batch, "ef")
        alone = hip_engine.backward(batch, f_grad=gf)
        zeros = hip_engine.backward(batch, np.zeros(2, np.float32), f_grad=gf)
        ones = hip_engine.backward(batch, np.ones(2, np.float32), f_grad=gf)
        energy = hip_engine.backward(batch)
    finally:
        batch.free()
    scale = float(np.abs(ones).max())
    assert np.abs(alone - zeros).max() <= 1e-6 * scale and np.abs(alone - ones).max() > 1e-3 * scale
    assert np.abs((alone + energy) - ones).max() <= 1e-4 * scale
