"""What the unmodified reference returned in two CPU tests that used to import it live.

    python tests/golden/make_ref_check_golden.py      # needs the reference checkout (oracle/_refimport.py REFERENCE_ROOT)

  ref_combined_loss.npz   tests/test_trainer_cpu.py::test_combined_loss_equals_the_references: the reference's
                          chgnet.trainer.trainer.CombinedLoss on the test's seeded batch, for every (criterion, missing,
                          allow) case: loss, MAEs, MAE sizes and d loss / d prediction (autograd), keys ``<case>/<name>``
  ref_fresh_input.npz     tests/test_oracle_golden.py::test_oracle_matches_live_reference_on_fresh_input: the reference's
                          own converter (algorithm "fast", its compiled cygraph) on the test's random 5-atom cell, fed our
                          neighbour list, and its CHGNet.predict_graph(task "efsm", all extras) with weights_seed0, one thread
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle._refimport import load_reference  # noqa: E402

load_reference(fast_graph=True)
from chgnet.graph.converter import CrystalGraphConverter as RefConverter  # noqa: E402
from chgnet.model.model import CHGNet as RefCHGNet  # noqa: E402
from chgnet.trainer.trainer import CombinedLoss as RefLoss  # noqa: E402

GRAPH_KEYS = ("atom_graph", "directed2undirected", "undirected2directed", "bond_graph", "neighbor_image")


def combined_loss() -> dict:
    from test_trainer_cpu import LOSS_CASES, _batch, loss_kwargs

    out = {}
    for criterion, missing, allow in LOSS_CASES:
        targ, pred = _batch(np.random.default_rng(3), missing)
        tp = {"e": torch.tensor(pred["e"], requires_grad=True), "f": [torch.tensor(x, requires_grad=True) for x in pred["f"]],
              "s": [torch.tensor(x, requires_grad=True) for x in pred["s"]], "m": [torch.tensor(x, requires_grad=True) for x in pred["m"]]}
        tt = {"e": torch.tensor(targ["e"]), "f": [torch.tensor(x) for x in targ["f"]], "s": [torch.tensor(x) for x in targ["s"]],
              "m": [None if x is None else torch.tensor(x) for x in targ["m"]]}
        ref = RefLoss(**loss_kwargs(criterion, allow))(tt, tp)
        p = f"{criterion}_{int(missing)}_{int(allow)}/"
        out[p + "pred_e"] = pred["e"]
        out[p + "loss"] = np.float64(ref["loss"].detach())
        for k in "efsm":
            out[p + f"{k}_MAE"] = np.float64(ref[f"{k}_MAE"].detach() if torch.is_tensor(ref[f"{k}_MAE"]) else ref[f"{k}_MAE"])
            out[p + f"{k}_MAE_size"] = np.float64(int(ref[f"{k}_MAE_size"]))
        ref["loss"].backward()
        out[p + "grad_e"] = tp["e"].grad.numpy()
        out[p + "grad_f"] = np.concatenate([x.grad.numpy() for x in tp["f"]])
        out[p + "grad_s"] = np.concatenate([x.grad.numpy() for x in tp["s"]])
        out[p + "grad_m"] = np.concatenate([np.zeros(len(x)) if x.grad is None else x.grad.numpy() for x in tp["m"]])
    return out


def fresh_input() -> dict:
    from make_golden_helpers import DuckStructure
    from test_oracle_golden import fresh_structure

    from chgnet_amd.graph.converter import build_graph_arrays

    torch.set_num_threads(1)
    weights = dict(np.load(os.path.join(HERE, "weights_seed0.npz")))
    model = RefCHGNet()
    model.load_state_dict({k: torch.tensor(v) for k, v in weights.items()})
    s = fresh_structure()
    a = build_graph_arrays(s.frac_coords, s.lattice.matrix, 6.0, 3.0)
    nl = {"center": a["atom_graph"][:, 0].astype(np.int64), "neighbor": a["atom_graph"][:, 1].astype(np.int64),
          "image": a["image"].astype(np.int64), "distance": a["distance"]}
    conv = RefConverter(atom_graph_cutoff=6, bond_graph_cutoff=3, algorithm="fast")
    assert conv.algorithm == "fast"
    rg = conv(DuckStructure(s, nl))
    out = {f"graph/{k}": getattr(rg, k).numpy() for k in GRAPH_KEYS}
    ref = model.predict_graph(rg, task="efsm", return_site_energies=True, return_atom_feas=True, return_crystal_feas=True)
    out.update({f"out/{k}": np.asarray(v) for k, v in ref.items()})
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "ref_combined_loss.npz"), **combined_loss())
    np.savez_compressed(os.path.join(HERE, "ref_fresh_input.npz"), **fresh_input())
