"""``CHGNetCalculator`` -- the ASE-facing surface of the reference
(chgnet/model/dynamics.py:58-181) on top of the HIP engine.

ASE is an optional dependency (absent in the build container): when it imports, the class derives
from ``ase.calculators.calculator.Calculator`` so ASE optimisers / MD drivers can use it unchanged;
otherwise a minimal base with the same ``results`` / ``get_*`` contract is used so that the
in-repo MD smoke driver and the tests still work.
"""

from __future__ import annotations

import numpy as np

from chgnet_amd.graph.structure import Lattice, Structure
from chgnet_amd.model import CHGNet

GPA_TO_EV_A3 = 1.0 / 160.21766208   # ase.units.GPa

try:  # pragma: no cover - exercised only where ASE is installed
    from ase.calculators.calculator import Calculator, all_changes, all_properties

    HAVE_ASE = True
except ImportError:
    HAVE_ASE = False
    all_changes, all_properties = [], []

    class Calculator:  # minimal stand-in with ASE's attribute contract
        def __init__(self, **kwargs) -> None:  # noqa: ARG002
            self.results: dict = {}
            self.atoms = None

        def calculate(self, atoms=None, properties=None, system_changes=None) -> None:  # noqa: ARG002
            self.atoms = atoms

        def get_potential_energy(self, atoms=None):
            self.calculate(atoms)
            return self.results["energy"]

        def get_forces(self, atoms=None):
            self.calculate(atoms)
            return self.results["forces"]

        def get_stress(self, atoms=None):
            self.calculate(atoms)
            return self.results["stress"]


def atoms_to_structure(atoms) -> Structure:
    """ASE ``Atoms`` (or anything with get_cell / get_scaled_positions / get_atomic_numbers) or one
    of our / pymatgen's structures -> ``Structure`` (replaces AseAtomsAdaptor, dynamics.py:156)."""
    if hasattr(atoms, "frac_coords") and hasattr(atoms, "lattice"):
        return atoms
    cell = np.asarray(atoms.get_cell()[:] if hasattr(atoms.get_cell(), "__getitem__") else atoms.get_cell())
    return Structure(Lattice(cell), np.asarray(atoms.get_atomic_numbers()), np.asarray(atoms.get_scaled_positions(wrap=False)))


def voigt(s: np.ndarray) -> np.ndarray:
    """3x3 stress (any leading axes) -> ASE Voigt order xx, yy, zz, yz, xz, xy."""
    return np.stack([s[..., 0, 0], s[..., 1, 1], s[..., 2, 2], s[..., 1, 2], s[..., 0, 2], s[..., 0, 1]], axis=-1)


def report_isolated_atoms(model: CHGNet, structures: list) -> None:
    """Isolated atoms of ``structures`` are reported like ``predict_structure`` does (warn / error / ignore), once per structure.
    The graphs are built on the device to count them; the host converter phrases the report only when there are any."""
    conv = model.graph_converter
    if conv.on_isolated_atoms == "ignore":
        return
    eng = model.engine
    batch = eng.build_prepared(eng.prepare_structures(structures), conv.atom_graph_cutoff, conv.bond_graph_cutoff)
    n_iso = batch.packed.n_isolated
    batch.free()
    if n_iso:
        for s in structures:
            conv(s)


class CHGNetCalculator(Calculator):
    """CHGNet Calculator for ASE applications."""

    implemented_properties = ("energy", "forces", "stress", "magmoms", "energies")

    def __init__(self, model: CHGNet | None = None, *, use_device: str | None = None, check_cuda_mem: bool = False,  # noqa: ARG002
                 stress_weight: float = GPA_TO_EV_A3, on_isolated_atoms: str = "warn", return_site_energies: bool = False,
                 **kwargs) -> None:
        """Same arguments as the reference (dynamics.py:63-107).  Like the reference (dynamics.py:156-157) every call rebuilds the
        graph -- here on the device (``chg_batch_build``), ~0.2 ms for a 256-atom cell.

        (Rounds 2-5 had a ``skin`` option that kept a graph with both cutoffs enlarged by a skin resident and only moved the atoms.
        It was exact -- the envelope is zero beyond the cutoff -- but computed 1.3x the bonds and 2.5x the angles to save that 0.2 ms
        and ran 25 % SLOWER than rebuilding; removed in round 6.)"""
        if "skin" in kwargs:
            raise TypeError("CHGNetCalculator(skin=...) was removed: rebuilding the exact-cutoff graph on the device every call is faster")
        super().__init__(**kwargs)
        if model is None:
            self.model = CHGNet.load(verbose=False, use_device=use_device)
        else:
            self.model = model.to(use_device) if use_device is not None else model
        self.device = self.model.device
        self.model.graph_converter.set_isolated_atom_response(on_isolated_atoms)
        self.stress_weight = stress_weight
        self.return_site_energies = return_site_energies
        self.n_graph_builds = 0
        print(f"CHGNet will run on {self.device}")

    @classmethod
    def from_file(cls, path: str, use_device: str | None = None, **kwargs) -> "CHGNetCalculator":
        return cls(model=CHGNet.from_file(path), use_device=use_device, **kwargs)

    @property
    def version(self) -> str | None:
        return self.model.version

    @property
    def n_params(self) -> int:
        return self.model.n_params

    def calculate(self, atoms=None, properties=None, system_changes=None, task: str = "efsm") -> None:
        properties = properties or all_properties
        system_changes = system_changes or all_changes
        super().calculate(atoms=atoms, properties=properties, system_changes=system_changes)
        structure = atoms_to_structure(atoms)
        self.n_graph_builds += 1   # graph rebuilt every call like dynamics.py:156-157, but on the device
        pred = self.model.predict_structure(structure, task=task, return_crystal_feas=True,
                                            return_site_energies=self.return_site_energies)
        extensive_factor = len(structure) if self.model.is_intensive else 1
        key_map = {"e": ("energy", extensive_factor), "f": ("forces", 1), "m": ("magmoms", 1), "s": ("stress", self.stress_weight)}
        self.results.update({long_key: pred[key] * factor for key, (long_key, factor) in key_map.items() if key in pred})
        self.results["free_energy"] = self.results["energy"]
        self.results["crystal_fea"] = pred["crystal_fea"]
        if self.return_site_energies:
            self.results["energies"] = pred["site_energies"]
