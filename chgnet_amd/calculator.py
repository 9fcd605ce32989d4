"""``CHGNetCalculator`` -- the ASE-facing surface of the reference
(chgnet/model/dynamics.py:58-181) on top of the HIP engine.

ASE is an optional dependency (absent in the build container): when it imports, the class derives
from ``ase.calculators.calculator.Calculator`` so ASE optimisers / MD drivers can use it unchanged;
otherwise a minimal base with the same ``results`` / ``get_*`` contract is used so that the
in-repo MD smoke driver and the tests still work.
"""

from __future__ import annotations

import warnings

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
    of our / pymatgen's structures -> ``Structure`` (replaces AseAtomsAdaptor, dynamics.py:156).  The ``constraints`` of an
    ASE-like object become the ``selective_dynamics`` site property ([n, 3], True = free: pymatgen's convention), as
    AseAtomsAdaptor does: ``FixAtoms`` (``index``) and ``FixCartesian`` (``index``, ``mask`` with True = held, ASE >= 3.23),
    matched by class name; any other constraint is reported with a ``UserWarning`` and left out."""
    if hasattr(atoms, "frac_coords") and hasattr(atoms, "lattice"):
        return atoms
    cell = np.asarray(atoms.get_cell()[:] if hasattr(atoms.get_cell(), "__getitem__") else atoms.get_cell())
    structure = Structure(Lattice(cell), np.asarray(atoms.get_atomic_numbers()), np.asarray(atoms.get_scaled_positions(wrap=False)))
    constraints = getattr(atoms, "constraints", None)
    if constraints is None:
        return structure
    if not isinstance(constraints, (list, tuple)):
        constraints = [constraints]
    n = len(structure)
    held, seen = np.zeros((n, 3), bool), False
    for c in constraints:
        name = type(c).__name__
        if name not in ("FixAtoms", "FixCartesian"):
            warnings.warn(f"constraint {name} is not supported by the device drivers and is ignored (FixAtoms and FixCartesian are honoured)",
                          UserWarning, stacklevel=2)
            continue
        index = np.atleast_1d(np.asarray(c.index))
        if index.dtype == bool:
            index = np.flatnonzero(index)
        if index.size and (index.min() < -n or index.max() >= n):
            raise ValueError(f"constraint {name} names atom {int(index.max() if index.max() >= n else index.min())} of a structure with {n} atoms")
        held[index] |= True if name == "FixAtoms" else np.asarray(c.mask, bool).reshape(-1, 3)
        seen = True
    if seen:
        structure.add_site_property("selective_dynamics", (~held).tolist())
    return structure


def normalize_fixed(entry, n: int) -> np.ndarray | None:
    """One ``fixed_atoms`` entry -> mask [n, 3] uint8 with 1 = held (``None`` stays ``None``): a sequence of atom indices, a bool [n]
    array (True = the whole atom is held) or a bool [n, 3] array (True = the component is held).  ``ValueError`` for anything else."""
    if entry is None:
        return None
    a = np.asarray(entry)
    mask = np.zeros((n, 3), np.uint8)
    if a.dtype == bool:
        if a.shape == (n,):
            mask[a] = 1
        elif a.shape == (n, 3):
            mask[a] = 1
        else:
            raise ValueError(f"a bool fixed_atoms mask must have shape ({n},) or ({n}, 3), got {a.shape}")
        return mask
    if a.size == 0:
        return mask
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError("fixed_atoms must be a sequence of atom indices, a bool [n] array or a bool [n, 3] array")
    if a.min() < -n or a.max() >= n:
        raise ValueError(f"fixed_atoms index {int(a.max() if a.max() >= n else a.min())} is out of range for {n} atoms")
    mask[a] = 1
    return mask


def structure_fixed(structure, fixed_atoms=None) -> np.ndarray | None:
    """The mask [n, 3] uint8 (1 = held) of one structure: ``fixed_atoms`` when given, else its ``selective_dynamics`` site property
    ([n, 3], True = free); ``None`` when there is neither."""
    n = len(structure)
    if fixed_atoms is not None:
        return normalize_fixed(fixed_atoms, n)
    sd = (getattr(structure, "site_properties", None) or {}).get("selective_dynamics")
    if sd is None:
        return None
    sd = np.asarray(sd)
    if sd.shape != (n, 3):
        raise ValueError(f"selective_dynamics must have shape ({n}, 3), got {sd.shape}")
    return (~sd.astype(bool)).astype(np.uint8)


def check_fixed(mask: np.ndarray | None, *, moving_cell: bool, needs_dof: bool, what: str = "the structure") -> None:
    """The refusals of ``chg_relax_set_fixed`` / ``chg_md_set_fixed``, raised as ``ValueError`` before anything reaches the device."""
    if mask is None:
        return
    held = mask.astype(bool).sum(axis=1)
    if moving_cell and np.any((held != 0) & (held != 3)):
        raise ValueError(f"{what} holds only some cartesian components of atom {int(np.flatnonzero((held != 0) & (held != 3))[0])}: that has "
                         "no meaning while the cell moves (hold the whole atom, or keep the cell fixed)")
    if needs_dof and held.sum() == 3 * len(mask):
        raise ValueError(f"{what} has no free component left for the thermostat")


def join_fixed(masks: list, n_atoms) -> np.ndarray | None:
    """Per-structure masks (``None``: nothing held) -> one [N, 3] uint8 array for the handle, or ``None`` when nothing is held at all."""
    if all(m is None or not m.any() for m in masks):
        return None
    return np.ascontiguousarray(np.concatenate([np.zeros((int(n), 3), np.uint8) if m is None else m for m, n in zip(masks, n_atoms)]))


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
