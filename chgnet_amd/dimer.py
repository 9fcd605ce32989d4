"""``DimerSearch`` -- batched saddle search from one basin on the device.

``NudgedElasticBand`` finds the saddle between two known minima.  When only the starting basin is known -- surveying the hops around a
defect -- the dimer method (Henkelman & Jonsson 1999) walks uphill along the softest mode instead: a search is two images, the centre
``R`` and ``R + delta N``, whose force difference gives the curvature along the axis ``N`` and the torque that turns ``N`` towards the
softest mode; the centre then follows its force with the component along ``N`` inverted.  The host route is ASE's ``MinModeAtoms``
driving ``CHGNetCalculator`` one image at a time.  Every image of every search is an independent structure for the graph build and the
force sweep, so here the whole search runs behind the C-ABI (``chg_dimer_*``, include/chgnet_hip.h): the images of all searches are one
device batch, one step kernel (csrc/kernels_dimer.h) rotates (one trial image per rotation, the centre is not evaluated again) or
translates (one FIRE optimizer per search), and searches that have stopped drop out of the next graph build.  A batch gives every
search the result it would get alone.  tests/dimer_ref.py restates the step in float64 NumPy; DESIGN.md "Dimer saddle search" gives
the layout.

The cell is fixed and the positions are unwrapped.  Known limit: where every curvature is positive the search climbs along the softest
mode only, so a start deep inside the basin with a poor mode can run away along a soft mode that leads nowhere -- displace along the
intended hop first (``displace``), or start from a band (``from_band``).  Check a saddle that was found with
``chgnet_amd.phonons.vineyard_prefactor``: it refuses anything but exactly one unstable mode.

``fixed_atoms`` takes the forms ``StructOptimizer`` takes (atom indices, bool [n] or bool [n, 3], True = held; without the keyword the
``selective_dynamics`` of the structure); held components of the mode are zeroed before it is normalised.
"""

from __future__ import annotations

import ctypes

import numpy as np

from chgnet_amd import _lib
from chgnet_amd.calculator import CHGNetCalculator, atoms_to_structure, check_fixed, join_fixed, report_isolated_atoms, structure_fixed
from chgnet_amd.graph.structure import Lattice, Structure, atomic_numbers_of
from chgnet_amd.relax import FIRE_DEFAULTS, STATUS_NAMES


def _cart(s) -> np.ndarray:
    return np.asarray(s.frac_coords, np.float64) @ np.asarray(s.lattice.matrix, np.float64)


class DimerSearch:
    """One saddle search: a structure inside a basin and a first guess of the direction out of it."""

    def __init__(self, structure, mode, model=None, *, dimer_separation: float = 0.01, max_rotations: int = 4, angle_tol: float = 0.05,
                 fixed_atoms=None, use_device: str | None = None, on_isolated_atoms: str = "warn") -> None:
        self.structure = atoms_to_structure(structure)
        n = len(self.structure)
        mode = np.array(mode, np.float64)
        if mode.shape != (n, 3) or not np.all(np.isfinite(mode)):
            raise ValueError(f"the mode must be a finite array of shape ({n}, 3), got shape {mode.shape}")
        self.dimer_separation, self.max_rotations, self.angle_tol = float(dimer_separation), int(max_rotations), float(angle_tol)
        if not 0.0 < self.dimer_separation <= 0.5:
            raise ValueError(f"{dimer_separation=} must lie in (0, 0.5] A")
        if not 0 <= self.max_rotations <= _lib.DIMER_MAX_ROTATIONS or self.max_rotations != max_rotations:
            raise ValueError(f"{max_rotations=} must be an integer from 0 to {_lib.DIMER_MAX_ROTATIONS}")
        if not 1e-4 <= self.angle_tol < np.pi / 4:
            raise ValueError(f"{angle_tol=} must lie in [1e-4, pi/4) rad")
        self.fixed = structure_fixed(self.structure, fixed_atoms)
        check_fixed(self.fixed, moving_cell=False, needs_dof=False, what="the search")
        if self.fixed is not None:
            mode[self.fixed.astype(bool)] = 0.0
        norm = np.sqrt((mode * mode).sum())
        if not norm > 0.0:
            raise ValueError("the mode has no free component" if self.fixed is not None else "the mode is zero")
        self.mode = mode / norm
        if isinstance(model, CHGNetCalculator):
            self.calculator = model
        else:
            self.calculator = CHGNetCalculator(model=model, use_device=use_device, on_isolated_atoms=on_isolated_atoms)

    # ------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def displace(structure, atoms, radius: float = 3.0, stdev: float = 0.1, seed: int = 0):
        """-> (displaced structure, mode [n, 3]).  The atoms within ``radius`` (A, minimum image) of any of ``atoms`` (indices; they
        are included) get a Gaussian displacement of standard deviation ``stdev`` (A) per component from ``seed``; the mode is that
        displacement, normalised: the search starts off the minimum and looks where it was pushed."""
        s = atoms_to_structure(structure)
        n = len(s)
        centres = np.atleast_1d(np.asarray(atoms, np.int64))
        if centres.size == 0 or centres.min() < 0 or centres.max() >= n:
            raise ValueError(f"atoms must name at least one of the {n} atoms")
        if not float(stdev) > 0.0 or not float(radius) >= 0.0:
            raise ValueError(f"{stdev=} must be positive and {radius=} non-negative")
        frac, lat = np.asarray(s.frac_coords, np.float64), np.asarray(s.lattice.matrix, np.float64)
        d = frac[:, None, :] - frac[None, centres, :]
        d -= np.round(d)
        near = (np.sqrt(((d @ lat) ** 2).sum(-1)) <= float(radius)).any(axis=1)
        near[centres] = True
        disp = np.zeros((n, 3))
        disp[near] = np.random.default_rng(seed).normal(0.0, float(stdev), (int(near.sum()), 3))
        out = Structure(Lattice(lat), np.asarray(atomic_numbers_of(s), np.int32), frac + disp @ np.linalg.inv(lat))
        return out, disp / np.sqrt((disp * disp).sum())

    @classmethod
    def from_band(cls, band, index: int | None = None, **kwargs) -> DimerSearch:
        """Polish the saddle of a band: ``band`` is a ``NudgedElasticBand`` result (its climbing image is taken) or a list of images
        (``energies`` unknown: ``index`` is needed).  Without ``index`` and without a climbing image the interior image of highest
        energy is taken.  The mode is the normalised ``R[i+1] - R[i-1]`` of the unwrapped images."""
        if isinstance(band, dict):
            images = list(band["images"])
            if index is None:
                index = band.get("climbing_image")
            if index is None:
                index = 1 + int(np.argmax(np.asarray(band["energies"])[1:-1]))
        else:
            images = [atoms_to_structure(s) for s in band]
            if index is None:
                raise ValueError("a list of images carries no energies: give the index of the image to start from")
        index = int(index)
        if not 1 <= index <= len(images) - 2:
            raise ValueError(f"{index=} must name an interior image of the {len(images)}")
        mode = _cart(images[index + 1]) - _cart(images[index - 1])
        return cls(images[index], mode, **kwargs)

    # ------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _params(fmax, steps, fire_kwargs: dict) -> dict:
        unknown = set(fire_kwargs) - set(FIRE_DEFAULTS)
        if unknown:
            raise TypeError(f"FIRE got unexpected keyword argument(s) {sorted(unknown)}")
        fmax, steps = float(fmax), int(steps)
        if fmax < 0 or steps < 0:
            raise ValueError(f"fmax and steps must be non-negative, got {fmax=}, {steps=}")
        return {"fmax": fmax, "steps": steps, **{k: fire_kwargs.get(k, v) for k, v in FIRE_DEFAULTS.items()}}

    @staticmethod
    def _run(searches: list, p: dict, log: bool, verbose: bool, keep_frames: bool) -> list[dict]:
        """Run ``searches`` (they share a calculator and the dimer parameters) as one ``chg_dimer`` handle; with ``log`` the handle is
        downloaded after every evaluation, and every translation decision is one line / one frame; one result dict per search."""
        first = searches[0]
        model = first.calculator.model
        eng, conv = model.engine, model.graph_converter
        prep = eng.prepare_structures([s.structure for s in searches])
        n_at = np.diff(prep.atom_off)
        S, N = prep.n_struct, int(prep.atom_off[-1])
        params = _lib.DimerParams(fmax=p["fmax"], max_steps=p["steps"], max_rotations=first.max_rotations, dt=p["dt"], maxstep=p["maxstep"],
                                  dtmax=p["dtmax"], finc=p["finc"], fdec=p["fdec"], astart=p["astart"], fa=p["fa"], nmin=int(p["Nmin"]),
                                  reserved=0, delta=first.dimer_separation, angle_tol=first.angle_tol, r_atom=conv.atom_graph_cutoff,
                                  r_bond=conv.bond_graph_cutoff, numerical_tol=1e-8)
        host = prep.host()
        modes = np.ascontiguousarray(np.concatenate([s.mode for s in searches]), np.float64)
        handle = ctypes.c_void_p()
        eng._check(eng.lib.chg_dimer_create(eng.handle, ctypes.byref(host), modes.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                            ctypes.byref(params), ctypes.byref(handle)))
        mask = join_fixed([s.fixed for s in searches], n_at)
        if mask is not None:
            rc = eng.lib.chg_dimer_set_fixed(eng.handle, handle, mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
            if rc != 0:
                eng.lib.chg_dimer_free(eng.handle, handle)
                eng._check(rc)
        scale = n_at.astype(np.float64) if model.is_intensive else np.ones(S)

        def download() -> dict:
            out = {"frac": np.empty((N, 3)), "mode": np.empty((N, 3)), "force": np.empty((N, 3)), "image_energy": np.empty((S, 2), np.float32),
                   "curvature": np.empty(S), "fmax": np.empty(S), "n_steps": np.empty(S, np.int32), "n_rotations": np.empty(S, np.int32),
                   "n_evaluated": np.empty(S, np.int32), "status": np.empty(S, np.int32), "phase": np.empty(S, np.int32)}
            eng._check(eng.lib.chg_dimer_download(eng.handle, handle, ctypes.byref(_lib.fill_out(_lib.DimerOutHost(), out))))
            return out

        def frame(d: dict, k: int) -> dict:
            sl = slice(prep.atom_off[k], prep.atom_off[k + 1])
            return {"energy": float(d["image_energy"][k, 0]) * scale[k], "positions": d["frac"][sl] @ prep.lattice[k], "forces": d["force"][sl].copy(),
                    "mode": d["mode"][sl].copy(), "curvature": float(d["curvature"][k]), "fmax": float(d["fmax"][k])}

        trajs = [[] for _ in searches] if log and keep_frames else None
        n_active = ctypes.c_int32(S)
        try:
            if log:
                # a translation decision was taken by search k when its step count went up (the centre it reports has moved on, so the
                # frame keeps the centre downloaded before) or when it stopped
                steps_seen, active = np.zeros(S, np.int32), np.ones(S, bool)
                before = download()
                while n_active.value > 0:
                    eng._check(eng.lib.chg_dimer_run(eng.handle, handle, 1, ctypes.byref(n_active)))
                    d = download()
                    for k in np.flatnonzero(active):
                        if d["n_steps"][k] == steps_seen[k] and d["status"][k] == 0:
                            continue
                        f = frame(d, k)
                        f["positions"] = frame(before, k)["positions"]
                        if trajs is not None:
                            trajs[k].append(f)
                        if verbose:
                            print(f"Dimer[{k}]: {steps_seen[k]:4d}  E = {f['energy']:.6f} eV  max|F| = {f['fmax']:.6f} eV/A  curvature = "
                                  f"{f['curvature']:.4f} eV/A^2  rotations = {d['n_rotations'][k]}  {STATUS_NAMES[d['status'][k]]}")
                    steps_seen, active, before = d["n_steps"].copy(), d["status"] == 0, d
            else:
                while n_active.value > 0:
                    eng._check(eng.lib.chg_dimer_run(eng.handle, handle, 1 << 30, ctypes.byref(n_active)))
            d = download()
        finally:
            eng.lib.chg_dimer_free(eng.handle, handle)

        results = []
        for k, s in enumerate(searches):
            f = frame(d, k)
            sl = slice(prep.atom_off[k], prep.atom_off[k + 1])
            final = Structure(Lattice(prep.lattice[k]), prep.z[sl].copy(), d["frac"][sl].copy())
            if s.fixed is not None:
                final.add_site_property("selective_dynamics", (s.fixed == 0).tolist())
            res = {"final_structure": final, "energy": f["energy"], "forces": f["forces"], "mode": f["mode"], "curvature": f["curvature"],
                   "fmax": f["fmax"], "n_steps": int(d["n_steps"][k]), "n_rotations": int(d["n_rotations"][k]),
                   "n_evaluated": int(d["n_evaluated"][k]), "status": STATUS_NAMES[d["status"][k]], "converged": bool(d["status"][k] == 1)}
            if trajs is not None:
                res["trajectory"] = trajs[k]
            results.append(res)
        return results

    # ------------------------------------------------------------------------------------------------------------------------
    def run(self, fmax: float = 0.05, steps: int = 500, trajectory: bool = False, verbose: bool = False, **fire_kwargs) -> dict:
        """Search until the curvature along the mode is negative and the largest force on an atom is below ``fmax`` (eV/A), for at
        most ``steps`` translations.  Leaves the centre and the mode where the search stopped in ``self.structure`` / ``self.mode``
        and returns ``final_structure``, ``energy`` (eV, of the centre), ``forces`` [n, 3] (eV/A, held components 0), ``mode`` [n, 3],
        ``curvature`` (eV/A^2, along the mode), ``fmax``, ``n_steps`` (translations), ``n_rotations``, ``n_evaluated`` (structures
        predicted), ``status``, ``converged`` (and ``trajectory``: one dict per translation decision with ``energy``, ``positions``,
        ``forces``, ``mode``, ``curvature``, ``fmax``)."""
        return DimerSearch.run_batch([self], fmax=fmax, steps=steps, trajectory=trajectory, verbose=verbose, **fire_kwargs)[0]

    @staticmethod
    def run_batch(searches, modes=None, *, fmax: float = 0.05, steps: int = 500, trajectory: bool = False, verbose: bool = False,
                  model=None, dimer_separation: float = 0.01, max_rotations: int = 4, angle_tol: float = 0.05, fixed_atoms=None,
                  **fire_kwargs) -> list[dict]:
        """``run`` for many searches at once, each independent (same result as ``run`` on it alone); one result per search, in order.
        ``searches``: ``DimerSearch`` objects, or structures with ``modes`` (then ``model`` and the dimer keywords build the searches;
        ``fixed_atoms`` applies to every one).  Searches are chunked by atoms like ``relax_batch`` (two images each); a chunk whose
        batch does not fit in device memory is split in two and run again.  Searches that differ in model or dimer parameters run in
        groups of their own."""
        from chgnet_amd.model import _plan_chunks, _run_splitting  # noqa: PLC0415

        searches = list(searches)
        if modes is not None:
            modes = list(modes)
            if len(modes) != len(searches):
                raise ValueError(f"{len(searches)} structures but {len(modes)} modes")
            calc = model if isinstance(model, CHGNetCalculator) else CHGNetCalculator(model=model)
            searches = [DimerSearch(s, m, calc, dimer_separation=dimer_separation, max_rotations=max_rotations, angle_tol=angle_tol,
                                    fixed_atoms=fixed_atoms) for s, m in zip(searches, modes)]
        p = DimerSearch._params(fmax, steps, fire_kwargs)
        results: list = [None] * len(searches)
        groups: dict = {}
        for i, s in enumerate(searches):
            groups.setdefault((id(s.calculator.model), s.dimer_separation, s.max_rotations, s.angle_tol), []).append(i)
        for members in groups.values():
            model_ = searches[members[0]].calculator.model

            def run(chunk):
                return DimerSearch._run([searches[i] for i in chunk], p, trajectory or verbose, verbose, trajectory)

            atoms = [2 * len(searches[i].structure) for i in members]
            for a, b in _plan_chunks(atoms, 1, model_.min_atoms_per_batch):
                chunk = members[a:b]
                report_isolated_atoms(model_, [searches[i].structure for i in chunk])
                for i, res in zip(chunk, _run_splitting(run, chunk)):
                    results[i] = res
                    searches[i].structure, searches[i].mode = res["final_structure"], res["mode"]
        return results
