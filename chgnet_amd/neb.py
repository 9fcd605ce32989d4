"""``NudgedElasticBand`` -- batched transition-state search on the device.

The host route to a migration barrier is ASE's ``NEB`` driving ``CHGNetCalculator`` one image at a time.  Every image of every band
is an independent structure for the graph build and the force sweep, so here the whole search runs behind the C-ABI (``chg_neb_*``,
include/chgnet_hip.h): the images of all bands are one device batch, one step kernel (csrc/kernels_neb.h) forms the improved tangents
(Henkelman & Jonsson 2000), the spring forces and the climbing image and advances ONE FIRE optimizer per band, and bands that have
stopped drop out of the next graph build.  A batch gives every band the result it would get alone.  tests/neb_ref.py restates the
step in float64 NumPy; DESIGN.md "Nudged elastic band" gives the layout.

All images of a band share one cell and one species order; the cell is fixed and the end points never move.  The state holds unwrapped
cartesian positions: ``interpolate`` applies the minimum image once, the band then takes plain differences between neighbouring
images (images built by hand must be unwrapped the same way).  Not offered: variable cells, IDPP interpolation, spline fits,
energy-weighted springs, optimizers other than FIRE.

``fixed_atoms`` takes the forms ``StructOptimizer`` takes (atom indices, bool [n] or bool [n, 3], True = held; without the keyword
the ``selective_dynamics`` of the first image) and holds the same components in every image.
"""

from __future__ import annotations

import ctypes

import numpy as np

from chgnet_amd import _lib
from chgnet_amd.calculator import CHGNetCalculator, atoms_to_structure, check_fixed, join_fixed, report_isolated_atoms, structure_fixed
from chgnet_amd.graph.structure import Lattice, Structure, atomic_numbers_of
from chgnet_amd.relax import FIRE_DEFAULTS, STATUS_NAMES

MIN_IMAGES, MAX_IMAGES = 3, _lib.NEB_MAX_IMAGES


def _species(s) -> np.ndarray:
    return np.asarray(atomic_numbers_of(s), np.int32)


def _same_frame(a, b) -> str | None:
    """Why two structures cannot be images of one band (None: they can)."""
    if len(a) != len(b):
        return "differ in atom count"
    if not np.array_equal(_species(a), _species(b)):
        return "differ in species order"
    if not np.array_equal(np.asarray(a.lattice.matrix, np.float64), np.asarray(b.lattice.matrix, np.float64)):
        return "differ in cell"
    return None


class NudgedElasticBand:
    """One band of images between two minima, relaxed on the device towards the minimum-energy path."""

    def __init__(self, images, model=None, *, spring_constant: float = 0.1, climb: bool = False, fixed_atoms=None,
                 use_device: str | None = None, on_isolated_atoms: str = "warn") -> None:
        self.images = [atoms_to_structure(s) for s in images]
        if not MIN_IMAGES <= len(self.images) <= MAX_IMAGES:
            raise ValueError(f"a band takes {MIN_IMAGES} to {MAX_IMAGES} images, got {len(self.images)}")
        for i, s in enumerate(self.images[1:], 1):
            why = _same_frame(self.images[0], s)
            if why:
                raise ValueError(f"image {i} and image 0 {why}")
        if not float(spring_constant) >= 0.0:
            raise ValueError(f"{spring_constant=} must be non-negative")
        self.spring_constant, self.climb = float(spring_constant), bool(climb)
        self.fixed = structure_fixed(self.images[0], fixed_atoms)
        check_fixed(self.fixed, moving_cell=False, needs_dof=False, what="the band")
        if isinstance(model, CHGNetCalculator):
            self.calculator = model
        else:
            self.calculator = CHGNetCalculator(model=model, use_device=use_device, on_isolated_atoms=on_isolated_atoms)

    # ------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def interpolate(initial, final, n_images: int) -> list[Structure]:
        """``n_images`` structures (the end points included) linear in fractional coordinates along the minimum-image displacement
        from ``initial`` to ``final``; the coordinates are left unwrapped, so neighbouring images differ by plain differences."""
        a, b = atoms_to_structure(initial), atoms_to_structure(final)
        why = _same_frame(a, b)
        if why:
            raise ValueError(f"the end points {why}")
        if not MIN_IMAGES <= int(n_images) <= MAX_IMAGES:
            raise ValueError(f"a band takes {MIN_IMAGES} to {MAX_IMAGES} images, got {n_images}")
        fa = np.asarray(a.frac_coords, np.float64)
        d = np.asarray(b.frac_coords, np.float64) - fa
        d -= np.round(d)
        z, lat = _species(a), np.asarray(a.lattice.matrix, np.float64)
        out = [Structure(Lattice(lat), z.copy(), fa + d * (i / (n_images - 1))) for i in range(1, n_images - 1)]
        return [a, *out, Structure(Lattice(lat), z.copy(), fa + d)]

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
    def _run(bands: list, p: dict, climb: list, frame_every: int | None, verbose: bool, keep_frames: bool) -> list[dict]:
        """Run ``bands`` (they share a calculator and ``climb[0]``) as one ``chg_neb`` handle, downloading every ``frame_every``
        evaluations (None: at the end only) for the log and, with ``keep_frames``, the trajectory; one result dict per band."""
        model = bands[0].calculator.model
        eng, conv = model.engine, model.graph_converter
        structs = [s for b in bands for s in b.images]
        prep = eng.prepare_structures(structs)
        n_at = np.diff(prep.atom_off)
        band_off = np.concatenate([[0], np.cumsum([len(b.images) for b in bands])]).astype(np.int32)
        nb, B, N = len(bands), prep.n_struct, int(prep.atom_off[-1])
        params = _lib.NebParams(fmax=p["fmax"], max_steps=p["steps"], climb=int(climb[0]), dt=p["dt"], maxstep=p["maxstep"], dtmax=p["dtmax"],
                                finc=p["finc"], fdec=p["fdec"], astart=p["astart"], fa=p["fa"], nmin=int(p["Nmin"]), reserved=0,
                                spring=bands[0].spring_constant, r_atom=conv.atom_graph_cutoff, r_bond=conv.bond_graph_cutoff, numerical_tol=1e-8)
        host = prep.host()
        handle = ctypes.c_void_p()
        eng._check(eng.lib.chg_neb_create(eng.handle, ctypes.byref(host), band_off.ctypes.data_as(_lib.c_int_p), nb, ctypes.byref(params),
                                          ctypes.byref(handle)))
        mask = join_fixed([b.fixed for b in bands for _ in b.images], n_at)
        if mask is not None:
            rc = eng.lib.chg_neb_set_fixed(eng.handle, handle, mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
            if rc != 0:
                eng.lib.chg_neb_free(eng.handle, handle)
                eng._check(rc)
        scale = n_at.astype(np.float64) if model.is_intensive else np.ones(B)

        def download() -> dict:
            out = {"frac": np.empty((N, 3)), "energy": np.empty(B, np.float32), "force": np.empty((N, 3), np.float32),
                   "neb_fmax": np.empty(nb), "climbing_image": np.empty(nb, np.int32), "n_steps": np.empty(nb, np.int32),
                   "status": np.empty(nb, np.int32), "n_evaluated": np.empty(nb, np.int32)}
            eng._check(eng.lib.chg_neb_download(eng.handle, handle, ctypes.byref(_lib.fill_out(_lib.NebOutHost(), out))))
            return out

        def frame(d: dict, k: int) -> dict:
            i0, i1 = band_off[k], band_off[k + 1]
            sl = slice(prep.atom_off[i0], prep.atom_off[i1])
            M = i1 - i0
            lat = prep.lattice[i0]
            return {"energies": d["energy"][i0:i1].astype(np.float64) * scale[i0:i1], "positions": (d["frac"][sl] @ lat).reshape(M, -1, 3),
                    "frac": d["frac"][sl].reshape(M, -1, 3).copy(), "forces": d["force"][sl].astype(np.float64).reshape(M, -1, 3),
                    "neb_fmax": float(d["neb_fmax"][k])}

        trajs = [[] for _ in bands] if frame_every and keep_frames else None
        n_active = ctypes.c_int32(nb)
        try:
            active = np.ones(nb, bool)
            interval = frame_every or max(1, p["steps"] + 1)      # frame_every: loginterval when frames or the log are asked for
            first = True
            while n_active.value > 0:
                eng._check(eng.lib.chg_neb_run(eng.handle, handle, 1 if first else interval, ctypes.byref(n_active)))
                first = False
                if frame_every:
                    d = download()
                    idx = d["n_steps"] - (d["status"] == 0)      # the evaluation just taken is frame number n_steps (stopped) or n_steps - 1
                    for k in np.flatnonzero(active):
                        if trajs is not None and idx[k] % frame_every == 0:
                            trajs[k].append(frame(d, k))
                        if verbose and idx[k] % frame_every == 0:
                            e = d["energy"][band_off[k]:band_off[k + 1]].astype(np.float64) * scale[band_off[k]:band_off[k + 1]]
                            print(f"NEB[{k}]: {idx[k]:4d}  barrier = {e.max() - e[0]:.6f} eV  max|G| = {d['neb_fmax'][k]:.6f} eV/A  "
                                  f"{STATUS_NAMES[d['status'][k]]}")
                    active = d["status"] == 0
            d = download()
        finally:
            eng.lib.chg_neb_free(eng.handle, handle)

        results = []
        for k, band in enumerate(bands):
            f = frame(d, k)
            i0 = band_off[k]
            z, lat = prep.z[prep.atom_off[i0]:prep.atom_off[i0 + 1]], prep.lattice[i0]
            images = [Structure(Lattice(lat), z.copy(), fr) for fr in f["frac"]]
            if band.fixed is not None:
                for s in images:
                    s.add_site_property("selective_dynamics", (band.fixed == 0).tolist())
            e = f["energies"]
            hops = np.sqrt((np.diff(f["positions"], axis=0) ** 2).sum((1, 2)))
            res = {"images": images, "energies": e, "forces": f["forces"], "neb_fmax": f["neb_fmax"],
                   "climbing_image": int(d["climbing_image"][k]) if d["climbing_image"][k] >= 0 else None,
                   "barrier": float(e.max() - e[0]), "reverse_barrier": float(e.max() - e[-1]),
                   "reaction_coordinate": np.concatenate([[0.0], np.cumsum(hops)]), "n_steps": int(d["n_steps"][k]),
                   "status": STATUS_NAMES[d["status"][k]], "converged": bool(d["status"][k] == 1), "n_evaluated": int(d["n_evaluated"][k])}
            if trajs is not None:
                res["trajectory"] = trajs[k]
            results.append(res)
        return results

    # ------------------------------------------------------------------------------------------------------------------------
    def run(self, fmax: float = 0.05, steps: int = 500, climb: bool | None = None, verbose: bool = False, trajectory: bool = False,
            loginterval: int = 1, **fire_kwargs) -> dict:
        """Relax the band until the largest NEB force on an atom is below ``fmax`` (eV/A).  ``climb``: None keeps the band's own
        setting.  Every call builds a fresh optimizer from the current images and leaves the relaxed images in ``self.images``, so a
        two-stage search is ``run(...)`` followed by ``run(..., climb=True)``.  Returns ``images``, ``energies`` [M] (eV), ``forces``
        [M, n, 3] (the engine's, eV/A), ``neb_fmax``, ``climbing_image`` (None without climbing), ``barrier`` = max(E) - E[0],
        ``reverse_barrier``, ``reaction_coordinate`` [M] (cumulative, A), ``n_steps``, ``status``, ``converged`` (and ``trajectory``:
        one dict per logged evaluation with ``energies``, ``positions``, ``forces``, ``neb_fmax``)."""
        return NudgedElasticBand.run_batch([self], fmax=fmax, steps=steps, climb=climb, verbose=verbose, trajectory=trajectory,
                                           loginterval=loginterval, **fire_kwargs)[0]

    @staticmethod
    def run_batch(bands, fmax: float = 0.05, steps: int = 500, climb: bool | None = None, verbose: bool = False, trajectory: bool = False,
                  loginterval: int = 1, **fire_kwargs) -> list[dict]:
        """``run`` for many bands at once, each an independent search (same result as ``run`` on it alone); one result per band, in
        order.  Bands are chunked by atoms like ``relax_batch`` and a band is never split across chunks; a chunk whose batch does not
        fit in device memory is split in two and run again.  Bands that differ in model, spring constant or climbing run in groups
        of their own."""
        from chgnet_amd.model import _plan_chunks, _run_splitting  # noqa: PLC0415

        bands = list(bands)
        p = NudgedElasticBand._params(fmax, steps, fire_kwargs)
        loginterval = int(loginterval)
        if loginterval < 1:
            raise ValueError(f"{loginterval=} must be positive")
        results: list = [None] * len(bands)
        groups: dict = {}
        for i, b in enumerate(bands):
            c = b.climb if climb is None else bool(climb)
            groups.setdefault((id(b.calculator.model), b.spring_constant, c), []).append(i)
        for (_, _, c), members in groups.items():
            model = bands[members[0]].calculator.model

            def run(chunk, c=c):
                return NudgedElasticBand._run([bands[i] for i in chunk], p, [c], loginterval if trajectory or verbose else None, verbose,
                                              trajectory)

            atoms = [sum(len(s) for s in bands[i].images) for i in members]
            for a, b in _plan_chunks(atoms, 1, model.min_atoms_per_batch):
                chunk = members[a:b]
                report_isolated_atoms(model, [s for i in chunk for s in bands[i].images])
                for i, res in zip(chunk, _run_splitting(run, chunk)):
                    results[i] = res
                    bands[i].images = res["images"]
        return results
