"""The float64 restatement of the dimer saddle search (tests/dimer_ref.py) against closed forms, the host side of ``DimerSearch``
(``displace``, ``from_band``, the refusals) and ``vineyard_prefactor``.  No GPU.

Surface: the one of tests/test_neb_cpu.py with stiffer spectators.  Atom 0 moves on E = (x^2 - 1)^2 + 4 (y - 0.6 (1 - x^2))^2 + 3 z^2,
every spectator sits on a tether 3 |d|^2.  Minima at (+-1, 0) with E = 0, saddle at (0, 0.6) with E = 1 exactly and Hessian
eigenvalues -4 and 8 there; the z and spectator curvatures are 6, so along the valley the path mode is the softest one.  A search
converged to fmax at negative curvature has |F| < fmax on every atom, so in the quadratic region its energy is within
fmax^2 (1/8 + 1/32) ~ 1.6e-7 of 1 (the two in-plane modes of atom 0; the tethers add fmax^2 / 12 each at most); the bound below,
1e-5, is the NEB test's and leaves the same wide margin for anharmonicity.
"""

from __future__ import annotations

import numpy as np
import pytest

import dimer_ref
from dimer_ref import PROBE, TRIAL, Dimer, dimer_host, extrapolate, fit_rotation, modified_force
from relax_ref import CONVERGED, FIRE, MAX_STEPS, RUNNING

KAPPA, C, FMAX, MAX_TRANSLATIONS = 4.0, 0.6, 1e-3, 300
CELL = np.eye(3) * 20.0


def _home(a):
    return np.array([2.0 * a, 0.3 * a, 0.0])


def surface(R):
    """R [n, 3] -> (E, F [n, 3])."""
    x, y, z = R[0]
    w = y - C * (1.0 - x * x)
    E = (x * x - 1.0) ** 2 + KAPPA * w * w + 3.0 * z * z
    F = np.zeros_like(R)
    F[0] = (-(4.0 * x * (x * x - 1.0) + 2.0 * KAPPA * w * 2.0 * C * x), -2.0 * KAPPA * w, -6.0 * z)
    for a in range(1, len(R)):
        d = R[a] - _home(a)
        E += 3.0 * (d @ d)
        F[a] = -6.0 * d
    return E, F


def evaluate(X):
    EF = [surface(x) for x in X]
    return np.array([e for e, _ in EF]), np.array([f for _, f in EF])


def toy_search(n, seed, max_rotations=4, fixed=None, steps=MAX_TRANSLATIONS, x0=-0.5):
    """On the valley floor at x0, rattled by 0.02; the mode is e_x plus 0.3 of noise."""
    rng = np.random.default_rng(seed)
    R = np.array([[x0, C * (1.0 - x0 * x0), 0.0]] + [_home(a) for a in range(1, n)]) + 0.02 * rng.normal(size=(n, 3))
    mode = 0.3 * rng.normal(size=(n, 3))
    mode[0, 0] += 1.0
    return Dimer(R, mode, CELL, max_rotations=max_rotations, fixed=fixed, fmax=FMAX, steps=steps)


def test_surface_closed_forms():
    for x in (-1.0, 1.0):
        e, f = surface(np.array([[x, 0.0, 0.0]]))
        assert e == 0.0 and np.all(f == 0.0)
    e, f = surface(np.array([[0.0, C, 0.0]]))
    assert e == 1.0 and np.all(f == 0.0)
    h = 1e-4
    s = np.array([[0.0, C, 0.0]])
    H = np.array([[-(surface(s + h * np.eye(3)[j])[1][0, i] - surface(s - h * np.eye(3)[j])[1][0, i]) / (2 * h) for j in range(3)] for i in range(3)])
    assert np.allclose(H, np.diag([-4.0, 2.0 * KAPPA, 6.0]), atol=1e-6)


@pytest.mark.parametrize("max_rotations", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_search_finds_the_saddle(n, max_rotations):
    worst = np.zeros(3)
    for seed in range(10):
        dm = toy_search(n, seed, max_rotations)
        N0 = dm.N.copy()
        structures = dimer_host(dm, evaluate, f32=True)
        E = surface(dm.R)[0]
        x, y = dm.R[0, :2]
        print(f"n={n} rot={max_rotations} seed={seed}: {dm.steps} translations, {dm.rot_total} rotations, {structures} structures, "
              f"|E-1|={abs(E - 1):.2e} x={x:.2e} y-c={y - C:.2e} curvature={dm.curvature:.5f}")
        assert dm.status == CONVERGED and dm.steps <= MAX_TRANSLATIONS, (seed, dm.status, dm.steps)
        assert abs(E - 1.0) <= 1e-5 and abs(x) <= 1e-3 and abs(y - C) <= 1e-3, seed
        assert abs(dm.curvature + 4.0) <= 0.05 and dm.curvature == dm.C0, seed
        assert abs((dm.N * dm.N).sum() - 1.0) < 1e-12 and abs(dm.N[0, 0]) > 0.99 and not np.array_equal(dm.N, N0), seed
        assert structures >= 2 * dm.steps + dm.rot_total                      # two per translation decision, one per rotation
        worst = np.maximum(worst, [abs(E - 1.0), abs(x), abs(y - C)])
    print("worst", worst)


def _quadratic(n, seed):
    """A random symmetric H [3n, 3n] with eigenvalues in [-2, 6], one of them negative, and forces F(X) = -H (X - X0)."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.normal(size=(3 * n, 3 * n)))[0]
    lam = np.concatenate([[-2.0], rng.uniform(1.0, 6.0, 3 * n - 1)])
    H = (Q * lam) @ Q.T
    X0 = rng.normal(size=(n, 3))

    def ev(X):
        F = np.array([-(H @ (x - X0).ravel()).reshape(n, 3) for x in X])
        return np.zeros(len(X)), F

    return H, X0, Q, ev


@pytest.mark.parametrize("n", [1, 2, 4])
def test_rotation_alone_is_exact_on_a_quadratic_form(n):
    """No translation allowed (steps = 0): after one fit the extrapolated F1 is the force at R + delta N for the NEW N, and the new N
    is the softest direction in the plane of the rotation -- the fit is exact for a quadratic."""
    H, X0, _, ev = _quadratic(n, 5 + n)
    rng = np.random.default_rng(n)
    dm = Dimer(X0 + 0.3 * rng.normal(size=(n, 3)), rng.normal(size=(n, 3)), CELL, max_rotations=1, fmax=1e-9, steps=0)
    R0 = dm.R.copy()
    dm.advance(*ev(dm.staged()))
    assert dm.status == RUNNING and dm.phase == TRIAL and dm.phi1 >= dm.angle_tol and len(dm.staged()) == 1
    N, Th, C_before = dm.N.ravel().copy(), dm.Theta.ravel().copy(), dm.C0
    assert abs(N @ Th) < 1e-12 and abs(Th @ Th - 1.0) < 1e-12
    assert abs(C_before - N @ H @ N) < 1e-9 and abs(dm.gn - np.linalg.norm(H @ N - (N @ H @ N) * N)) < 1e-9
    dm.advance(*ev(dm.staged()))
    Nn = dm.N.ravel()
    assert np.abs(dm.F1 - (dm.F0 - dm.delta * (H @ Nn).reshape(n, 3))).max() <= 1e-12
    plane = np.array([[N @ H @ N, N @ H @ Th], [Th @ H @ N, Th @ H @ Th]])
    assert abs(dm.C0 - np.linalg.eigvalsh(plane)[0]) < 1e-9 and dm.C0 < C_before
    assert (dm.rot, dm.rot_total, dm.status, dm.steps) == (1, 1, MAX_STEPS, 0) and np.array_equal(dm.R, R0)


def test_both_signs_of_the_shift():
    """atan2(b1, a1) / 2 is the maximum of the fit; it is moved to the neighbouring minimum on the side of 0."""
    for mean, a1, b1, phi1, want in ((0.5, 1.0, -0.7, 0.3, np.pi / 2), (0.5, -1.0, -0.7, 0.2, np.pi / 2), (0.5, 1.0, 0.7, 0.3, -np.pi / 2),
                                     (-2.0, -0.4, 0.9, 0.6, -np.pi / 2), (0.0, 2.0, -1e-3, 0.1, np.pi / 2)):
        curve = lambda phi: mean + a1 * np.cos(2 * phi) + b1 * np.sin(2 * phi)  # noqa: E731
        phim, a1_fit, shift = fit_rotation(curve(0.0), curve(phi1), b1, phi1)
        assert shift == want and abs(a1_fit - a1) < 1e-12
        assert abs(curve(phim) - (mean - np.hypot(a1, b1))) < 1e-12 and abs(phim) <= np.pi / 2
    assert fit_rotation(1.0, 1.0, 0.0, 0.3)[2] == 0.0          # a flat fit has no maximum: no shift, no rotation
    rng = np.random.default_rng(0)
    F0, HN, HT = rng.normal(size=(3, 4, 3))
    for phi1, phim in ((0.3, 0.7), (0.2, -0.4), (0.05, 1.2)):    # the extrapolation is exact when the force is linear in the axis
        at = lambda phi: F0 - 0.01 * (HN * np.cos(phi) + HT * np.sin(phi))  # noqa: E731
        assert np.abs(extrapolate(F0, at(0.0), at(phi1), phi1, phim) - at(phim)).max() < 1e-14


def test_no_torque_means_no_rotation_and_no_nan():
    H = np.diag([-1.0, 2.0, 3.0])
    ev = lambda X: (np.zeros(len(X)), np.array([-(H @ x.ravel()).reshape(1, 3) for x in X]))  # noqa: E731
    dm = Dimer([[0.5, 0.1, 0.0]], [[1.0, 0.0, 0.0]], CELL, fmax=1e-6, steps=5)
    dm.advance(*ev(dm.staged()))
    assert dm.gn == 0.0 and dm.phi1 == 0.0 and dm.phase == PROBE and dm.rot_total == 0 and dm.steps == 1
    assert np.all(np.isfinite(dm.R)) and np.all(np.isfinite(dm.Theta)) and abs(dm.C0 + 1.0) < 1e-12
    dimer_host(dm, ev)
    assert dm.status == MAX_STEPS and dm.rot_total == 0 and np.all(np.isfinite(dm.R)) and np.array_equal(dm.N, [[1.0, 0.0, 0.0]])


def test_max_rotations_zero_follows_the_mode_as_given():
    dm = toy_search(3, 0, max_rotations=0)
    N0 = dm.N.copy()
    structures = dimer_host(dm, evaluate, f32=True)
    assert dm.rot_total == 0 and np.array_equal(dm.N, N0) and dm.status in (CONVERGED, MAX_STEPS)
    assert structures == 2 * (dm.steps + 1)                   # every evaluation was a PROBE


def test_translation_in_a_convex_region_climbs_along_the_mode_only():
    dm = toy_search(3, 1, max_rotations=0, x0=-0.95)         # near the minimum: every curvature is positive
    R0, N = dm.R.copy(), dm.N.copy()
    E, F = evaluate(dm.staged())
    dm.advance(E, F)
    assert dm.C0 > 0 and dm.steps == 1 and dm.phase == PROBE
    G = -(F[0] * N).sum() * N
    assert np.array_equal(modified_force(F[0], N, dm.C0), G)
    assert np.allclose(dm.R - R0, FIRE["dt"] ** 2 * G, rtol=0, atol=1e-15)      # the first FIRE step from v = 0, far below maxstep
    assert E[0] < surface(dm.R)[0]                            # uphill
    G = modified_force(F[0], N, -1.0)
    assert np.allclose(G, F[0] - 2.0 * (F[0] * N).sum() * N) and abs((G * N).sum() + (F[0] * N).sum()) < 1e-15


def test_held_components_never_move_and_stay_zero_in_the_mode():
    n = 3
    fixed = np.zeros((n, 3), bool)
    fixed[1] = True               # a whole spectator
    fixed[0, 2] = True            # and z of the moving atom
    dm = toy_search(n, 2, fixed=fixed)
    R0 = dm.R.copy()
    assert np.all(dm.N[fixed] == 0.0) and abs((dm.N ** 2).sum() - 1.0) < 1e-15
    seen_trial = False
    while dm.status == RUNNING:
        seen_trial |= dm.phase == TRIAL
        assert np.array_equal(dm.staged()[:, fixed], np.broadcast_to(R0[fixed], (len(dm.staged()), fixed.sum())))
        dm.advance(*evaluate(dm.staged()))
        assert np.all(dm.N[fixed] == 0.0) and np.all(dm.Theta[fixed] == 0.0) and np.all(dm.v[fixed] == 0.0) and np.all(dm.F0[fixed] == 0.0)
    assert dm.status == CONVERGED and seen_trial and dm.steps > 10
    assert np.array_equal(dm.R[fixed], R0[fixed]) and np.abs(dm.R[~fixed] - R0[~fixed]).max() > 1e-2
    with pytest.raises(ValueError, match="no free component"):
        Dimer(R0, np.where(fixed, 1.0, 0.0), CELL, fixed=fixed)


def test_parameter_refusals():
    ok = dict(positions=np.zeros((1, 3)), mode=np.ones((1, 3)), lattice=CELL)
    Dimer(**ok, delta=0.5, max_rotations=0, angle_tol=1e-4)
    for bad in (dict(delta=0.0), dict(delta=0.51), dict(max_rotations=-1), dict(max_rotations=33), dict(angle_tol=9e-5), dict(angle_tol=np.pi / 4)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            Dimer(**ok, **bad)
    assert (dimer_ref.DELTA, dimer_ref.MAX_ROTATIONS, dimer_ref.ANGLE_TOL) == (0.01, 4, 0.05)


# ---- the host side of DimerSearch ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device():
    """A calculator that is never used: the constructor of ``DimerSearch`` takes it as it is."""
    from chgnet_amd.calculator import CHGNetCalculator

    return CHGNetCalculator.__new__(CHGNetCalculator)


def _cube(n_side=3, a=2.5):
    from chgnet_amd.graph.structure import Lattice, Structure

    g = np.stack(np.meshgrid(*[np.arange(n_side)] * 3, indexing="ij"), -1).reshape(-1, 3) / n_side
    return Structure(Lattice(np.eye(3) * a * n_side), [3] * len(g), g)


def test_displace_moves_the_neighbourhood_and_returns_its_direction():
    from chgnet_amd.dimer import DimerSearch

    s = _cube()
    out, mode = DimerSearch.displace(s, [0], radius=2.6, stdev=0.1, seed=4)
    disp = (out.frac_coords - s.frac_coords) @ s.lattice.matrix
    moved = np.flatnonzero(np.abs(disp).max(1) > 0)
    d = s.frac_coords - s.frac_coords[0]
    d -= np.round(d)
    want = np.flatnonzero(np.sqrt(((d @ s.lattice.matrix) ** 2).sum(1)) <= 2.6)
    assert np.array_equal(moved, want) and len(want) == 7          # the atom and its six neighbours, through the cell faces too
    assert abs((mode ** 2).sum() - 1.0) < 1e-15 and np.allclose(mode * np.sqrt((disp ** 2).sum()), disp, atol=1e-14)
    assert 0.03 < np.abs(disp[moved]).mean() < 0.2
    again, mode2 = DimerSearch.displace(s, [0], radius=2.6, stdev=0.1, seed=4)
    assert np.array_equal(again.frac_coords, out.frac_coords) and np.array_equal(mode, mode2)
    assert not np.array_equal(DimerSearch.displace(s, [0], radius=2.6, seed=5)[1], mode)
    only, _ = DimerSearch.displace(s, 13, radius=0.0)
    assert np.flatnonzero(np.abs(only.frac_coords - s.frac_coords).max(1) > 0).tolist() == [13]
    with pytest.raises(ValueError, match="atoms"):
        DimerSearch.displace(s, [27])
    with pytest.raises(ValueError, match="stdev"):
        DimerSearch.displace(s, [0], stdev=0.0)


def test_from_band_takes_the_climbing_image_and_the_chord(no_device):
    from chgnet_amd.dimer import DimerSearch
    from chgnet_amd.graph.structure import Lattice, Structure

    lat = Lattice(np.diag([4.0, 5.0, 6.0]))
    frac = [np.array([[0.9 + 0.05 * i, 0.5 + 0.01 * i * i, 0.5], [0.1, 0.1, 0.1]]) for i in range(5)]       # unwrapped: through the face
    images = [Structure(lat, [3, 8], f) for f in frac]
    chord = lambda i: (frac[i + 1] - frac[i - 1]) @ lat.matrix  # noqa: E731
    unit = lambda m: m / np.sqrt((m * m).sum())  # noqa: E731
    res = {"images": images, "energies": np.array([0.0, 0.3, 0.2, 0.5, 0.1]), "climbing_image": 2}
    dm = DimerSearch.from_band(res, model=no_device)
    assert dm.structure is images[2] and np.allclose(dm.mode, unit(chord(2)), atol=1e-15) and np.all(dm.mode[1] == 0.0)
    res["climbing_image"] = None
    assert DimerSearch.from_band(res, model=no_device).structure is images[3]            # the highest interior image
    dm = DimerSearch.from_band(images, index=1, model=no_device, dimer_separation=0.02, max_rotations=0, angle_tol=0.1, fixed_atoms=[1])
    assert dm.structure is images[1] and np.allclose(dm.mode, unit(chord(1)), atol=1e-15)
    assert (dm.dimer_separation, dm.max_rotations, dm.angle_tol) == (0.02, 0, 0.1) and dm.fixed.tolist() == [[0, 0, 0], [1, 1, 1]]
    with pytest.raises(ValueError, match="index"):
        DimerSearch.from_band(images, model=no_device)
    for index in (0, 4):
        with pytest.raises(ValueError, match="interior"):
            DimerSearch.from_band(images, index=index, model=no_device)


def test_constructor_refusals(no_device):
    from chgnet_amd.dimer import DimerSearch

    s = _cube(2)
    mode = np.zeros((8, 3))
    mode[0, 0] = 2.0
    dm = DimerSearch(s, mode, no_device)
    assert dm.mode[0, 0] == 1.0 and (dm.dimer_separation, dm.max_rotations, dm.angle_tol) == (0.01, 4, 0.05)
    for kwargs, word in ((dict(dimer_separation=0.0), "dimer_separation"), (dict(dimer_separation=0.6), "dimer_separation"),
                         (dict(max_rotations=-1), "max_rotations"), (dict(max_rotations=33), "max_rotations"),
                         (dict(angle_tol=1e-5), "angle_tol"), (dict(angle_tol=0.8), "angle_tol"), (dict(fixed_atoms=[0]), "no free component")):
        with pytest.raises(ValueError, match=word):
            DimerSearch(s, mode, no_device, **kwargs)
    with pytest.raises(ValueError, match="zero"):
        DimerSearch(s, np.zeros((8, 3)), no_device)
    with pytest.raises(ValueError, match="shape"):
        DimerSearch(s, np.ones((7, 3)), no_device)
    held = DimerSearch(s, np.ones((8, 3)), no_device, fixed_atoms=np.eye(8, 3, dtype=bool))
    assert held.mode[0, 0] == 0.0 and abs((held.mode ** 2).sum() - 1.0) < 1e-15


# ---- vineyard_prefactor -------------------------------------------------------------------------------------------------------
def _toy_hessian(n, lam):
    """Diagonal in the basis of the non-translations, 0 on the translations: [3n, 3n] with the eigenvalues lam [3n - 3] there."""
    from chgnet_amd.elastic import translation_complement

    q = translation_complement(n)
    return (q * np.asarray(lam, np.float64)) @ q.T


def test_vineyard_prefactor_on_toy_hessians():
    import chgnet_amd
    from chgnet_amd.dynamics import ATOMIC_MASSES
    from chgnet_amd.phonons import _THZ, gamma_frequencies, vineyard_prefactor

    assert chgnet_amd.vineyard_prefactor is vineyard_prefactor
    s = _cube(2)                                              # 8 Li: equal masses, so the toy eigenvalues are those of the dynamical matrix
    m = ATOMIC_MASSES[3]
    rng = np.random.default_rng(0)
    lam_min, lam_sad = rng.uniform(1.0, 9.0, 21), np.concatenate([[-1.5], rng.uniform(1.0, 9.0, 20)])
    h_min, h_sad = _toy_hessian(8, lam_min), _toy_hessian(8, lam_sad)
    want = np.sqrt(np.prod(lam_min) / np.prod(lam_sad[1:]) / m) * _THZ
    got = vineyard_prefactor(s, h_min, s, h_sad)
    assert got == pytest.approx(want, rel=1e-10)
    nu_min, nu_sad = gamma_frequencies(s, h_min), gamma_frequencies(s, h_sad)      # the same number from the frequencies themselves
    assert got == pytest.approx(np.prod(nu_min[3:]) / np.prod(nu_sad[4:]), rel=1e-8) and nu_sad[0] < 0
    # every mode stiffer by 4 at the minimum: 2^21 times the rate; a translation added to either Hessian changes nothing
    assert vineyard_prefactor(s, 4.0 * h_min, s, h_sad) == pytest.approx(2.0 ** 21 * want, rel=1e-10)
    t = np.tile(np.eye(3), (8, 1))
    assert vineyard_prefactor(s, h_min + 7.0 * t @ t.T, s, h_sad - 3.0 * t @ t.T) == pytest.approx(want, rel=1e-10)
    # refusals: a saddle of second order, a saddle that is a minimum, a flat mode at the saddle, a minimum that is none
    two = lam_sad.copy()
    two[5] = -0.2
    for bad in (two, lam_min, np.concatenate([[-1.5, 0.0], lam_sad[2:]])):
        with pytest.raises(ValueError, match="saddle"):
            vineyard_prefactor(s, h_min, s, _toy_hessian(8, bad))
    with pytest.raises(ValueError, match="minimum"):
        vineyard_prefactor(s, h_sad, s, h_sad)
    with pytest.raises(ValueError, match="shape"):
        vineyard_prefactor(s, h_min[:-3, :-3], s, h_sad)
    with pytest.raises(ValueError, match="differ"):
        vineyard_prefactor(s, h_min, _cube(3), h_sad)


def test_ctypes_structs_mirror_the_c_header(tmp_path):
    """``chg_dimer_params`` and ``chg_dimer_out_host`` as gcc lays them out from include/chgnet_hip.h == the ctypes mirrors, field by
    field; the entry points arrived without a bump of the interface version."""
    import ctypes
    import os
    import subprocess

    from chgnet_amd import _lib
    from conftest import REPO

    fields = {"chg_dimer_params": _lib.DimerParams, "chg_dimer_out_host": _lib.DimerOutHost}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "chgnet_hip.h"', "int main(void) {"]
    for cname, cls in fields.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", f"-I{os.path.join(REPO, 'include')}", str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in fields.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert _lib.ABI_VERSION == 5 and {"chg_dimer_create", "chg_dimer_run", "chg_test_dimer_step"} <= set(_lib.EXPORTED_SYMBOLS)
    assert (_lib.DIMER_SD, _lib.DIMER_SI, _lib.DIMER_MAX_ROTATIONS) == (dimer_ref.SD, dimer_ref.SI, 32)
