"""The float64 restatement of the nudged elastic band (tests/neb_ref.py) against closed forms, and the host side of
``NudgedElasticBand.interpolate``.  No GPU.

Surface: atom 0 moves on E = (x^2 - 1)^2 + kappa (y - c (1 - x^2))^2 (+ a harmonic tether in z), spectator atoms sit on harmonic
tethers.  Minima at (+-1, 0) with E = 0, saddle at (0, c) with E = 1 exactly and Hessian eigenvalues -4 and 2 kappa there.  A band
converged to fmax with the climbing image on the saddle has |G| = |F| < fmax on that image, so its energy is within
fmax^2 (1/8 + 1/(4 kappa)) ~ 2e-7 of 1 in the quadratic region; the bound below, 1e-5, leaves a wide margin for anharmonicity.
"""

from __future__ import annotations

import numpy as np
import pytest

from neb_ref import Band, neb_forces, neb_host, tangent
from relax_ref import CONVERGED

KAPPA, C, SPRING, FMAX, MAX_STEPS = 4.0, 0.6, 0.1, 1e-3, 300


def _home(a):
    return np.array([2.0 * a, 0.3 * a, 0.0])


def surface(R):
    """R [n, 3] -> (E, F [n, 3])."""
    x, y, z = R[0]
    w = y - C * (1.0 - x * x)
    E = (x * x - 1.0) ** 2 + KAPPA * w * w + 1.5 * z * z
    F = np.zeros_like(R)
    F[0] = (-(4.0 * x * (x * x - 1.0) + 2.0 * KAPPA * w * 2.0 * C * x), -2.0 * KAPPA * w, -3.0 * z)
    for a in range(1, len(R)):
        d = R[a] - _home(a)
        E += d @ d
        F[a] = -2.0 * d
    return E, F


def evaluate(R):
    EF = [surface(r) for r in R]
    return np.array([e for e, _ in EF]), np.array([f for _, f in EF])


def toy_band(M, n, climb, fixed=None, seed=1):
    A = np.array([[-1.0, 0.0, 0.0]] + [_home(a) for a in range(1, n)])
    B = A.copy()
    B[0, 0] = 1.0
    R = np.array([A + (B - A) * i / (M - 1) for i in range(M)])
    R[1:-1] += 0.05 * np.random.default_rng(seed).normal(size=R[1:-1].shape)
    return Band(R, np.eye(3) * 20.0, k=SPRING, climb=climb, fixed=fixed, fmax=FMAX, steps=MAX_STEPS)


def test_surface_closed_forms():
    for x in (-1.0, 1.0):
        e, f = surface(np.array([[x, 0.0, 0.0]]))
        assert e == 0.0 and np.all(f == 0.0)
    e, f = surface(np.array([[0.0, C, 0.0]]))
    assert e == 1.0 and np.all(f == 0.0)
    h = 1e-4   # Hessian at the saddle by central differences of the force: diag(-4, 2 kappa) in (x, y)
    H = np.array([[-(surface(np.array([[0.0, C, 0.0]]) + h * np.eye(3)[j])[1][0, i] - surface(np.array([[0.0, C, 0.0]]) - h * np.eye(3)[j])[1][0, i])
                   / (2 * h) for j in range(2)] for i in range(2)])
    assert np.allclose(H, np.diag([-4.0, 2.0 * KAPPA]), atol=1e-6)


@pytest.mark.parametrize(("M", "n"), [(4, 2), (5, 3), (6, 3), (7, 2)])
def test_climbing_band_finds_the_saddle(M, n):
    band = toy_band(M, n, True)
    E, _ = neb_host(band, evaluate)
    barrier = E.max() - E[0]
    print(f"M={M} n={n}: steps {band.steps}, barrier {barrier:.10f}, neb_fmax {band.neb_fmax:.3e}")
    assert band.status == CONVERGED and band.steps <= MAX_STEPS
    assert abs(barrier - 1.0) <= 1e-5
    top = band.R[band.ci, 0]
    assert band.ci == int(np.argmax(E)) and abs(top[0]) < 1e-3 and abs(top[1] - C) < 1e-3
    assert np.array_equal(band.R[0], toy_band(M, n, True).R[0]) and np.array_equal(band.R[-1], toy_band(M, n, True).R[-1])


def test_band_without_climbing_misses_the_saddle():
    band = toy_band(6, 3, False)
    E, _ = neb_host(band, evaluate)
    barrier = E.max() - E[0]
    print(f"steps {band.steps}, barrier {barrier:.10f}")
    assert band.status == CONVERGED and band.steps <= MAX_STEPS and band.ci == -1
    assert barrier < 0.95     # an even number of images straddles the saddle


def test_every_tangent_branch():
    rng = np.random.default_rng(3)
    tp, tm = rng.normal(size=(4, 3)), rng.normal(size=(4, 3))
    unit = lambda t: t / np.sqrt((t * t).sum())  # noqa: E731
    assert np.array_equal(tangent(tp, tm, 3.0, 2.0, 1.0), unit(tp))                       # rising
    assert np.array_equal(tangent(tp, tm, 1.0, 2.0, 3.0), unit(tm))                       # falling
    assert np.allclose(tangent(tp, tm, 2.0, 3.0, 1.5), unit(tp * 1.5 + tm * 1.0))         # maximum, E[i+1] > E[i-1]
    assert np.allclose(tangent(tp, tm, 1.5, 3.0, 2.0), unit(tp * 1.0 + tm * 1.5))         # maximum, E[i+1] < E[i-1]
    assert np.allclose(tangent(tp, tm, 2.0, 1.0, 1.5), unit(tp * 1.0 + tm * 0.5))         # minimum, E[i+1] > E[i-1]
    assert np.allclose(tangent(tp, tm, 1.5, 1.0, 2.0), unit(tp * 0.5 + tm * 1.0))         # minimum, E[i+1] < E[i-1]
    # exact ties take the weighted branches
    assert np.allclose(tangent(tp, tm, 2.0, 2.0, 1.0), unit(tp))                          # E[i+1] == E[i] > E[i-1]: dmin = 0 on t-
    assert np.allclose(tangent(tp, tm, 2.0, 1.0, 1.0), unit(tp))                          # E[i+1] > E[i] == E[i-1]
    assert np.allclose(tangent(tp, tm, 1.0, 1.0, 2.0), unit(tm))                          # E[i+1] == E[i] < E[i-1]: E[i+1] < E[i-1]
    assert np.allclose(tangent(tp, tm, 1.0, 2.0, 2.0), unit(tm))                          # E[i] == E[i-1] > E[i+1]
    assert np.allclose(tangent(tp, tm, 2.0, 1.0, 2.0), unit(tp + tm))                     # E[i+1] == E[i-1]: equal weights
    assert np.array_equal(tangent(tp, tm, 1.0, 1.0, 1.0), np.zeros_like(tp))              # all equal: length 0 stays 0
    for args in ((3.0, 2.0, 1.0), (2.0, 3.0, 1.5), (2.0, 1.0, 2.0)):
        assert abs(np.sqrt((tangent(tp, tm, *args) ** 2).sum()) - 1.0) < 1e-15


def test_spring_term_pulls_towards_the_farther_neighbour():
    # three images on a line, no true force, the middle one nearer to image 0: the spring pushes it along +tau, towards image 2
    R = np.zeros((3, 2, 3))
    R[1, 0, 0], R[2, 0, 0] = 0.3, 1.0
    G, ci = neb_forces(R, np.array([0.0, 1.0, 2.0]), np.zeros_like(R), k=0.1, climb=False)
    assert ci == -1 and np.allclose(G[1, 0], [0.1 * (0.7 - 0.3), 0.0, 0.0], atol=1e-16) and np.all(G[1, 1] == 0.0) and np.all(G[[0, 2]] == 0.0)
    G, _ = neb_forces(R, np.array([2.0, 1.0, 0.0]), np.zeros_like(R), k=0.1, climb=False)      # falling: tau = t-, same direction
    assert np.allclose(G[1, 0], [0.04, 0.0, 0.0], atol=1e-16)
    # the true force keeps only its part perpendicular to tau; the climbing image has it inverted along tau and no spring
    F = np.zeros_like(R)
    F[1, 0] = (1.0, 2.0, 0.0)
    G, _ = neb_forces(R, np.array([0.0, 1.0, 2.0]), F, k=0.1, climb=False)
    assert np.allclose(G[1, 0], [0.04, 2.0, 0.0], atol=1e-15)
    G, ci = neb_forces(R, np.array([0.0, 1.0, 2.0]), F, k=0.1, climb=True)
    assert ci == 1 and np.allclose(G[1, 0], [-1.0, 2.0, 0.0], atol=1e-15)


def test_climbing_image_first_index_wins_ties():
    R = np.cumsum(np.ones((6, 1, 3)), axis=0)
    _, ci = neb_forces(R, np.array([0.0, 1.0, 3.0, 3.0, 1.0, 5.0], np.float32), np.zeros_like(R), climb=True)
    assert ci == 2


def test_held_component_never_moves():
    M, n = 5, 3
    fixed = np.zeros((M, n, 3), bool)
    fixed[:, 1] = True            # a whole spectator
    fixed[:, 0, 2] = True         # and z of the moving atom
    band = toy_band(M, n, True, fixed=fixed)
    R0 = band.R.copy()
    E, _ = neb_host(band, evaluate)
    assert band.status == CONVERGED and band.steps > 10
    assert np.array_equal(band.R[fixed], R0[fixed])
    assert np.all(band.G[fixed] == 0.0) and np.all(band.v[fixed[1:-1]] == 0.0)
    assert np.abs(band.R[1:-1][~fixed[1:-1]] - R0[1:-1][~fixed[1:-1]]).max() > 1e-3
    z, d = band.R[band.ci, 0, 2], band.R[band.ci, 1] - _home(1)   # what is held in the climbing image keeps its tether energy
    assert z == R0[band.ci, 0, 2] != 0.0 and abs(E.max() - E[0] - (1.0 + 1.5 * z * z + d @ d)) <= 1e-5


def test_interpolate_takes_the_minimum_image_across_a_cell_face():
    from chgnet_amd.graph.structure import Lattice, Structure
    from chgnet_amd.neb import NudgedElasticBand

    lat = Lattice(np.diag([4.0, 5.0, 6.0]))
    a = Structure(lat, [3, 8], [[0.95, 0.5, 0.5], [0.1, 0.1, 0.1]])
    b = Structure(lat, [3, 8], [[0.05, 0.5, 0.5], [0.1, 0.2, 0.1]])
    images = NudgedElasticBand.interpolate(a, b, 5)
    assert len(images) == 5 and images[0] is a
    x = np.array([s.frac_coords[0, 0] for s in images])
    assert np.allclose(x, [0.95, 0.975, 1.0, 1.025, 1.05], atol=1e-15)          # through the face, left unwrapped
    assert np.allclose([s.frac_coords[1, 1] for s in images], [0.1, 0.125, 0.15, 0.175, 0.2], atol=1e-15)
    assert all(np.array_equal(s.lattice.matrix, lat.matrix) and np.array_equal(s.atomic_numbers, a.atomic_numbers) for s in images)
    with pytest.raises(ValueError, match="species"):
        NudgedElasticBand.interpolate(a, Structure(lat, [8, 3], b.frac_coords), 5)
    with pytest.raises(ValueError, match="cell"):
        NudgedElasticBand.interpolate(a, Structure(Lattice(np.diag([4.0, 5.0, 6.5])), [3, 8], b.frac_coords), 5)
    with pytest.raises(ValueError, match="images"):
        NudgedElasticBand.interpolate(a, b, 2)


def test_ctypes_structs_mirror_the_c_header(tmp_path):
    """``chg_neb_params`` and ``chg_neb_out_host`` as gcc lays them out from include/chgnet_hip.h == the ctypes mirrors, field by
    field; the entry points arrived without a bump of the interface version."""
    import ctypes
    import os
    import subprocess

    from chgnet_amd import _lib
    from conftest import REPO

    fields = {"chg_neb_params": _lib.NebParams, "chg_neb_out_host": _lib.NebOutHost}
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
    assert _lib.ABI_VERSION == 5 and {"chg_neb_create", "chg_neb_run", "chg_test_neb_step"} <= set(_lib.EXPORTED_SYMBOLS)
    assert (_lib.NEB_SD, _lib.NEB_SI, _lib.NEB_MAX_IMAGES) == (24, 4, 66)
