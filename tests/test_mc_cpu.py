"""Canonical Monte Carlo without a GPU: the NumPy restatement (tests/mc_ref.py) samples the Boltzmann distribution with exactly the
rules of DESIGN.md "Monte Carlo", the stream and edge rules hold, and the binding mirrors the header."""

from __future__ import annotations

import ctypes
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from mc_ref import DISPLACE, SWAP, McRef, atom_lists, block
from md_ref import KB

SEEDS = (7, (1 << 32) + 12345, 99)
CELL = np.eye(3) * 20.0

# ---- detailed balance of swaps: five sites on a ring, species A A A B C --------------------------------------------------------------
RING_SPECIES = np.array([1, 1, 1, 2, 3])
J = {(1, 2): 0.05, (1, 3): -0.04, (2, 3): 0.08}


def ring_energy_of(occ) -> float:
    return sum(J.get(tuple(sorted((int(occ[s]), int(occ[(s + 1) % 5])))), 0.0) for s in range(5))


def ring_calc(species):
    """calc(positions, cell): atom a sits on site round(x_a); nearest-neighbour energies on the ring of five sites."""
    def calc(r, cell):  # noqa: ARG001
        occ = np.empty(5, int)
        occ[np.rint(r[:, 0]).astype(int)] = species
        return ring_energy_of(occ)
    return calc


@pytest.mark.parametrize("seed", SEEDS)
def test_swaps_sample_the_boltzmann_distribution(seed):
    temperature, trials = 600.0, 20000
    positions = np.stack([np.arange(5.0), np.zeros(5), np.zeros(5)], axis=1)
    ref = McRef(positions, CELL, RING_SPECIES, temperature_k=temperature, seed=seed, swap_probability=1.0, calc=ring_calc(RING_SPECIES))
    occupations = sorted(set(itertools.permutations(RING_SPECIES.tolist())))
    assert len(occupations) == 20
    visits = dict.fromkeys(occupations, 0)
    ref.run(0)
    for _ in range(trials):
        ref.propose()
        ref.decide(ref.calc(ref.trial_positions(), CELL))
        visits[tuple(ref.species_on_sites().tolist())] += 1
    weights = np.array([math.exp(-ring_energy_of(o) / (KB * temperature)) for o in occupations])
    weights /= weights.sum()
    freq = np.array([visits[o] for o in occupations]) / trials
    tv = 0.5 * np.abs(freq - weights).sum()
    acceptance = ref.counts[SWAP][1] / ref.counts[SWAP][0]
    print(f"seed {seed}: total variation {tv:.4f}, acceptance {acceptance:.3f}")
    assert tv < 0.03
    assert ref.counts[SWAP][0] == trials and ref.counts[DISPLACE][0] == 0
    assert 0.55 < acceptance < 0.75               # near 0.645: both branches of the decision are exercised
    assert ref.n_samples == trials


# ---- displacements: four atoms in independent isotropic wells ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_displacements_give_equipartition(seed):
    temperature, trials, drop, kspring = 600.0, 40000, 2000, 5.0

    def calc(r, cell):  # noqa: ARG001
        return 0.5 * kspring * float((r * r).sum())

    ref = McRef(np.zeros((4, 3)), CELL, [3, 3, 3, 3], temperature_k=temperature, seed=seed, swap_probability=0.0, max_displacement=0.12,
                calc=calc)
    ref.run(drop)
    s0, n0, c0 = ref.sum_e, ref.n_samples, list(ref.counts[DISPLACE])
    ref.run(trials - drop)
    mean = (ref.sum_e - s0) / (ref.n_samples - n0)
    expected = 1.5 * 4 * KB * temperature
    acceptance = (ref.counts[DISPLACE][1] - c0[1]) / (ref.counts[DISPLACE][0] - c0[0])
    print(f"seed {seed}: <E> / (6 kB T) - 1 = {mean / expected - 1:+.4f}, acceptance {acceptance:.3f}")
    assert abs(mean / expected - 1.0) < 0.05
    assert 0.5 < acceptance < 0.66                # about 0.58
    assert ref.counts[SWAP][0] == 0


# ---- stream, slot and edge rules ------------------------------------------------------------------------------------------------------
def _mixed(seed, **kw):
    rng = np.random.default_rng(5)
    positions = rng.uniform(0.0, 4.0, (7, 3))
    species = [3, 25, 3, 8, 25, 8, 8]
    target = rng.uniform(0.0, 4.0, (7, 3))

    def calc(r, cell):  # noqa: ARG001
        return 0.3 * float(((r - target) ** 2).sum())

    return McRef(positions, CELL, species, seed=seed, calc=calc, **{"temperature_k": 900.0, "swap_probability": 0.5, **kw})


def test_stream_is_a_function_of_seed_and_trial_number():
    a, b = _mixed(11), _mixed(11)
    fa = a.run(13) + a.run(21)
    fb = b.run(34)
    assert len(fa) == len(fb) == 35
    for x, y in zip(fa, fb):
        assert (x["trial"], x["kind"], x["i"], x["j"], x["accepted"]) == (y["trial"], y["kind"], y["i"], y["j"], y["accepted"])
        assert x["u_acc"] == y["u_acc"] and np.array_equal(x["positions"], y["positions"]) and np.array_equal(x["site"], y["site"])
    assert a.sum_e == b.sum_e and a.counts == b.counts
    assert block(11, 5, 1) == block(11, 5, 1) != block(12, 5, 1)
    assert all(0.0 < u < 1.0 for k in range(50) for u in block((1 << 64) - 1, k, 0))
    c = _mixed(12)
    assert [f["u_acc"] for f in c.run(34)] != [f["u_acc"] for f in fb]


def test_zero_temperature_is_greedy_and_zero_difference_is_accepted():
    ref = _mixed(3, temperature_k=0.0)
    energies = [f["e_cur"] for f in ref.run(200)]
    assert all(b <= a for a, b in zip(energies, energies[1:]))
    assert 0 < ref.counts[SWAP][1] + ref.counts[DISPLACE][1] < 200
    # a swap of two atoms in a constant energy landscape: dE == 0 exactly, accepted at any temperature, 0 K included
    for t in (0.0, 300.0):
        flat = McRef(np.arange(9.0).reshape(3, 3), CELL, [1, 2, 3], temperature_k=t, seed=1, calc=lambda r, cell: 1.25)  # noqa: ARG005
        flat.run(25)
        assert flat.counts[SWAP] == [25, 25]


def test_swap_probability_zero_and_one_never_draw_the_other_kind():
    only_swaps, only_moves = _mixed(4, swap_probability=1.0), _mixed(4, swap_probability=0.0)
    assert {f["kind"] for f in only_swaps.run(300)[1:]} == {SWAP}
    assert {f["kind"] for f in only_moves.run(300)[1:]} == {DISPLACE}
    assert only_swaps.counts[DISPLACE] == [0, 0] and only_moves.counts[SWAP] == [0, 0]
    for f in only_swaps.run(0) + only_swaps.run(50):
        assert only_swaps.species[f["i"]] != only_swaps.species[f["j"]]        # a swap always joins two species


def test_held_atoms_and_other_species_are_never_picked():
    fixed = np.array([1, 0, 0, 1, 0, 0, 0], bool)
    ref = _mixed(8, fixed=fixed, swap_species=(3, 25))
    movable, swappable, gstart, gsize = atom_lists(ref.species, (3, 25), fixed)
    assert movable == [1, 2, 4, 5, 6] and swappable == [2, 1, 4] and gstart == [0, 1, 1] and gsize == [1, 2, 2]
    frames = ref.run(400)
    start = frames[0]["positions"]
    picked = set()
    for f in frames[1:]:
        picked.add(f["i"])
        if f["kind"] == SWAP:
            picked.add(f["j"])
            assert {f["i"], f["j"]} <= {1, 2, 4}
    assert picked == {1, 2, 4, 5, 6}
    assert np.array_equal(frames[-1]["positions"][fixed], start[fixed])
    assert np.array_equal(frames[-1]["site"][fixed], np.flatnonzero(fixed))


def test_skip_group_pick_is_uniform_over_the_other_species():
    """A A A B C: the partner of an A is B or C with equal weight, the partner of B is one of the three A or C."""
    ref = McRef(np.zeros((5, 3)), CELL, RING_SPECIES, seed=21, calc=lambda r, cell: 0.0)  # noqa: ARG005
    pairs = {}
    for _ in range(6000):
        m = ref.propose()
        pairs[(m["i"], m["j"])] = pairs.get((m["i"], m["j"]), 0) + 1
    assert set(pairs) == {(i, j) for i in range(5) for j in range(5) if RING_SPECIES[i] != RING_SPECIES[j]}
    # P(i, j) = 1/5 * 1/(5 - n_g(i)): 1/10 from an A, 1/20 from B or C
    for (i, _), n in pairs.items():
        expected = 6000 * (0.1 if i < 3 else 0.05)
        assert abs(n - expected) < 5 * math.sqrt(expected)


# ---- binding and ABI ---------------------------------------------------------------------------------------------------------------------
MC_SYMBOLS = ("chg_mc_create", "chg_mc_set_temperatures", "chg_mc_run", "chg_mc_download", "chg_mc_free", "chg_test_mc_step")


def test_header_binding_and_library_carry_the_entry_points_without_a_bump():
    from chgnet_amd import _lib

    header = open(os.path.join(REPO, "include", "chgnet_hip.h")).read()
    assert int(re.search(r"#define\s+CHG_ABI_VERSION\s+(\d+)", header).group(1)) == 5 == _lib.ABI_VERSION
    lib = _lib.load()
    assert int(lib.chg_abi_version()) == 5
    for name in MC_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(rf"\bint\s+{name}\s*\(", header), name
    assert re.search(r"CHG_MC_RUNNING\s*=\s*0,\s*CHG_MC_NONFINITE\s*=\s*1", header)


def test_ctypes_structs_mirror_the_c_header(tmp_path):
    """``chg_mc_params`` and ``chg_mc_out_host`` as gcc lays them out == the ctypes mirrors, field by field."""
    from chgnet_amd import _lib

    fields = {"chg_mc_params": _lib.McParams, "chg_mc_out_host": _lib.McOutHost}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "chgnet_hip.h"', "int main(void) {"]
    for cname, cls in fields.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("counts %d scalars %d moves %d\\n", CHG_MC_COUNTS, CHG_MC_FRAME_SCALARS, CHG_MC_FRAME_MOVES);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", f"-I{os.path.join(REPO, 'include')}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = dict(line.split() for line in out[:-1])
    for cname, cls in fields.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert out[-1] == f"counts {_lib.MC_COUNTS} scalars {_lib.MC_FRAME_SCALARS} moves {_lib.MC_FRAME_MOVES}"


def _limn():
    from chgnet_amd.graph.structure import Lattice, Structure

    return Structure(Lattice(np.eye(3) * 4.0), ["Li", "Mn", "O", "O"], [[0, 0, 0], [0.5, 0.5, 0.5], [0.5, 0, 0], [0, 0.5, 0]])


@pytest.mark.parametrize(("kwargs", "error", "match"), [
    (dict(temperature=-1.0), ValueError, "temperature"),
    (dict(temperature=float("nan")), ValueError, "temperature"),
    (dict(temperature="hot"), TypeError, "temperature"),
    (dict(swap_probability=1.5), ValueError, "swap_probability"),
    (dict(swap_probability=-0.1), ValueError, "swap_probability"),
    (dict(max_displacement=-0.1), ValueError, "max_displacement"),
    (dict(max_displacement=float("inf")), ValueError, "max_displacement"),
    (dict(loginterval=0), ValueError, "loginterval"),
    (dict(loginterval=1.5), ValueError, "loginterval"),
    (dict(seed=1.5), ValueError, "seed"),
    (dict(seed="7"), TypeError, "seed"),
    (dict(swap_species="Li"), TypeError, "swap_species"),
    (dict(swap_species=("Li", "Xx")), ValueError, "unknown element"),
    (dict(swap_species=("Li", 2.5)), TypeError, "swap_species"),
    (dict(swap_species=("Li",)), ValueError, "at least two"),
    (dict(swap_species=("Co", "Ni")), ValueError, "none of the free atoms"),
    (dict(fixed_atoms=[4]), ValueError, "out of range"),
    (dict(fixed_atoms=np.zeros((4, 3), bool)), ValueError, "shape"),
    (dict(fixed_atoms=[0.5]), TypeError, "fixed_atoms"),
    (dict(fixed_atoms=[0, 1, 2, 3], swap_probability=0.5), ValueError, "every atom is held"),
])
def test_argument_validation_needs_no_device(kwargs, error, match):
    from chgnet_amd.montecarlo import MonteCarlo

    with pytest.raises(error, match=match):
        MonteCarlo(_limn(), model=object(), **kwargs)


def test_arguments_are_normalised_and_the_package_exports_the_class():
    import chgnet_amd
    from chgnet_amd.montecarlo import MCTrajectory, MonteCarlo

    assert chgnet_amd.MonteCarlo is MonteCarlo and chgnet_amd.MCTrajectory is MCTrajectory
    mc = MonteCarlo(_limn(), model=object(), swap_species=("Mn", 3), seed=(1 << 64) - 1, fixed_atoms=np.array([False, False, True, False]),
                    temperature=0, swap_probability=0.25)
    assert mc.swap_z.tolist() == [3, 25] and mc.seed == (1 << 64) - 1 and mc._held.tolist() == [0, 0, 1, 0]
    assert mc.temperature == 0.0 and mc.cfg == {"swap_probability": 0.25, "max_displacement": 0.1, "loginterval": 1}
    assert mc.species_on_sites().tolist() == [3, 25, 8, 8] and mc.atoms is mc._input
    with pytest.raises(ValueError, match="nothing has run yet"):
        mc.best
    with pytest.raises(ValueError, match="one entry per structure"):
        MonteCarlo.run_batch([_limn(), _limn()], 5, temperatures=[300.0], model=object())
    tr = MCTrajectory([3, 25, 8])
    tr.sites.append(np.array([1, 0, 2]))
    assert tr.species_on_sites[0].tolist() == [25, 3, 8]
