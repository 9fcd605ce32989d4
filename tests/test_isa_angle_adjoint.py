"""Static checks on the per-atom angle adjoints (csrc/kernels_angle_w.h k_angle_bwd_w) in the device assembly of ``engine_predict.hip``,
compiled like tests/test_isa_split_addr.py.  Address, move and load instructions only:

* no instantiation spills a scalar or a vector register (both kernels sat at the scalar-register ceiling and kept 20-32 scalars in
  vector lanes, each reload a ``v_readlane``), and none touches scratch;
* the 32-bit twins form fewer 64-bit addresses than before;
* the tile loop reads its rows as ONE 16-byte record (``global_load_dwordx4``) per row, no longer as single-dword index loads."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# per-atom instantiations <HIDDEN, TEAM = false, ZS>: mangled prefix -> what the kernel was before the records, measured at commit
# d7a9985 with the same flags and compiler, 32-bit twin: static v_lshl_add_u64 + v_mad_u64_u32, single-dword global loads in the whole
# kernel, global_load_dwordx4 inside the tile loop (the bars are "strictly fewer" / "strictly fewer" / "strictly more")
PARENT = {
    "k_angle_bwd_wILb1ELb0ELb1E": {"u64": 82, "dword": 19, "x4_loop": 24},       # BondConv adjoint reading the kept z rows
    "k_angle_bwd_wILb1ELb0ELb0E": {"u64": 82, "dword": 19, "x4_loop": 44},       # BondConv adjoint gathering its table rows
    "k_angle_bwd_wILb0ELb0ELb0E": {"u64": 59, "dword": 25, "x4_loop": 36},       # AngleUpdate adjoint
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    from chgnet_amd import build

    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_angle_adjoint") / "engine_predict.s"
    flags = [f for f in build.HIP_FLAGS if not f.startswith("-W")]
    cmd = [hipcc, *flags, "-w", f"-I{build.INCLUDE}", f"-I{build.CSRC}", "--cuda-device-only", "-S",
           os.path.join(build.CSRC, "engine_predict.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    text = out.read_text()
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(_ZN\w+):", text, re.M)]
    starts.append((len(text), "END"))
    bodies = {name: text[a:b] for (a, name), (b, _) in zip(starts, starts[1:])}
    meta = {}
    for block in re.split(r"\n  - \.agpr_count:", text)[1:]:                # one metadata entry per kernel
        field = lambda key: re.search(rf"\.{key}:\s+(\S+)", block).group(1)  # noqa: E731
        meta[field("name")] = {key: int(field(key)) for key in ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count")}
    return bodies, meta


def _count(body: str, pattern: str) -> int:
    rx = re.compile(r"^\s+(?:" + pattern + r")\b", re.M)
    return len(rx.findall(body))


def _twins(bodies: dict, key: str) -> tuple[str, str]:
    """(64-bit, 32-bit) instantiation of the kernel whose mangled name contains ``key``: the address mode is the last template argument."""
    last = {n: re.search(r"Lb([01])EEEv", n[n.index(key):]) for n in bodies if key in n}
    a64 = [n for n, m in last.items() if m and m.group(1) == "0"]
    a32 = [n for n, m in last.items() if m and m.group(1) == "1"]
    assert len(a64) == 1 and len(a32) == 1, (key, a64, a32)
    return a64[0], a32[0]


def _tile_loop(body: str) -> str:
    """The tile loop: the first loop of depth 2 (inside the loop over the wave's atoms), from its label to its last back edge."""
    lines = body.split("\n")
    i = next(k for k, l in enumerate(lines) if "Inner Loop Header: Depth=2" in l)
    while not re.match(r"^\.LBB\d+_\d+:", lines[i]):
        i -= 1
    label = lines[i].split(":")[0]
    back = [k for k, l in enumerate(lines) if k > i and re.search(r"s_c?branch\w*\s+" + re.escape(label) + r"\b", l)]
    assert back, f"no back edge to {label}"
    return "\n".join(lines[i:back[-1] + 1])


def test_no_instantiation_spills(isa):
    bodies, meta = isa
    names = [n for n in bodies if "k_angle_bwd_w" in n]
    assert len(names) == 9, names                     # 3 per-atom kernels x 2 address modes + 3 TEAM kernels
    for name in names:
        m = meta[name]
        print(f"{name}: {m}")
        assert m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 256
        assert "scratch_" not in bodies[name], name


def test_32_bit_twins_form_fewer_64_bit_addresses_than_before(isa):
    bodies, _ = isa
    for key, parent in PARENT.items():
        n64, n32 = _twins(bodies, key)
        c64 = _count(bodies[n64], r"v_lshl_add_u64|v_mad_u64_u32")
        c32 = _count(bodies[n32], r"v_lshl_add_u64|v_mad_u64_u32")
        print(f"{key}: 64-bit address instructions: 64-bit twin {c64}, 32-bit twin {c32} (before: {parent['u64']})")
        assert c32 < parent["u64"], (key, c32, parent["u64"])
        assert c32 < c64, (key, c64, c32)
        # what is left sits in the prologue (staging from the fp32 weights when no prebuilt image is passed); in the tile loop only the
        # AngleUpdate adjoint's four predicated stores of the angle-gradient rows (mfma_tile.h scatter_rows64_add) still form one each
        loop = _count(_tile_loop(bodies[n32]), r"v_lshl_add_u64|v_mad_u64_u32")
        print(f"{key}: {loop} of them inside the 32-bit twin's tile loop")
        assert loop <= 4, f"{key}: {loop} 64-bit addresses formed inside the 32-bit twin's tile loop"


def test_tile_loop_reads_one_record_per_row(isa):
    bodies, _ = isa
    for key, parent in PARENT.items():
        for name in _twins(bodies, key):
            dword = _count(bodies[name], r"global_load_dword ")
            loop = _tile_loop(bodies[name])
            dword_loop, x4_loop = _count(loop, r"global_load_dword "), _count(loop, r"global_load_dwordx4")
            print(f"{name}: single-dword loads {dword} (before: {parent['dword']}), in the tile loop {dword_loop}; "
                  f"dwordx4 in the tile loop {x4_loop} (before: {parent['x4_loop']})")
            assert dword < parent["dword"], (name, dword)
            assert dword_loop == 0, (name, dword_loop)
            assert x4_loop > parent["x4_loop"], (name, x4_loop)
