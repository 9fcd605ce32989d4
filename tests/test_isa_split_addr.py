"""Static checks on the device assembly of ``engine_predict.hip`` (compiled like tests/test_isa_invariants.py) for the two things the
tile kernels stopped issuing:

* the operand split (csrc/mfma_split.h split8) reads the f16 high half in a mixed-precision FMA instead of converting it back to f32:
  the kernels contain ``v_fma_mix*`` and fewer ``v_cvt_f32_f16*`` than before;
* the large-batch kernels exist in two address modes (csrc/mfma_tile.h grow, last template parameter): the 32-bit twin forms fewer
  64-bit row addresses (``v_mad_u64_u32`` + ``v_lshl_add_u64``) than its 64-bit twin.

Every instantiation stays without spills inside 256 registers, and both AtomConv forward twins keep the latch free of waits."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# static v_cvt_f32_f16* per kernel before the change, measured at commit 58cdd64 (same flags, same compiler); the bar is
# "strictly fewer than these"
PARENT_CVT_F32_F16 = {
    "k_atomconv_fwdILi8E": 48,
    "k_atomconv_bwdILb0E": 96,
    "k_angleILb1ELb0ELi8ELb0E": 48,          # BondConv forward (row order)
    "k_angleupd_fwd_a": 16,
    "k_angle_bwd_wILb1ELb0ELb0E": 124,       # BondConv adjoint, per atom
    "k_angle_bwd_wILb1ELb0ELb1E": 108,       # ... reading the kept z rows
    "k_angle_bwd_wILb0ELb0ELb0E": 64,        # AngleUpdate adjoint, per atom
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    from chgnet_amd import build

    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_split_addr") / "engine_predict.s"
    flags = [f for f in build.HIP_FLAGS if not f.startswith("-W")]
    cmd = [hipcc, *flags, "-w", f"-I{build.INCLUDE}", f"-I{build.CSRC}", "--cuda-device-only", "-S",
           os.path.join(build.CSRC, "engine_predict.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    text = out.read_text()
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(_ZN\w+):", text, re.M)]
    starts.append((len(text), "END"))
    bodies = {name: text[a:b] for (a, name), (b, _) in zip(starts, starts[1:])}
    meta = {m.group(1): (int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)}
    return bodies, meta


def _count(body: str, pattern: str) -> int:
    rx = re.compile(r"^\s+(?:" + pattern + r")\b", re.M)
    return len(rx.findall(body))


def _twins(bodies: dict, key: str) -> tuple[str, str]:
    """(64-bit, 32-bit) instantiation of the kernel whose mangled name starts with ``key``: the address mode is the last template argument."""
    last = {n: re.search(r"Lb([01])EEEv", n[n.index(key):]) for n in bodies if key in n}
    a64 = [n for n, m in last.items() if m and m.group(1) == "0"]
    a32 = [n for n, m in last.items() if m and m.group(1) == "1"]
    assert len(a64) == 1 and len(a32) == 1, (key, a64, a32)
    return a64[0], a32[0]


def test_both_address_modes_exist_and_do_not_spill(isa):
    bodies, meta = isa
    for key in PARENT_CVT_F32_F16:
        for name in _twins(bodies, key):
            vgprs, spills = meta[name]
            assert spills == 0, f"{name}: {spills} spilled registers ({vgprs} VGPRs)"
            assert vgprs <= 256
            assert "scratch_load" not in bodies[name] and "scratch_store" not in bodies[name], name


def test_32_bit_twins_form_fewer_64_bit_addresses(isa):
    bodies, _ = isa
    for key in PARENT_CVT_F32_F16:
        n64, n32 = _twins(bodies, key)
        c64 = _count(bodies[n64], r"v_mad_u64_u32|v_lshl_add_u64")
        c32 = _count(bodies[n32], r"v_mad_u64_u32|v_lshl_add_u64")
        print(f"{key}: 64-bit address instructions {c64} -> {c32}")
        assert c32 < c64, (key, c64, c32)


def test_split_uses_the_mixed_precision_fma(isa):
    bodies, _ = isa
    for key, parent in PARENT_CVT_F32_F16.items():
        for name in _twins(bodies, key):
            mix = _count(bodies[name], r"v_fma_mix\w*")
            cvt = _count(bodies[name], r"v_cvt_f32_f16\w*")
            print(f"{name}: v_fma_mix* {mix}, v_cvt_f32_f16* {cvt} (before: {parent})")
            assert mix > 0, name
            assert cvt < parent, (name, cvt, parent)


def test_both_atomconv_forward_twins_keep_the_latch_free_of_waits(isa):
    """tests/test_isa_invariants.py checks the first instantiation it finds; both must hold the rule: no wait on the vector-memory
    counter between the loop body's last atomic and the back edge."""
    bodies, _ = isa
    for name in _twins(bodies, "k_atomconv_fwdILi8E"):
        lines = bodies[name].split("\n")
        headers = [i for i, l in enumerate(lines) if "Loop Header: Depth=1" in l]
        assert headers, name
        before = lines[max(0, headers[-1] - 60):headers[-1]]
        last_atomic = max((i for i, l in enumerate(before) if "global_atomic_add" in l), default=None)
        assert last_atomic is not None, f"{name}: latch block without the closing atomics"
        waits = [l.strip() for l in before[last_atomic:] if re.search(r"s_waitcnt\s+vmcnt", l)]
        assert not waits, f"{name}: waits behind the closing atomics: {waits}"


def test_split_statement_carries_its_wait_states_for_the_matrix_pipe(isa):
    """The low planes written inside split8's asm statement are the B operand of the next v_mfma; a vector-ALU write needs two wait
    states before a matrix instruction reads it and the compiler sees no producer inside the string (it would leave one): every such
    statement ends with `s_nop 1`."""
    bodies, _ = isa
    blocks = 0
    for name, body in bodies.items():
        for m in re.finditer(r";;#ASMSTART\n(.*?);;#ASMEND", body, re.S):
            lines = [l.strip() for l in m.group(1).split("\n") if l.strip()]
            if not any(l.startswith("v_fma_mix") for l in lines):
                continue
            blocks += 1
            assert lines[-1] == "s_nop 1", f"{name}: split statement ends with `{lines[-1]}`"
    assert blocks > 0
