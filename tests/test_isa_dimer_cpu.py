"""The dimer step kernel (csrc/kernels_dimer.h) on the device assembly of ``engine_dimer.hip`` (hipcc cross-compiles without a GPU):
both instantiations keep their state in registers -- no spilled register, no scratch."""
import os
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def dimer_isa(tmp_path_factory):
    from chgnet_amd import build

    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_dimer") / "engine_dimer.s"
    flags = [f for f in build.HIP_FLAGS if not f.startswith("-W")]
    cmd = [hipcc, *flags, "-w", f"-I{build.INCLUDE}", f"-I{build.CSRC}", "--cuda-device-only", "-S",
           os.path.join(build.CSRC, "engine_dimer.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    text = out.read_text()
    meta = {}
    for block in re.split(r"\n  - \.agpr_count:", text)[1:]:                # one metadata entry per kernel
        field = lambda key: re.search(rf"\.{key}:\s+(\S+)", block).group(1)  # noqa: E731
        meta[field("name")] = {key: int(field(key)) for key in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    return meta


def test_dimer_step_kernels_keep_their_state_in_registers(dimer_isa):
    hits = sorted(name for name in dimer_isa if "12k_dimer_step" in name)     # mangled: length, then name
    assert len(hits) == 2, f"k_dimer_step<false> and <true> not found among {sorted(dimer_isa)}"
    assert any("ILb0E" in name for name in hits) and any("ILb1E" in name for name in hits), hits
    for name in hits:
        m = dimer_isa[name]
        print(name, m)
        assert m["vgpr_spill_count"] == 0, f"{name}: {m}"
        assert m["private_segment_fixed_size"] == 0, f"{name}: {m}"
