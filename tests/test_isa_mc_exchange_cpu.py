"""The replica-exchange kernel (csrc/kernels_mc_exchange.h) on the device assembly of ``engine_mc.hip`` (hipcc cross-compiles without a
GPU): it keeps its state in registers -- no spilled register, no scratch."""
import os
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def mc_isa(tmp_path_factory):
    from chgnet_amd import build

    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_mc_exchange") / "engine_mc.s"
    flags = [f for f in build.HIP_FLAGS if not f.startswith("-W")]
    cmd = [hipcc, *flags, "-w", f"-I{build.INCLUDE}", f"-I{build.CSRC}", "--cuda-device-only", "-S",
           os.path.join(build.CSRC, "engine_mc.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    text = out.read_text()
    meta = {}
    for block in re.split(r"\n  - \.agpr_count:", text)[1:]:                # one metadata entry per kernel
        field = lambda key: re.search(rf"\.{key}:\s+(\S+)", block).group(1)  # noqa: E731
        meta[field("name")] = {key: int(field(key)) for key in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                                                "group_segment_fixed_size")}
    return meta


def test_mc_exchange_kernel_keeps_its_state_in_registers(mc_isa):
    hits = [name for name in mc_isa if "13k_mc_exchange" in name]            # mangled: length, then name
    assert len(hits) == 1, f"k_mc_exchange not found among {sorted(mc_isa)}"
    m = mc_isa[hits[0]]
    print(hits[0], m)
    assert m["vgpr_spill_count"] == 0, m
    assert m["private_segment_fixed_size"] == 0, m
