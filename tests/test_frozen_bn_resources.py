"""Register budget of the frozen-BatchNorm backward kernel (csrc/bn_frozen.hip, k_bn_frozen_unfold): no VGPR / SGPR spills and
no scratch.  Compiles the file to gfx950 assembly with the build's own flags (no GPU needed) and reads the kernel descriptor."""
import importlib
import os
import re
import subprocess
import tempfile

import pytest

build = importlib.import_module("3dod_amd.build")


def kernel_meta(asm, name):
    """fields of the .amdhsa metadata entry of the kernel whose mangled name contains `name`"""
    for b in asm.split("  - .agpr_count:")[1:]:
        m = re.search(r"\.name:\s+(\S+)", b)
        if m and name in m.group(1):
            return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                                                     r"group_segment_fixed_size):\s+(\d+)", b)}
    raise AssertionError("kernel not found: " + name)


@pytest.mark.timeout(300)
def test_frozen_bn_unfold_has_no_spills_and_no_scratch():
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(build.CSRC, "bn_frozen.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "bn_frozen.s")
        cmd = [build.HIPCC] + [f for f in build.COMMON if f != "-fPIC"] + build.EXTRA.get("bn_frozen.hip", []) + \
              ["-S", "--cuda-device-only", src, "-o", out]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    meta = kernel_meta(asm, "k_bn_frozen_unfold")
    assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta["private_segment_fixed_size"] == 0, meta
    assert meta["group_segment_fixed_size"] <= 64 * 1024, meta
