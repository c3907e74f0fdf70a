"""Register budget of the ablation proposal samplers (csrc/propose_samplers.hip): one workgroup per object keeps up to 4 x 6
values per thread in registers across a block-wide sort, and the depth-ray variants call sinf / atan2f -- none of the six
kernels may spill or use scratch.  Compiles the file to gfx950 assembly with the build's own flags (no GPU needed) and reads
the .amdhsa metadata of every kernel in it."""
import importlib
import os
import re
import subprocess
import tempfile

import pytest

build = importlib.import_module("3dod_amd.build")
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels_meta(asm):
    """{mangled kernel name: metadata fields} of every kernel of the .amdhsa metadata"""
    out = {}
    for b in asm.split("  - .agpr_count:")[1:]:
        m = re.search(r"\.name:\s+(\S+)", b)
        if m:
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(FIELDS), b)}
    return out


@pytest.mark.timeout(300)
def test_no_sampler_kernel_spills_or_uses_scratch():
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    assert build.EXTRA["propose_samplers.hip"] == ["-ffp-contract=off"]
    src = os.path.join(build.CSRC, "propose_samplers.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "propose_samplers.s")
        cmd = [build.HIPCC] + [f for f in build.COMMON if f != "-fPIC"] + build.EXTRA["propose_samplers.hip"] + \
              ["-S", "--cuda-device-only", src, "-o", out]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    meta = kernels_meta(asm)
    samplers = {k: v for k, v in meta.items() if "k_propose_sampler" in k}
    assert len(samplers) == 6 and len(meta) == 6, sorted(meta)          # one instantiation per mode, nothing else in the file
    for name, m in meta.items():
        assert set(m) == set(FIELDS), (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 8 * 1024, (name, m)      # a 4 KB sort buffer or two 1 KB histograms
