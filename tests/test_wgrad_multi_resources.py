"""Register / LDS budget of the grouped weight-gradient kernel (csrc/conv.hip, k_conv_wgrad_f32_multi): no scratch, no spills,
and no more VGPRs or LDS than the largest k_conv_wgrad_f32<TM, KS> it contains, so that three blocks per CU still fit (the
launch plan counts on one resident round of 3 x 256 blocks).  Compiles the file to gfx950 assembly with the build's own flags
(no GPU needed) and reads the kernel descriptors."""
import importlib
import os
import re
import subprocess
import tempfile

import pytest

build = importlib.import_module("3dod_amd.build")
FIELDS = r"\.(vgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)"


def kernels_meta(asm):
    """mangled kernel name -> metadata fields"""
    out = {}
    for b in asm.split("  - .agpr_count:")[1:]:
        m = re.search(r"\.name:\s+(\S+)", b)
        if m:
            out[m.group(1)] = {k: int(v) for k, v in re.findall(FIELDS, ".agpr_count:" + b)}
    return out


@pytest.mark.timeout(600)
def test_wgrad_multi_fits_three_blocks_per_cu():
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(build.CSRC, "conv.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "conv.s")
        cmd = [build.HIPCC] + [f for f in build.COMMON if f != "-fPIC"] + build.EXTRA.get("conv.hip", []) + \
              ["-S", "--cuda-device-only", src, "-o", out]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        meta = kernels_meta(open(out).read())
    multi = [v for k, v in meta.items() if "k_conv_wgrad_f32_multi" in k]
    assert len(multi) == 1, sorted(meta)
    multi = multi[0]
    solo = [meta[k] for tm in (64, 128) for ks in (1, 3) for k in meta if ("k_conv_wgrad_f32ILi%dELi%dE" % (tm, ks)) in k]
    assert len(solo) == 4, sorted(meta)
    assert multi["vgpr_spill_count"] == 0 and multi["sgpr_spill_count"] == 0, multi
    assert multi["private_segment_fixed_size"] == 0, multi
    assert multi["vgpr_count"] <= max(s["vgpr_count"] for s in solo), (multi, solo)
    assert multi["agpr_count"] <= max(s["agpr_count"] for s in solo), (multi, solo)
    assert multi["group_segment_fixed_size"] <= max(s["group_segment_fixed_size"] for s in solo), (multi, solo)
    # three blocks (one wave per SIMD each) per CU: 512 registers per SIMD lane, 160 KB of LDS
    assert 3 * multi["vgpr_count"] <= 512, multi
    assert 3 * multi["group_segment_fixed_size"] <= 160 * 1024, multi
