"""Register budget of the MNASNet kernels (csrc/mnasnet.hip): no VGPR / SGPR spills, no scratch and no AGPRs in any kernel of the
file, at most 16 KiB of static LDS.  Compiles it to gfx950 assembly with the build's own flags (no GPU needed) and reads the kernel
descriptors' metadata fields only.

VGPR counts when this test was written (f32 / bf16 x stride 1 / 2; the test prints the current ones): k_dwk_fwd 3x3 (8 channels
per thread) 140 .. 146 and 5x5 (4 channels per thread) 154 .. 162, 16 / 8 KiB LDS for the statistics rows; k_dw5_bwd_data 132 ..
134; k_dw5_wgrad 134 .. 138 (4 KiB LDS); k_dw5_wgrad_reduce 6; k_bna_reduce 65 .. 82 (16 KiB LDS); k_bna_apply 72 .. 80; k_cs_reduce 24 (8 KiB LDS); k_cs_final 8."""
import importlib
import os
import re
import subprocess
import tempfile

import pytest

build = importlib.import_module("3dod_amd.build")

FIELDS = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")
KERNELS = ["k_dwk_fwd", "k_dw5_bwd_data", "k_dw5_wgrad", "k_dw5_wgrad_reduce", "k_bna_reduce", "k_bna_apply", "k_cs_reduce",
           "k_cs_final"]


def kernels_meta(asm):
    """[(mangled name, {field: value})] of every kernel in the .amdhsa metadata"""
    out = []
    for b in asm.split("  - .agpr_count:")[1:]:
        b = ".agpr_count:" + b
        m = re.search(r"\.name:\s+(\S+)", b)
        out.append((m.group(1), {k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(FIELDS), b)}))
    return out


@pytest.mark.timeout(300)
def test_mnasnet_kernels_have_no_spills_no_scratch_no_agprs():
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(build.CSRC, "mnasnet.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "mnasnet.s")
        cmd = [build.HIPCC] + [f for f in build.COMMON if f != "-fPIC"] + build.EXTRA.get("mnasnet.hip", []) + \
              ["-S", "--cuda-device-only", src, "-o", out]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    metas = kernels_meta(asm)
    # forward: f32 / bf16 x k 3 / 5 x stride 1 / 2; 5x5 backward-data and weight gradient: f32 / bf16 x stride 1 / 2; the
    # weight-gradient reduce; BatchNorm backward reduce and apply: f32 / bf16 x mask from out / from x; the column sum: f32 /
    # bf16 reduce and its final pass
    assert len(metas) == 8 + 2 * 4 + 1 + 2 * 4 + 3, [n for n, _ in metas]
    for fam in KERNELS:
        mine = [(n, m) for n, m in metas if fam in n and (fam != "k_dw5_wgrad" or "reduce" not in n)]
        assert mine, fam
        print(fam, "VGPRs", sorted(m["vgpr_count"] for _, m in mine), "LDS", max(m["group_segment_fixed_size"] for _, m in mine))
    for name, m in metas:
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["agpr_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 16 * 1024, (name, m)
