"""Register budget of the ShuffleNetV2 kernels (csrc/shufflenet.hip): no VGPR / SGPR spills, no scratch and no AGPRs in any
kernel of the file.  Compiles it to gfx950 assembly with the build's own flags (no GPU needed) and reads the kernel
descriptors' metadata fields only.

VGPR counts when this test was written (f32 / bf16 x stride 1 / 2; the test prints the current ones): k_dw_fwd 140 .. 146 (16 KiB
LDS for the statistics rows), k_dw_bwd_data 108 .. 116, k_dw_wgrad 108 .. 114 (8 KiB LDS), k_dw_wgrad_reduce 6, k_tail_fwd 20 / 22,
k_tail_bwd 18, k_padded_pack 22."""
import importlib
import os
import re
import subprocess
import tempfile

import pytest

build = importlib.import_module("3dod_amd.build")

FIELDS = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")
KERNELS = ["k_dw_fwd", "k_dw_bwd_data", "k_dw_wgrad", "k_dw_wgrad_reduce", "k_tail_fwd", "k_tail_bwd", "k_padded_pack"]


def kernels_meta(asm):
    """[(mangled name, {field: value})] of every kernel in the .amdhsa metadata"""
    out = []
    for b in asm.split("  - .agpr_count:")[1:]:
        b = ".agpr_count:" + b
        m = re.search(r"\.name:\s+(\S+)", b)
        out.append((m.group(1), {k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(FIELDS), b)}))
    return out


@pytest.mark.timeout(300)
def test_shufflenet_kernels_have_no_spills_no_scratch_no_agprs():
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(build.CSRC, "shufflenet.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "shufflenet.s")
        cmd = [build.HIPCC] + [f for f in build.COMMON if f != "-fPIC"] + build.EXTRA.get("shufflenet.hip", []) + \
              ["-S", "--cuda-device-only", src, "-o", out]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    metas = kernels_meta(asm)
    # 4 instantiations (f32 / bf16 x stride 1 / 2) of the three depthwise kernels, 2 of either tail kernel, reduce and pack
    assert len(metas) == 3 * 4 + 2 * 2 + 2, [n for n, _ in metas]
    for fam in KERNELS:
        mine = [(n, m) for n, m in metas if fam in n and (fam != "k_dw_wgrad" or "reduce" not in n)]
        assert mine, fam
        print(fam, "VGPRs", sorted(m["vgpr_count"] for _, m in mine), "LDS", max(m["group_segment_fixed_size"] for _, m in mine))
    for name, m in metas:
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["agpr_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 16 * 1024, (name, m)
