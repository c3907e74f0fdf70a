"""Register and LDS budget of the ResNet shortcut-tail kernels (csrc/resnet.hip): no VGPR / SGPR spills, no scratch and no AGPRs in
any kernel of the file, at most 16 KiB of static LDS.  Compiles it to gfx950 assembly with the build's own flags (no GPU needed)
and reads the kernel descriptors' metadata fields only.

VGPR counts when this test was written (f32 / bf16; the test prints the current ones): k_bnp_apply_fused 88 (4.5 KiB LDS: the
statistics lanes of one slice), k_bnp_apply 88, k_bnp_finalize / k_bnp_finalize_lanes 19 (4 KiB LDS: the tree), k_bnp_stats_lanes
17, k_bnp_bwd_reduce 101 .. 106 (8 KiB LDS: one sum's rows at a time), k_bnp_bwd_finalize 30 (8 KiB LDS), k_bnp_bwd_apply 100 .. 111."""
import importlib
import os
import re
import subprocess
import tempfile

import pytest

build = importlib.import_module("3dod_amd.build")

FIELDS = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")
# family -> instantiations (templates: f32 and bf16)
KERNELS = {"k_bnp_apply_fused": 2, "k_bnp_apply": 2, "k_bnp_finalize": 1, "k_bnp_stats_lanes": 1, "k_bnp_finalize_lanes": 1,
           "k_bnp_bwd_reduce": 2, "k_bnp_bwd_finalize": 1, "k_bnp_bwd_apply": 2}


def kernels_meta(asm):
    """[(mangled name, {field: value})] of every kernel in the .amdhsa metadata"""
    out = []
    for b in asm.split("  - .agpr_count:")[1:]:
        b = ".agpr_count:" + b
        m = re.search(r"\.name:\s+(\S+)", b)
        out.append((m.group(1), {k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(FIELDS), b)}))
    return out


def _family(name):
    m = re.search(r"\d+(k_bnp_[a-z_]+?)(?:I[ft]E|E)", name)
    return m.group(1) if m else None


@pytest.mark.timeout(300)
def test_resnet_kernels_have_no_spills_no_scratch_no_agprs():
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(build.CSRC, "resnet.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "resnet.s")
        cmd = [build.HIPCC] + [f for f in build.COMMON if f != "-fPIC"] + build.EXTRA.get("resnet.hip", []) + \
              ["-S", "--cuda-device-only", src, "-o", out]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    metas = kernels_meta(asm)
    seen = {}
    for name, m in metas:
        fam = _family(name)
        assert fam in KERNELS, name
        seen.setdefault(fam, []).append(m)
    assert {f: len(v) for f, v in seen.items()} == KERNELS, [n for n, _ in metas]
    for fam, ms in seen.items():
        print(fam, "VGPRs", sorted(m["vgpr_count"] for m in ms), "LDS", max(m["group_segment_fixed_size"] for m in ms))
    for name, m in metas:
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["agpr_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 16 * 1024, (name, m)
