"""Register and LDS budget of the GroupNorm kernels (csrc/groupnorm.hip): no VGPR / SGPR spills, no scratch and no AGPRs in any
kernel of the file, at most 16 KiB of static LDS.  Compiles it to gfx950 assembly with the build's own flags (no GPU needed) and
reads the kernel descriptors' metadata fields only.

VGPR counts when this test was written (the test prints the current ones): k_gn_rows 36 .. 84 (no LDS: pixel lanes are folded
with cross-lane adds), k_gn_apply 26 .. 56, k_gn_small 48 .. 90 (12 KiB LDS: lane partials, then the sample's coefficient rows,
and the channel totals), k_gn_finalize_fwd 22 and k_gn_finalize_bwd 46 (4 KiB: the double tree), k_gn_param_grads 22 (8 KiB)."""
import importlib
import os
import re
import subprocess
import tempfile

import pytest

build = importlib.import_module("3dod_amd.build")

FIELDS = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")
# family -> instantiations (templates: f32 and bf16, each forward and backward)
KERNELS = {"k_gn_rows": 4, "k_gn_apply": 4, "k_gn_small": 4, "k_gn_finalize_fwd": 1, "k_gn_finalize_bwd": 1,
           "k_gn_param_grads": 1}


def kernels_meta(asm):
    """[(mangled name, {field: value})] of every kernel in the .amdhsa metadata"""
    out = []
    for b in asm.split("  - .agpr_count:")[1:]:
        b = ".agpr_count:" + b
        m = re.search(r"\.name:\s+(\S+)", b)
        out.append((m.group(1), {k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(FIELDS), b)}))
    return out


def _family(name):
    m = re.search(r"\d+(k_gn_[a-z_]+?)(?:I[ft]Lb[01]EE|E)", name)
    return m.group(1) if m else None


@pytest.mark.timeout(300)
def test_groupnorm_kernels_have_no_spills_no_scratch_no_agprs():
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(build.CSRC, "groupnorm.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "groupnorm.s")
        cmd = [build.HIPCC] + [f for f in build.COMMON if f != "-fPIC"] + build.EXTRA.get("groupnorm.hip", []) + \
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
