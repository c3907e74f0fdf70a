"""Register budget of the BatchNorm kernels (csrc/conv.hip, k_bn_*): none uses scratch or spills, and none needs more VGPRs than
the kernel it replaced or was derived from had before the ReLU mask came from the pre-activation -- the backward kernels run
six to eight waves per SIMD to hide their memory latency, and the mask's gamma / beta must not cost them a wave.  Compiles the
file to gfx950 assembly with the build's own flags (no GPU needed) and reads the kernel descriptors.

The MASKX = true instantiations of the backward kernels (the ReLU mask from the pre-activation) give a thread 4 channels
instead of 8, so gamma and beta of its channels fit next to mean / invstd: 44 - 49 VGPRs against the 62 - 75 of the kernels
that read the output.  With 8 channels per thread they needed 64 - 90."""
import importlib
import os
import re
import subprocess
import tempfile

import pytest

build = importlib.import_module("3dod_amd.build")
FIELDS = r"\.(vgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)"
# VGPRs of the kernels before this change, by kernel and storage type (f = float32, t = bf16); the MASKX = true instantiations
# (Lb1) are held to the same number as the MASKX = false ones (Lb0), which are the earlier kernels
BEFORE = {
    "k_bn_finalize": 19, "k_bn_bwd_finalize": 16,
    "k_bn_applyIf": 60, "k_bn_applyIt": 62, "k_bn_apply_fusedIf": 61, "k_bn_apply_fusedIt": 60,
    "k_bn_bwd_reduceIf": 70, "k_bn_bwd_reduceIt": 65, "k_bn_bwd_apply_fusedIf": 74, "k_bn_bwd_apply_fusedIt": 75,
    "k_bn_bwd_applyIf": 62, "k_bn_bwd_applyIt": 65,
    # the two-launch finalize: each step against the single kernel it splits
    "k_bn_stats_lanes": 19, "k_bn_finalize_lanes": 19,
}


def kernels_meta(asm):
    """mangled kernel name -> metadata fields"""
    out = {}
    for b in asm.split("  - .agpr_count:")[1:]:
        m = re.search(r"\.name:\s+(\S+)", b)
        if m:
            out[m.group(1)] = {k: int(v) for k, v in re.findall(FIELDS, ".agpr_count:" + b)}
    return out


def _key(mangled):
    m = re.match(r"_Z\d+(k_bn_[a-z_]+?)(I[ft])?(Lb[01])?E*(?:v|PK)", mangled)
    return (m.group(1) + (m.group(2) or ""), m.group(3)) if m else None


@pytest.mark.timeout(600)
def test_bn_kernels_keep_their_registers():
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(build.CSRC, "conv.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "conv.s")
        cmd = [build.HIPCC] + [f for f in build.COMMON if f != "-fPIC"] + build.EXTRA.get("conv.hip", []) + \
              ["-S", "--cuda-device-only", src, "-o", out]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        meta = kernels_meta(open(out).read())
    seen, over = {}, {}
    for name, m in meta.items():
        if "k_bn_" not in name:
            continue
        key = _key(name)
        assert key is not None and key[0] in BEFORE, name
        seen[key] = m
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["agpr_count"] == 0, (name, m)
        if m["vgpr_count"] > BEFORE[key[0]]:
            over[key] = (m["vgpr_count"], BEFORE[key[0]])
    # every kernel is there: the plain ones once, the three backward kernels in both storage types with and without MASKX
    want = {(k, None) for k in BEFORE if "bwd_reduce" not in k and "bwd_apply" not in k}
    want |= {(k, mx) for k in BEFORE if "bwd_reduce" in k or "bwd_apply" in k for mx in ("Lb0", "Lb1")}
    assert set(seen) == want, (sorted(seen, key=str), sorted(want, key=str))
    assert not over, f"(VGPRs, bound) of the kernels above their bound: {over}"
