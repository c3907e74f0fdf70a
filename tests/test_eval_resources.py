"""Register budget of the evaluation kernels (csrc/eval.hip): the matching kernel keeps a (tier, IoU, index) key per lane
across a 64-lane shuffle reduction and loops over thresholds, detections and ground truths -- it may not spill or use scratch.
The IoU kernel's 3D pair body uses indexed local arrays (clipped polygons) and is exempt, as k_box3d_overlap is.  Compiles the
file to gfx950 assembly with the build's own flags (no GPU needed) and reads the .amdhsa metadata of its kernels."""
import importlib
import os
import subprocess
import tempfile

import pytest

from tests.test_propose_samplers_resources import FIELDS, kernels_meta

build = importlib.import_module("3dod_amd.build")


@pytest.mark.timeout(300)
def test_matching_kernel_does_not_spill_or_use_scratch():
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    assert build.EXTRA["eval.hip"] == ["-ffp-contract=off"]
    src = os.path.join(build.CSRC, "eval.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "eval.s")
        cmd = [build.HIPCC] + [f for f in build.COMMON if f != "-fPIC"] + build.EXTRA["eval.hip"] + \
              ["-S", "--cuda-device-only", src, "-o", out]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    meta = kernels_meta(asm)
    assert len(meta) == 2, sorted(meta)
    match = [v for k, v in meta.items() if "k_eval_match_groups" in k]
    iou = [v for k, v in meta.items() if "k_eval_iou_groups" in k]
    assert len(match) == 1 and len(iou) == 1, sorted(meta)
    m = match[0]
    assert set(m) == set(FIELDS), m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert m["group_segment_fixed_size"] == 0, m                       # IoU rows are read from global memory: no cap on D x G
    assert iou[0]["vgpr_spill_count"] == 0 and iou[0]["sgpr_spill_count"] == 0, iou[0]
