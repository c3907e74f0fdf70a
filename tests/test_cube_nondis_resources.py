"""Register budget of the non-disentangled 3D-head loss kernels (csrc/cube_head.hip: k_cube_nondis_fwd / _bwd and the two
small select kernels around them): no VGPR / SGPR spills and no scratch; and the disentangled kernels k_cube_loss<false> /
<true> next to them in the same file keep the registers and the scratch they had before the new kernels were added.  Compiles the
file to gfx950 assembly with the build's own flags (no GPU needed) and reads the kernel descriptors."""
import importlib
import os
import subprocess
import tempfile

import pytest

from test_frozen_bn_resources import kernel_meta

build = importlib.import_module("3dod_amd.build")

# vgpr_count / private_segment_fixed_size of k_cube_loss<> compiled from the commit before the non-disentangled kernels
CUBE_LOSS_BEFORE = {"k_cube_lossILb0EE": (240, 0), "k_cube_lossILb1EE": (450, 80)}


@pytest.fixture(scope="module")
def asm():
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(build.CSRC, "cube_head.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "cube_head.s")
        cmd = [build.HIPCC] + [f for f in build.COMMON if f != "-fPIC"] + build.EXTRA.get("cube_head.hip", []) + \
              ["-S", "--cuda-device-only", src, "-o", out]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        return open(out).read()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["k_cube_nondis_fwd", "k_cube_nondis_bwd", "k_cube_select_norm", "k_cube_select_bwd_zraw"])
def test_nondis_kernels_have_no_spills_and_no_scratch(asm, name):
    meta = kernel_meta(asm, name)
    assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta["private_segment_fixed_size"] == 0, meta


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", sorted(CUBE_LOSS_BEFORE))
def test_disentangled_kernels_keep_their_registers(asm, name):
    meta = kernel_meta(asm, name)
    assert (meta["vgpr_count"], meta["private_segment_fixed_size"]) == CUBE_LOSS_BEFORE[name], meta
