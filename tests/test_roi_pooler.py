"""CPU: MODEL.ROI_BOX_HEAD / ROI_CUBE_HEAD .POOLER_TYPE 'ROIAlign' / 'ROIPool' and POOLER_SAMPLING_RATIO > 0 through the host model
-- the model builds from a config with each of them (it used to die on a bare assert) and both poolers report the settings,
ROIAlignRotated / unknown types / negative ratios raise and name the built set, ROIPool is refused under CR_DETERMINISTIC=1, the
default pooler still passes no keyword (the CPU stand-in of the op has four parameters), the new entry points are declared and
bound -- and the register budget of the new and re-instantiated kernels of csrc/detection.hip (no spills, no scratch; compiled to
gfx950 assembly with the build's own flags, no GPU needed)."""
import importlib
import inspect
import os
import subprocess
import tempfile

import pytest
import torch

from test_frozen_bn_resources import kernel_meta

build = importlib.import_module("3dod_amd.build")
ops = importlib.import_module("3dod_amd.hipops")
syn = importlib.import_module("3dod_amd.synthetic")
ROOT = os.path.dirname(build.HERE)
B, C = "MODEL.ROI_BOX_HEAD.", "MODEL.ROI_CUBE_HEAD."
# name -> (overrides, (box type, box ratio), (cube type, cube ratio))
SETTINGS = {
    "ratio2": ([B + "POOLER_SAMPLING_RATIO", 2, C + "POOLER_SAMPLING_RATIO", 2], ("ROIAlignV2", 2), ("ROIAlignV2", 2)),
    "roialign": ([B + "POOLER_TYPE", "ROIAlign", C + "POOLER_TYPE", "ROIAlign"], ("ROIAlign", 0), ("ROIAlign", 0)),
    "roipool": ([B + "POOLER_TYPE", "ROIPool", C + "POOLER_TYPE", "ROIPool"], ("ROIPool", 0), ("ROIPool", 0)),
    "cube_ratio2": ([C + "POOLER_SAMPLING_RATIO", 2], ("ROIAlignV2", 0), ("ROIAlignV2", 2)),
}
BUILT = "ROIAlignV2.*ROIAlign.*ROIPool"


def build_model(config, extra):
    modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
    cfg = syn.make_cfg(os.path.join(ROOT, "configs", config), overrides=["MODEL.DEVICE", "cpu", "VIS_PERIOD", 0, "log", False] + list(extra))
    torch.manual_seed(0)
    return modeling.build_model(cfg)


@pytest.mark.parametrize("config", ["cubercnn_DLA34_FPN.yaml", "Omni_combined.yaml", "BoxNet.yaml"])
@pytest.mark.parametrize("name", list(SETTINGS))
def test_model_builds_with_the_pooler_settings(config, name):
    extra, box, cube = SETTINGS[name]
    rh = build_model(config, extra).roi_heads
    poolers = [(rh.box_pooler, box)] + ([(rh.cube_pooler, cube)] if hasattr(rh, "cube_pooler") else [])
    assert len(poolers) == (1 if config == "BoxNet.yaml" else 2)          # (BoxNet's head has no 3D pooler)
    for p, (ptype, ratio) in poolers:
        assert (p.pooler_type, p.sampling_ratio) == (ptype, ratio)
        want = {}
        if ptype != "ROIAlignV2":
            want["pooler_type"] = ptype
        if ratio:
            want["sampling_ratio"] = ratio
        assert p.options() == want


def test_default_pooler_passes_no_keyword():
    """the CPU stand-in of the op (oracle/cpu_backend.roi_align_pyramid) has four parameters and serves the default pooler"""
    rh = build_model("cubercnn_DLA34_FPN.yaml", []).roi_heads
    assert rh.box_pooler.options() == {} and rh.cube_pooler.options() == {}
    assert (rh.box_pooler.pooler_type, rh.box_pooler.sampling_ratio) == ("ROIAlignV2", 0)
    O = importlib.import_module("oracle.cpu_backend")
    assert len(inspect.signature(O.roi_align_pyramid).parameters) == 4
    sig = inspect.signature(ops.roi_align_pyramid).parameters
    assert sig["pooler_type"].default == "ROIAlignV2" and sig["sampling_ratio"].default == 0
    assert sig["pooler_type"].kind is inspect.Parameter.KEYWORD_ONLY and sig["sampling_ratio"].kind is inspect.Parameter.KEYWORD_ONLY


@pytest.mark.parametrize("head", [B, C])
def test_unbuilt_values_raise_and_name_the_built_set(head):
    for extra in ([head + "POOLER_TYPE", "ROIAlignRotated"], [head + "POOLER_TYPE", "RoIWarp"], [head + "POOLER_SAMPLING_RATIO", -1]):
        with pytest.raises(ValueError, match=BUILT):
            build_model("cubercnn_DLA34_FPN.yaml", extra)
    with pytest.raises(ValueError, match=BUILT):
        ops.pooler_type_code("ROIAlignRotated", 0)
    with pytest.raises(ValueError, match=BUILT):
        ops.pooler_type_code("ROIAlign", -2)
    assert ops.pooler_type_code("ROIAlignV2", 0) == (0, 0) and ops.pooler_type_code("ROIAlign", 3) == (1, 3)
    assert ops.pooler_type_code("ROIPool", 2) == (2, 0)                   # ROIPool has no sampling grid


def test_roipool_is_refused_in_the_deterministic_mode(monkeypatch):
    monkeypatch.setenv("CR_DETERMINISTIC", "1")
    for head in (B, C):
        with pytest.raises(ValueError, match="CR_DETERMINISTIC"):
            build_model("cubercnn_DLA34_FPN.yaml", [head + "POOLER_TYPE", "ROIPool"])
    build_model("cubercnn_DLA34_FPN.yaml", SETTINGS["roialign"][0])       # the RoIAlign types have the tile-owner backward
    monkeypatch.setenv("CR_DETERMINISTIC", "0")
    build_model("cubercnn_DLA34_FPN.yaml", SETTINGS["roipool"][0])


def test_new_entry_points_are_declared_and_bound():
    _lib = importlib.import_module("3dod_amd._lib")
    header = open(os.path.join(ROOT, "include", "cr3dod.h")).read()
    for name in ("cr_roi_pool_fwd", "cr_roi_pool_bwd", "cr_roi_pool_bwd_set"):
        assert name in _lib.SIGNATURES and ("int %s(cr_ctx* ctx" % name) in header
        decl = header.split("int %s(" % name)[1].split(");")[0]
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    # additions keep the ABI version
    assert "cr_abi_version(void) { return 5; }" in open(os.path.join(build.CSRC, "cr_ctx.hip")).read()


@pytest.fixture(scope="module")
def asm():
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(build.CSRC, "detection.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "detection.s")
        cmd = [build.HIPCC] + [f for f in build.COMMON if f != "-fPIC"] + build.EXTRA.get("detection.hip", []) + \
              ["-S", "--cuda-device-only", src, "-o", out]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        return open(out).read()


# mangled-name fragments: kernel, storage type (f float / t bf16 bits), and the geometry parameter Li0E (default) / Li1E (new) /
# Li2E (the default geometry behind the new entry points; its tile-owner backward is the default launch)
KERNELS = ["14k_roi_pool_fwdIf", "14k_roi_pool_fwdIt", "14k_roi_pool_bwdIf", "14k_roi_pool_bwdIt"] + \
          [k % (t, g) for g in (0, 1, 2) for t in "ft" for k in ("11k_roi_alignILb0E%sLi%dE", "15k_roi_align_bwdI%sLi%dE",
                                                              "19k_roi_align_bwd_sepILi7E%sLi8ELi%dE", "19k_roi_align_bwd_sepILi7E%sLi1ELi%dE",
                                                              "15k_roi_bwd_tilesILi7E%sLi%dE")
           if not (g == 2 and "tiles" in k)] + \
          ["10k_roi_bboxILi7ELi0E", "10k_roi_bboxILi7ELi1E"]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", KERNELS)
def test_roi_kernels_have_no_spills_and_no_scratch(asm, name):
    meta = kernel_meta(asm, name)
    assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta["private_segment_fixed_size"] == 0, meta
    assert meta["group_segment_fixed_size"] <= 160 * 1024, meta
