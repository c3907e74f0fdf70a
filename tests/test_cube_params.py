"""CPU: MODEL.ROI_CUBE_HEAD.POSE_TYPE 'quaternion' / 'euler', USE_CONFIDENCE 0 and DIMS_PRIORS_FUNC 'sigmoid' through the host
model -- the model builds from a config with each of them (it used to raise), the CubeHead has the reference's parameters
(tests/golden/cubehead_layers_*.npz from the reference's own CubeHead, generator tests/golden/make_golden_cubehead_params.py) and
outputs, forward_fused returns the layout of the configured pose width and no uncertainty offset without confidence, unknown
values raise and name the built set, the weak head takes its tensor composition for the new pose types, the restated pytorch3d
conversions are rotations and give the hand-computed matrices -- and the register budget of the three new kernels of
csrc/cube_head.hip (no spills, no scratch; compiled to gfx950 assembly with the build's own flags, no GPU needed)."""
import importlib
import math
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

from test_frozen_bn_resources import kernel_meta

build = importlib.import_module("3dod_amd.build")
ops = importlib.import_module("3dod_amd.hipops")
util = importlib.import_module("3dod_amd.cubercnn.util.math_util")
syn = importlib.import_module("3dod_amd.synthetic")
d2 = importlib.import_module("3dod_amd.d2lite")
H = "MODEL.ROI_CUBE_HEAD."
OPTIONS = {"quaternion": [H + "POSE_TYPE", "quaternion"], "euler": [H + "POSE_TYPE", "euler"], "noconf": [H + "USE_CONFIDENCE", 0.0],
           "sigmoid": [H + "DIMS_PRIORS_FUNC", "sigmoid"]}


def build_model(extra):
    modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
    cfg = syn.make_cfg(None, overrides=["MODEL.DEVICE", "cpu"] + list(extra))
    torch.manual_seed(0)
    return cfg, modeling.build_model(cfg)


@pytest.mark.parametrize("name", list(OPTIONS))
def test_model_builds_with_the_option(name):
    cfg, model = build_model(OPTIONS[name])
    rh, ch = model.roi_heads, model.roi_heads.cube_head
    K = rh.num_classes
    width = {"quaternion": 4, "euler": 3}.get(name, 6)
    assert ch.bbox_3D_pose.out_features == K * width
    assert hasattr(ch, "bbox_3D_uncertainty") == (name != "noconf")
    opt = rh.cube_options()
    want = {"quaternion": {"pose_type": "quaternion"}, "euler": {"pose_type": "euler"}, "noconf": {"use_conf": False}}.get(name)
    if name == "sigmoid":
        assert set(opt) == {"dims_func", "priors_std"} and opt["dims_func"] == "sigmoid"
        assert torch.equal(opt["priors_std"], rh.priors_dims_per_cat.detach()[0, :, 1, :])
    else:
        assert opt == want
    # nothing is passed for the default family: the stand-in of the ops (oracle/cpu_backend.py) has no such arguments
    assert build_model([])[1].roi_heads.cube_options() == {}


def test_unknown_option_values_raise_and_name_the_built_set():
    with pytest.raises(ValueError, match="6d.*euler.*quaternion"):
        build_model([H + "POSE_TYPE", "axis_angle"])
    with pytest.raises(ValueError, match="exp.*sigmoid"):
        build_model([H + "DIMS_PRIORS_FUNC", "tanh"])
    build_model([H + "DIMS_PRIORS_FUNC", "tanh", H + "DIMS_PRIORS_ENABLED", False])      # not read without priors (roi_heads.py:2392)
    with pytest.raises(ValueError, match="6d.*euler.*quaternion"):
        ops.pose_type_code("rodrigues")
    with pytest.raises(ValueError, match="exp.*sigmoid"):
        ops.dims_func_code("log", torch.ones(3, 3), torch.ones(3, 3))
    with pytest.raises(ValueError, match="priors_std"):
        ops.dims_func_code("sigmoid", torch.ones(3, 3), None)
    assert ops.dims_func_code("sigmoid", None, None) == 0 and ops.dims_func_code("sigmoid", torch.ones(3, 3), torch.ones(3, 3)) == 1
    with pytest.raises(ValueError, match="USE_CONFIDENCE"):          # one predicate for the predictor and the loss: > 0 or exactly 0
        build_model([H + "USE_CONFIDENCE", -1.0])
    # the pair the reference cannot run itself stays refused
    with pytest.raises(ValueError, match="DIMS_PRIORS_ENABLED"):
        build_model([H + "DISENTANGLED_LOSS", False, H + "USE_CONFIDENCE", 0.0])
    build_model([H + "DISENTANGLED_LOSS", False, H + "DIMS_PRIORS_ENABLED", False, H + "USE_CONFIDENCE", 0.0])


@pytest.fixture()
def oracle_backend():
    """the product's host modules run on the oracle backend for the duration of one test (as in test_dense_golden.py)"""
    O = importlib.import_module("oracle.cpu_backend")
    saved = {n: importlib.import_module(n).ops for n in O.PATCHED}
    O.install()
    yield O
    for n, o in saved.items():
        importlib.import_module(n).ops = o


LAYERS = {"quat": ("quaternion", True, 4), "euler": ("euler", True, 3), "noconf": ("6d", False, 6)}


@pytest.mark.parametrize("name", list(LAYERS))
def test_cube_head_matches_the_reference_layers(golden_dir, oracle_backend, name):
    """state-dict names and shapes of the reference's CubeHead, the seeded initialisation of its FC trunk (same creation order),
    its outputs on its input, and forward_fused's layout"""
    pose_type, use_conf, pw = LAYERS[name]
    ch_mod = importlib.import_module("3dod_amd.cubercnn.modeling.roi_heads.cube_head")
    G = {k: torch.tensor(v) for k, v in np.load(os.path.join(golden_dir, "cubehead_layers_%s.npz" % name)).items() if k != "notes"}
    c = lambda k: G["cube_" + k]
    K, fc_dim, num_fc, C, Hh, W = [int(v) for v in c("cfg")]
    cfg = syn.make_cfg()
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = K
    cfg.MODEL.ROI_CUBE_HEAD.FC_DIM = fc_dim
    cfg.MODEL.ROI_CUBE_HEAD.NUM_FC = num_fc
    cfg.MODEL.ROI_CUBE_HEAD.POSE_TYPE = pose_type
    cfg.MODEL.ROI_CUBE_HEAD.USE_CONFIDENCE = 1.0 if use_conf else 0.0
    torch.manual_seed(int(c("seed")))
    head = ch_mod.CubeHead(cfg, d2.ShapeSpec(channels=C, height=Hh, width=W))
    sd = {k[len("cube_sd."):]: v for k, v in G.items() if k.startswith("cube_sd.")}
    mine = head.state_dict()
    assert list(mine) == list(sd), "same parameter names, in the reference's creation order"
    assert {k: tuple(v.shape) for k, v in mine.items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert tuple(mine["bbox_3D_pose.weight"].shape) == (K * pw, fc_dim)
    assert ("bbox_3D_uncertainty.weight" in mine) == use_conf
    for k, v in mine.items():
        if ".fc" in k or k.endswith(".bias") and "bbox_3D_pose" not in k:      # (the generator moved the predictors' weights)
            assert torch.equal(v, sd[k]), k
    head.load_state_dict(sd)
    head = head.eval()
    x = c("x").permute(0, 2, 3, 1).contiguous().flatten(1)
    with torch.no_grad():
        d, z, dims, pose, unc = head(x)
        raw, layout = head.forward_fused(x)
    assert tuple(layout) == (0, 2 * K, 5 * K, (5 + pw) * K, (6 + pw) * K if use_conf else -1)
    assert raw.shape[1] >= (6 + pw + (1 if use_conf else 0)) * K
    assert torch.allclose(raw[:, 5 * K:(5 + pw) * K], head.bbox_3D_pose(head.feature_generator(c("x").flatten(1))), atol=1e-5)
    assert torch.allclose(raw[:, (5 + pw) * K:(6 + pw) * K].reshape(-1, K, 1), z, atol=1e-5)
    assert (unc is None) == (not use_conf)
    for nm, got in (("deltas", d), ("z", z), ("dims", dims), ("pose", pose)) + ((("uncert", unc),) if use_conf else ()):
        ref = c(nm)
        assert tuple(got.shape) == tuple(ref.shape), nm
        assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5), (nm, float((got - ref).abs().max()))


def test_weak_head_takes_the_tensor_composition_for_the_new_pose_types():
    dt = importlib.import_module("3dod_amd.cubercnn.modeling.dense_train")
    dev = types.SimpleNamespace(type="cuda")
    for pose_type, want in (("6d", True), ("quaternion", False), ("euler", False)):
        rh = types.SimpleNamespace(_median_fn=None, _plane_cls=None, _ransac_triples=None, _hull_fn=None, _focal_fn=None,
                                   loss_functions=["dims", "iou", "z"], use_confidence=1.0, dims_priors_enabled=True,
                                   dims_priors_func="exp", pose_type=pose_type)
        assert dt.weak_fusable(rh, 16, dev) is want, pose_type


def _is_rotation(R):
    eye = torch.eye(3, dtype=R.dtype).expand_as(R)
    return bool(torch.allclose(R @ R.transpose(-1, -2), eye, atol=1e-12)) and bool(torch.allclose(torch.linalg.det(R), torch.ones(R.shape[0], dtype=R.dtype), atol=1e-12))


def test_restated_conversions_are_rotations_and_match_hand_cases():
    g = torch.Generator().manual_seed(3)
    q = torch.randn(200, 4, generator=g, dtype=torch.float64)
    q[:20, 0] = 0.0                                       # a zero real part counts as positive
    e = torch.randn(200, 3, generator=g, dtype=torch.float64) * 3
    assert _is_rotation(util.quaternion_pose_to_matrix(q)) and _is_rotation(util.euler_angles_to_matrix(e, "XYZ"))
    # q and -q are the same rotation; the sign rule makes the normalised real part non-negative
    assert torch.allclose(util.quaternion_pose_to_matrix(q), util.quaternion_pose_to_matrix(-q), atol=1e-12)
    assert torch.equal(util.quaternion_pose_to_matrix(torch.tensor([[3.0, 0.0, 0.0, 0.0], [-0.5, 0.0, 0.0, 0.0]])),
                       torch.eye(3).expand(2, 3, 3))
    # quaternion of a rotation by 90 degrees about z: (cos 45, 0, 0, sin 45), scaled by 2
    Rz = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    s = math.sqrt(0.5)
    assert torch.allclose(util.quaternion_pose_to_matrix(torch.tensor([[2 * s, 0, 0, 2 * s]], dtype=torch.float64))[0], Rz, atol=1e-12)
    assert torch.allclose(util.quaternion_pose_to_matrix(torch.tensor([[0.0, 0, 0, 1.0]], dtype=torch.float64))[0],
                          torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=torch.float64)), atol=1e-12)
    h = math.pi / 2
    Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
    Ry = torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]], dtype=torch.float64)
    got = util.euler_angles_to_matrix(torch.tensor([[h, 0, 0], [0, h, 0], [0, 0, h], [0, 0, 0]], dtype=torch.float64), "XYZ")
    for R, want in zip(got, (Rx, Ry, Rz, torch.eye(3, dtype=torch.float64))):
        assert torch.allclose(R, want, atol=1e-12)
    # the order of the product: Rx(a) Ry(b) Rz(c)
    a = torch.tensor([[0.3, -0.7, 1.1]], dtype=torch.float64)
    one = lambda ax, t: util.euler_angles_to_matrix(torch.tensor([[t if ax == 0 else 0, t if ax == 1 else 0, t if ax == 2 else 0]],
                                                                 dtype=torch.float64), "XYZ")[0]
    assert torch.allclose(util.euler_angles_to_matrix(a, "XYZ")[0], one(0, 0.3) @ one(1, -0.7) @ one(2, 1.1), atol=1e-12)
    with pytest.raises(ValueError):
        util.euler_angles_to_matrix(a, "XXY")


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


# (the length prefix of the mangled name tells k_cube_select_param from k_cube_select_param_bwd)
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["19k_cube_select_param", "23k_cube_select_param_bwd", "25k_cube_decode_infer_param"])
def test_param_kernels_have_no_spills_and_no_scratch(asm, name):
    meta = kernel_meta(asm, name)
    assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta["private_segment_fixed_size"] == 0, meta


def test_new_entry_points_are_declared_and_bound():
    _lib = importlib.import_module("3dod_amd._lib")
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "cr3dod.h")).read()
    for name in ("cr_cube_select_param", "cr_cube_select_param_bwd", "cr_cube_decode_infer_param"):
        assert name in _lib.SIGNATURES and ("int %s(cr_ctx* ctx" % name) in header
        decl = header.split("int %s(" % name)[1].split(");")[0]
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
