"""GPU: the 3D head with MODEL.ROI_CUBE_HEAD.POSE_TYPE 'quaternion' / 'euler', USE_CONFIDENCE 0 and DIMS_PRIORS_FUNC 'sigmoid':
cr_cube_select_param / cr_cube_select_param_bwd / cr_cube_decode_infer_param (csrc/cube_head.hip) around the loss kernels of the
default family.

  * selection forward and backward against the same definition evaluated by torch on the CPU in float64, for every pose type x
    prior function x confidence on / off (see test_selection_matches_float64 for the tolerance and the measured figures), for
    four depth cases (clusters and direct with 3 bins, sigmoid, log: bin choice, decode, the norm rows and the raw-depth gradient of
    the non-disentangled loss), for the old 6D kernels on the same inputs, and where the sigmoid prior underflows to 0;
  * losses and gradients against the REFERENCE'S OWN ROIHeads3D._forward_cube (tests/golden/cubehead_train_<case>.npz, generator
    tests/golden/make_golden_cubehead_params.py) through ops.cube_head_loss + ops.cube_reduce at the tolerances the project holds
    for this head: disentangled cases losses 1e-5 max(1, |ref|) and gradients w.r.t. every head output within 2e-4 of that
    gradient's scale (its largest magnitude), as tests/test_cubehead_golden.py; nondis_noconf losses 2e-5 and gradients rtol 5e-4 /
    atol 5e-6, as tests/test_gpu_cube_nondis.py; empty slots exactly 0;
  * the eval goldens through ops.cube_decode_infer: corners, centres, dimensions, poses at 1e-4, merged scores at 1e-5 relative,
    including the reference's score rule without confidence (the last column of its cube_3D = projected centre y x ratio);
  * the default path launches what it launched: bit-equal to the old entry points called directly;
  * a model with each option trains two steps through solver.make_train_step with the graph cache on, and infers."""
import ctypes
import importlib
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dod_amd.hipops")
_lib = importlib.import_module("3dod_amd._lib")
util = importlib.import_module("3dod_amd.cubercnn.util.math_util")
DEV = torch.device("cuda:0")
POSE_W = {"6d": 6, "quaternion": 4, "euler": 3}


# ------------------------------------------------------------------------------------------------ selection against float64
def sel_case(pose_type, conf, z_type="direct", bins=1):
    """B = 3 images x kf = 23 slots (n = 69: two 64-lane blocks), K = 3 classes, S = 27 > kf; slot (1, 4) is invalid, slot (2, 7)
    has the class index K (background).  bins > 1: the depth block has bins * K columns [bin][class], with scale centres inside
    the range of the box diagonals and depth statistics per (class, bin).  All inputs float32, made on the CPU."""
    g = torch.Generator().manual_seed(7)
    B, kf, K, S, G = 3, 23, 3, 27, 5
    pw = POSE_W[pose_type]
    width = (5 + pw + bins + (1 if conf else 0)) * K
    ld = (width + 15) // 16 * 16
    n = B * kf
    raw = torch.randn(n, ld, generator=g)
    layout = (0, 2 * K, 5 * K, (5 + pw) * K, (5 + pw + bins) * K if conf else -1)
    if conf:
        raw[:, layout[4]:layout[4] + K] = raw[:, layout[4]:layout[4] + K] * 0.5 + 0.4          # some below the clip at 0.01
    cls = torch.randint(0, K, (B, S), generator=g)
    valid = torch.ones(B, S, dtype=torch.bool)
    valid[1, 4] = False
    cls[2, 7] = K
    gt_idx = torch.randint(0, G, (B, S), generator=g)
    if pose_type == "quaternion":                          # a zero real part (counts as positive) and a negative one
        o = layout[2]
        raw[0, o + 4 * int(cls[0, 0])] = 0.0
        raw[1, o + 4 * int(cls[0, 1])] = -0.8
    gt3d = torch.rand(B, G, 9, generator=g) * 3 + 0.5
    gtpose = util.rotation_6d_to_matrix(torch.randn(B * G, 6, generator=g)).reshape(B, G, 3, 3).contiguous()
    pri_mean = torch.rand(K, 3, generator=g) * 0.8 + 0.3
    pri_std = torch.rand(K, 3, generator=g) * 0.8 + 0.05   # mean - 3 std is negative for some: the clip of the lower bound at 0
    meta = torch.tensor([[500.0, 510.0, 250.0, 260.0, 1.1], [600.0, 590.0, 255.0, 245.0, 0.9], [450.0, 455.0, 256.0, 256.0, 1.0]])
    boxes = torch.rand(n, 4, generator=g) * 100
    boxes[:, 2:] += boxes[:, :2] + 20
    up = {k: torch.randn(n, d, generator=g) for k, d in (("dxy", 2), ("zr", 1), ("dr", 3), ("Ra", 9), ("u", 1), ("usel", 1))}
    g2 = torch.Generator().manual_seed(8)
    z_scales = torch.sort(torch.rand(K, bins, generator=g2) * 140 + 30, dim=1).values if bins > 1 else None
    z_stats = torch.stack((torch.rand(K, bins, generator=g2) * 8 + 2, torch.rand(K, bins, generator=g2) * 1.5 + 0.3), -1) if bins > 1 else None
    return dict(z_type=z_type, bins=bins, z_scales=z_scales, z_stats=z_stats, B=B, kf=kf, K=K, S=S, G=G, n=n, ld=ld, pw=pw, raw=raw, layout=layout, cls=cls, valid=valid, gt_idx=gt_idx,
                gt3d=gt3d, gtpose=gtpose, pri_mean=pri_mean, pri_std=pri_std, meta=meta, boxes=boxes, up=up)


def sel_definition(c, raw, pose_type, dims_func, conf, dtype):
    """what cr_cube_select_param writes into the five head chunks of buf39 (+ the prior chunk), as torch expressions in `dtype`"""
    K, n, kf, pw = c["K"], c["n"], c["kf"], c["pw"]
    cls0 = c["cls"][:, :kf].reshape(-1)
    v = c["valid"][:, :kf].reshape(-1) & (cls0 >= 0) & (cls0 < K)
    cl = cls0.clamp(0, K - 1)
    ar = torch.arange(n)
    o_d2, o_dims, o_pose, o_z, o_unc = c["layout"]
    seg = lambda o, d: raw[:, o:o + K * d].reshape(n, K, d)[ar, cl]
    dxy, dr, pose = seg(o_d2, 2), seg(o_dims, 3), seg(o_pose, pw)
    bins = c["bins"]
    zall = raw[:, o_z:o_z + K * bins]
    T = lambda t: None if t is None else t.to(dtype)
    zr = util.cluster_depth(zall.reshape(n, bins, K, 1) if bins > 1 else zall.reshape(n, K, 1), cl, c["boxes"].to(dtype), T(c["z_scales"]),
                            c["z_type"], T(c["z_stats"]))[:, None]
    mean, std = c["pri_mean"].to(dtype)[cl], c["pri_std"].to(dtype)[cl]
    if dims_func == "sigmoid":
        dims = util.scaled_sigmoid(dr, min=(mean - 3 * std).clip(0.0), max=mean + 3 * std)
        dr, prior = torch.log(dims), torch.ones_like(mean)
    else:
        dims, prior = torch.exp(dr.clip(max=5)) * mean, mean
    if pose_type == "quaternion":
        Ra = util.quaternion_pose_to_matrix(pose)
    elif pose_type == "euler":
        Ra = util.euler_angles_to_matrix(pose, "XYZ")
    else:
        Ra = util.rotation_6d_to_matrix(pose)
    u = seg(o_unc, 1).clip(0.01) if conf else torch.zeros(n, 1, dtype=dtype)
    return dict(dxy=dxy, zr=zr, dr=dr, Ra=Ra.reshape(n, 9), u=u, prior=prior, dims=dims), v, cl


def sel_reference(c, pose_type, dims_func, conf, dtype):
    """forward chunks and the gradient of sum(upstream * chunk) over the valid RoIs w.r.t. raw, in `dtype` on the CPU"""
    raw = c["raw"].to(dtype).requires_grad_(True)
    out, v, cl = sel_definition(c, raw, pose_type, dims_func, conf, dtype)
    up = {k: t.to(dtype) for k, t in c["up"].items()}
    tot = sum((up[k] * out[k] * v[:, None]).sum() for k in ("dxy", "zr", "dr", "Ra"))
    if conf:
        tot = tot + ((up["u"] + up["usel"]) * out["u"] * v[:, None]).sum()
    tot.backward()
    return {k: t.detach() for k, t in out.items()}, raw.grad, v, cl


def sel_kernels(c, pose_type, dims_func, conf, norm=False, g_zraw=None):
    T = lambda t: t.to(DEV).contiguous()
    n, B, kf, K = c["n"], c["B"], c["kf"], c["K"]
    raw = T(c["raw"])
    buf = torch.full((39 * n,), float("nan"), device=DEV)
    validf = torch.empty((n,), dtype=torch.uint8, device=DEV)
    clsc = torch.empty((n,), dtype=torch.int32, device=DEV)
    lay = (ctypes.c_int * 5)(*c["layout"])
    pm, ps = T(c["pri_mean"]), T(c["pri_std"])
    boxes = T(c["boxes"])
    pc, dc = ops.pose_type_code(pose_type), ops.dims_func_code(dims_func, pm, ps)
    norm3 = torch.full((3 * n,), float("nan"), device=DEV) if norm else None
    zc = ops.z_config(c["z_type"], c["bins"], None if c["z_scales"] is None else T(c["z_scales"]),
                      None if c["z_stats"] is None else T(c["z_stats"]))
    _lib.call("cr_cube_select_param", raw, c["ld"], lay, K, T(c["cls"]), T(c["valid"].to(torch.uint8)), T(c["gt_idx"]), B, c["S"], kf,
              c["G"], T(c["gt3d"]), T(c["gtpose"].reshape(B, -1, 9)), pm, T(c["meta"]), buf, validf, clsc, zc[0], zc[1], zc[2], zc[3],
              boxes, pc, dc, ps if dc else None, norm3)
    up = {k: T(t.reshape(-1)) for k, t in c["up"].items()}
    g_raw = torch.full_like(raw, float("nan"))
    _lib.call("cr_cube_select_param_bwd", raw, c["ld"], lay, K, B, kf, validf, clsc, up["dxy"], up["zr"], up["dr"], up["Ra"],
              up["u"] if conf else None, up["usel"] if conf else None, g_raw, zc[0], zc[1], zc[2], zc[3], boxes, pc, dc, pm,
              ps if dc else None, g_zraw)
    torch.cuda.synchronize()
    ch = [t.cpu() for t in ops._chunks(buf, n)]
    names = ("dxy", "zr", "dr", "Ra", "u", "K4", "v2r", "prior", "gt2d", "gtz", "gtdims", "gtR")
    out = {k: t.reshape(n, -1) for k, t in zip(names, ch)}
    return out, g_raw.cpu(), validf.cpu(), clsc.cpu(), None if norm3 is None else norm3.cpu().reshape(3, n)


def rel_err(a, ref):
    """largest error of `a` against the float64 `ref`, relative to the largest magnitude of `ref`"""
    scale = float(ref.abs().max())
    return float((a.double() - ref).abs().max()) / scale if scale > 0 else float(a.abs().max())


@pytest.mark.parametrize("conf", [True, False])
@pytest.mark.parametrize("dims_func", ["exp", "sigmoid"])
@pytest.mark.parametrize("pose_type", ["6d", "quaternion", "euler"])
def test_selection_matches_float64(pose_type, dims_func, conf):
    """Forward: the chunks dxy / zr / dr / Ra / u / prior of buf39 and the decoded dimensions exp(min(dr, 5)) * prior.  Backward:
    the dense gradient of sum(upstream * chunk).  Error measure: largest deviation from the float64 evaluation relative to the
    largest magnitude of that quantity; per case the worst quantity counts.  Tolerance: 4 x the float32 noise floor of the case =
    the same torch expressions evaluated in float32 on the CPU against float64 (the kernel may associate sums differently).
    Measured on the MI355X over the 12 cases: forward, worst kernel error 1.18e-6 where the floor is 5.67e-7 (6d: the Gram-Schmidt
    of a nearly parallel pair), quaternion 2.3e-7 / 2.4e-7, euler 1.65e-7 / 8.2e-8; backward, worst kernel error 1.41e-7 where the
    floor is 2.43e-7, smallest floor 7.8e-8 (quaternion with confidence, kernel 1.1e-7).
    Exact: validity flags, clamped classes, ground-truth chunks (the safe cuboid on empty slots), zero gradient rows on empty
    slots and zero gradient entries off the RoI's class."""
    c = sel_case(pose_type, conf)
    ref, gref, v, cl = sel_reference(c, pose_type, dims_func, conf, torch.float64)
    f32, g32, _, _ = sel_reference(c, pose_type, dims_func, conf, torch.float32)
    got, ggot, validf, clsc, _ = sel_kernels(c, pose_type, dims_func, conf)
    n, K, kf, pw = c["n"], c["K"], c["kf"], c["pw"]
    assert torch.equal(validf.bool(), v) and torch.equal(clsc.long(), cl)
    assert int((~v).sum()) == 2
    got["dims"] = torch.exp(got["dr"].clip(max=5)) * got["prior"]
    keys = ("dxy", "zr", "dr", "Ra", "u", "prior", "dims")
    floor_f = max(rel_err(f32[k], ref[k]) for k in keys)
    err_f = max(rel_err(got[k], ref[k]) for k in keys)
    vm = v[:, None]
    floor_b, err_b = rel_err(g32, gref), rel_err(ggot, gref)
    print("select_param %s/%s/conf=%d forward: kernel %.3g floor %.3g | backward: kernel %.3g floor %.3g"
          % (pose_type, dims_func, conf, err_f, floor_f, err_b, floor_b))
    assert torch.isfinite(ggot).all() and all(torch.isfinite(got[k]).all() for k in got)
    assert err_f <= 4 * floor_f, (err_f, floor_f)
    assert err_b <= 4 * floor_b, (err_b, floor_b)
    if not conf:
        assert float(got["u"].abs().max()) == 0.0
    # ground truth and camera chunks: copies
    b_of = torch.arange(n) // kf
    gi = c["gt_idx"][:, :kf].reshape(-1)
    g3 = c["gt3d"][b_of, gi]
    safe = torch.tensor([256.0, 256.0, 5.0, 1.0, 1.0, 1.0]).expand(n, 6)
    want = torch.where(vm, g3[:, :6], safe)
    assert torch.equal(torch.cat([got["gt2d"], got["gtz"], got["gtdims"]], 1), want)
    assert torch.equal(got["gtR"], c["gtpose"][b_of, gi].reshape(n, 9))
    assert torch.equal(got["K4"], c["meta"][b_of, :4]) and torch.equal(got["v2r"][:, 0], c["meta"][b_of, 4])
    # exact zeros of the dense gradient
    own = torch.zeros(n, c["ld"], dtype=torch.bool)
    o_d2, o_dims, o_pose, o_z, o_unc = c["layout"]
    for o, d in ((o_d2, 2), (o_dims, 3), (o_pose, pw), (o_z, 1)) + (((o_unc, 1),) if conf else ()):
        for e in range(d):
            own[torch.arange(n), o + cl * d + e] = True
    own &= vm
    assert float(ggot[~own].abs().max()) == 0.0
    assert float(ggot[~v].abs().max()) == 0.0 and int((ggot[v] != 0).sum()) > 0


def test_selection_writes_the_norm_rows_and_adds_the_raw_depth_gradient():
    """the two extras the non-disentangled loss needs from the selection: norm3 = [raw depth | 0 | 1] for Z_TYPE 'direct', and
    g_zraw added to the depth column of the valid RoIs -- both exact"""
    c = sel_case("euler", False)
    n, K = c["n"], c["K"]
    _, g0, validf, clsc, _ = sel_kernels(c, "euler", "exp", False)
    zraw = torch.randn(n, generator=torch.Generator().manual_seed(1))
    _, g1, _, _, norm = sel_kernels(c, "euler", "exp", False, norm=True, g_zraw=zraw.to(DEV))
    col = c["layout"][3] + clsc.long()
    ar = torch.arange(n)
    assert torch.equal(norm[0], c["raw"][ar, col]) and float(norm[1].abs().max()) == 0.0 and bool((norm[2] == 1.0).all())
    want = g0.clone()
    vv = validf.bool()
    want[ar[vv], col[vv]] = g0[ar[vv], col[vv]] + zraw[vv]       # dz = 1 for 'direct': one float32 addition on both sides
    assert torch.equal(g1, want)


@pytest.mark.parametrize("z_type,bins", [("clusters", 3), ("direct", 3), ("sigmoid", 1), ("log", 1)])
def test_selection_depth_types_match_float64(z_type, bins):
    """the depth path of the parametrised selection (bin choice, Z_TYPE decode and its derivative, cluster statistics) on a
    quaternion / sigmoid-prior / confidence layout: decoded depth and dense gradient against float64 at 4 x the float32 floor as
    above; the norm rows [raw depth of the RoI's (bin, class) column | cluster mean | std] are copies; g_zraw lands on that column
    only, to one fused-multiply-add's rounding (2^-23 (|without| + |with|))."""
    c = sel_case("quaternion", True, z_type, bins)
    ref, gref, v, cl = sel_reference(c, "quaternion", "sigmoid", True, torch.float64)
    f32, g32, _, _ = sel_reference(c, "quaternion", "sigmoid", True, torch.float32)
    got, g0, validf, clsc, _ = sel_kernels(c, "quaternion", "sigmoid", True)
    n, K = c["n"], c["K"]
    floor_f, err_f = rel_err(f32["zr"], ref["zr"]), rel_err(got["zr"], ref["zr"])
    floor_b, err_b = rel_err(g32, gref), rel_err(g0, gref)
    print("select_param depth %s/bins=%d forward: kernel %.3g floor %.3g | backward: kernel %.3g floor %.3g"
          % (z_type, bins, err_f, floor_f, err_b, floor_b))
    assert err_f <= 4 * floor_f, (err_f, floor_f)
    assert err_b <= 4 * floor_b, (err_b, floor_b)
    zraw = torch.randn(n, generator=torch.Generator().manual_seed(1))
    _, g1, _, _, norm = sel_kernels(c, "quaternion", "sigmoid", True, norm=True, g_zraw=zraw.to(DEV))
    ar = torch.arange(n)
    bin_ = torch.zeros(n, dtype=torch.long)
    if bins > 1:
        b = c["boxes"].double()
        diag = ((b[:, 3] - b[:, 1]) ** 2 + (b[:, 2] - b[:, 0]) ** 2).sqrt()
        bin_ = (c["z_scales"].double()[cl] - diag[:, None]).abs().argmin(1)
    col = c["layout"][3] + bin_ * K + cl
    assert torch.equal(norm[0], c["raw"][ar, col])
    if z_type == "clusters":
        assert torch.equal(norm[1], c["z_stats"][cl, bin_, 0]) and torch.equal(norm[2], c["z_stats"][cl, bin_, 1])
    else:
        assert float(norm[1].abs().max()) == 0.0 and bool((norm[2] == 1.0).all())
    at = torch.zeros_like(g0, dtype=torch.bool)
    at[ar[v], col[v]] = True
    assert torch.equal(g1[~at], g0[~at])
    d = (g1[at].double() - (g0[at].double() + zraw[v].double())).abs()
    assert bool((d <= 2.0 ** -23 * (g0[at].abs() + g1[at].abs()).double()).all()), float(d.max())
    assert float((g1[at] - g0[at]).abs().max()) > 0.1


def test_param_kernels_on_the_default_options_match_the_old_kernels():
    """6d / exp / confidence through cr_cube_select(_bwd), the default family's own kernels, which share their device helpers
    (rot6d, rot6d_bwd, the meta / ground-truth copy, the dense-row scatter) with cr_cube_select_param(_bwd) but stay separate
    kernels because their output bits are pinned: the old kernels are held to the same float64 definition at the same 4 x float32
    floor as the new ones in test_selection_matches_float64, and the copies, flags and zero patterns of old and new are identical.
    Old and new are not compared to each other at a bound of their own: inside two different kernels the compiler contracts the
    same source expression differently, and the Gram-Schmidt of this case's nearly parallel pairs amplifies that (measured: the
    forward rotations differ by 1.28e-6 of the scale where the float32 floor of the case is 5.67e-7, each within 4 x floor of
    float64)."""
    c = sel_case("6d", True)
    ref, gref, v, cl = sel_reference(c, "6d", "exp", True, torch.float64)
    f32, g32, _, _ = sel_reference(c, "6d", "exp", True, torch.float32)
    got, g_new, validf, clsc, _ = sel_kernels(c, "6d", "exp", True)
    T = lambda t: t.to(DEV).contiguous()
    n, B, kf, K = c["n"], c["B"], c["kf"], c["K"]
    raw, boxes = T(c["raw"]), T(c["boxes"])
    buf = torch.empty((39 * n,), device=DEV)
    vf = torch.empty((n,), dtype=torch.uint8, device=DEV)
    cc = torch.empty((n,), dtype=torch.int32, device=DEV)
    lay = (ctypes.c_int * 5)(*c["layout"])
    _lib.call("cr_cube_select", raw, c["ld"], lay, K, T(c["cls"]), T(c["valid"].to(torch.uint8)), T(c["gt_idx"]), B, c["S"], kf, c["G"],
              T(c["gt3d"]), T(c["gtpose"].reshape(B, -1, 9)), T(c["pri_mean"]), T(c["meta"]), buf, vf, cc, 0, 1, None, None, boxes)
    up = {k: T(t.reshape(-1)) for k, t in c["up"].items()}
    g_old = torch.empty_like(raw)
    _lib.call("cr_cube_select_bwd", raw, c["ld"], lay, K, B, kf, vf, cc, up["dxy"], up["zr"], up["dr"], up["Ra"], up["u"], up["usel"],
              g_old, 0, 1, None, None, boxes)
    names = ("dxy", "zr", "dr", "Ra", "u", "K4", "v2r", "prior", "gt2d", "gtz", "gtdims", "gtR")
    old = {k: t.cpu().reshape(n, -1) for k, t in zip(names, ops._chunks(buf, n))}
    g_old = g_old.cpu()
    assert torch.equal(vf.cpu(), validf) and torch.equal(cc.cpu(), clsc)
    for k in names:
        if k != "Ra":                                      # gathers, the clip and the ground truth: copies in both kernels
            assert torch.equal(old[k], got[k]), k
    keys = ("dxy", "zr", "dr", "Ra", "u", "prior")
    floor_f = max(rel_err(f32[k], ref[k]) for k in keys)
    err_f = max(rel_err(old[k], ref[k]) for k in keys)
    floor_b, err_b = rel_err(g32, gref), rel_err(g_old, gref)
    print("cr_cube_select 6d/exp/conf=1 forward: kernel %.3g floor %.3g | backward: kernel %.3g floor %.3g | old vs new: Ra %.3g grad %.3g"
          % (err_f, floor_f, err_b, floor_b, rel_err(got["Ra"], old["Ra"].double()), rel_err(g_new, g_old.double())))
    assert err_f <= 4 * floor_f and err_b <= 4 * floor_b, (err_f, floor_f, err_b, floor_b)
    assert torch.equal(g_old == 0, g_new == 0)


def test_sigmoid_prior_stays_finite_where_the_sigmoid_underflows():
    """lower bound 0 (mean - 3 std < 0) and a raw dimension of -120: the decoded dimension underflows to 0; the stored logarithm and
    the whole gradient row stay finite and the gradient of that column is 0, as the reference's"""
    c = sel_case("euler", False)
    K = c["K"]
    c["pri_std"] = c["pri_mean"].clone()                  # mean - 3 std < 0 for every class: lower bound 0
    cl0 = int(c["cls"][0, 0])
    col = c["layout"][1] + 3 * cl0 + 1
    c["raw"][0, col] = -120.0
    got, g, validf, _, _ = sel_kernels(c, "euler", "sigmoid", False)
    assert bool(validf[0]) and bool(torch.isfinite(got["dr"]).all()) and bool(torch.isfinite(g).all())
    assert float(g[0, col]) == 0.0 and float(torch.exp(got["dr"][0, 1])) < 1e-29


# ------------------------------------------------------------------------------------------------ reference goldens: training
TRAIN = {   # case -> (pose leaf, pose type, confidence, prior function, disentangled)
    "noconf": ("pose6", "6d", False, "exp", True),
    "sigmoid": ("pose6", "6d", True, "sigmoid", True),
    "noconf_sigmoid": ("pose6", "6d", False, "sigmoid", True),
    "nondis_noconf": ("pose6", "6d", False, "exp", False),
    "quat": ("pose4", "quaternion", True, "exp", True),
    "euler": ("pose3", "euler", True, "exp", True),
}


def fused_raw(g, leaf, pw, conf, rows):
    """the fixture's head outputs laid out like CubeHead.forward_fused: [deltas 2K | dims 3K | pose pw K | z K | (uncert K)]"""
    T = lambda k: torch.tensor(g[k]).to(DEV)
    K = g["in_deltas"].shape[1]
    width = (6 + pw + (1 if conf else 0)) * K
    ld = (width + 15) // 16 * 16
    src = torch.zeros((rows, ld), device=DEV)
    src[:, 0:2 * K] = T("in_deltas").reshape(rows, -1)
    src[:, 2 * K:5 * K] = T("in_dims").reshape(rows, -1)
    src[:, 5 * K:(5 + pw) * K] = T("in_" + leaf).reshape(rows, -1)
    src[:, (5 + pw) * K:(6 + pw) * K] = T("in_z").reshape(rows, -1)
    if conf:
        src[:, (6 + pw) * K:(7 + pw) * K] = T("in_uncert")
    return src, (0, 2 * K, 5 * K, (5 + pw) * K, (6 + pw) * K if conf else -1), K


def meta_rows(g, ratio_column):
    rows = []
    for k, r in zip(g["Ks"], g["ratios"]):
        r = float(r)
        v2r = util.compute_virtual_scale_from_focal_spaces(float(k[1, 1]), 512.0 * r, 512.0, 512.0)
        rows.append([float(k[0, 0]) / r, float(k[1, 1]) / r, float(k[0, 2]) / r, float(k[1, 2]) / r, float(v2r)] + ([r] if ratio_column else []))
    return torch.tensor(rows, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("case", list(TRAIN))
def test_losses_and_gradients_match_reference(golden_dir, case):
    leaf, pose_type, conf, dims_func, disentangled = TRAIN[case]
    pw = POSE_W[pose_type]
    g = np.load(os.path.join(golden_dir, "cubehead_train_%s.npz" % case), allow_pickle=False)
    T = lambda k: torch.tensor(g[k]).to(DEV)
    n_per = g["n_per"].tolist()
    B, kf = len(n_per), max(n_per) + 2
    n = B * kf
    src, layout, K = fused_raw(g, leaf, pw, conf, sum(n_per))
    slot = torch.cat([torch.arange(c) + b * kf for b, c in enumerate(n_per)]).to(DEV)          # golden row -> dense slot
    raw = torch.zeros((n, src.shape[1]), device=DEV)
    raw[slot] = src
    raw.requires_grad_(True)
    S, G = kf + 3, max(n_per)
    cls = torch.full((B, S), K, dtype=torch.int64, device=DEV)
    valid = torch.zeros((B, S), dtype=torch.bool, device=DEV)
    gt_idx = torch.zeros((B, S), dtype=torch.int64, device=DEV)
    gt3d = torch.zeros((B, G, 9), device=DEV)
    gtpose = torch.eye(3, device=DEV).expand(B, G, 3, 3).clone()
    boxes = torch.zeros((B, kf, 4), device=DEV)
    boxes[..., 2:] = 10.0
    off = 0
    for b, c in enumerate(n_per):                                            # every RoI gets its own ground-truth row
        cls[b, :c] = T("gt_classes")[off:off + c]
        valid[b, :c] = True
        gt_idx[b, :c] = torch.arange(c, device=DEV)
        gt3d[b, :c] = T("gt_boxes3D")[off:off + c]
        gtpose[b, :c] = T("gt_poses")[off:off + c]
        boxes[b, :c] = T("proposal_boxes")[off:off + c]
        off += c
    priors = T("priors")[0, :, 0, :].contiguous() if disentangled else None
    kw = {}
    if pose_type != "6d":
        kw["pose_type"] = pose_type
    if dims_func != "exp":
        kw.update(dims_func=dims_func, priors_std=T("priors")[0, :, 1, :].contiguous())
    if not disentangled:
        kw["disentangled"] = False
    L, u_sel, dec, buf, validf = ops.cube_head_loss(raw, layout, K, cls, valid, gt_idx, kf, gt3d, gtpose, priors, meta_rows(g, False),
                                                    boxes.reshape(n, 4), allocentric=True, chamfer_pose=True, use_conf=conf,
                                                    joint=True, **kw)
    red, _ = ops.cube_reduce(L, u_sel, buf, dec, validf, inverse_z=False)
    # weights of make_golden_cubehead.py: dims 20, xy 1, z 1, pose 7, joint 1, uncertainty use_confidence (x loss_w_3d 1)
    w = torch.tensor([20.0, 1.0, 1.0, 7.0, 1.0, 1.0 if conf else 0.0], device=DEV)
    names = ["loss_dims", "loss_xy", "loss_z", "loss_pose", "loss_joint"] + (["uncert"] if conf else [])
    assert sorted("Cube/" + nm for nm in names) == sorted(str(k) for k in g["loss_keys"])      # no Cube/uncert without confidence
    ltol = 1e-5 if disentangled else 2e-5
    bad = []
    for i, nm in enumerate(names):
        ref, got = float(g["loss_Cube_" + nm]), float(red[i] * w[i])
        print(case, nm, got, ref, abs(got - ref) / max(1.0, abs(ref)))
        if not abs(got - ref) <= ltol * max(1.0, abs(ref)):
            bad.append((nm, got, ref))
    assert not bad, bad
    (red * w).sum().backward()
    gr = raw.grad[slot]
    cuts = [("deltas", 0, 2), ("dims", 2, 3), (leaf, 5, pw), ("z", 5 + pw, 1)] + ([("uncert", 6 + pw, 1)] if conf else [])
    for nm, o, d in cuts:
        ref = g["grad_" + nm]
        got = gr[:, o * K:(o + d) * K].reshape(ref.shape).cpu().numpy()
        if disentangled:
            scale = float(np.abs(ref).max())
            err = float(np.abs(got - ref).max())
            print(case, "grad", nm, err / scale)
            assert err <= 2e-4 * scale, (nm, err, scale)
        else:
            np.testing.assert_allclose(got, ref, rtol=5e-4, atol=5e-6, err_msg=nm)
    empty = torch.ones(n, dtype=torch.bool, device=DEV)
    empty[slot] = False
    assert float(raw.grad[empty].abs().max()) == 0.0
    assert float(raw.grad[:, (6 + pw + (1 if conf else 0)) * K:].abs().max()) == 0.0             # the padding columns


# ------------------------------------------------------------------------------------------------ reference goldens: inference
EVAL = {k: v for k, v in TRAIN.items() if k != "nondis_noconf"}


@pytest.mark.parametrize("case", list(EVAL))
def test_decode_matches_reference_eval_golden(golden_dir, case):
    leaf, pose_type, conf, dims_func, _ = EVAL[case]
    pw = POSE_W[pose_type]
    g = np.load(os.path.join(golden_dir, "cubehead_eval_%s.npz" % case), allow_pickle=False)
    T = lambda k: torch.tensor(g[k]).to(DEV)
    n = g["in_deltas"].shape[0]
    raw, layout, K = fused_raw(g, leaf, pw, conf, n)
    n_per = g["n_per"].tolist()
    img = torch.repeat_interleave(torch.arange(len(n_per)), torch.tensor(n_per)).to(DEV)
    kw = {}
    if pose_type != "6d":
        kw["pose_type"] = pose_type
    if dims_func != "exp":
        kw.update(dims_func=dims_func, priors_std=T("priors")[0, :, 1, :].contiguous())
    if not conf:
        kw["use_conf"] = False
    o = ops.cube_decode_infer(raw, layout, K, T("classes"), img, T("pred_boxes"), meta_rows(g, True), T("priors")[0, :, 0, :].contiguous(),
                              allocentric=True, **kw).cpu().numpy()
    chk = lambda got, key, rtol=1e-4, atol=1e-5: np.testing.assert_allclose(got, g[key], rtol=rtol, atol=atol, err_msg=key)
    chk(o[:, 18:42].reshape(n, 8, 3), "out_pred_bbox3D")
    chk(o[:, 0:3], "out_pred_center_cam")
    chk(o[:, 6:8], "out_pred_center_2D")
    chk(o[:, 3:6], "out_pred_dimensions")
    chk(o[:, 9:18].reshape(n, 3, 3), "out_pred_pose")
    # the merged score (roi_heads.py:2711-2712); without confidence the 3D factor is the projected centre's y x ratio
    score = np.sqrt(g["scores_2d"] * o[:, 8])
    print(case, "score rel err", float(np.abs(score / g["out_scores"] - 1).max()))
    chk(score, "out_scores", rtol=1e-5, atol=0.0)
    if not conf:
        assert np.array_equal(o[:, 8], o[:, 7])


# ------------------------------------------------------------------------------------------------ the default path
def test_default_keywords_launch_the_old_entry_points(golden_dir):
    """ops.cube_head_loss / ops.cube_decode_infer with default keywords, and with the defaults written out, are bit-equal to
    cr_cube_select + cr_cube_loss_fwd / _bwd + cr_cube_select_bwd and to cr_cube_decode_infer called directly"""
    g = np.load(os.path.join(golden_dir, "cubehead_train.npz"), allow_pickle=False)
    T = lambda k: torch.tensor(g[k]).to(DEV)
    n = g["in_deltas"].shape[0]
    src, layout, K = fused_raw(g, "pose6", 6, True, n)
    B, kf, S, G = 1, n, n + 2, n
    cls = torch.full((B, S), K, dtype=torch.int64, device=DEV)
    cls[0, :n] = T("gt_classes")
    valid = torch.zeros((B, S), dtype=torch.bool, device=DEV)
    valid[0, :n] = True
    valid[0, 3] = False
    gt_idx = torch.zeros((B, S), dtype=torch.int64, device=DEV)
    gt_idx[0, :n] = torch.arange(n, device=DEV)
    gt3d, gtpose = T("gt_boxes3D")[None].contiguous(), T("gt_poses")[None].contiguous()
    meta = meta_rows(g, False)[:1].contiguous()
    boxes = T("proposal_boxes").contiguous()
    priors = T("priors")[0, :, 0, :].contiguous()
    gl = torch.randn(n, 5, generator=torch.Generator().manual_seed(2)).to(DEV)
    gus = torch.randn(n, generator=torch.Generator().manual_seed(3)).to(DEV)

    def through_ops(**kw):
        raw = src.clone().requires_grad_(True)
        L, u_sel, dec, buf, validf = ops.cube_head_loss(raw, layout, K, cls, valid, gt_idx, kf, gt3d, gtpose, priors, meta, boxes, **kw)
        ((L * gl).sum() + (u_sel * gus).sum()).backward()
        return L.detach(), u_sel.detach(), dec, buf, validf, raw.grad
    a = through_ops()
    b = through_ops(pose_type="6d", dims_func="exp", priors_std=None, use_conf=True)
    # the old entry points, directly
    lay = (ctypes.c_int * 5)(*layout)
    buf = torch.empty((39 * n,), device=DEV)
    validf = torch.empty((n,), dtype=torch.uint8, device=DEV)
    clsc = torch.empty((n,), dtype=torch.int32, device=DEV)
    _lib.call("cr_cube_select", src, src.shape[1], lay, K, cls, valid.to(torch.uint8), gt_idx, B, S, kf, G, gt3d,
              gtpose.reshape(1, -1, 9), priors, meta, buf, validf, clsc, 0, 1, None, None, boxes)
    ch, arr = ops._cube_loss_ins(buf, boxes, n)
    L = torch.empty((n, 5), device=DEV)
    dec = torch.empty((n, 17), device=DEV)
    _lib.call("cr_cube_loss_fwd", arr, n, 1, 1, 1, 1, L, dec)
    g_dxy, g_zr, g_dr, g_Ra, g_u = ops._cube_grads(n, DEV)
    _lib.call("cr_cube_loss_bwd", arr, n, 1, 1, 1, 1, gl, g_dxy, g_zr, g_dr, g_Ra, g_u)
    g_raw = torch.empty_like(src)
    _lib.call("cr_cube_select_bwd", src, src.shape[1], lay, K, B, kf, validf, clsc, g_dxy, g_zr, g_dr, g_Ra, g_u, gus, g_raw, 0, 1,
              None, None, boxes)
    direct = (L, ch[4].clone(), dec, buf, validf, g_raw)
    for x, y, z in zip(a, b, direct):
        assert torch.equal(x, y) and torch.equal(x, z)
    # inference
    e = np.load(os.path.join(golden_dir, "cubehead_eval.npz"), allow_pickle=False)
    E = lambda k: torch.tensor(e[k]).to(DEV)
    m = e["in_deltas"].shape[0]
    raw, layout, K = fused_raw(e, "pose6", 6, True, m)
    n_per = e["n_per"].tolist()
    img = torch.repeat_interleave(torch.arange(len(n_per)), torch.tensor(n_per)).to(DEV)
    meta6 = meta_rows(e, True)
    pri = E("priors")[0, :, 0, :].contiguous()
    o0 = ops.cube_decode_infer(raw, layout, K, E("classes"), img, E("pred_boxes"), meta6, pri)
    o1 = ops.cube_decode_infer(raw, layout, K, E("classes"), img, E("pred_boxes"), meta6, pri, pose_type="6d", use_conf=True,
                               dims_func="exp", priors_std=None)
    o2 = torch.empty((m, 42), device=DEV)
    _lib.call("cr_cube_decode_infer", raw, raw.shape[1], (ctypes.c_int * 5)(*layout), K, E("classes"), img.to(torch.int32),
              E("pred_boxes"), meta6, pri, m, 1, o2, 0, 1, None, None)
    assert torch.equal(o0, o1) and torch.equal(o0, o2)
    # and the parametrised kernels on the default options compute the same decode (not bit-pinned: another kernel)
    c5 = (ctypes.c_int * 5)(*layout)
    o3 = torch.empty((m, 42), device=DEV)
    _lib.call("cr_cube_decode_infer_param", raw, raw.shape[1], c5, K, E("classes"), img.to(torch.int32), E("pred_boxes"), meta6, pri, m,
              1, o3, 0, 1, None, None, 0, 0, None)
    assert torch.allclose(o0, o3, rtol=1e-6, atol=1e-6)


def test_unknown_values_and_bad_layouts_raise():
    c = sel_case("quaternion", True)
    T = lambda t: t.to(DEV).contiguous()
    args = (T(c["raw"]), c["layout"], c["K"], T(c["cls"]), T(c["valid"]), T(c["gt_idx"]), c["kf"], T(c["gt3d"]), T(c["gtpose"]),
            T(c["pri_mean"]), T(c["meta"]), T(c["boxes"]))
    with pytest.raises(ValueError, match="6d.*euler.*quaternion"):
        ops.cube_head_loss(*args, pose_type="axis_angle")
    with pytest.raises(ValueError, match="exp.*sigmoid"):
        ops.cube_head_loss(*args, pose_type="quaternion", dims_func="tanh")
    with pytest.raises(ValueError, match="priors_std"):
        ops.cube_head_loss(*args, pose_type="quaternion", dims_func="sigmoid")
    # a pose block that does not fit the row: refused by the entry point, nothing is launched
    bad = (0, 6, 15, c["ld"] - 2, c["layout"][4])
    with pytest.raises(_lib.CrError, match="does not fit"):
        ops.cube_head_loss(args[0], bad, *args[2:], pose_type="quaternion")


# ------------------------------------------------------------------------------------------------ end to end
H = "MODEL.ROI_CUBE_HEAD."
E2E = {"quaternion": ([H + "POSE_TYPE", "quaternion"], "quat", 4), "euler": ([H + "POSE_TYPE", "euler"], "euler", 3),
       "noconf": ([H + "USE_CONFIDENCE", 0.0], "noconf", 6), "sigmoid": ([H + "DIMS_PRIORS_FUNC", "sigmoid"], "sigmoid", 6)}


@pytest.mark.parametrize("name", list(E2E))
def test_model_trains_and_infers_with_the_option(golden_dir, monkeypatch, name):
    """2 x 128^2 images, two steps of solver.make_train_step with the per-shape graph cache on, then inference on the same model"""
    extra, case, pw = E2E[name]
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    monkeypatch.setenv("CR_GRAPHS", "dense")
    cfg, model, opt, syn, solver = bt.build(DEV, seed=0, lr=0.0025, extra=extra)
    rh = model.roi_heads
    K = rh.num_classes
    assert rh.cube_head.bbox_3D_pose.out_features == pw * K
    step = solver.make_train_step(cfg, model, opt, world_size=1)
    torch.manual_seed(5)
    with d2.EventStorage(0) as storage:
        for i in range(2):
            b = syn.make_batch(2, 900 + i, size=128)
            for d in b:
                d["image"], d["instances"] = d["image"].to(DEV), d["instances"].to(DEV)
            step(b)
        rep = step.report()
        logged = set(storage.latest())
    assert model._graphed is not None
    assert rep["iterations_explode"] == 0 and math.isfinite(rep["total_loss"]), rep
    ref_keys = set(str(k) for k in np.load(os.path.join(golden_dir, "cubehead_train_%s.npz" % case))["loss_keys"])
    assert {k for k in rep if k.startswith("Cube/")} == ref_keys, rep
    assert all(math.isfinite(rep[k]) for k in ref_keys), rep
    assert ("Cube/conf" in logged) == (name != "noconf")
    gw = rh.cube_head.bbox_3D_pose.weight._cr_grad           # the parameter's view of the optimizer's flat gradient (last step)
    assert gw.numel() == pw * K * rh.cube_head.bbox_3D_pose.in_features
    assert bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0.0
    model.eval()
    rh.box_predictor.test_score_thresh = 0.0
    with torch.no_grad():
        out = model(syn.make_batch(2, 5, size=128, with_gt=False))
    total = 0
    for o in out:
        inst = o["instances"]
        m = len(inst)
        total += m
        assert tuple(inst.pred_bbox3D.shape) == (m, 8, 3) and tuple(inst.pred_pose.shape) == (m, 3, 3)
        assert tuple(inst.pred_center_cam.shape) == (m, 3) and tuple(inst.pred_center_2D.shape) == (m, 2)
        assert tuple(inst.pred_dimensions.shape) == (m, 3) and tuple(inst.scores.shape) == (m,)
        for f in ("pred_bbox3D", "pred_pose", "pred_center_cam", "pred_center_2D", "pred_dimensions"):
            assert bool(torch.isfinite(inst.get(f)).all()), f
        R = inst.pred_pose.double()
        assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3, dtype=torch.float64, device=R.device).expand_as(R), atol=1e-4)
    assert total > 0
