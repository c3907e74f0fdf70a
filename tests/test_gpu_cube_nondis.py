"""GPU: the 3D head trained with the non-disentangled losses (MODEL.ROI_CUBE_HEAD.DISENTANGLED_LOSS False, roi_heads.py:2516-2560,
2587-2591): cr_cube_select + cr_cube_select_norm, cr_cube_nondis_fwd / _bwd, cr_cube_reduce(_bwd), cr_cube_select_bwd +
cr_cube_select_bwd_zraw through ops.cube_head_loss(..., disentangled=False) / ops.cube_reduce, against the REFERENCE'S OWN
ROIHeads3D._forward_cube (tests/golden/cubehead_train_nondis*.npz; generator tests/golden/make_golden_cubehead_nondis.py) at the
tolerances of test_gpu_dense_golden.py for the same head: reduced weighted losses 2e-5 max(1, |ref|), gradients w.r.t. the head
outputs rtol 5e-4 / atol 5e-6, empty slots exactly 0.  Saturated depth / clipped dimensions, the untouched default path, the train
step end to end (per-shape graph cache on and off) and run-to-run bit equality."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

import cube_nondis_f64 as F

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dod_amd.hipops")
DEV = torch.device("cuda:0")


def slots(g, z_type):
    """the fixture's RoIs on padded (B, kf) slots, as test_dense_cube_head_loss_matches_reference_train_golden builds them"""
    util = importlib.import_module("3dod_amd.cubercnn.util.math_util")
    T = lambda k: torch.tensor(g[k]).to(DEV)
    n_per = g["n_per"].tolist()
    B, kf, K = len(n_per), max(n_per) + 2, g["in_deltas"].shape[1]
    bins = g["priors_z_scales"].shape[1] if "priors_z_scales" in g.files else 1
    n = B * kf
    ld = ((12 + bins) * K + 15) // 16 * 16
    slot = torch.cat([torch.arange(c) + b * kf for b, c in enumerate(n_per)]).to(DEV)          # golden row -> dense slot
    raw = torch.zeros((n, ld), device=DEV)
    src = torch.zeros((sum(n_per), ld), device=DEV)
    src[:, 0:2 * K] = T("in_deltas").reshape(-1, 2 * K)
    src[:, 2 * K:5 * K] = T("in_dims").reshape(-1, 3 * K)
    src[:, 5 * K:11 * K] = T("in_pose6").reshape(-1, 6 * K)
    src[:, 11 * K:(11 + bins) * K] = T("in_z").reshape(-1, bins * K)
    src[:, (11 + bins) * K:(12 + bins) * K] = T("in_uncert")
    raw[slot] = src
    layout = (0, 2 * K, 5 * K, 11 * K, (11 + bins) * K)
    zc = ops.z_config(z_type, bins, T("priors_z_scales") if bins > 1 else None, T("priors_z_stats") if bins > 1 else None)
    S = kf + 3
    cls = torch.full((B, S), K, dtype=torch.int64, device=DEV)
    valid = torch.zeros((B, S), dtype=torch.bool, device=DEV)
    gt_idx = torch.zeros((B, S), dtype=torch.int64, device=DEV)
    G = max(n_per)
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
    rows = []
    for k, r in zip(g["Ks"], g["ratios"]):
        r = float(r)
        v2r = util.compute_virtual_scale_from_focal_spaces(float(k[1, 1]), 512.0 * r, 512.0, 512.0)
        rows.append([float(k[0, 0]) / r, float(k[1, 1]) / r, float(k[0, 2]) / r, float(k[1, 2]) / r, float(v2r)])
    meta = torch.tensor(rows, dtype=torch.float32, device=DEV)
    return dict(raw=raw, layout=layout, K=K, cls=cls, valid=valid, gt_idx=gt_idx, kf=kf, gt3d=gt3d, gtpose=gtpose, meta=meta,
                boxes=boxes.reshape(n, 4), zc=zc, slot=slot, n=n, bins=bins, B=B)


def evaluate(s, w, priors=None, allocentric=True, chamfer_pose=True, joint=True, inverse_z=False, **kw):
    """-> (red (6) detached, gradient of sum(red * w) w.r.t. the predictor output); kw: disentangled=..."""
    raw = s["raw"].clone().requires_grad_(True)
    L, u_sel, dec, buf, validf = ops.cube_head_loss(raw, s["layout"], s["K"], s["cls"], s["valid"], s["gt_idx"], s["kf"], s["gt3d"],
                                                    s["gtpose"], priors, s["meta"], s["boxes"], allocentric=allocentric,
                                                    chamfer_pose=chamfer_pose, use_conf=True, joint=joint, z_cfg=s["zc"], **kw)
    red, stats = ops.cube_reduce(L, u_sel, buf, dec, validf, inverse_z=inverse_z)
    (red * w).sum().backward()
    return red.detach(), raw.grad, L.detach(), stats


def load(golden_dir, suffix):
    return np.load(os.path.join(golden_dir, "cubehead_train_nondis%s.npz" % suffix), allow_pickle=False)


@pytest.mark.parametrize("suffix", list(F.CASES))
def test_nondis_losses_and_gradients_match_reference(golden_dir, suffix):
    z_type, opt = F.CASES[suffix]
    g = load(golden_dir, suffix)
    s = slots(g, z_type)
    K, bins, slot = s["K"], s["bins"], s["slot"]
    w_joint = opt.get("w_joint", 1.0)
    # weights of make_golden_cubehead.py: dims 20, xy 1, z 1, pose 7, joint 1, uncertainty 1 (x loss_w_3d 1)
    w = torch.tensor([20.0, 1.0, 1.0, 7.0, w_joint, 1.0], device=DEV)
    red, grad, _, _ = evaluate(s, w, allocentric=opt.get("allocentric", True), chamfer_pose=opt.get("chamfer_pose", True),
                               joint=w_joint > 0, inverse_z=opt.get("inverse_z", False), disentangled=False)
    names = ["loss_dims", "loss_xy", "loss_z", "loss_pose", "loss_joint", "uncert"]
    bad = []
    for i, nm in enumerate(names):
        if nm == "loss_joint" and w_joint == 0:
            assert "loss_Cube_loss_joint" not in g.files
            continue
        ref, got = float(g["loss_Cube_" + nm]), float(red[i] * w[i])
        print(suffix, nm, got, ref, abs(got - ref) / max(1.0, abs(ref)))
        if not abs(got - ref) <= 2e-5 * max(1.0, abs(ref)):
            bad.append((nm, got, ref))
    assert not bad, bad
    gr = grad[slot]
    np.testing.assert_allclose(gr[:, 0:2 * K].reshape(-1, K, 2).cpu().numpy(), g["grad_deltas"], rtol=5e-4, atol=5e-6)
    np.testing.assert_allclose(gr[:, 2 * K:5 * K].reshape(-1, K, 3).cpu().numpy(), g["grad_dims"], rtol=5e-4, atol=5e-6)
    np.testing.assert_allclose(gr[:, 5 * K:11 * K].reshape(-1, K, 6).cpu().numpy(), g["grad_pose6"], rtol=5e-4, atol=5e-6)
    np.testing.assert_allclose(gr[:, 11 * K:(11 + bins) * K].reshape(g["grad_z"].shape).cpu().numpy(), g["grad_z"], rtol=5e-4, atol=5e-6)
    np.testing.assert_allclose(gr[:, (11 + bins) * K:(12 + bins) * K].cpu().numpy(), g["grad_uncert"], rtol=5e-4, atol=5e-6)
    empty = torch.ones(s["n"], dtype=torch.bool, device=DEV)
    empty[slot] = False
    assert float(grad[empty].abs().max()) == 0.0


def _zcol(s, g, rows):
    """(golden rows -> column of the RoI's depth output, its class, its uncertainty): bin by the float64 rule of cube_nondis_f64"""
    K, bins = s["K"], s["bins"]
    cls = np.asarray(g["gt_classes"]).astype(np.int64)
    bin_ = np.zeros(len(cls), dtype=np.int64)
    if bins > 1:
        box = np.asarray(g["proposal_boxes"], dtype=np.float64)
        diag = np.sqrt((box[:, 2] - box[:, 0]) ** 2 + (box[:, 3] - box[:, 1]) ** 2)
        bin_ = np.argmin(np.abs(np.asarray(g["priors_z_scales"], dtype=np.float64)[cls] - diag[:, None]), axis=1)
    return [11 * K + int(bin_[r]) * K + int(cls[r]) for r in rows]


@pytest.mark.parametrize("suffix,z_type", [("_zsigmoid", "sigmoid"), ("_zlog", "log"), ("_bins3_clusters", "clusters")])
def test_saturated_depth_has_finite_exact_gradients(golden_dir, suffix, z_type):
    """raw depth +-40 on a few RoIs, joint weight 0 so that only the z term reaches the depth column: no 0/0 from a decode whose
    derivative underflows; for log / clusters the gradient is sign * w_z * sqrt(2) exp(-u) / count, for sigmoid it underflows to
    (below) 1e-12 like the reference's"""
    g = load(golden_dir, suffix)
    s = slots(g, z_type)
    K, bins, slot = s["K"], s["bins"], s["slot"]
    rows = [0, 3, 8, 12, 20]
    vals = [40.0, -40.0, 40.0, -40.0, 40.0]
    cols = _zcol(s, g, rows)
    cls = np.asarray(g["gt_classes"]).astype(np.int64)
    for r, c, v in zip(rows, cols, vals):
        s["raw"][slot[r], c] = v
    w_z = 1.5
    w = torch.tensor([20.0, 1.0, w_z, 7.0, 0.0, 1.0], device=DEV)
    red, grad, L, _ = evaluate(s, w, joint=False, disentangled=False)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(red).all())
    count = len(cls)
    for r, c, v in zip(rows, cols, vals):
        got = float(grad[slot[r], c].double())
        u = max(float(np.float64(g["in_uncert"][r, cls[r]])), 0.01)
        full = w_z * math.sqrt(2.0) * math.exp(-u) / count
        print(suffix, r, v, got, full)
        if z_type == "sigmoid":
            assert abs(got) < 1e-12, (r, got)
        else:
            # raw = +-40 is far above / below every target of these fixtures: the sign of the residual is the sign of raw
            assert abs(got - math.copysign(full, v)) <= 1e-6 * full, (r, got, math.copysign(full, v))


def test_dims_term_acts_above_the_clip_and_the_joint_term_does_not(golden_dir):
    """raw dimensions of 6.0 (> the clip at 5): the dims term still pulls with +w_dims sqrt(2) exp(-u) / (3 count); the joint term,
    which sees exp(min(raw, 5)), adds nothing there"""
    g = load(golden_dir, "")
    cls = np.asarray(g["gt_classes"]).astype(np.int64)
    rows = [1, 5, 9, 15]
    got = {}
    for joint in (False, True):
        s = slots(g, "direct")
        K, slot = s["K"], s["slot"]
        for r in rows:
            s["raw"][slot[r], 2 * K + 3 * int(cls[r]):2 * K + 3 * int(cls[r]) + 3] = 6.0
        w = torch.tensor([20.0, 1.0, 1.0, 7.0, 1.0 if joint else 0.0, 1.0], device=DEV)
        _, grad, _, _ = evaluate(s, w, joint=joint, disentangled=False)
        assert bool(torch.isfinite(grad).all())
        got[joint] = torch.stack([grad[slot[r], 2 * K + 3 * int(cls[r]):2 * K + 3 * int(cls[r]) + 3] for r in rows])
    for i, r in enumerate(rows):
        u = max(float(np.float64(g["in_uncert"][r, cls[r]])), 0.01)
        full = 20.0 * math.sqrt(2.0) * math.exp(-u) / (3.0 * len(cls))          # log(gt dims) < 6 for every object: sign +
        assert float(np.log(np.float64(g["gt_boxes3D"][r, 3:6])).max()) < 6.0
        for k in range(3):
            assert abs(float(got[False][i, k].double()) - full) <= 1e-6 * full, (r, k, float(got[False][i, k]), full)
    assert torch.equal(got[False], got[True])


def test_default_path_is_untouched(golden_dir):
    """disentangled=True and a call without the argument: bit-equal losses and gradients on the disentangled fixture"""
    g = np.load(os.path.join(golden_dir, "cubehead_train.npz"), allow_pickle=False)
    s = slots(g, "direct")
    priors = torch.tensor(g["priors"]).to(DEV)[0, :, 0, :].contiguous()
    w = torch.tensor([20.0, 1.0, 1.0, 7.0, 1.0, 1.0], device=DEV)
    r0, g0, L0, _ = evaluate(s, w, priors=priors)
    r1, g1, L1, _ = evaluate(s, w, priors=priors, disentangled=True)
    assert torch.equal(r0, r1) and torch.equal(g0, g1) and torch.equal(L0, L1)
    for i, nm in enumerate(["loss_dims", "loss_xy", "loss_z", "loss_pose", "loss_joint", "uncert"]):      # and still the reference's
        ref = float(g["loss_Cube_" + nm])
        assert abs(float(r0[i] * w[i]) - ref) <= 2e-5 * max(1.0, abs(ref)), nm
    with pytest.raises(ValueError, match="DIMS_PRIORS_ENABLED"):
        evaluate(s, w, priors=priors, disentangled=False)


def test_run_to_run_bit_equal(golden_dir):
    g = load(golden_dir, "")
    w = torch.tensor([20.0, 1.0, 1.0, 7.0, 1.0, 1.0], device=DEV)
    a = evaluate(slots(g, "direct"), w, disentangled=False)
    b = evaluate(slots(g, "direct"), w, disentangled=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


NONDIS = ["MODEL.ROI_CUBE_HEAD.DISENTANGLED_LOSS", False, "MODEL.ROI_CUBE_HEAD.DIMS_PRIORS_ENABLED", False]
CUBE_KEYS = ["Cube/loss_dims", "Cube/loss_xy", "Cube/loss_z", "Cube/loss_pose", "Cube/loss_joint", "Cube/uncert"]


@pytest.mark.parametrize("extra", [[], ["MODEL.ROI_CUBE_HEAD.Z_TYPE", "clusters", "MODEL.ROI_CUBE_HEAD.CLUSTER_BINS", 3]])
def test_model_trains_with_the_non_disentangled_loss(extra):
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    cfg, model, opt, syn2, solver = bt.build(DEV, extra=NONDIS + extra)
    rh = model.roi_heads
    assert not rh.disentangled_loss and not rh.dims_priors_enabled
    if extra:
        K = rh.num_classes
        with torch.no_grad():
            rh.priors_z_scales.copy_(torch.tensor([40.0, 120.0, 300.0]).expand(K, 3))
            rh.priors_z_stats.copy_(torch.tensor([[3.0, 0.8], [6.0, 1.5], [12.0, 3.0]]).expand(K, 3, 2))
    step = solver.TrainStep(cfg, model, opt, world_size=1)
    with d2.EventStorage(0):
        step(syn2.make_batch(2, 3))
        step(syn2.make_batch(2, 4))
        rep = step.report()
    assert rep["iterations_explode"] == 0 and math.isfinite(rep["total_loss"]), rep
    assert all(k in rep and math.isfinite(rep[k]) for k in CUBE_KEYS), rep


def test_graph_cache_on_and_off_agree(monkeypatch):
    """the step do_train runs (solver.make_train_step): first step's total loss with the per-shape graph cache on and off"""
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")

    def run(mode):
        monkeypatch.setenv("CR_GRAPHS", mode)
        cfg, model, opt, syn, solver = bt.build(DEV, seed=0, lr=0.0025, extra=NONDIS)
        step = solver.make_train_step(cfg, model, opt, world_size=1)
        tot = []
        torch.manual_seed(5)
        with d2.EventStorage(0):
            for i in range(2):
                b = syn.make_batch(2, 900 + i, size=256)
                for d in b:
                    d["image"], d["instances"] = d["image"].to(DEV), d["instances"].to(DEV)
                step(b)
                tot.append(step.report()["total_loss"])
        rep = step.report()
        return tot, rep, model
    te, re_, me = run("none")
    tg, rg, mg = run("dense")
    assert me._graphed is None and mg._graphed is not None
    assert re_["iterations_explode"] == 0 and rg["iterations_explode"] == 0
    assert all(math.isfinite(t) for t in te + tg)
    assert all(k in rg for k in CUBE_KEYS)
    assert abs(tg[0] - te[0]) < 1e-3 * abs(te[0]), (tg, te)
