"""Weakly supervised 3D head against tests/golden/weakhead_{a,b}.npz = outputs of the REFERENCE's
ROIHeads3DScore._forward_cube on the same inputs (tests/golden/make_golden_weakhead.py).  On CPU the two device kernels
are replaced by their oracle restatements (oracle/weak.py) through the head's test hooks; tests/test_gpu_weakhead.py
runs the HIP path against the same vectors."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

d2 = importlib.import_module("3dod_amd.d2lite")
syn = importlib.import_module("3dod_amd.synthetic")
util = importlib.import_module("3dod_amd.cubercnn.util.math_util")
W = importlib.import_module("3dod_amd.cubercnn.modeling.roi_heads.weak_losses")
score = importlib.import_module("3dod_amd.cubercnn.modeling.roi_heads.roi_heads_score")
rh = importlib.import_module("3dod_amd.cubercnn.modeling.roi_heads.roi_heads")

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def scene_maps(Ks, seed_gen, size=512):
    """must mirror tests/golden/make_golden_weakhead.py:scene_maps"""
    depth, ground = [], []
    for i, K in enumerate(Ks):
        f = float(K[0][0])
        v = torch.arange(size, dtype=torch.float32).view(-1, 1).expand(size, size)
        z = torch.where(v > size / 2 + 8, 1.5 * f / (v - size / 2).clamp(min=1.0), torch.full_like(v, 8.0)).clamp(max=8.0)
        z = z + torch.randn(size, size, generator=seed_gen) * 0.01
        depth.append(z)
        ground.append((v > size / 2 + 40) if i != 1 else torch.tensor([[1]]))
    depth_maps = d2.ImageList(torch.stack(depth), [(size, size)] * len(Ks))
    gt = torch.zeros(len(Ks), size, size, dtype=torch.bool)
    for i, m in enumerate(ground):
        gt[i, :m.shape[0], :m.shape[1]] = m.bool()
    return depth_maps, d2.ImageList(gt, [tuple(m.shape) for m in ground])


def replay_generator(seed, K_classes=50, n_per=(7, 1, 9)):
    """the golden script's make_case draws, in order, from one generator; replay them to reach the depth-noise draws"""
    g = torch.Generator().manual_seed(seed)
    batch = syn.make_batch(3, seed)
    for b, n in zip(batch, n_per):
        torch.randint(0, len(b["instances"]), (n,), generator=g)
        torch.randn(n, 4, generator=g)
        torch.randn(n, 4, generator=g)
    n = sum(n_per)
    for shape in ((n, K_classes, 2), (n, K_classes, 1), (n, K_classes, 3), (n, K_classes, 6), (n, K_classes)):
        torch.randn(*shape, generator=g)
    torch.rand(1, K_classes, 2, 3, generator=g)
    return g, batch


def object_masks(batch, size=512):
    """must mirror tests/golden/make_golden_weakhead.py:object_masks"""
    masks, keys = [], []
    for b in batch:
        gt = b["instances"]
        for j, (box, k) in enumerate(zip(gt.gt_boxes.tensor.tolist(), gt.gt_boxes3D[:, 0].tolist())):
            x1, y1, x2, y2 = box
            cx, cy, w, h = (x1 + x2) / 2, (y1 + y2) / 2, (x2 - x1) * 0.85, (y2 - y1) * 0.85
            m = torch.zeros(1, size, size, dtype=torch.bool)
            if j != 1:
                m[0, int(cy - h / 2):int(cy + h / 2), int(cx - w / 2):int(cx + w / 2)] = True
                m[0, int(cy - h / 2):int(cy - h / 4), int(cx - w / 2):int(cx - w / 4)] = False
            masks.append(m)
            keys.append(k)
    return masks, keys


def build_head(rec, dev, hooks):
    """an ROIHeads3DScore shell (no conv trunk: pooler and cube head are replaced by the recorded head outputs)"""
    self = score.ROIHeads3DScore.__new__(score.ROIHeads3DScore)
    torch.nn.Module.__init__(self)
    cfgv = dict(in_features=["p2"], num_classes=50, scale_roi_boxes=0.0, virtual_depth=True, virtual_focal=512.0,
                cluster_bins=1, use_confidence=1.0, dims_priors_enabled=True, dims_priors_func="exp", allocentric_pose=True,
                z_type="direct", disentangled_loss=True, chamfer_pose=True, loss_w_3d=1.0, loss_w_iou=1.0, loss_w_seg=2.5,
                loss_w_pose=7.0, loss_w_normal_vec=20.0, loss_w_z=1.0, loss_w_dims=20.0, loss_w_depth=1.0,
                inverse_z_weight=False, loss_functions=[str(x) for x in rec["loss_functions"]])
    for k, v in cfgv.items():
        setattr(self, k, v)
    self.train()
    self.priors_dims_per_cat = torch.nn.Parameter(torch.tensor(rec["priors"], device=dev))
    self._median_fn, self._plane_cls = hooks[:2]
    self._hull_fn, self._focal_fn = hooks[2:] if len(hooks) > 2 else (None, None)
    self.segmentor = None
    self._ransac_triples = [torch.as_tensor(t, device=dev) for t in rec["triples"]] if "triples" in rec else None
    return self


def run_case(name, dev, hooks):
    rec = dict(np.load(os.path.join(GOLD, name)))
    seed = int(rec["depth_seed"])
    g, batch = replay_generator(seed)
    Ks = [b["K"] for b in batch]
    depth_maps, ground_maps = scene_maps(Ks, g)
    assert [tuple(s) for s in ground_maps.image_sizes] == [tuple(s) for s in rec["ground_sizes"].tolist()]
    depth_maps = d2.ImageList(depth_maps.tensor.to(dev), depth_maps.image_sizes)
    ground_maps = d2.ImageList(ground_maps.tensor.to(dev), ground_maps.image_sizes)
    self = build_head(rec, dev, hooks)
    t = lambda k: torch.tensor(rec[k], device=dev)
    leaves = {k: t("in_" + k).requires_grad_(True) for k in ("deltas", "z", "dims", "pose6", "uncert")}
    n = leaves["z"].shape[0]
    pose = util.rotation_6d_to_matrix(leaves["pose6"].view(-1, 6)).view(n, -1, 3, 3)
    self.cube_pooler = lambda feats, boxes: torch.zeros(n, 4, device=dev)
    self.cube_head = lambda x: (leaves["deltas"], leaves["z"], leaves["dims"], pose, leaves["uncert"])
    instances, start = [], 0
    for m in rec["n_per"].tolist():
        inst = d2.Instances((512, 512))
        sl = slice(start, start + m)
        inst.proposal_boxes = d2.Boxes(t("proposal_boxes")[sl])
        inst.pred_boxes = d2.Boxes(t("pred_boxes")[sl])
        inst.gt_boxes = d2.Boxes(t("gt_boxes")[sl])
        inst.gt_classes, inst.gt_boxes3D, inst.gt_poses = t("gt_classes")[sl], t("gt_boxes3D")[sl], t("gt_poses")[sl]
        instances.append(inst)
        start += m
    Ks_t = [torch.tensor(k) for k in rec["Ks"]]
    masks = first = None
    if "with_masks" in rec and bool(rec["with_masks"]):
        mlist, keys = object_masks(batch)
        masks = [m.to(dev) for m in mlist]
        first = {}
        for k in keys:
            first.setdefault(k, len(first))
    with d2.EventStorage(1) as storage:
        pred, losses = self._forward_cube({"p2": None}, instances, Ks_t, [(512, 512)] * 3, rec["ratios"].tolist(), masks, first,
                                          ground_maps, depth_maps)
        sum(losses.values()).sum().backward()
    return rec, pred, losses, leaves


def check_case(name, dev, hooks, tol=2e-4):
    rec, pred, losses, leaves = run_case(name, dev, hooks)
    want = {k[len("loss_"):].replace("Cube_", "Cube/"): v for k, v in rec.items() if k.startswith("loss_") and k != "loss_functions"}
    assert set(losses) == set(want), (sorted(losses), sorted(want))
    for k, v in want.items():
        got = float(losses[k].detach().reshape(-1)[0])
        assert got == pytest.approx(float(np.asarray(v).reshape(-1)[0]), rel=tol, abs=tol), k
    for k, leaf in leaves.items():
        ref = rec["grad_" + k]
        g = leaf.grad.detach().cpu().numpy()
        assert np.abs(g - ref).max() <= tol * max(1.0, np.abs(ref).max()), (k, np.abs(g - ref).max(), np.abs(ref).max())
    for f in ("pred_bbox3D", "pred_center_cam", "pred_center_2D", "pred_dimensions", "pred_pose", "scores"):
        got = torch.cat([i.get(f) for i in pred]).detach().cpu().numpy()
        assert np.allclose(got, rec["out_" + f], rtol=1e-4, atol=1e-4), f


@pytest.mark.parametrize("name", ["weakhead_a.npz", "weakhead_b.npz", "weakhead_c.npz", "weakhead_d.npz"])
def test_forward_cube_matches_reference_cpu(name):
    from oracle import weak as ow
    check_case(name, torch.device("cpu"), (ow.box_median, ow.Plane, ow.hull8, ow.polygon_focal))


def test_product_path_refuses_cpu():
    lib = importlib.import_module("3dod_amd._lib")
    with pytest.raises(lib.CrError):
        check_case("weakhead_a.npz", torch.device("cpu"), (None, None))


def test_loss_pieces():
    # pose alignment: identical rotations -> 0, single-box images are skipped, all single -> None
    R = util.rotation_6d_to_matrix(torch.randn(1, 6)).expand(4, 3, 3).contiguous()
    assert float(W.pose_alignment_loss(R, [4])) == pytest.approx(0.0, abs=1e-6)
    assert W.pose_alignment_loss(R[:2], [1, 1]) is None
    two = W.pose_alignment_loss(torch.cat([R, R[:1]]), [4, 1])
    assert float(two) == pytest.approx(0.0, abs=1e-6)
    # GIoU: identical boxes 0, disjoint boxes > 1
    b = torch.tensor([[0., 0., 10., 10.]])
    assert float(W.generalized_box_iou_loss(b, b)) == pytest.approx(0.0, abs=1e-6)
    assert float(W.generalized_box_iou_loss(b, b + 100)) > 1.0
    # dims hinge: inside one sigma -> 0; NaN prior -> None
    mean, std = torch.ones(2, 3), torch.full((2, 3), 0.5)
    w, h, l = W.dim_hinge_loss(mean, std, torch.tensor([[1.2, 1.0, 2.0], [1.0, 1.0, 1.0]]))
    assert w.tolist() == [0.0, 0.0] and l.tolist() == pytest.approx([1.0, 0.0])
    assert W.dim_hinge_loss(mean, std * float("nan"), mean) == (None, None, None)
    # depth under the centre, clamped 10 px inside
    dm = d2.ImageList(torch.arange(2 * 40 * 50, dtype=torch.float32).view(2, 40, 50), [(40, 50), (30, 50)])
    z = W.pseudo_gt_z_point(dm, torch.tensor([[25.7, 20.2], [-5.0, 100.0]]), [1, 1])
    assert z.tolist() == [20 * 50 + 25.0, 40 * 50 + (30 - 11) * 50 + 10.0]
    # box medians: ordering [with area..., without area...] inside an image, lower median
    from oracle import weak as ow
    boxes = torch.tensor([[60., 5., 70., 9.], [10., 10., 13., 12.], [0., 0., 2., 2.]])      # first one lies outside the 50-wide map
    t = W.pseudo_gt_z_box(dm, boxes, [2, 1], median_fn=ow.box_median)
    win = dm.tensor[0, 10:12, 10:13].flatten().sort().values
    assert t.tolist() == [float(win[(6 - 1) // 2]), float(dm.tensor[0, 10, 39]), float(dm.tensor[1, :2, :2].flatten().sort().values[1])]
