"""Golden vectors for the 3D head trained with the NON-disentangled losses (MODEL.ROI_CUBE_HEAD.DISENTANGLED_LOSS False,
roi_heads.py:2516-2560, 2587-2591): the REFERENCE's own ROIHeads3D._forward_cube on CPU in training mode, driven like
make_golden_cubehead.py drives it (same inputs, same stand-ins, same loss weights) with disentangled_loss = False and
dims_priors_enabled = False (with the priors enabled the reference itself fails at roi_heads.py:2532).  pytorch3d's
so3_relative_angle is stood in by weak_losses.so3_relative_angle, as in make_golden_weakhead.py.

Nine files cubehead_train_nondis*.npz with the keys of cubehead_train*.npz: five depth parametrisations and four options on
'direct' (tests/cube_nondis_f64.py:CASES).  A file is only written if, recomputed in float64, (a) no absolute-difference
residual of the xy / dims / z / joint terms is within 1e-5 of zero, (b) every trace(P T^T) lies in [-1 - 1e-4, 3 + 1e-4],
and (c) the reference returned a Cube/loss_pose entry (it drops the term when so3_relative_angle raises).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cubehead_nondis.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_cubehead as M  # noqa: E402  (imports the reference under the stub finder; does not run its main())
import cube_nondis_f64 as F  # noqa: E402

M.ref_rh.so3_relative_angle = importlib.import_module("3dod_amd.cubercnn.modeling.roi_heads.weak_losses").so3_relative_angle

SEEDS = {"": 31, "_zsigmoid": 33, "_zlog": 33, "_bins3_direct": 35, "_bins3_clusters": 35, "_egocentric": 37, "_inverse_z": 38,
         "_nojoint": 39, "_l1pose": 40}


def run(seed, z_type="direct", cluster_bins=1, allocentric=True, inverse_z=False, w_joint=1.0, chamfer_pose=True):
    instances, Ks, ratios, head, priors = M.make_case(seed, True)
    K_classes = head["z"].shape[1]
    z_scales = z_stats = None
    if cluster_bins > 1:
        g2 = torch.Generator().manual_seed(seed + 100)
        n = head["z"].shape[0]
        head["z"] = torch.randn(n, cluster_bins, K_classes, 1, generator=g2) * 0.5 + (0.0 if z_type == "clusters" else 3.0)
        z_scales = torch.sort(torch.rand(K_classes, cluster_bins, generator=g2) * 250 + 20, dim=1).values
        z_stats = torch.stack((torch.rand(K_classes, cluster_bins, generator=g2) * 8 + 2,
                               torch.rand(K_classes, cluster_bins, generator=g2) * 1.5 + 0.3), dim=-1)
    if z_type == "log":
        head["z"] = head["z"] - 1.5
    elif z_type == "sigmoid":
        head["z"] = head["z"] - 6.0
    leaves = {k: v.clone().requires_grad_(True) for k, v in head.items()}
    pose = M.my_util.rotation_6d_to_matrix(leaves["pose6"].view(-1, 6)).view(leaves["pose6"].shape[0], -1, 3, 3)
    n = leaves["z"].shape[0]
    self = types.SimpleNamespace()
    cfgv = dict(in_features=["p2"], training=True, num_classes=50, scale_roi_boxes=0.0, virtual_depth=True,
                virtual_focal=512.0, cluster_bins=cluster_bins, use_confidence=1.0, dims_priors_enabled=False,
                dims_priors_func="exp", allocentric_pose=allocentric, z_type=z_type, disentangled_loss=False,
                chamfer_pose=chamfer_pose, loss_w_3d=1.0, loss_w_xy=1.0, loss_w_z=1.0, loss_w_dims=20.0, loss_w_pose=7.0,
                loss_w_joint=w_joint, inverse_z_weight=inverse_z)
    for k, v in cfgv.items():
        setattr(self, k, v)
    self.priors_dims_per_cat = priors
    if cluster_bins > 1:
        self.priors_z_scales = z_scales
        self.priors_z_stats = z_stats
    self.cube_pooler = lambda feats, boxes: torch.zeros(n, 4)
    self.cube_head = lambda x: (leaves["deltas"], leaves["z"], leaves["dims"], pose, leaves["uncert"])
    C = M.ref_rh.ROIHeads3D
    for name in ("l1_loss", "chamfer_loss", "scale_proposals", "safely_reduce_losses"):
        setattr(self, name, types.MethodType(getattr(C, name), self))
    _, losses = C._forward_cube(self, {"p2": None}, instances, Ks, [(512, 512)] * 3, ratios)
    assert "Cube/loss_pose" in losses, "the reference dropped the pose term (so3_relative_angle raised)"
    rec = {"in_" + k: v.numpy() for k, v in head.items()}
    rec["priors"] = priors.numpy()
    if cluster_bins > 1:
        rec["priors_z_scales"], rec["priors_z_stats"] = z_scales.numpy(), z_stats.numpy()
    rec["ratios"] = np.array(ratios, np.float32)
    rec["Ks"] = torch.stack(Ks).numpy()
    rec["n_per"] = np.array([len(i) for i in instances])
    rec["proposal_boxes"] = torch.cat([i.proposal_boxes.tensor for i in instances]).numpy()
    rec["pred_boxes"] = torch.cat([i.pred_boxes.tensor for i in instances]).numpy()
    rec["gt_classes"] = torch.cat([i.gt_classes for i in instances]).numpy()
    rec["gt_boxes3D"] = torch.cat([i.gt_boxes3D for i in instances]).numpy()
    rec["gt_poses"] = torch.cat([i.gt_poses for i in instances]).numpy()
    sum(losses.values()).backward()
    for k, v in losses.items():
        rec["loss_" + k.replace("/", "_")] = v.detach().numpy()
    for k, v in leaves.items():
        rec["grad_" + k] = v.grad.numpy()
    rec["notes"] = np.array("reference ROIHeads3D._forward_cube (roi_heads.py:2237-2679), training, disentangled_loss False, "
                            "dims_priors_enabled False; third-party symbols stood in (Instances/Boxes/select_foreground_proposals/"
                            "event storage/axis_angle_to_matrix/rotation_6d_to_matrix/so3_relative_angle): parity unpinned for "
                            "those, pinned for the reference's own arithmetic")
    return rec


if __name__ == "__main__":
    for suffix, (z_type, opt) in F.CASES.items():
        rec = run(SEEDS[suffix], z_type, cluster_bins=3 if "bins3" in suffix else 1, **opt)
        F.check_conditions(F.terms(rec, z_type, **opt))
        assert all(np.isfinite(v).all() for k, v in rec.items() if k.startswith(("loss_", "grad_")))
        np.savez_compressed(os.path.join(HERE, "cubehead_train_nondis%s.npz" % suffix), **rec)
        print(suffix or "(direct)", {k: float(v) for k, v in rec.items() if k.startswith("loss_")})
