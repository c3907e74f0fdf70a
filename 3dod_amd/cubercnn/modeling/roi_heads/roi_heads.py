"""ROIHeads3D -- the stock Cube R-CNN 2D+3D head, cubercnn/modeling/roi_heads/roi_heads.py:1948-2851 of the
reference, on top of a detectron2 StandardROIHeads stand-in [third-party, restated].

Heavy ops: ROIAlign over the FPN pyramid (cr_roi_align_*), FC layers (library GEMM, bf16).  The per-RoI
decode and the disentangled corner losses are small float32 torch expressions on the device (n <= 128 FG
RoIs per image)."""
import os
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ....d2lite import (ROI_HEADS_REGISTRY, ROI_BOX_HEAD_REGISTRY, Boxes, Instances, ShapeSpec, Matcher, cat,
                        pairwise_iou, pairwise_ioa, get_event_storage)
from .... import hipops as ops
from ....hipops import pose_type_code, dims_func_code, pooler_type_code
from ...util import math_util as util
from ..backbone.fpn import c2_xavier_fill, to_channels_last
from .cube_head import build_cube_head, fc_nhwc
from .fast_rcnn import FastRCNNOutputs

E_CONSTANT = 2.71828183
SQRT_2_CONSTANT = 1.41421356
bf16 = torch.bfloat16


def build_roi_heads(cfg, input_shape, priors=None):
    """roi_heads.py:72-77."""
    name = cfg.MODEL.ROI_HEADS.NAME
    return ROI_HEADS_REGISTRY.get(name)(cfg, input_shape, priors=priors)


class ROIPooler(nn.Module):
    """detectron2 ROIPooler [third-party]: level assignment + pooling, fused in one kernel.  POOLER_TYPE ROIAlignV2 (the
    reference's config), ROIAlign or ROIPool; POOLER_SAMPLING_RATIO 0 (adaptive grid) or a fixed number of samples per bin
    and axis (ROIPool has no sampling grid and ignores it).  ROIAlignRotated is not built.
    Output is (R, out, out, C) bf16 -- NHWC, flattened by the heads in (h,w,c) order."""

    def __init__(self, output_size, scales, sampling_ratio, pooler_type):
        super().__init__()
        pooler_type_code(pooler_type, sampling_ratio)          # ValueError naming the built values
        if pooler_type == "ROIPool" and os.environ.get("CR_DETERMINISTIC", "0") not in ("", "0"):
            raise ValueError("POOLER_TYPE ROIPool is not built for CR_DETERMINISTIC=1: its backward adds with float32 atomics, "
                             "which fix no order; the bit-reproducible poolers are ROIAlignV2 and ROIAlign")
        self.output_size = output_size
        self.scales = tuple(scales)
        self.pooler_type = pooler_type
        self.sampling_ratio = sampling_ratio

    def options(self):
        """the ops.roi_align_pyramid keywords of POOLER_TYPE / POOLER_SAMPLING_RATIO, each passed only when it differs from
        its default: the CPU stand-in of the op (oracle/cpu_backend.py) states the default pooler and has no such arguments"""
        opt = {}
        if self.pooler_type != "ROIAlignV2":
            opt["pooler_type"] = self.pooler_type
        if self.sampling_ratio != 0 and self.pooler_type != "ROIPool":
            opt["sampling_ratio"] = self.sampling_ratio
        return opt

    def pool(self, x: List[torch.Tensor], rois):
        """rois (R,5) [image index, x1,y1,x2,y2] over the maps x (fine -> coarse)"""
        return ops.roi_align_pyramid(x, rois, self.scales, self.output_size, **self.options())

    def forward(self, x: List[torch.Tensor], box_lists: List[Boxes]):
        rois = cat([torch.cat([b.tensor.new_full((len(b), 1), i), b.tensor], 1) for i, b in enumerate(box_lists)], 0)
        return self.pool(x, rois)


BOX_HEAD_NORMS = ("", "GN")


@ROI_BOX_HEAD_REGISTRY.register()
class FastRCNNConvFCHead(nn.Sequential):
    """detectron2 FastRCNNConvFCHead [third-party, restated]: NUM_CONV x (conv 3x3 pad 1 -> norm -> relu), flatten,
    NUM_FC x (fc -> relu).  conv_norm "" (convolutions with bias, ReLU in the conv epilogue) or "GN" (bias-free convolutions,
    each with its own torch.nn.GroupNorm(32, CONV_DIM) registered as `conv{k}.norm`).  The convolutions run on the cr_conv2d_*
    kernels over the RoI tiles as a batch (N = RoIs, H = W = pooler resolution)."""

    def __init__(self, input_shape: ShapeSpec, *, conv_dims, fc_dims, conv_norm=""):
        super().__init__()
        if conv_norm not in BOX_HEAD_NORMS:
            raise ValueError('built: MODEL.ROI_BOX_HEAD.NORM "" / "GN"; got NORM "{}"'.format(conv_norm))
        if len(fc_dims) == 0:
            raise ValueError("built: MODEL.ROI_BOX_HEAD.NUM_FC >= 1 (the predictors read a flat feature); got NUM_FC 0")
        self._output_size = (input_shape.channels, input_shape.height, input_shape.width)
        self.conv_norm_relus = []
        for k, conv_dim in enumerate(conv_dims):
            cin = self._output_size[0]
            pow2 = lambda v: v >= 8 and v & (v - 1) == 0
            if not (pow2(cin) and pow2(conv_dim) and conv_dim % 16 == 0 and (conv_norm == "" or conv_dim % 32 == 0)):
                raise ValueError("built: MODEL.ROI_BOX_HEAD.CONV_DIM (and the pooled channel count) a power of two >= 16 -- the "
                                 "3x3 convolution kernels take a power-of-two input width in both directions and Cout % 16 == 0"
                                 "{}; got conv{} {} -> {}".format(", GroupNorm(32) C % 32 == 0" if conv_norm else "", k + 1, cin,
                                                                  conv_dim))
            conv = nn.Conv2d(cin, conv_dim, kernel_size=3, padding=1, bias=conv_norm == "")
            if conv_norm == "GN":
                conv.norm = nn.GroupNorm(32, conv_dim)
            self.add_module("conv{}".format(k + 1), conv)
            self.conv_norm_relus.append(conv)
            self._output_size = (conv_dim, self._output_size[1], self._output_size[2])
        # fc1's weight columns keep the reference's (c,h,w) order over the NHWC-flattened map it is applied to
        self._in_chw = self._output_size
        self._conv_norm = conv_norm
        self.fcs = []
        for k, fc_dim in enumerate(fc_dims):
            fc = nn.Linear(int(np.prod(self._output_size)), fc_dim)
            self.add_module("fc{}".format(k + 1), fc)
            self.add_module("fc_relu{}".format(k + 1), nn.ReLU())
            self.fcs.append(fc)
            self._output_size = fc_dim
        for layer in self.conv_norm_relus:             # fvcore c2_msra_fill
            nn.init.kaiming_normal_(layer.weight, mode="fan_out", nonlinearity="relu")
            if layer.bias is not None:
                nn.init.constant_(layer.bias, 0)
        for layer in self.fcs:
            c2_xavier_fill(layer)
        to_channels_last(self)

    def forward(self, x):
        """x (R, H, W, C) bf16."""
        for conv in self.conv_norm_relus:
            if self._conv_norm == "GN":
                n = conv.norm
                x = ops.conv_gn_act(x, conv.weight, (n.weight, n.bias, n.num_groups, n.eps), 1, 1, relu=True)
            else:
                x = ops.conv_bias_act(x, conv.weight, conv.bias, 1, 1, relu=True)
        h = fc_nhwc(x.flatten(1), self.fcs[0], self._in_chw, relu=True)
        for fc in self.fcs[1:]:
            h = ops.linear(h, fc.weight, fc.bias, relu=True)
        return h

    @property
    def output_shape(self):
        return ShapeSpec(channels=self._output_size)


def select_foreground_proposals(proposals, bg_label):
    fg_proposals, fg_selection_masks = [], []
    for proposals_per_image in proposals:
        gt_classes = proposals_per_image.gt_classes
        fg_selection_mask = (gt_classes != -1) & (gt_classes != bg_label)
        fg_idxs = fg_selection_mask.nonzero().squeeze(1)
        fg_proposals.append(proposals_per_image[fg_idxs])
        fg_selection_masks.append(fg_selection_mask)
    return fg_proposals, fg_selection_masks


class StandardROIHeads(nn.Module):
    def __init__(self, *, num_classes, batch_size_per_image, positive_fraction, proposal_matcher,
                 proposal_append_gt=True, box_in_features, box_pooler, box_head, box_predictor,
                 train_on_pred_boxes=False, **kwargs):
        super().__init__()
        self.num_classes = num_classes
        self.batch_size_per_image = batch_size_per_image
        self.positive_fraction = positive_fraction
        self.proposal_matcher = proposal_matcher
        self.proposal_append_gt = proposal_append_gt
        self.in_features = self.box_in_features = box_in_features
        self.box_pooler = box_pooler
        self.box_head = box_head
        self.box_predictor = box_predictor
        self.train_on_pred_boxes = train_on_pred_boxes

    @classmethod
    def from_config(cls, cfg, input_shape):
        in_features = cfg.MODEL.ROI_HEADS.IN_FEATURES
        pooler_resolution = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        pooler_scales = tuple(1.0 / input_shape[k].stride for k in in_features)
        in_channels = [input_shape[f].channels for f in in_features]
        assert len(set(in_channels)) == 1, in_channels
        in_channels = in_channels[0]
        box_pooler = ROIPooler(output_size=pooler_resolution, scales=pooler_scales,
                               sampling_ratio=cfg.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO,
                               pooler_type=cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE)
        shape = ShapeSpec(channels=in_channels, height=pooler_resolution, width=pooler_resolution)
        head_cls = ROI_BOX_HEAD_REGISTRY.get(cfg.MODEL.ROI_BOX_HEAD.NAME)
        box_head = head_cls(shape, conv_dims=[cfg.MODEL.ROI_BOX_HEAD.CONV_DIM] * cfg.MODEL.ROI_BOX_HEAD.NUM_CONV,
                            fc_dims=[cfg.MODEL.ROI_BOX_HEAD.FC_DIM] * cfg.MODEL.ROI_BOX_HEAD.NUM_FC,
                            conv_norm=cfg.MODEL.ROI_BOX_HEAD.NORM)
        return {
            "num_classes": cfg.MODEL.ROI_HEADS.NUM_CLASSES,
            "batch_size_per_image": cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE,
            "positive_fraction": cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION,
            "proposal_matcher": Matcher(cfg.MODEL.ROI_HEADS.IOU_THRESHOLDS, cfg.MODEL.ROI_HEADS.IOU_LABELS,
                                        allow_low_quality_matches=False),
            "proposal_append_gt": cfg.MODEL.ROI_HEADS.PROPOSAL_APPEND_GT,
            "box_in_features": in_features,
            "box_pooler": box_pooler,
            "box_head": box_head,
            "box_predictor": None,
            "train_on_pred_boxes": cfg.MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES,
        }


@ROI_HEADS_REGISTRY.register()
class ROIHeads3D(StandardROIHeads):
    def __init__(self, cfg, input_shape: Dict[str, ShapeSpec], priors=None):
        ret = StandardROIHeads.from_config(cfg, input_shape)
        ret["box_predictor"] = FastRCNNOutputs(cfg, ret["box_head"].output_shape)
        super().__init__(**ret)
        c = cfg.MODEL.ROI_CUBE_HEAD
        self.scale_roi_boxes = c.SCALE_ROI_BOXES
        self.allocentric_pose = c.ALLOCENTRIC_POSE
        self.chamfer_pose = c.CHAMFER_POSE
        self.virtual_depth = c.VIRTUAL_DEPTH
        self.virtual_focal = c.VIRTUAL_FOCAL
        self.loss_w_3d = c.LOSS_W_3D
        self.loss_w_xy = c.LOSS_W_XY
        self.loss_w_z = c.LOSS_W_Z
        self.loss_w_dims = c.LOSS_W_DIMS
        self.loss_w_pose = c.LOSS_W_POSE
        self.loss_w_joint = c.LOSS_W_JOINT
        self.disentangled_loss = c.DISENTANGLED_LOSS
        self.inverse_z_weight = c.INVERSE_Z_WEIGHT
        self.test_scale = cfg.INPUT.MIN_SIZE_TEST
        self.ignore_thresh = cfg.MODEL.RPN.IGNORE_THRESHOLD
        self.z_type = c.Z_TYPE
        self.pose_type = c.POSE_TYPE
        self.use_confidence = c.USE_CONFIDENCE
        self.cluster_bins = c.CLUSTER_BINS
        self.dims_priors_enabled = c.DIMS_PRIORS_ENABLED
        self.dims_priors_func = c.DIMS_PRIORS_FUNC
        if self.z_type not in ('direct', 'sigmoid', 'log', 'clusters'):
            raise ValueError("built: Z_TYPE 'direct' / 'sigmoid' / 'log' / 'clusters'; got Z_TYPE '{}'".format(self.z_type))
        if not self.disentangled_loss and self.dims_priors_enabled:
            # roi_heads.py:2532 divides gt_dims (n,3) by the stacked prior mean / std (n,2,3): a broadcasting error for n > 2
            raise ValueError("DISENTANGLED_LOSS False is built with DIMS_PRIORS_ENABLED False only: with DIMS_PRIORS_ENABLED True "
                             "the reference itself fails (roi_heads.py:2532), so there is nothing to reproduce")
        if self.z_type == 'clusters' and self.cluster_bins <= 1:
            raise ValueError('To use z_type of priors, there must be more than 1 cluster bin')       # roi_heads.py:2044
        if self.use_confidence < 0:
            raise ValueError("USE_CONFIDENCE is the weight of the uncertainty term: >= 0, got {}".format(self.use_confidence))
        if self.loss_w_3d > 0:
            pose_type_code(self.pose_type)           # raise on values the kernels do not decode, naming the built set
            if self.dims_priors_enabled:
                dims_func_code(self.dims_priors_func)
        if self.loss_w_3d > 0:
            in_features = cfg.MODEL.ROI_HEADS.IN_FEATURES
            pooler_scales = tuple(1.0 / input_shape[k].stride for k in in_features)
            self.cube_pooler = ROIPooler(output_size=c.POOLER_RESOLUTION, scales=pooler_scales,
                                         sampling_ratio=c.POOLER_SAMPLING_RATIO, pooler_type=c.POOLER_TYPE)
            in_channels = [input_shape[f].channels for f in in_features][0]
            shape = ShapeSpec(channels=in_channels, width=c.POOLER_RESOLUTION, height=c.POOLER_RESOLUTION)
            self.cube_head = build_cube_head(cfg, shape)
            if self.dims_priors_enabled and priors is not None:
                self.priors_dims_per_cat = nn.Parameter(torch.FloatTensor(priors['priors_dims_per_cat']).unsqueeze(0))
            else:
                self.priors_dims_per_cat = nn.Parameter(torch.ones(1, self.num_classes, 2, 3))
            # the depth can be clustered by the 2D scale of the box (roi_heads.py:2032-2051): scale centres per (class, bin) and,
            # for Z_TYPE 'clusters', the depth mean / std of every cluster
            bins = priors.get('priors_bins') if (priors is not None and self.cluster_bins > 1) else None
            if bins is not None:
                self.priors_z_scales = nn.Parameter(torch.stack([torch.FloatTensor(prior[1]) for prior in bins]))
            else:
                self.priors_z_scales = nn.Parameter(torch.ones(self.num_classes, self.cluster_bins))
            if self.z_type == 'clusters':
                if bins is None:
                    self.priors_z_stats = nn.Parameter(torch.ones(self.num_classes, self.cluster_bins, 2).float())
                else:
                    self.priors_z_stats = nn.Parameter(torch.cat([torch.FloatTensor(prior[2]).unsqueeze(0) for prior in bins]))

    def cube_options(self):
        """the ops.cube_head_loss / ops.cube_decode_infer keywords of POSE_TYPE, USE_CONFIDENCE 0 and DIMS_PRIORS_FUNC, each
        passed only when it differs from its default: the CPU stand-in of these ops (oracle/cpu_backend.py) states the default
        family and has no such arguments, so it raises instead of computing something else"""
        opt = {}
        if self.pose_type != '6d':
            opt["pose_type"] = self.pose_type
        if not self.use_confidence > 0:
            opt["use_conf"] = False
        if self.dims_priors_enabled and self.dims_priors_func != 'exp':
            opt["dims_func"] = self.dims_priors_func
            opt["priors_std"] = self.priors_dims_per_cat.detach()[0, :, 1, :].contiguous()
        return opt

    def z_cfg(self):
        """how a RoI's depth is read from the predictor output (ops.z_config): Z_TYPE, CLUSTER_BINS and the cluster tables"""
        return ops.z_config(self.z_type, self.cluster_bins, self.priors_z_scales if self.cluster_bins > 1 else None,
                            getattr(self, "priors_z_stats", None))

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def label_and_sample_proposals(self, proposals: List[Instances], targets: List[Instances]) -> List[Instances]:
        """roi_heads.py:2773-2840 under its reference name and signature, computed by the fused kernels of the static-shape
        path (dense_train.roi_label_and_sample: ground truth appended, IoU matching, ignore rule, IoU-weighted sampling of
        <= 25 % foreground up to BATCH_SIZE_PER_IMAGE): per image an Instances with `proposal_boxes`, `gt_classes`
        (num_classes = background) and, for images with objects, every `gt_*` field of the matched target.  Foreground
        rows come first.  `objectness_logits` is not carried (nothing downstream reads it)."""
        from ..dense_train import GTBatch, roi_label_and_sample
        dev = proposals[0].proposal_boxes.tensor.device
        B, P = len(proposals), max(1, max(len(p) for p in proposals))
        boxes = torch.zeros((B, P, 4), device=dev)
        scores = torch.full((B, P), float("-inf"), device=dev)
        for i, p in enumerate(proposals):
            boxes[i, :len(p)] = p.proposal_boxes.tensor
            scores[i, :len(p)] = p.objectness_logits.clamp(min=-3.0e38) if p.has("objectness_logits") else 0.0
        gt = GTBatch(targets, dev)
        samp = roi_label_and_sample(self, boxes, scores, gt)
        out = []
        for i, t in enumerate(targets):
            keep = samp["valid"][i]
            inst = Instances(proposals[i].image_size)
            inst.proposal_boxes = Boxes(samp["boxes"][i][keep])
            inst.gt_classes = samp["classes"][i][keep]
            if int((t.gt_classes >= 0).sum()) > 0:
                gi = samp["gt_idx"][i][keep].long()       # GTBatch keeps the target order (ignore rows stay addressable)
                for name, value in t.get_fields().items():
                    if name.startswith("gt_") and not inst.has(name):
                        inst.set(name, value[gi])
            out.append(inst)
        return out

    def forward(self, images, features, proposals, Ks, im_scales_ratio, targets=None):
        """roi_heads.py:2116-2157.  images: ImageList (only sizes are used)."""
        im_dims = [tuple(s) for s in images.image_sizes]
        if self.training:
            # Training runs on the static-shape path (modeling/dense_train.py behind RCNN3D.dense_train): matching, ignore
            # rule and IoU-weighted sampling are fused kernels there.  The per-image Instances-list formulation of
            # label_and_sample_proposals (roi_heads.py:2737-2840 of the reference) is test infrastructure: it lives in
            # oracle/list_path.py and is attached by oracle.list_path.install(roi_heads) (tests only).
            if not hasattr(self, "_forward_cube_list") and self.loss_w_3d > 0 and type(self)._forward_cube is ROIHeads3D._forward_cube:
                raise RuntimeError("ROIHeads3D.forward(training) on proposal lists: use the static-shape path "
                                   "(model.dense_train = True); the list formulation is oracle/list_path.py")
            proposals = self.label_and_sample_proposals(proposals, targets)
            losses = self._forward_box(features, proposals)
            if self.loss_w_3d > 0:
                instances_3d, losses_cube = self._forward_cube(features, proposals, Ks, im_dims, im_scales_ratio)
                losses.update(losses_cube)
            else:
                instances_3d = None
            return instances_3d, losses
        if isinstance(proposals, list) and not np.any([isinstance(p, Instances) for p in proposals]):
            pred_instances = []
            for proposal, im_dim in zip(proposals, im_dims):
                pred_instances_i = Instances(im_dim)
                pred_instances_i.pred_boxes = Boxes(proposal['gt_bbox2D'])
                pred_instances_i.pred_classes = proposal['gt_classes']
                pred_instances_i.scores = torch.ones_like(proposal['gt_classes']).float()
                pred_instances.append(pred_instances_i)
        else:
            fused = self._infer_padded(features, proposals, Ks, im_dims, im_scales_ratio)
            if fused is not None:
                return fused, {}
            pred_instances = self._forward_box(features, proposals)
        if self.loss_w_3d > 0:
            pred_instances = self._forward_cube(features, pred_instances, Ks, im_dims, im_scales_ratio)
        return pred_instances, {}

    def _infer_padded(self, features, proposals, Ks, im_dims, im_scales_ratio):
        """inference on the RPN's padded proposal slots (every image P slots, empty ones with objectness -inf) with ONE host wait
        at the end: box head -> ops.det_select (softmax, threshold, decode + clip, class-wise NMS, top detections: fast_rcnn.py:
        57-116 as five launches) -> the 3D head on the (B, D) padded detections (_forward_cube's inference branch, roi_heads.py:
        2353-2436, 2682-2735) -> the counts come to the host and the Instances are cut from the padded arrays.  Returns None
        when the inputs are not of that form, or when an image has more candidates than the selection looks at and too few
        survivors among them (ops.det_select's overflow flag): the caller then takes the per-image path."""
        import os
        bp = self.box_predictor
        # (CLS_AGNOSTIC_BBOX_REG takes the per-image route, fast_rcnn_inference: ops.det_select accepts 4-wide deltas, but this route
        # has no test with that option)
        if (os.environ.get("CR_INFER_FUSED", "1") == "0" or not proposals or getattr(self, "_forward_cube_list", None) is not None
                or getattr(bp, "cls_agnostic_bbox_reg", False)
                or not all(isinstance(p, Instances) and p.has("objectness_logits") for p in proposals)):
            return None
        B, P = len(proposals), len(proposals[0])
        D = int(bp.test_topk_per_image)
        pb = torch.cat([p.proposal_boxes.tensor for p in proposals])
        if P == 0 or not pb.is_cuda or any(len(p) != P for p in proposals) or not (0 < D <= 512):
            return None
        dev = pb.device
        K = self.num_classes
        feats = [features[f] for f in self.box_in_features]
        predictions = bp(self.box_head(self.box_pooler(feats, [x.proposal_boxes for x in proposals])))
        obj = torch.cat([p.objectness_logits for p in proposals]).float()
        hw = torch.tensor([[float(s[0]), float(s[1])] for s in im_dims], dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
        t = bp.box2box_transform
        ob, osc, ocls, orow, ofull, ocnt = ops.det_select(predictions[0], predictions[1], pb, obj, hw, B, P, K, t.weights, t.scale_clamp,
                                                          bp.test_score_thresh, bp.test_nms_thresh, D)
        out = None
        if self.loss_w_3d > 0:
            flat = Boxes(ob.view(B * D, 4))
            scaled = self.scale_proposals([flat])[0].tensor
            idx = torch.arange(B, device=dev).repeat_interleave(D)
            rois = torch.cat([idx[:, None].float(), scaled], 1)
            cube_features = self.cube_pooler.pool([features[f] for f in self.in_features], rois).flatten(1)
            raw, layout = self.cube_head.forward_fused(cube_features)
            rows = []
            for k, r, d in zip(Ks, im_scales_ratio, im_dims):
                k = torch.as_tensor(k, dtype=torch.float32)
                v2r = util.compute_virtual_scale_from_focal_spaces(float(k[1, 1]), float(d[0]) * float(r), self.virtual_focal,
                                                                   float(d[0])) if self.virtual_depth else 1.0
                rows.append([float(k[0, 0]) / r, float(k[1, 1]) / r, float(k[0, 2]) / r, float(k[1, 2]) / r, float(v2r), float(r)])
            meta6 = torch.tensor(rows, dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
            priors = self.priors_dims_per_cat.detach()[0, :, 0, :].contiguous() if self.dims_priors_enabled else None
            out = ops.cube_decode_infer(raw, layout, K, ocls.reshape(-1), idx, flat.tensor, meta6, priors,
                                        allocentric=self.allocentric_pose, z_cfg=self.z_cfg(), **self.cube_options()).view(B, D, 42)
            score3 = (osc * out[:, :, 8]) ** (1 / 2)
        counts = ocnt.tolist()                                   # the one host wait of the step
        if any(c[1] for c in counts):
            return None
        results = []
        for b in range(B):
            n = counts[b][0]
            inst = Instances(im_dims[b])
            inst.pred_boxes = Boxes(ob[b, :n])
            inst.scores_full = ofull[b, :n]
            inst.pred_classes = ocls[b, :n]
            if out is None:
                inst.scores = osc[b, :n]
            else:
                o = out[b, :n]
                inst.scores = score3[b, :n]
                inst.pred_bbox3D = o[:, 18:42].reshape(n, 8, 3)
                inst.pred_center_cam = o[:, 0:3]
                inst.pred_center_2D = o[:, 6:8]
                inst.pred_dimensions = o[:, 3:6]
                inst.pred_pose = o[:, 9:18].reshape(n, 3, 3)
            results.append(inst)
        return results

    def _forward_box(self, features, proposals):
        """roi_heads.py:2160-2204."""
        feats = [features[f] for f in self.box_in_features]
        box_features = self.box_pooler(feats, [x.proposal_boxes for x in proposals])
        box_features = self.box_head(box_features)
        predictions = self.box_predictor(box_features)
        del box_features
        if self.training:
            losses = self.box_predictor.losses(predictions, proposals)
            pred_boxes = self.box_predictor.predict_boxes_for_gt_classes(predictions, proposals)
            for proposals_per_image, pred_boxes_per_image in zip(proposals, pred_boxes):
                proposals_per_image.pred_boxes = Boxes(pred_boxes_per_image)
            return losses
        pred_instances, _ = self.box_predictor.inference(predictions, proposals)
        return pred_instances

    def l1_loss(self, vals, target):
        return torch.abs(vals - target)          # F.smooth_l1_loss(beta=0, reduction='none'), roi_heads.py:2206-2207

    def chamfer_loss(self, vals, target):
        """roi_heads.py:2209-2215."""
        B = vals.shape[0]
        xx = vals.view(B, 8, 1, 3)
        yy = target.view(B, 1, 8, 3)
        l1_dist = (xx - yy).abs().sum(-1)
        return l1_dist.min(1).values.mean(-1) + l1_dist.min(2).values.mean(-1)

    def scale_proposals(self, proposal_boxes):
        """roi_heads.py:2217-2235 (including its use of the width for the height)."""
        if self.scale_roi_boxes > 0:
            out = []
            for boxes in proposal_boxes:
                centers = boxes.get_centers()
                widths = boxes.tensor[:, 2] - boxes.tensor[:, 0]
                heights = boxes.tensor[:, 2] - boxes.tensor[:, 0]
                x1 = centers[:, 0] - 0.5 * widths * self.scale_roi_boxes
                x2 = centers[:, 0] + 0.5 * widths * self.scale_roi_boxes
                y1 = centers[:, 1] - 0.5 * heights * self.scale_roi_boxes
                y2 = centers[:, 1] + 0.5 * heights * self.scale_roi_boxes
                out.append(Boxes(torch.stack([x1, y1, x2, y2], dim=1)))
            return out
        return proposal_boxes

    # ------------------------------------------------------------------ cube branch
    def _forward_cube(self, features, instances, Ks, im_current_dims, im_scales_ratio):
        """roi_heads.py:2237-2735.  Inference: one ROIAlign over the kept detections, the shared FCs + one predictor GEMM and
        the fused decode kernel (`_infer_cube_fused`).  Training runs on the static-shape path (dense_train.cube_head_losses);
        the per-image Instances-list formulation written like the reference (torch expressions, used by the golden tests as the
        CPU statement of the same arithmetic) is test infrastructure: oracle/cube_list.py, attached by
        oracle.list_path.install_heads()."""
        listed = getattr(self, "_forward_cube_list", None)
        if self.training or not all(b.pred_boxes.tensor.is_cuda for b in instances):
            if listed is None:
                raise RuntimeError("ROIHeads3D._forward_cube on instance lists in training mode / on CPU tensors: the product "
                                   "trains on the static-shape path (model.dense_train = True) and has no CPU path; the list "
                                   "formulation is oracle/cube_list.py")
            if self.training and not self.disentangled_loss:
                raise RuntimeError("the list formulation (oracle/cube_list.py) states the disentangled losses only; "
                                   "DISENTANGLED_LOSS False trains on the static-shape path (dense_train.cube_head_losses)")
            return listed(features, instances, Ks, im_current_dims, im_scales_ratio)
        boxes = [x.pred_boxes for x in instances]
        if sum(len(b) for b in boxes) == 0:
            return instances                          # roi_heads.py:2278-2279: nothing to decode
        return self._infer_cube_fused([features[f] for f in self.in_features], instances, self.scale_proposals(boxes), boxes,
                                      torch.cat([x.pred_classes for x in instances]), Ks, im_current_dims, im_scales_ratio)

    def _infer_cube_fused(self, feats, instances, boxes_scaled, boxes, box_classes, Ks, im_current_dims, im_scales_ratio):
        """inference decode + packing (roi_heads.py:2353-2436, 2682-2735) on the fused path: one ROIAlign, the shared
        FCs + one predictor GEMM, one decode kernel (cr_cube_decode_infer, or cr_cube_decode_infer_param off the default pose
        type / confidence / prior function); the torch expressions of _forward_cube stay the CPU / oracle statement of the same
        arithmetic (tests/test_gpu_model.py compares the two).  Column 8 of the decode is the 3D score factor: exp(-uncertainty),
        or with USE_CONFIDENCE 0 what the reference's merge reads there, the projected centre's y (roi_heads.py:2693-2716)."""
        dev = feats[0].device
        counts = [len(b) for b in boxes]
        n = sum(counts)
        idx = torch.repeat_interleave(torch.arange(len(counts), device=dev), torch.tensor(counts, device=dev))
        rois = torch.cat([idx[:, None].float(), torch.cat([b.tensor for b in boxes_scaled])], 1)
        cube_features = self.cube_pooler.pool(feats, rois).flatten(1)
        raw, layout = self.cube_head.forward_fused(cube_features)
        rows = []
        for k, r, d in zip(Ks, im_scales_ratio, im_current_dims):
            k = torch.as_tensor(k, dtype=torch.float32)
            v2r = util.compute_virtual_scale_from_focal_spaces(float(k[1, 1]), float(d[0]) * float(r), self.virtual_focal,
                                                               float(d[0])) if self.virtual_depth else 1.0
            rows.append([float(k[0, 0]) / r, float(k[1, 1]) / r, float(k[0, 2]) / r, float(k[1, 2]) / r, float(v2r), float(r)])
        meta6 = torch.tensor(rows, dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
        priors = self.priors_dims_per_cat.detach()[0, :, 0, :].contiguous() if self.dims_priors_enabled else None
        out = ops.cube_decode_infer(raw, layout, self.num_classes, box_classes, idx, torch.cat([b.tensor for b in boxes]),
                                    meta6, priors, allocentric=self.allocentric_pose, z_cfg=self.z_cfg(), **self.cube_options())
        for inst, o, cls_i in zip(instances, out.split(counts), box_classes.split(counts)):
            m = o.shape[0]
            inst.scores = (inst.scores * o[:, 8]) ** (1 / 2) if inst.has('scores') else o[:, 8]
            if not inst.has('pred_classes'):
                inst.pred_classes = cls_i
            inst.pred_bbox3D = o[:, 18:42].reshape(m, 8, 3)
            inst.pred_center_cam = o[:, 0:3]
            inst.pred_center_2D = o[:, 6:8]
            inst.pred_dimensions = o[:, 3:6]
            inst.pred_pose = o[:, 9:18].reshape(m, 3, 3)
        return instances

    def safely_reduce_losses(self, loss, absent_if_none=False):
        """roi_heads.py:2843-2851: mean over the finite entries; with none, `loss.mean()*0.0` exactly like the
        reference (NaN for NaN/Inf input, which its divergence guard then catches).  Branch-free on the device.
        absent_if_none: the reference drops the joint loss entirely in that case (roi_heads.py:2676) -> 0."""
        valid = (~(loss.isinf())) & (~(loss.isnan()))
        cnt = valid.sum()
        s = torch.where(valid, loss, torch.zeros_like(loss)).sum()
        none = s * 0.0 if absent_if_none else loss.mean() * 0.0
        return torch.where(cnt > 0, s / cnt.clamp(min=1), none)
