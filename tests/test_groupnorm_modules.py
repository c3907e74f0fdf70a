"""CPU: structure of the GroupNorm options -- FPN(norm="GN") and FastRCNNConvFCHead(conv_norm="GN") (detectron2's public
definitions restated: state-dict keys, shapes, which layers carry a bias, the norm modules), the values that are not built, and
that configs/cubercnn_DLA34_FPN_GN.yaml builds a model whose norm parameters get SOLVER.WEIGHT_DECAY_NORM.  No kernel runs."""
import importlib
import os

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
d2 = importlib.import_module("3dod_amd.d2lite")
fpn_mod = importlib.import_module("3dod_amd.cubercnn.modeling.backbone.fpn")
rh_mod = importlib.import_module("3dod_amd.cubercnn.modeling.roi_heads.roi_heads")


class StubTrunk(fpn_mod.Backbone):
    CH = {"p2": 64, "p3": 128, "p4": 256, "p5": 512}

    def __init__(self):
        super().__init__()
        self._out_features = list(self.CH)
        self._out_feature_channels = dict(self.CH)
        self._out_feature_strides = {k: 2 ** (i + 2) for i, k in enumerate(self.CH)}


def make_fpn(norm, fuse_type="sum"):
    return fpn_mod.FPN(StubTrunk(), ["p2", "p3", "p4", "p5"], 256, norm=norm, top_block=fpn_mod.LastLevelMaxPool(),
                       fuse_type=fuse_type)


PLAIN_KEYS = sorted("fpn_{}{}.{}".format(kind, s, p) for kind in ("lateral", "output") for s in (2, 3, 4, 5)
                    for p in ("weight", "bias"))


def test_fpn_without_norm_keeps_its_keys():
    fpn = make_fpn("")
    assert sorted(fpn.state_dict().keys()) == PLAIN_KEYS
    assert all(c.bias is not None and not hasattr(c, "norm") for c in fpn.lateral_convs + fpn.output_convs)


def test_fpn_gn_structure():
    torch.manual_seed(0)
    fpn = make_fpn("GN")
    sd = fpn.state_dict()
    want = {}
    for s, cin in zip((2, 3, 4, 5), (64, 128, 256, 512)):
        want["fpn_lateral{}.weight".format(s)] = (256, cin, 1, 1)
        want["fpn_output{}.weight".format(s)] = (256, 256, 3, 3)
        for kind in ("lateral", "output"):
            want["fpn_{}{}.norm.weight".format(kind, s)] = (256,)
            want["fpn_{}{}.norm.bias".format(kind, s)] = (256,)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    for c in fpn.lateral_convs + fpn.output_convs:
        assert c.bias is None
        assert isinstance(c.norm, nn.GroupNorm) and c.norm.num_groups == 32 and c.norm.num_channels == 256
        assert bool((c.norm.weight == 1).all()) and bool((c.norm.bias == 0).all())
        assert c.weight.is_contiguous(memory_format=torch.channels_last)
        # c2_xavier_fill = kaiming_uniform_(a=1): |w| <= sqrt(3 / fan_in)
        fan_in = c.weight[0].numel()
        assert float(c.weight.detach().abs().max()) <= (3.0 / fan_in) ** 0.5 + 1e-7
    assert list(fpn.output_shape().keys()) == ["p2", "p3", "p4", "p5", "p6"]
    assert make_fpn("GN", "avg")._fuse_type == "avg"


@pytest.mark.parametrize("norm", ["BN", "SyncBN", "LN"])
def test_fpn_other_norms_raise(norm):
    with pytest.raises(ValueError) as e:
        make_fpn(norm)
    assert '""' in str(e.value) and '"GN"' in str(e.value) and norm in str(e.value)


def make_head(conv_dims, fc_dims, conv_norm, channels=256):
    return rh_mod.FastRCNNConvFCHead(d2.ShapeSpec(channels=channels, height=7, width=7), conv_dims=conv_dims, fc_dims=fc_dims,
                                     conv_norm=conv_norm)


def test_box_head_gn_structure():
    torch.manual_seed(0)
    head = make_head([256, 256], [1024], "GN")
    want = {"conv1.weight": (256, 256, 3, 3), "conv1.norm.weight": (256,), "conv1.norm.bias": (256,),
            "conv2.weight": (256, 256, 3, 3), "conv2.norm.weight": (256,), "conv2.norm.bias": (256,),
            "fc1.weight": (1024, 256 * 7 * 7), "fc1.bias": (1024,)}
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == want
    for conv in (head.conv1, head.conv2):
        assert conv.bias is None and conv.padding == (1, 1) and conv.kernel_size == (3, 3)
        assert isinstance(conv.norm, nn.GroupNorm) and conv.norm.num_groups == 32
        # c2_msra_fill = kaiming_normal_(fan_out, relu): std = sqrt(2 / (Cout * 9))
        std = (2.0 / (256 * 9)) ** 0.5
        assert abs(float(conv.weight.detach().std()) / std - 1.0) < 0.02
    assert head.fcs == [head.fc1] and head.output_shape.channels == 1024
    assert head._in_chw == (256, 7, 7)


def test_box_head_plain_convs_have_a_bias_and_change_fc1_width():
    head = make_head([64], [1024], "")
    assert sorted(head.state_dict().keys()) == ["conv1.bias", "conv1.weight", "fc1.bias", "fc1.weight"]
    assert bool((head.conv1.bias == 0).all()) and not hasattr(head.conv1, "norm")
    assert tuple(head.fc1.weight.shape) == (1024, 64 * 7 * 7) and head._in_chw == (64, 7, 7)
    # NUM_CONV 0: today's head
    assert sorted(make_head([], [1024, 1024], "").state_dict().keys()) == ["fc1.bias", "fc1.weight", "fc2.bias", "fc2.weight"]


def test_box_head_values_that_are_not_built_raise():
    with pytest.raises(ValueError) as e:
        make_head([256], [1024], "LN")
    assert '""' in str(e.value) and '"GN"' in str(e.value) and "LN" in str(e.value)
    with pytest.raises(ValueError) as e:
        make_head([96, 96], [1024], "GN")
    assert "power of two" in str(e.value) and "96" in str(e.value)
    with pytest.raises(ValueError) as e:
        make_head([96], [1024], "")
    assert "power of two" in str(e.value)
    with pytest.raises(ValueError) as e:
        make_head([256], [], "GN")
    assert "NUM_FC" in str(e.value)


def test_gn_config_builds_and_norm_parameters_take_the_norm_weight_decay():
    syn = importlib.import_module("3dod_amd.synthetic")
    modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
    sb = importlib.import_module("3dod_amd.cubercnn.solver.build")
    cfg = syn.make_cfg(os.path.join(ROOT, "configs", "cubercnn_DLA34_FPN_GN.yaml"),
                       overrides=["MODEL.DEVICE", "cpu", "VIS_PERIOD", 0, "log", False, "SOLVER.WEIGHT_DECAY_NORM", 0.0625])
    assert cfg.MODEL.FPN.NORM == "GN" and cfg.MODEL.ROI_BOX_HEAD.NORM == "GN"
    assert cfg.MODEL.ROI_BOX_HEAD.NUM_CONV == 4 and cfg.MODEL.ROI_BOX_HEAD.NUM_FC == 1
    assert cfg.MODEL.BACKBONE.NAME == "build_dla_from_vision_fpn_backbone"
    model = modeling.build_model(cfg)
    names = {id(p): n for n, p in model.named_parameters()}
    wd = {names[id(p)]: w for p, _, w in sb._param_groups(cfg, model)}
    gn = [n for n in wd if ".norm." in n]
    levels = len(cfg.MODEL.FPN.IN_FEATURES)                  # a lateral and an output norm per level, 4 box-head norms
    assert len(gn) == 2 * (2 * levels + 4), gn               # weight and bias each
    assert all(n.startswith("backbone.fpn_") or n.startswith("roi_heads.box_head.conv") for n in gn)
    assert all(wd[n] == 0.0625 for n in gn), {n: wd[n] for n in gn}
    assert wd["roi_heads.box_head.conv1.weight"] == cfg.SOLVER.WEIGHT_DECAY
    assert isinstance(model.roi_heads.box_head.conv4.norm, nn.GroupNorm)
    assert "roi_heads.box_head.fc2.weight" not in wd and "roi_heads.box_head.conv1.bias" not in wd
