"""CPU: the ShuffleNetV2 x1.0 FPN backbone builds from configs/cubercnn_shufflenet_FPN.yaml with torchvision's module tree
(restated: torchvision is absent, parity unpinned) and the reference's output shapes; its padded-layout helpers round-trip."""
import importlib
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    syn = importlib.import_module("3dod_amd.synthetic")
    modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
    cfg = syn.make_cfg(os.path.join(ROOT, "configs", "cubercnn_shufflenet_FPN.yaml"),
                       overrides=["MODEL.DEVICE", "cpu", "VIS_PERIOD", 0, "log", False])
    torch.manual_seed(0)
    return cfg, modeling.build_model(cfg)


def test_config_builds():
    cfg, model = _build()
    assert cfg.MODEL.BACKBONE.NAME == "build_shufflenet_fpn_backbone"
    bu = model.backbone.bottom_up
    # torchvision's shufflenet_v2_x1_0 has 2 278 604 parameters, its classifier (1024 -> 1000 with bias) 1 025 000 of them
    assert sum(p.numel() for p in bu.parameters()) == 2278604 - 1025000 == 1253604
    assert sum(p.numel() for p in bu.conv5.parameters()) == 464 * 1024 + 2 * 1024 == 477184
    sd = bu.state_dict()
    assert len(sd) == 336
    keys = model.state_dict()
    for k, shape in (("backbone.bottom_up.conv1.0.weight", (24, 3, 3, 3)),
                     ("backbone.bottom_up.stage2.0.branch1.0.weight", (24, 1, 3, 3)),
                     ("backbone.bottom_up.stage3.1.branch2.3.weight", (116, 1, 3, 3)),
                     ("backbone.bottom_up.stage4.3.branch2.5.weight", (232, 232, 1, 1)),
                     ("backbone.bottom_up.conv5.1.running_var", (1024,)),
                     ("backbone.fpn_lateral3.weight", (256, 116, 1, 1))):
        assert k in keys, k
        assert tuple(keys[k].shape) == shape, (k, keys[k].shape)
    shapes = bu.output_shape()
    assert {k: v.channels for k, v in shapes.items()} == {'p2': 24, 'p3': 116, 'p4': 232, 'p5': 464, 'p6': 464}
    assert {k: v.stride for k, v in shapes.items()} == {'p2': 4, 'p3': 8, 'p4': 16, 'p5': 32, 'p6': 64}
    assert list(shapes.keys()) == ['p2', 'p3', 'p4', 'p5', 'p6']
    fpn_shapes = model.backbone.output_shape()
    assert list(fpn_shapes.keys()) == ['p2', 'p3', 'p4', 'p5', 'p6']          # no top block: no p7
    assert all(v.channels == 256 for v in fpn_shapes.values())
    assert model.backbone.top_block is None


def test_creation_order_and_empty_branch1():
    cfg, model = _build()
    bu = model.backbone.bottom_up
    assert list(bu._modules) == ["conv1", "maxpool", "stage2", "stage3", "stage4", "conv5"]
    assert [len(getattr(bu, s)) for s in ("stage2", "stage3", "stage4")] == [4, 8, 4]
    for s in ("stage2", "stage3", "stage4"):
        for i, u in enumerate(getattr(bu, s)):
            assert list(u._modules) == ["branch1", "branch2"]
            assert u.stride == (2 if i == 0 else 1)
            assert len(u.branch1) == (5 if i == 0 else 0), (s, i)           # stride-1 units: an empty branch1
            assert [type(m).__name__ for m in u.branch2] == ["Conv2d", "BatchNorm2d", "ReLU", "Conv2d", "BatchNorm2d", "Conv2d",
                                                             "BatchNorm2d", "ReLU"]
    assert [type(m).__name__ for m in bu.stage2[0].branch1] == ["Conv2d", "BatchNorm2d", "Conv2d", "BatchNorm2d", "ReLU"]
    dw = bu.stage3[0].branch1[0]
    assert dw.groups == 116 and dw.stride == (2, 2) and dw.padding == (1, 1) and dw.bias is None
    assert [type(m).__name__ for m in bu.conv5] == ["Conv2d", "BatchNorm2d", "ReLU"]


def test_default_initialisation():
    """torchvision applies no initialisation of its own: BatchNorm weight 1 / bias 0, conv weights kaiming_uniform(a=sqrt(5)),
    i.e. |w| <= 1 / sqrt(fan_in)"""
    cfg, model = _build()
    bu = model.backbone.bottom_up
    for m in bu.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert bool((m.weight == 1).all()) and bool((m.bias == 0).all())
            assert bool((m.running_mean == 0).all()) and bool((m.running_var == 1).all())
        elif isinstance(m, torch.nn.Conv2d):
            fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            assert float(m.weight.detach().abs().max()) <= fan_in ** -0.5 + 1e-7
            assert float(m.weight.detach().abs().max()) > 0.5 * fan_in ** -0.5
            assert m.weight.is_contiguous(memory_format=torch.channels_last)


def test_conv5_stays_out_of_the_optimizer():
    """conv5 is never run: in the reference its parameters receive no gradient and torch.optim skips them.  Here they do not
    require one, so the optimizer's parameter groups never see them (no weight decay on a zero gradient)."""
    cfg, model = _build()
    solver = importlib.import_module("3dod_amd.cubercnn.solver.build")
    bu = model.backbone.bottom_up
    conv5 = {id(p) for p in bu.conv5.parameters()}
    assert len(conv5) == 3 and not any(p.requires_grad for p in bu.conv5.parameters())
    grouped = {id(p) for p, _, _ in solver._param_groups(cfg, model)}
    assert not (conv5 & grouped)
    others = [p for n, p in bu.named_parameters() if not n.startswith("conv5.")]
    assert others and all(p.requires_grad and id(p) in grouped for p in others)


def test_padded_layout_round_trip():
    sn = importlib.import_module("3dod_amd.cubercnn.modeling.backbone.shufflenet")
    assert [sn.pad_width(c) for c in (24, 58, 116, 232)] == [32, 64, 128, 256]
    x = torch.arange(2 * 3 * 116, dtype=torch.float32).reshape(2, 3, 116) + 1
    ph = sn.to_physical(x, 2, 58)
    assert tuple(ph.shape) == (2, 3, 128)
    assert bool((ph[..., 58:64] == 0).all()) and bool((ph[..., 122:] == 0).all())
    assert torch.equal(ph[..., :58], x[..., :58]) and torch.equal(ph[..., 64:122], x[..., 58:])
    assert torch.equal(sn.to_logical(ph, 2, 58), x)


def test_trunk_fails_loudly_off_the_gpu():
    cfg, model = _build()
    lib = importlib.import_module("3dod_amd._lib")
    with pytest.raises(lib.CrError), torch.no_grad():
        model.backbone(torch.zeros(1, 64, 64, 4))
