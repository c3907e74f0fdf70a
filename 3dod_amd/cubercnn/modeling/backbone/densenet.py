"""DenseNet-121 trunk + FPN on the HIP kernels -- cubercnn/modeling/backbone/densenet.py:10-64 of the reference, which takes
`torchvision.models.densenet121(...).features` [third-party, absent here: module tree, initialisation and state-dict keys
(`base.denseblock3.denselayer24.conv2.weight`, `base.transition1.conv.weight`, `base.norm5.running_var`, ...) restated from
its public definition -> parity unpinned w.r.t. torchvision].  nn.Conv2d / nn.BatchNorm2d are parameter containers only.

A dense block is ONE call (ops.dense_block): a shared NHWC feature buffer that every layer reads a prefix of and appends 32
channels to, batch statistics computed once per channel (csrc/densenet.hip) -- no torch.cat, no per-layer statistics pass over
features whose statistics cannot have changed.  The transitions' norm and norm5 reuse the block's statistics table."""
from collections import OrderedDict

import torch.nn as nn

from ....d2lite import BACKBONE_REGISTRY, ShapeSpec
from .... import hipops as ops
from .fpn import FPN, Backbone, to_channels_last
from .dla import _conv_bn

GROWTH_RATE, BN_SIZE, BLOCK_CONFIG, NUM_INIT_FEATURES = 32, 4, (6, 12, 24, 16), 64


class _DenseLayer(nn.Module):
    """torchvision _DenseLayer (drop_rate 0): BN-ReLU-conv1x1 (bn_size * growth channels) -> BN-ReLU-conv3x3 (growth channels).
    The arithmetic of a whole block runs in ops.dense_block; this is its parameter container."""

    def __init__(self, num_input_features, growth_rate, bn_size):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(num_input_features)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv1 = nn.Conv2d(num_input_features, bn_size * growth_rate, kernel_size=1, stride=1, bias=False)
        self.norm2 = nn.BatchNorm2d(bn_size * growth_rate)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(bn_size * growth_rate, growth_rate, kernel_size=3, stride=1, padding=1, bias=False)


class _DenseBlock(nn.ModuleDict):
    """torchvision _DenseBlock: denselayer1..L, each reading the concatenation of the block input and all earlier outputs"""

    def __init__(self, num_layers, num_input_features, bn_size, growth_rate):
        super().__init__()
        for i in range(num_layers):
            self.add_module("denselayer%d" % (i + 1), _DenseLayer(num_input_features + i * growth_rate, growth_rate, bn_size))

    def forward(self, x):
        """-> (concatenated features, their batch-statistics table)"""
        return ops.dense_block(x, list(self.values()))


class _Transition(nn.Sequential):
    """torchvision _Transition: BN-ReLU-conv1x1 (half the channels)-AvgPool2d(2, 2)"""

    def __init__(self, num_input_features, num_output_features):
        super().__init__()
        self.norm = nn.BatchNorm2d(num_input_features)
        self.relu = nn.ReLU(inplace=True)
        self.conv = nn.Conv2d(num_input_features, num_output_features, kernel_size=1, stride=1, bias=False)
        self.pool = nn.AvgPool2d(kernel_size=2, stride=2)

    def forward(self, x, stats=None):
        a = ops.bn_act(x, self.norm, True, stats)
        return ops.avgpool2x2(ops.conv_bias_act(a, self.conv.weight, None, 1, 0))


def _densenet121_features():
    feats = nn.Sequential(OrderedDict([
        ("conv0", nn.Conv2d(3, NUM_INIT_FEATURES, kernel_size=7, stride=2, padding=3, bias=False)),
        ("norm0", nn.BatchNorm2d(NUM_INIT_FEATURES)),
        ("relu0", nn.ReLU(inplace=True)),
        ("pool0", nn.MaxPool2d(kernel_size=3, stride=2, padding=1)),
    ]))
    num_features = NUM_INIT_FEATURES
    for i, num_layers in enumerate(BLOCK_CONFIG):
        feats.add_module("denseblock%d" % (i + 1), _DenseBlock(num_layers, num_features, BN_SIZE, GROWTH_RATE))
        num_features += num_layers * GROWTH_RATE
        if i != len(BLOCK_CONFIG) - 1:
            feats.add_module("transition%d" % (i + 1), _Transition(num_features, num_features // 2))
            num_features //= 2
    feats.add_module("norm5", nn.BatchNorm2d(num_features))
    for m in feats.modules():                         # torchvision's initialisation
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight)
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
    return feats


class DenseNetBackbone(Backbone):
    """densenet.py:10-38: p2 / p3 / p4 = the raw outputs of denseblock1 / 2 / 3, p5 = norm5(denseblock4) without a ReLU,
    p6 = max_pool2d(p5, kernel_size=1, stride=2)."""

    def __init__(self, cfg, input_shape, pretrained=False):
        super().__init__()
        self.base = _densenet121_features()
        self._out_feature_channels = {'p2': 256, 'p3': 512, 'p4': 1024, 'p5': 1024, 'p6': 1024}
        self._out_feature_strides = {'p2': 4, 'p3': 8, 'p4': 16, 'p5': 32, 'p6': 64}
        self._out_features = ['p2', 'p3', 'p4', 'p5', 'p6']
        to_channels_last(self)

    def stem(self, x):
        b = self.base
        return ops.maxpool3x3s2(_conv_bn(x, b.conv0, b.norm0, relu=True))

    def forward(self, x):
        b = self.base
        p2, s1 = b.denseblock1(self.stem(x))
        p3, s2 = b.denseblock2(b.transition1(p2, s1))
        p4, s3 = b.denseblock3(b.transition2(p3, s2))
        d4, s4 = b.denseblock4(b.transition3(p4, s3))
        p5 = ops.bn_act(d4, b.norm5, False, s4)
        p6 = ops.subsample2x(p5)                       # F.max_pool2d(p5, kernel_size=1, stride=2, padding=0), densenet.py:31
        return {'p2': p2, 'p3': p3, 'p4': p4, 'p5': p5, 'p6': p6}


@BACKBONE_REGISTRY.register()
def build_densenet_fpn_backbone(cfg, input_shape: ShapeSpec, priors=None):
    """densenet.py:41-64 (ImageNet weights cannot be fetched offline -> random init); no top block: p6 comes from the trunk."""
    bottom_up = DenseNetBackbone(cfg, input_shape, pretrained=False)
    return FPN(bottom_up=bottom_up, in_features=cfg.MODEL.FPN.IN_FEATURES, out_channels=cfg.MODEL.FPN.OUT_CHANNELS,
               norm=cfg.MODEL.FPN.NORM, fuse_type=cfg.MODEL.FPN.FUSE_TYPE)
