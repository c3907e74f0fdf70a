"""MNASNet-1.0 trunk + FPN on the HIP kernels -- cubercnn/modeling/backbone/mnasnet.py:10-63 of the reference, which takes
`torchvision.models.mnasnet1_0(...).layers` [third-party, absent here: module tree, state-dict keys (`base.9.0.layers.3.weight`,
`base.15.running_var`, ...), BatchNorm momentum 1 - 0.9997 and the kaiming_normal(fan_out) initialisation restated from its
public definition (alpha 1.0) -> parity unpinned w.r.t. torchvision].  nn.Conv2d / nn.BatchNorm2d are parameter containers only.

Channel layout.  The widths 24 / 40 / 72 / 120 are no multiples of 16, so inside the trunk every activation lives in the PADDED
physical NHWC layout of the ShuffleNetV2 trunk with single-half maps: a width is rounded up to the next multiple of 16 (32 / 48
/ 80 / 128, everything else unchanged).  Pointwise convolutions then run on the existing kernels, depthwise 3x3 / 5x5
convolutions and every BatchNorm backward of the trunk on csrc/mnasnet.hip (cr_bn_bwd_anyc at every width: it adds the
per-channel sums across threads in double).  Parameters, state dict, optimizer
and output_shape() keep the logical shapes: ops.PaddedPack makes zero-padded compute copies of all of them in one launch per
forward pass and gathers their gradients back in one launch.  Pad channels are exactly zero, forward and backward.  The FPN
reads p2..p6 in the physical layout through padded copies of its lateral weights (lateral_weights()).

A block is three calls: expand 1x1 + BN + ReLU, depthwise k x k + BN + ReLU, project 1x1 + BN; the residual add of a stride-1
block rides in the third call's BatchNorm pass and its gradient travels through the input's gradient slot."""
import torch
import torch.nn as nn

from ....d2lite import BACKBONE_REGISTRY, ShapeSpec
from .... import hipops as ops
from .fpn import FPN, Backbone, to_channels_last
from .shufflenet import _Packed, _bn_entries, _pw_entry

BN_MOMENTUM = 1 - 0.9997
# torchvision MNASNet(alpha=1.0): (in, out, kernel, stride, expansion, repeats) of layers[8:14]
STACKS = ((16, 24, 3, 2, 3, 3), (24, 40, 5, 2, 3, 3), (40, 80, 5, 2, 6, 3), (80, 96, 3, 1, 6, 2), (96, 192, 5, 2, 6, 4),
          (192, 320, 3, 1, 6, 1))


def pad_width(c):
    """physical width of c logical channels: the next multiple of 16"""
    return (c + 15) // 16 * 16


def to_physical(x, wl):
    """(..., wl) logical channels -> the padded layout (..., pad_width(wl)); plain torch ops (tests, tools)"""
    assert x.shape[-1] == wl
    return torch.nn.functional.pad(x, (0, pad_width(wl) - wl)).contiguous()


def to_logical(x, wl):
    """the logical view of a padded map: (..., pad_width(wl)) -> (..., wl)"""
    assert x.shape[-1] == pad_width(wl)
    return x[..., :wl]


def _row(c):
    return (1, c, pad_width(c))


def _dw_entry(name, conv, rows):
    kk = conv.kernel_size[0] ** 2
    return {"name": name, "get": (lambda m=conv: m.weight), "rows": rows, "cols": (1, kk, kk), "shape": (rows[0] * rows[2], kk),
            "grad": True}


def _bn(c):
    return nn.BatchNorm2d(c, momentum=BN_MOMENTUM)


def _call_pw(x, P, k, bn, relu, residual=None):
    return ops.conv_bn_act_live(x, P[k + ".weight"], P[bn + ".weight"], P[bn + ".bias"], P[bn + ".running_mean"],
                                P[bn + ".running_var"], 1, 0, relu, *P["hyper"][bn], residual=residual, wide_sums=True)


def _call_dw(x, P, k, bn, ksize, stride):
    return ops.dwconv_bn_act(x, P[k + ".weight"], P[bn + ".weight"], P[bn + ".bias"], P[bn + ".running_mean"],
                             P[bn + ".running_var"], ksize, stride, True, *P["hyper"][bn])


class _InvertedResidual(nn.Module):
    """torchvision mnasnet._InvertedResidual: expand 1x1, depthwise k x k, project 1x1 (+ input)"""

    def __init__(self, in_ch, out_ch, kernel_size, stride, expansion_factor):
        super().__init__()
        if stride not in (1, 2):
            raise ValueError(f"stride should be 1 or 2 instead of {stride}")
        if kernel_size not in (3, 5):
            raise ValueError(f"kernel_size should be 3 or 5 instead of {kernel_size}")
        mid_ch = in_ch * expansion_factor
        self.apply_residual = in_ch == out_ch and stride == 1
        self.layers = nn.Sequential(
            nn.Conv2d(in_ch, mid_ch, 1, bias=False), _bn(mid_ch), nn.ReLU(inplace=True),
            nn.Conv2d(mid_ch, mid_ch, kernel_size, padding=kernel_size // 2, stride=stride, groups=mid_ch, bias=False),
            _bn(mid_ch), nn.ReLU(inplace=True),
            nn.Conv2d(mid_ch, out_ch, 1, bias=False), _bn(out_ch))
        self.widths = (in_ch, mid_ch, out_ch)
        self.kernel_size, self.stride = kernel_size, stride
        _init(self)
        to_channels_last(self)

    def pack_entries(self, prefix=""):
        rin, rmid, rout = (_row(c) for c in self.widths)
        L, p = self.layers, prefix + "layers."
        return ([_pw_entry(p + "0.weight", L[0], rmid, rin)] + _bn_entries(p + "1.", L[1], rmid) +
                [_dw_entry(p + "3.weight", L[3], rmid)] + _bn_entries(p + "4.", L[4], rmid) +
                [_pw_entry(p + "6.weight", L[6], rout, rmid)] + _bn_entries(p + "7.", L[7], rout))

    def _hyper(self, prefix):
        return {prefix + k: (m.eps, m.momentum, m.training) for k, m in self.named_modules() if isinstance(m, nn.BatchNorm2d)}

    def forward(self, x, P=None, prefix=""):
        """x: the physical input map (to_physical(logical, in_ch)) -> the physical output (pad_width(out_ch) channels).
        P: the padded parameters when the trunk has packed them for all blocks at once"""
        packed = None
        if P is None:
            packed = self.__dict__.get("_packed")
            if packed is None:
                packed = self.__dict__["_packed"] = _Packed(self.pack_entries())
            P = packed.run()
            P["hyper"] = self._hyper("")
        p = prefix + "layers."
        # the expansion is created first: it is the accumulating consumer of x's gradient slot, the residual add the second
        a = _call_pw(x, P, p + "0", p + "1", True)
        b = _call_dw(a, P, p + "3", p + "4", self.kernel_size, self.stride)
        out = _call_pw(b, P, p + "6", p + "7", False, x if self.apply_residual else None)
        if packed is not None:
            packed.finish()
        return out


def _stack(in_ch, out_ch, kernel_size, stride, exp_factor, repeats):
    first = _InvertedResidual(in_ch, out_ch, kernel_size, stride, exp_factor)
    return nn.Sequential(first, *[_InvertedResidual(out_ch, out_ch, kernel_size, 1, exp_factor) for _ in range(1, repeats)])


def _init(module):
    """torchvision MNASNet: kaiming_normal_(mode="fan_out", nonlinearity="relu") on conv weights, BatchNorm weight 1 / bias 0"""
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)


class MNASNetBackbone(Backbone):
    """mnasnet.py:10-38: p2 = base[0:9], p3 = base[9], p4 = base[10:12], p5 = base[12:14], p6 = max_pool2d(p5, kernel_size=1,
    stride=2).  base[14:17] (the 320 -> 1280 head convolution) belongs to the module and the state dict and is never run; in
    the reference its parameters receive no gradient, so the optimizer never touches them -- here they do not require one.
    forward() returns PHYSICAL maps (see the module docstring); logical_features() is their logical view."""

    WIDTHS = {'p2': 24, 'p3': 40, 'p4': 96, 'p5': 320, 'p6': 320}
    STAGES = {'p2': (8,), 'p3': (9,), 'p4': (10, 11), 'p5': (12, 13)}       # the stacks of a stage (p2: after the stem)

    def __init__(self, cfg, input_shape, pretrained=False):
        super().__init__()
        layers = [nn.Conv2d(3, 32, 3, padding=1, stride=2, bias=False), _bn(32), nn.ReLU(inplace=True),
                  nn.Conv2d(32, 32, 3, padding=1, stride=1, groups=32, bias=False), _bn(32), nn.ReLU(inplace=True),
                  nn.Conv2d(32, 16, 1, padding=0, stride=1, bias=False), _bn(16)]
        layers += [_stack(*s) for s in STACKS]
        layers += [nn.Conv2d(320, 1280, 1, padding=0, stride=1, bias=False), _bn(1280), nn.ReLU(inplace=True)]
        self.base = nn.Sequential(*layers)
        for m in layers[:8] + layers[14:]:              # the blocks have initialised themselves
            _init(m)
        for m in self.base[14:17]:
            for p in m.parameters():
                p.requires_grad_(False)
        self._out_feature_channels = dict(self.WIDTHS)
        self._out_feature_strides = {'p2': 4, 'p3': 8, 'p4': 16, 'p5': 32, 'p6': 64}
        self._out_features = ['p2', 'p3', 'p4', 'p5', 'p6']
        to_channels_last(self)
        for m in self.modules():                        # the optimizer's weight bank has nothing to prepare here
            if isinstance(m, nn.Conv2d):
                m.weight._cr_no_bank = True

    # ---- padded parameters -------------------------------------------------------------------------------------------
    def attach_laterals(self, laterals):
        """laterals: {feature name: the FPN's lateral nn.Conv2d}; their padded weights are made with the trunk's"""
        self.__dict__["_laterals"] = dict(laterals)
        self.__dict__["_packs"] = {}
        for conv in laterals.values():
            conv.weight._cr_no_bank = True

    def _stem_entries(self, cin):
        b = self.base
        r32, r16 = _row(32), _row(16)
        return ([{"name": "base.0.weight", "get": (lambda m=b[0]: m.weight), "rows": r32, "cols": (9, 3, cin),
                  "shape": (32, 3, 3, cin), "perm": (0, 3, 1, 2), "grad": True}] + _bn_entries("base.1.", b[1], r32) +
                [_dw_entry("base.3.weight", b[3], r32)] + _bn_entries("base.4.", b[4], r32) +
                [_pw_entry("base.6.weight", b[6], r16, r32)] + _bn_entries("base.7.", b[7], r16))

    def _blocks(self, stacks=range(8, 14)):
        return [(f"base.{i}.{j}.", blk) for i in stacks for j, blk in enumerate(self.base[i])]

    def _packed(self, cin):
        packs = self.__dict__.setdefault("_packs", {})
        if cin not in packs:
            ents = self._stem_entries(cin)
            for prefix, blk in self._blocks():
                ents += blk.pack_entries(prefix)
            for f, conv in self.__dict__.get("_laterals", {}).items():
                ents.append(_pw_entry("lateral." + f, conv, (1, conv.out_channels, conv.out_channels), _row(self.WIDTHS[f])))
            packs[cin] = _Packed(ents)
        return packs[cin]

    def _hyper(self):
        return {k: (m.eps, m.momentum, m.training) for k, m in self.named_modules() if isinstance(m, nn.BatchNorm2d)}

    def _stem(self, x, P):
        """base[0:8]: conv 3x3 / 2 + BN + ReLU, depthwise 3x3 + BN + ReLU, 1x1 to 16 channels + BN"""
        y = ops.conv_bn_act_live(x, P["base.0.weight"], P["base.1.weight"], P["base.1.bias"], P["base.1.running_mean"],
                                 P["base.1.running_var"], 2, 1, True, *P["hyper"]["base.1"], wide_sums=True)
        y = _call_dw(y, P, "base.3", "base.4", 3, 1)
        return _call_pw(y, P, "base.6", "base.7", False)

    def _stage(self, name, t, P):
        if name == 'p2':
            t = self._stem(t, P)
        for prefix, blk in self._blocks(self.STAGES[name]):
            t = blk(t, P, prefix)
        return t

    def stage(self, name, x, cin=4):
        """one stage alone ('p2': base[0:9] on the image, 'p3': base[9], 'p4': base[10:12], 'p5': base[12:14] on the physical
        map of the stage before) -> its physical output"""
        packed = self._packed(x.shape[-1] if name == 'p2' else cin)
        P = packed.run()
        P["hyper"] = self._hyper()
        out = self._stage(name, x, P)
        packed.finish()
        return out

    def forward(self, x):
        packed = self._packed(x.shape[-1])
        P = packed.run()
        P["hyper"] = self._hyper()
        outs, t = {}, x
        for name in ('p2', 'p3', 'p4', 'p5'):
            t = outs[name] = self._stage(name, t, P)
        outs['p6'] = ops.subsample2x(t)                 # F.max_pool2d(p5, kernel_size=1, stride=2, padding=0), mnasnet.py:31
        packed.finish()
        self.__dict__["_lateral_w"] = {f: P["lateral." + f] for f in self.__dict__.get("_laterals", {})}
        return outs

    def lateral_weights(self):
        """{feature name: padded lateral weight (zero columns at pad channels)} of the latest forward pass"""
        return self.__dict__.get("_lateral_w", {})

    def logical_features(self, outs):
        """the logical view of forward()'s maps: 24 / 40 / 96 / 320 / 320 channels"""
        return {k: to_logical(v, self.WIDTHS[k]) for k, v in outs.items()}


@BACKBONE_REGISTRY.register()
def build_mnasnet_fpn_backbone(cfg, input_shape: ShapeSpec, priors=None):
    """mnasnet.py:40-63 (ImageNet weights cannot be fetched offline -> random init); no top block: p6 comes from the trunk."""
    bottom_up = MNASNetBackbone(cfg, input_shape, pretrained=False)
    return FPN(bottom_up=bottom_up, in_features=cfg.MODEL.FPN.IN_FEATURES, out_channels=cfg.MODEL.FPN.OUT_CHANNELS,
               norm=cfg.MODEL.FPN.NORM, fuse_type=cfg.MODEL.FPN.FUSE_TYPE)
