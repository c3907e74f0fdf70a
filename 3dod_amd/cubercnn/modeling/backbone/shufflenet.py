"""ShuffleNetV2 x1.0 trunk + FPN on the HIP kernels -- cubercnn/modeling/backbone/shufflenet.py:10-69 of the reference, which
takes `torchvision.models.shufflenet_v2_x1_0(...)` [third-party, absent here: module tree, state-dict keys
(`stage3.1.branch2.3.weight`, `conv5.1.running_var`, ...) and the default PyTorch initialisation restated from its public
definition -> parity unpinned w.r.t. torchvision].  nn.Conv2d / nn.BatchNorm2d are parameter containers only.

Channel layout.  The branch widths 24 / 58 / 116 / 232 are no multiples of 16, so inside the trunk every activation lives in a
PADDED physical NHWC layout: each branch width is rounded up to the next power of two (32 / 64 / 128 / 256) and a unit's
two-half output is stored as [half 0 | pad | half 1 | pad] (physical widths 32 / 128 / 256 / 512).  Pointwise convolutions
and BatchNorms then run on the existing kernels; `x.chunk(2, 1)` is a 16-byte aligned half.  Parameters, state dict, optimizer
and output_shape() keep the logical shapes: ops.PaddedPack makes zero-padded compute copies of all of them in one launch per
forward pass and gathers their gradients back in one launch.  Pad channels are exactly zero, forward and backward.  The FPN
reads p2..p6 in the physical layout through padded copies of its lateral weights (lateral_weights()).

A stride-1 unit never splits its input: branch2's first 1x1 convolution reads the whole map through a weight whose columns
over the first half are zero, its backward-data adds the pass-through gradient in its epilogue (gradient slot), and the unit
tail (ops.shuffle_tail) writes concat + channel shuffle in one pass."""
import torch
import torch.nn as nn

from ....d2lite import BACKBONE_REGISTRY, ShapeSpec
from .... import hipops as ops
from .fpn import FPN, Backbone, to_channels_last

STAGES_REPEATS, STAGES_OUT_CHANNELS = (4, 8, 4), (24, 116, 232, 464, 1024)


def pad_width(c):
    """physical width of a branch of c logical channels: the next power of two"""
    p = 8
    while p < c:
        p *= 2
    return p


def to_physical(x, halves, wl):
    """(..., halves * wl) logical channels -> the padded layout (..., halves * pad_width(wl)); plain torch ops (tests, tools)"""
    wp = pad_width(wl)
    x = x.unflatten(-1, (halves, wl))
    return torch.nn.functional.pad(x, (0, wp - wl)).flatten(-2).contiguous()


def to_logical(x, halves, wl):
    """the logical view of a padded map: (..., halves * pad_width(wl)) -> (..., halves * wl)"""
    return x.unflatten(-1, (halves, pad_width(wl)))[..., :wl].flatten(-2)


def _bn_entries(prefix, bn, rows):
    shape = (rows[0] * rows[2],)
    ent = lambda n, grad: {"name": prefix + n, "get": (lambda m=bn, n=n: getattr(m, n)), "rows": rows, "cols": (1, 1, 1),
                           "shape": shape, "grad": grad, "bn": bn}
    return [ent("weight", True), ent("bias", True), ent("running_mean", False), ent("running_var", False)]


def _pw_entry(name, conv, rows, cols):
    """1x1 convolution (rows: output layout, cols: input layout)"""
    return {"name": name, "get": (lambda m=conv: m.weight), "rows": rows, "cols": cols,
            "shape": (rows[0] * rows[2], cols[0] * cols[2], 1, 1), "grad": True, "T": True}


def _dw_entry(name, conv, rows):
    return {"name": name, "get": (lambda m=conv: m.weight), "rows": rows, "cols": (1, 9, 9), "shape": (rows[0] * rows[2], 9),
            "grad": True}


class _Packed:
    """ops.PaddedPack over named entries: run() -> {name: padded tensor}; finish() copies the running statistics that
    train-mode BatchNorms updated in their padded copies back into the modules' buffers (one launch)"""

    def __init__(self, entries):
        self.entries = entries
        self.pack = ops.PaddedPack(entries)
        self.names = [e["name"] for e in entries]
        self.bns = []
        for e in entries:
            if "bn" in e and all(e["bn"] is not b for b in self.bns):
                self.bns.append(e["bn"])

    def run(self):
        return dict(zip(self.names, self.pack.run()))

    def finish(self):
        live = [b for b in self.bns if b.training]
        if live:
            self.pack.unpack([i for i, e in enumerate(self.entries) if not e["grad"] and any(e["bn"] is b for b in live)])


class InvertedResidual(nn.Module):
    """torchvision InvertedResidual.  in_layout: (halves, logical width) of the physical input map."""

    def __init__(self, inp, oup, stride, in_layout=None):
        super().__init__()
        if not 1 <= stride <= 2:
            raise ValueError("illegal stride value")
        self.stride = stride
        bf = oup // 2
        assert stride != 1 or inp == bf << 1
        if stride > 1:
            self.branch1 = nn.Sequential(
                nn.Conv2d(inp, inp, 3, stride, 1, groups=inp, bias=False), nn.BatchNorm2d(inp),
                nn.Conv2d(inp, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf), nn.ReLU(inplace=True))
        else:
            self.branch1 = nn.Sequential()
        self.branch2 = nn.Sequential(
            nn.Conv2d(inp if stride > 1 else bf, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf), nn.ReLU(inplace=True),
            nn.Conv2d(bf, bf, 3, stride, 1, groups=bf, bias=False), nn.BatchNorm2d(bf),
            nn.Conv2d(bf, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf), nn.ReLU(inplace=True))
        self.bf = bf
        self.in_layout = tuple(in_layout) if in_layout is not None else (2, bf)
        assert self.in_layout[0] * self.in_layout[1] == inp
        to_channels_last(self)

    def pack_entries(self, prefix=""):
        bf, (hin, win) = self.bf, self.in_layout
        row = (1, bf, pad_width(bf))
        lin = (hin, win, pad_width(win))
        b1, b2 = self.branch1, self.branch2
        ents = []
        if self.stride > 1:
            ents += [_dw_entry(prefix + "branch1.0.weight", b1[0], lin)] + _bn_entries(prefix + "branch1.1.", b1[1], lin)
            ents += [_pw_entry(prefix + "branch1.2.weight", b1[2], row, lin)] + _bn_entries(prefix + "branch1.3.", b1[3], row)
            ents += [_pw_entry(prefix + "branch2.0.weight", b2[0], row, lin)]
        else:                       # reads the whole unit input: zero columns over the first half, which passes through
            ents += [_pw_entry(prefix + "branch2.0.weight", b2[0], row, (2, bf, pad_width(bf), 1))]
        ents += _bn_entries(prefix + "branch2.1.", b2[1], row)
        ents += [_dw_entry(prefix + "branch2.3.weight", b2[3], row)] + _bn_entries(prefix + "branch2.4.", b2[4], row)
        ents += [_pw_entry(prefix + "branch2.5.weight", b2[5], row, row)] + _bn_entries(prefix + "branch2.6.", b2[6], row)
        return ents

    @staticmethod
    def _pw(x, P, k, bn, relu=True):
        return ops.conv_bn_act_live(x, P[k + ".weight"], P[bn + ".weight"], P[bn + ".bias"], P[bn + ".running_mean"],
                                    P[bn + ".running_var"], 1, 0, relu, *P["hyper"][bn])

    @staticmethod
    def _dw(x, P, k, bn, stride):
        return ops.dwconv_bn(x, P[k + ".weight"], P[bn + ".weight"], P[bn + ".bias"], P[bn + ".running_mean"],
                             P[bn + ".running_var"], stride, *P["hyper"][bn])

    def _hyper(self, prefix):
        mods = dict(self.named_modules())
        return {prefix + k: (m.eps, m.momentum, m.training) for k, m in mods.items() if isinstance(m, nn.BatchNorm2d)}

    def forward(self, x, P=None, prefix=""):
        """x: the physical input map (to_physical(logical, *in_layout)) -> the physical output (2 * pad_width(bf) channels).
        P: the padded parameters when the trunk has packed them for all units at once"""
        packed = None
        if P is None:
            packed = self.__dict__.get("_packed")
            if packed is None:
                packed = self.__dict__["_packed"] = _Packed(self.pack_entries())
            P = packed.run()
            P["hyper"] = self._hyper("")
        p = prefix
        # branch2's first convolution is created first: it is the accumulating consumer of x's gradient slot
        a = self._pw(x, P, p + "branch2.0", p + "branch2.1")
        if self.stride > 1:
            other = self._pw(self._dw(x, P, p + "branch1.0", p + "branch1.1", self.stride), P, p + "branch1.2", p + "branch1.3")
        else:
            other = x
        b = self._pw(self._dw(a, P, p + "branch2.3", p + "branch2.4", self.stride), P, p + "branch2.5", p + "branch2.6")
        out = ops.shuffle_tail(other, b, self.bf)
        if packed is not None:
            packed.finish()
        return out


class ShufflenetBackbone(Backbone):
    """shufflenet.py:10-43: p2 = maxpool(conv1(x)), p3 / p4 / p5 = stage2 / 3 / 4, p6 = max_pool2d(p5, kernel_size=1,
    stride=2).  conv5 belongs to the module and the state dict and is never run; in the reference its parameters receive no
    gradient, so the optimizer never touches them -- here they do not require one.  forward() returns PHYSICAL maps
    (see the module docstring); logical_features() is their logical view."""

    LAYOUTS = {'p2': (1, 24), 'p3': (2, 58), 'p4': (2, 116), 'p5': (2, 232), 'p6': (2, 232)}

    def __init__(self, cfg, input_shape, pretrained=False):
        super().__init__()
        c = STAGES_OUT_CHANNELS
        self.conv1 = nn.Sequential(nn.Conv2d(3, c[0], 3, 2, 1, bias=False), nn.BatchNorm2d(c[0]), nn.ReLU(inplace=True))
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        inp, layout = c[0], (1, c[0])
        for name, repeats, oup in zip(("stage2", "stage3", "stage4"), STAGES_REPEATS, c[1:4]):
            seq = [InvertedResidual(inp, oup, 2, layout)]
            seq += [InvertedResidual(oup, oup, 1) for _ in range(repeats - 1)]
            setattr(self, name, nn.Sequential(*seq))
            inp, layout = oup, (2, oup // 2)
        self.conv5 = nn.Sequential(nn.Conv2d(inp, c[4], 1, 1, 0, bias=False), nn.BatchNorm2d(c[4]), nn.ReLU(inplace=True))
        for p in self.conv5.parameters():
            p.requires_grad_(False)
        self._out_feature_channels = {'p2': 24, 'p3': 116, 'p4': 232, 'p5': 464, 'p6': 464}
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
        row = (1, 24, 32)
        return [{"name": "conv1.0.weight", "get": (lambda m=self.conv1[0]: m.weight), "rows": row, "cols": (9, 3, cin),
                 "shape": (32, 3, 3, cin), "perm": (0, 3, 1, 2), "grad": True}] + _bn_entries("conv1.1.", self.conv1[1], row)

    def _units(self):
        return [(f"{s}.{i}.", u) for s in ("stage2", "stage3", "stage4") for i, u in enumerate(getattr(self, s))]

    def _packed(self, cin, stem_only=False):
        packs = self.__dict__.setdefault("_packs", {})
        key = (cin, stem_only)
        if key not in packs:
            ents = self._stem_entries(cin)
            if not stem_only:
                for prefix, u in self._units():
                    ents += u.pack_entries(prefix)
                for f, conv in self.__dict__.get("_laterals", {}).items():
                    h, w = self.LAYOUTS[f]
                    ents.append(_pw_entry("lateral." + f, conv, (1, conv.out_channels, conv.out_channels), (h, w, pad_width(w))))
            packs[key] = _Packed(ents)
        return packs[key]

    def _hyper(self):
        return {k: (m.eps, m.momentum, m.training) for k, m in self.named_modules() if isinstance(m, nn.BatchNorm2d)}

    def _stem(self, x, P):
        y = ops.conv_bn_act_live(x, P["conv1.0.weight"], P["conv1.1.weight"], P["conv1.1.bias"], P["conv1.1.running_mean"],
                                 P["conv1.1.running_var"], 2, 1, True, *P["hyper"]["conv1.1"])
        return ops.maxpool3x3s2(y)

    def stem(self, x):
        """maxpool(conv1(x)) alone -> physical p2 (N, H/4, W/4, 32)"""
        packed = self._packed(x.shape[-1], stem_only=True)
        P = packed.run()
        P["hyper"] = self._hyper()
        out = self._stem(x, P)
        packed.finish()
        return out

    def forward(self, x):
        packed = self._packed(x.shape[-1])
        P = packed.run()
        P["hyper"] = self._hyper()
        outs = {'p2': self._stem(x, P)}
        t = outs['p2']
        for name, s in (('p3', "stage2"), ('p4', "stage3"), ('p5', "stage4")):
            for i, u in enumerate(getattr(self, s)):
                t = u(t, P, f"{s}.{i}.")
            outs[name] = t
        outs['p6'] = ops.subsample2x(t)                 # F.max_pool2d(p5, kernel_size=1, stride=2, padding=0), shufflenet.py:35
        packed.finish()
        self.__dict__["_lateral_w"] = {f: P["lateral." + f] for f in self.__dict__.get("_laterals", {})}
        return outs

    def lateral_weights(self):
        """{feature name: padded lateral weight (zero columns at pad channels)} of the latest forward pass"""
        return self.__dict__.get("_lateral_w", {})

    def logical_features(self, outs):
        """the logical view of forward()'s maps: 24 / 116 / 232 / 464 / 464 channels"""
        return {k: to_logical(v, *self.LAYOUTS[k]) for k, v in outs.items()}


@BACKBONE_REGISTRY.register()
def build_shufflenet_fpn_backbone(cfg, input_shape: ShapeSpec, priors=None):
    """shufflenet.py:46-69 (ImageNet weights cannot be fetched offline -> random init); no top block: p6 comes from the trunk."""
    bottom_up = ShufflenetBackbone(cfg, input_shape, pretrained=False)
    return FPN(bottom_up=bottom_up, in_features=cfg.MODEL.FPN.IN_FEATURES, out_channels=cfg.MODEL.FPN.OUT_CHANNELS,
               norm=cfg.MODEL.FPN.NORM, fuse_type=cfg.MODEL.FPN.FUSE_TYPE)
