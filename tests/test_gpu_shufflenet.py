"""GPU: the ShuffleNetV2 x1.0 trunk (cubercnn/modeling/backbone/shufflenet.py) on the kernels of csrc/shufflenet.hip.

torchvision is absent, so the reference here is a float64 restatement of torchvision's shufflenet_v2_x1_0 from plain
functionals (F.conv2d(..., groups=c), F.batch_norm, F.relu, chunk, cat, view / transpose for the shuffle, F.max_pool2d) over the
module's own state dict ("parity unpinned" w.r.t. torchvision).  Everything is compared in LOGICAL channels: the trunk's padded
physical maps go through shufflenet.to_logical first, and their pad channels must be exactly zero.

Bounds.  Kernels in isolation: the project's float32 module bound, 2e-5 relative L2 and 2e-4 max-norm; a bf16 output that is one
round-to-nearest of a float32 result: |got - ref| <= 2^-8 |ref| + 1e-6 max|ref|.  Units, trunk stages and gradients: the method of
tests/test_gpu_dla_types.py -- the restatement also runs in float32 on the CPU, its relative L2 distance from float64 is
`ref32_err`, and the product must stay within K_FWD * ref32_err (outputs, running statistics) or K_GRAD * ref32_err (gradients)
with that file's constants.  Every ratio is printed.  The unit tail only moves values: it is compared bit for bit.

Measured on MI355X.  Depthwise kernels (f32 outputs, weight gradients, statistics rows): relative L2 <= 1.4e-7, max-norm <= 3.1e-7;
bf16 outputs: worst |got - ref| - bound = -1.1e-6.  Units (ratio = error / ref32_err): output 1.00 .. 1.08 in train, frozen and eval
mode (K_FWD 2.966), running statistics 0.50 .. 0.91, gradients 0.74 .. 1.88 in train and 0.53 .. 1.64 in frozen mode (K_GRAD
2.31).  Trunk stages: 0.89 .. 1.09 in train and 0.91 .. 0.99 in eval mode; after load_state_dict 1.09, after an optimizer step 1.05.
The gradient of branch2.4.bias in train mode is zero in exact arithmetic (a per-channel shift ahead of a 1x1 convolution and a
train-mode BatchNorm is removed by that BatchNorm's mean): both the product and the float32 restatement leave rounding noise
there, relative errors of 1e8 against a float64 value of 1e-16, ratios 1.04 .. 1.28."""
import importlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16

K_FWD = 2.966          # tests/test_gpu_dla_types.py
K_GRAD = 2.31
L2_F32, MX_F32 = 2e-5, 2e-4
MOMENTUM, EPS = 0.1, 1e-5


def _mods():
    return (importlib.import_module("3dod_amd.cubercnn.modeling.backbone.shufflenet"),
            importlib.import_module("3dod_amd.cubercnn.modeling.backbone.fpn"),
            importlib.import_module("3dod_amd.hipops"), importlib.import_module("3dod_amd._lib"))


@pytest.fixture(autouse=True)
def fp32_mode():
    ops = importlib.import_module("3dod_amd.hipops")
    prev = ops.set_precision("fp32")
    yield
    ops.set_precision(prev)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _rel(got, ref):
    got, ref = got.detach().to("cpu", f64), ref.detach().to("cpu", f64)
    return float((got - ref).norm() / (ref.norm() + 1e-300)), float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def _bf16_excess(got, ref):
    got, ref = got.detach().to("cpu", f64), ref.detach().to("cpu", f64)
    return float(((got - ref).abs() - (2.0 ** -8 * ref.abs() + 1e-6 * ref.abs().max())).max())


def _randomise_bn(module, gen):
    """BatchNorm affine and running statistics as in test_blocks_against_float64 of tests/test_gpu_dla_types.py"""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=gen) + 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement: torchvision's shufflenet_v2_x1_0 from functionals over a state dict `p` (any dtype).  `new` (a dict)
# receives the running statistics every train-mode BatchNorm leaves behind.
# ---------------------------------------------------------------------------------------------------------------------
def _bn(t, p, k, training, new):
    rm, rv = p[k + ".running_mean"].detach().clone(), p[k + ".running_var"].detach().clone()
    y = F.batch_norm(t, rm, rv, p[k + ".weight"], p[k + ".bias"], training, MOMENTUM, EPS)
    if new is not None:
        new[k + ".running_mean"], new[k + ".running_var"] = rm, rv
    return y


def _channel_shuffle(x, groups=2):
    n, c, h, w = x.shape
    return x.view(n, groups, c // groups, h, w).transpose(1, 2).contiguous().view(n, c, h, w)


def _ref_unit(p, pre, x, stride, training, new=None):
    dw = lambda t, k: F.conv2d(t, p[k], None, stride, 1, 1, t.shape[1])

    def branch2(t):
        t = F.relu(_bn(F.conv2d(t, p[pre + "branch2.0.weight"]), p, pre + "branch2.1", training, new))
        t = _bn(dw(t, pre + "branch2.3.weight"), p, pre + "branch2.4", training, new)
        return F.relu(_bn(F.conv2d(t, p[pre + "branch2.5.weight"]), p, pre + "branch2.6", training, new))

    if stride == 1:
        x1, x2 = x.chunk(2, 1)
        out = torch.cat((x1, branch2(x2)), 1)
    else:
        t = _bn(dw(x, pre + "branch1.0.weight"), p, pre + "branch1.1", training, new)
        t = F.relu(_bn(F.conv2d(t, p[pre + "branch1.2.weight"]), p, pre + "branch1.3", training, new))
        out = torch.cat((t, branch2(x)), 1)
    return _channel_shuffle(out, 2)


STAGES = ["stem", "stage2", "stage3", "stage4"]
REPEATS = {"stage2": 4, "stage3": 8, "stage4": 4}


def _ref_stage(p, stage, x, training, new=None):
    if stage == "stem":
        t = F.relu(_bn(F.conv2d(x, p["conv1.0.weight"], None, 2, 1), p, "conv1.1", training, new))
        return F.max_pool2d(t, 3, 2, 1)
    for i in range(REPEATS[stage]):
        x = _ref_unit(p, f"{stage}.{i}.", x, 2 if i == 0 else 1, training, new)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# 1. the depthwise kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(2, 5, 7), (2, 6, 10), (1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", [24, 72, 256])
def test_depthwise_against_float64(C, shape, stride, dtype):
    """C = 24 and 72 are 3 and 9 channel groups of 8 (a partial workgroup column), 256 is two full ones; odd extents give
    stride-2 outputs of 3 x 4; a 1 x 1 map is all halo; (2, 6, 10) at stride 1 is M = 120 = two statistics rows, the second partial."""
    sn, fpn, ops, lib = _mods()
    N, H, W = shape
    gen = torch.Generator().manual_seed(100 * C + 10 * H + stride)
    exact = (lambda t: t.to(bf16).to(f32)) if dtype == bf16 else (lambda t: t)
    x = exact(torch.randn(N, C, H, W, generator=gen))
    w = torch.randn(C, 1, 3, 3, generator=gen) * 0.4
    bias = torch.randn(C, generator=gen)
    x64, w64 = x.to(f64).requires_grad_(True), w.to(f64).requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, stride, 1, 1, C)
    Ho, Wo = y64.shape[2], y64.shape[3]
    assert (Ho, Wo) == ((H - 1) // stride + 1, (W - 1) // stride + 1)
    dy = exact(torch.randn(N, C, Ho, Wo, generator=gen))
    acc = exact(torch.randn(N, C, H, W, generator=gen))
    dx64, dw64 = torch.autograd.grad((y64 * dy.to(f64)).sum(), [x64, w64])
    M = N * Ho * Wo
    tag = f"dw C={C} {shape} s{stride} {'bf16' if dtype == bf16 else 'f32'}"

    xg, wg, dyg = _nhwc(x).to(DEV, dtype), w.to(DEV), _nhwc(dy).to(DEV, dtype)
    nparts = (M + 63) // 64
    stats = torch.full((nparts, 2, C), float("nan"), device=DEV)
    y = ops.dwconv3x3_fwd_raw(xg, wg, stride, stats=stats)
    assert y.dtype == dtype and tuple(y.shape) == (N, Ho, Wo, C)
    yb = ops.dwconv3x3_fwd_raw(xg, wg, stride, bias=bias.to(DEV))
    dx = ops.dwconv3x3_bwd_data_raw(dyg, wg, xg.shape, stride)
    dxa = ops.dwconv3x3_bwd_data_raw(dyg, wg, xg.shape, stride, accumulate=_nhwc(acc).to(DEV, dtype))
    dw_new = torch.full((C, 3, 3), float("nan"), device=DEV)
    lib.call("cr_dwconv3x3_bwd_weight", dyg, xg, dw_new, N, H, W, C, stride, 0, int(dtype == f32),
             torch.empty(ops.dw_wgrad_splits(M) * C * 9, device=DEV), ops.dw_wgrad_splits(M) * C * 9)
    sink0 = torch.randn(C, 3, 3, generator=gen)
    sink = sink0.to(DEV).clone()
    assert ops.dwconv3x3_bwd_weight_raw(dyg, xg, stride, sink=sink) is None
    dw_ret = ops.dwconv3x3_bwd_weight_raw(dyg, xg, stride)

    y64n, dx64n = _nhwc(y64.detach()), _nhwc(dx64)
    figures = []
    if dtype == bf16:
        for name, got, ref in (("out", y, y64n), ("out+bias", yb, y64n + bias.to(f64)), ("dx", dx, dx64n),
                               ("dx+acc", dxa, dx64n + _nhwc(acc).to(f64))):
            ex = _bf16_excess(got, ref)
            print(f"{tag} {name}: worst |got - ref| - bound = {ex:.3g}")
            assert ex <= 0.0, (tag, name, ex)
    else:
        figures += [("out",) + _rel(y, y64n), ("out+bias",) + _rel(yb, y64n + bias.to(f64)), ("dx",) + _rel(dx, dx64n),
                    ("dx+acc",) + _rel(dxa, dx64n + _nhwc(acc).to(f64))]
    dw_ref = dw64.reshape(C, 3, 3)
    figures += [("dw written",) + _rel(dw_new, dw_ref), ("dw returned",) + _rel(dw_ret, dw_ref),
                ("dw added",) + _rel(sink.cpu().to(f64) - sink0.to(f64), dw_ref)]
    # statistics rows: the per-channel sums of the STORED output
    assert bool(torch.isfinite(stats).all()), "a statistics entry was not written"
    st = stats.to("cpu", f64).sum(0)
    ys = y.to("cpu", f64).reshape(M, C)
    mean, var = ys.mean(0), ys.var(0, unbiased=False)
    figures.append(("mean",) + _rel(st[0] / M, mean))
    m2 = (ys * ys).mean(0)
    figures.append(("E[y^2]",) + _rel(st[1] / M, m2))
    var_err = float(((st[1] / M - (st[0] / M) ** 2) - var).abs().max() / (m2.max() + 1e-300))
    print(f"{tag} var: max error / max E[y^2] {var_err:.3g}")
    assert var_err < MX_F32
    if nparts > 1:                                          # the rows are per 64 pixels in order
        figures.append(("stats row 0",) + _rel(stats[0, 0], ys[:64].sum(0)))
        figures.append(("stats row 1",) + _rel(stats[1, 0], ys[64:128].sum(0)))
    for name, l2, mx in figures:
        print(f"{tag} {name}: rel L2 {l2:.3g}, max-norm {mx:.3g}")
    for name, l2, mx in figures:
        assert l2 < L2_F32 and mx < MX_F32, (tag, name, l2, mx)


def test_depthwise_arguments_are_checked():
    sn, fpn, ops, lib = _mods()
    with pytest.raises(lib.CrError):
        ops.dwconv3x3_fwd_raw(torch.zeros(1, 4, 4, 12, device=DEV), torch.zeros(12, 3, 3, device=DEV), 1)     # C % 8 != 0
    x, w = torch.zeros(1, 4, 4, 16, device=DEV), torch.zeros(16, 3, 3, device=DEV)
    with pytest.raises(lib.CrError):
        ops.dwconv3x3_fwd_raw(x, w, 3)
    with pytest.raises(lib.CrError):
        lib.call("cr_dwconv3x3_bwd_data", x, w, torch.zeros_like(x), 1, 4, 4, 16, 3, 1, None)
    with pytest.raises(lib.CrError):                         # a workspace that is too small
        lib.call("cr_dwconv3x3_bwd_weight", x, x, torch.zeros_like(w), 1, 4, 4, 16, 1, 0, 1, torch.zeros(8, device=DEV), 8)
    with pytest.raises(lib.CrError):
        ops.dwconv3x3_fwd_raw(torch.zeros(1, 4, 4, 16), w.cpu(), 1)                                            # no CPU path


# ---------------------------------------------------------------------------------------------------------------------
# 2. the unit tail
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["passthrough", "two_branches"])
def test_unit_tail(kind, dtype):
    """out = channel_shuffle(cat(a, relu(bn(b)))) at logical bf = 58 (physical halves of 64): the BatchNorm + ReLU is the pass
    that precedes the tail (cr_bn_fwd), the tail moves values -- bit-exact, pads exactly zero; so is its backward against
    autograd of the restatement.  M = 2 * 3 * 11 = 66 pixels x 16 channel groups is more than one workgroup."""
    sn, fpn, ops, lib = _mods()
    bf, wp = 58, 64
    gen = torch.Generator().manual_seed(7)
    N, H, W = 2, 3, 11
    a = torch.randn(N, bf, H, W, generator=gen).to(dtype)
    b_raw = torch.randn(N, bf, H, W, generator=gen)
    gamma, beta = torch.rand(bf, generator=gen) + 0.5, torch.randn(bf, generator=gen) * 0.1
    b = F.relu(F.batch_norm(b_raw, None, None, gamma, beta, True, MOMENTUM, EPS)).to(dtype)
    R = torch.randn(N, 2 * bf, H, W, generator=gen).to(dtype)
    a_l, b_l = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = _channel_shuffle(torch.cat((a_l, b_l), 1), 2)
    da_ref, db_ref = torch.autograd.grad((ref.float() * R.float()).sum(), [a_l, b_l])
    bg = sn.to_physical(_nhwc(b), 1, bf).to(DEV).requires_grad_(True)
    if kind == "passthrough":          # a = the first half of the unit's input; the second half is something else entirely
        junk = torch.randn(N, bf, H, W, generator=gen).to(dtype)
        ag = sn.to_physical(_nhwc(torch.cat((a, junk), 1)), 2, bf).to(DEV).requires_grad_(True)
    else:
        ag = sn.to_physical(_nhwc(a), 1, bf).to(DEV).requires_grad_(True)
    out = ops.shuffle_tail(ag, bg, bf)
    assert tuple(out.shape) == (N, H, W, 2 * wp) and out.dtype == dtype
    assert torch.equal(sn.to_logical(out, 2, bf).cpu(), _nhwc(ref.detach()))
    assert bool((out[..., bf:wp] == 0).all()) and bool((out[..., wp + bf:] == 0).all()), "pad channels are not zero"
    dag, dbg = torch.autograd.grad(out, [ag, bg], sn.to_physical(_nhwc(R), 2, bf).to(DEV))
    assert torch.equal(dbg[..., :bf].cpu(), _nhwc(db_ref)) and bool((dbg[..., bf:] == 0).all())
    assert torch.equal(dag[..., :bf].cpu(), _nhwc(da_ref)) and bool((dag[..., bf:] == 0).all())
    assert tuple(dag.shape) == tuple(ag.shape)


def test_unit_tail_arguments_are_checked():
    sn, fpn, ops, lib = _mods()
    a, b = torch.zeros(1, 2, 2, 64, device=DEV), torch.zeros(1, 2, 2, 64, device=DEV)
    with pytest.raises(lib.CrError):
        ops.shuffle_tail(a, b, 65)                           # bf > wp
    with pytest.raises(lib.CrError):
        ops.shuffle_tail(torch.zeros(1, 2, 2, 60, device=DEV), torch.zeros(1, 2, 2, 60, device=DEV), 58)     # wp % 8 != 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. units against float64
# ---------------------------------------------------------------------------------------------------------------------
UNIT_CASES = {"s2_24to116": (24, 116, 2, (1, 24), (2, 6, 10)), "s1_116": (116, 116, 1, (2, 58), (2, 4, 4)),
              "s1_232": (232, 232, 1, (2, 116), (2, 4, 4))}


def _unit_reference(unit, x, R, stride, training, grad, dtype):
    p = {k: v.detach().clone().to(dtype) for k, v in unit.state_dict().items() if "num_batches" not in k}
    names = [k for k in p if "running" not in k]
    leaves = [p[k].requires_grad_(grad) for k in names]
    xr = x.to(dtype).requires_grad_(grad)
    new = {}
    out = _ref_unit(p, "", xr, stride, training, new)
    grads = torch.autograd.grad((out * R.to(dtype)).sum(), [xr] + leaves) if grad else ()
    return out.detach(), new, dict(zip(["x"] + names, grads)), names


def _run_unit(case, mode, seed=21):
    sn, fpn, ops, lib = _mods()
    inp, oup, stride, layout, (N, H, W) = UNIT_CASES[case]
    training, grad = mode == "train", mode != "eval"
    torch.manual_seed(seed)
    unit = sn.InvertedResidual(inp, oup, stride, layout)
    _randomise_bn(unit, torch.Generator().manual_seed(seed + 1))
    gen = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(N, inp, H, W, generator=gen)
    R = torch.randn(N, oup, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=gen)
    ref64 = _unit_reference(unit, x, R, stride, training, grad, f64)
    ref32 = _unit_reference(unit, x, R, stride, training, grad, f32)
    unit = unit.to(DEV)
    unit.train(training)
    xg = sn.to_physical(_nhwc(x), *layout).to(DEV).requires_grad_(grad)
    params = dict(unit.named_parameters())
    with torch.set_grad_enabled(grad):
        out = unit(xg)
    got_g = {}
    if grad:
        names = ref64[3]
        gs = torch.autograd.grad((sn.to_logical(out, 2, oup // 2) * _nhwc(R).to(DEV)).sum(), [xg] + [params[k] for k in names])
        got_g = dict(zip(["x"] + names, gs))
        gx = got_g["x"]
        pad = gx.unflatten(-1, (layout[0], sn.pad_width(layout[1])))[..., layout[1]:]
        assert bool((pad == 0).all()), "the input gradient's pad channels are not zero"
        got_g["x"] = _nchw(sn.to_logical(gx, *layout))
    return unit, out, got_g, ref64, ref32


@pytest.mark.parametrize("mode", ["train", "frozen", "eval"])
@pytest.mark.parametrize("case", list(UNIT_CASES))
def test_unit_against_float64(case, mode):
    """output, every BatchNorm's running statistics after one call and the gradients of the input and every parameter under a
    random cotangent, each within K * ref32_err of float64; frozen / eval: the running statistics keep their bits"""
    sn, fpn, ops, lib = _mods()
    unit, out, got_g, ref64, ref32 = _run_unit(case, mode)
    oup = UNIT_CASES[case][1]
    bf, wp = oup // 2, sn.pad_width(oup // 2)
    training = mode == "train"
    assert tuple(out.shape)[3] == 2 * wp and out.dtype == f32
    assert bool((out[..., bf:wp] == 0).all()) and bool((out[..., wp + bf:] == 0).all()), "pad channels are not zero"
    rows = [("out", K_FWD, _rel(_nchw(sn.to_logical(out, 2, bf)), ref64[0])[0], _rel(ref32[0], ref64[0])[0])]
    sd = unit.state_dict()
    assert len(ref64[1]) == 2 * (5 if UNIT_CASES[case][2] == 2 else 3)
    for k, v in ref64[1].items():
        if training:
            rows.append((k, K_FWD, _rel(sd[k], v)[0], _rel(ref32[1][k], v)[0]))
        else:
            assert torch.equal(sd[k].cpu().to(f64), v), f"{k} changed in {mode} mode"
    for k, g in got_g.items():
        assert tuple(g.shape) == tuple(ref64[2][k].shape), (k, g.shape)
        rows.append(("grad " + k, K_GRAD, _rel(g, ref64[2][k])[0], _rel(ref32[2][k], ref64[2][k])[0]))
    for name, K, err, r32 in rows:
        print(f"unit {case} {mode} {name}: error {err:.3g}, ref32_err {r32:.3g}, ratio {err / max(r32, 1e-300):.3f}")
    for name, K, err, r32 in rows:
        assert err <= K * r32, (case, mode, name, err, r32, err / max(r32, 1e-300), K)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the trunk stage by stage, 5. stale compute copies
# ---------------------------------------------------------------------------------------------------------------------
def _stage_refs(sd, x):
    """per mode and stage: the float64 input, the float64 result and ref32_err of the float32 CPU restatement"""
    p64 = {k: v.to(f64) for k, v in sd.items() if "num_batches" not in k}
    p32 = {k: v.to(f32) for k, v in p64.items()}
    refs = {}
    with torch.no_grad():
        for training in (True, False):
            t = x.to(f64)
            for stage in STAGES:
                o64 = _ref_stage(p64, stage, t, training)
                o32 = _ref_stage(p32, stage, t.to(f32), training)
                refs[(training, stage)] = (t, o64, _rel(o32, o64)[0])
                t = o64
    return refs


@pytest.fixture(scope="module")
def trunk():
    sn, fpn, ops, lib = _mods()
    torch.manual_seed(31)
    net = sn.ShufflenetBackbone(None, None)
    _randomise_bn(net, torch.Generator().manual_seed(32))
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(33))
    return net.to(DEV), sd0, _stage_refs(sd0, x), x


LAYOUT_IN = {"stage2": (1, 24), "stage3": (2, 58), "stage4": (2, 116)}
LAYOUT_OUT = {"stem": (1, 24), "stage2": (2, 58), "stage3": (2, 116), "stage4": (2, 232)}


def _gpu_stage(net, stage, xin):
    """xin: the stage's logical NCHW input -> its logical NHWC output"""
    sn, fpn, ops, lib = _mods()
    x = _nhwc(xin.to(f32))
    if stage == "stem":                                  # the RGB stem reads 4 channels in float32: 3 real + a zero
        x = torch.cat([x, torch.zeros(x.shape[0], x.shape[1], x.shape[2], 1)], 3).to(DEV).contiguous()
        out = net.stem(x)
    else:
        out = getattr(net, stage)(sn.to_physical(x, *LAYOUT_IN[stage]).to(DEV))
    h, wl = LAYOUT_OUT[stage]
    assert out.shape[3] == h * sn.pad_width(wl)
    assert bool((out.unflatten(-1, (h, sn.pad_width(wl)))[..., wl:] == 0).all()), "pad channels are not zero"
    return sn.to_logical(out, h, wl)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_trunk_stage_by_stage(trunk, mode):
    net, sd0, refs, x = trunk
    training = mode == "train"
    net.load_state_dict(sd0)
    net.train(training)
    ratios = {}
    shapes = {"stem": (2, 32, 32, 24), "stage2": (2, 16, 16, 116), "stage3": (2, 8, 8, 232), "stage4": (2, 4, 4, 464)}
    with torch.no_grad():
        for stage in STAGES:
            xin, o64, r32 = refs[(training, stage)]
            got = _gpu_stage(net, stage, xin)
            assert tuple(got.shape) == shapes[stage] == tuple(_nhwc(o64).shape), (stage, got.shape)
            err = _rel(_nchw(got), o64)[0]
            ratios[stage] = err / r32
            print(f"shufflenet {mode} {stage}: error {err:.3g}, ref32_err {r32:.3g}, ratio {ratios[stage]:.3f}")
    for stage, r in ratios.items():
        assert r <= K_FWD, (mode, stage, r, K_FWD)


def test_trunk_forward_shapes_and_p6(trunk):
    sn, fpn, ops, lib = _mods()
    net, sd0, refs, x = trunk
    net.load_state_dict(sd0)
    net.train()
    xg = torch.cat([_nhwc(x), torch.zeros(2, 128, 128, 1)], 3).to(DEV).contiguous()
    with torch.no_grad():
        phys = net(xg)
    out = net.logical_features(phys)
    assert list(out.keys()) == ["p2", "p3", "p4", "p5", "p6"]
    for name, (s, c) in {"p2": (32, 24), "p3": (16, 116), "p4": (8, 232), "p5": (4, 464), "p6": (2, 464)}.items():
        assert tuple(out[name].shape) == (2, s, s, c), (name, out[name].shape)
    assert [phys[k].shape[3] for k in phys] == [32, 128, 256, 512, 512]
    assert torch.equal(out["p6"], out["p5"][:, ::2, ::2])
    # the whole forward (one pack for all units) against the chained float64 stages: errors add up along the trunk, so the
    # bound is the sum of the stages' own
    err = _rel(_nchw(out["p3"]), refs[(True, "stage2")][1])[0]
    assert err <= K_FWD * (refs[(True, "stem")][2] + refs[(True, "stage2")][2])
    # conv5 is never run: its running statistics keep their bits
    sd = net.state_dict()
    assert torch.equal(sd["conv5.1.running_mean"].cpu(), sd0["conv5.1.running_mean"])
    assert torch.equal(sd["conv5.1.running_var"].cpu(), sd0["conv5.1.running_var"])
    assert not torch.equal(sd["stage2.0.branch1.1.running_mean"].cpu(), sd0["stage2.0.branch1.1.running_mean"])


def test_no_stale_copies_after_load_state_dict_and_optimizer_step(trunk):
    """the padded compute copies follow the parameters: after load_state_dict with other weights and after one optimizer step
    (parameters rewritten through raw pointers in the optimizer's flat buffer) stage2 matches the restatement on the NEW weights"""
    sn, fpn, ops, lib = _mods()
    solver = importlib.import_module("3dod_amd.cubercnn.solver.build")
    net, sd0, refs, x = trunk
    net.load_state_dict(sd0)
    net.eval()
    xin = refs[(False, "stage2")][0]
    with torch.no_grad():
        before = _gpu_stage(net, "stage2", xin)
    gen = torch.Generator().manual_seed(77)
    sd1 = {k: (v + 0.05 * torch.randn(v.shape, generator=gen) if v.dtype == f32 and "running_var" not in k else v.clone())
           for k, v in sd0.items()}
    net.load_state_dict(sd1)
    with torch.no_grad():
        got = _gpu_stage(net, "stage2", xin)
    assert _rel(got, before)[0] > 1e-3
    p = {k: v.to(f64) for k, v in sd1.items() if "num_batches" not in k}
    with torch.no_grad():
        o64 = _ref_stage(p, "stage2", xin, False)
        o32 = _ref_stage({k: v.to(f32) for k, v in p.items()}, "stage2", xin.to(f32), False)
    err, r32 = _rel(_nchw(got), o64)[0], _rel(o32, o64)[0]
    print(f"after load_state_dict: error {err:.3g}, ref32_err {r32:.3g}, ratio {err / r32:.3f}")
    assert err <= K_FWD * r32
    # one optimizer step
    params = [q for n, q in net.named_parameters() if q.requires_grad]
    opt = solver.FlatSGD([(q, 0.05, 0.0) for q in params], 0.9)
    net.train()
    xg = sn.to_physical(_nhwc(xin.to(f32)), 1, 24).to(DEV)
    out = net.stage2(xg)
    out.square().mean().backward()
    opt.collect_grads()
    assert all(float(ops.grad_sink(q).abs().sum()) > 0 for n, q in net.stage2.named_parameters()), "a parameter got no gradient"
    opt.step()
    net.eval()
    sd2 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    assert not torch.equal(sd2["stage2.1.branch2.0.weight"], sd1["stage2.1.branch2.0.weight"])
    with torch.no_grad():
        got2 = _gpu_stage(net, "stage2", xin)
    p = {k: v.to(f64) for k, v in sd2.items() if "num_batches" not in k}
    with torch.no_grad():
        o64 = _ref_stage(p, "stage2", xin, False)
        o32 = _ref_stage({k: v.to(f32) for k, v in p.items()}, "stage2", xin.to(f32), False)
    err, r32 = _rel(_nchw(got2), o64)[0], _rel(o32, o64)[0]
    print(f"after optimizer step: error {err:.3g}, ref32_err {r32:.3g}, ratio {err / r32:.3f}")
    assert err <= K_FWD * r32


# ---------------------------------------------------------------------------------------------------------------------
# 6. whole model
# ---------------------------------------------------------------------------------------------------------------------
def _build_model(seed=0):
    syn = importlib.import_module("3dod_amd.synthetic")
    modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
    solver = importlib.import_module("3dod_amd.cubercnn.solver")
    cfg = syn.make_cfg(os.path.join(ROOT, "configs", "cubercnn_shufflenet_FPN.yaml"),
                       overrides=["MODEL.DEVICE", "cuda:0", "VIS_PERIOD", 0, "log", False, "SOLVER.BASE_LR", 0.0025])
    torch.manual_seed(seed)
    model = modeling.build_model(cfg).to(DEV).train()
    opt = solver.build_optimizer(cfg, model)
    return cfg, model, opt, syn, solver


def test_pyramid_shapes():
    cfg, model, opt, syn, solver = _build_model()
    batch = syn.make_batch(2, 3, with_gt=False)
    with torch.no_grad():
        images, x = model.preprocess_image(batch)
        feats = model.backbone(x)
    assert list(feats.keys()) == ["p2", "p3", "p4", "p5", "p6"]              # no top block: no p7
    for name, s in (("p2", 128), ("p3", 64), ("p4", 32), ("p5", 16), ("p6", 8)):
        assert tuple(feats[name].shape) == (2, s, s, 256), (name, feats[name].shape)
    model.eval()
    with torch.no_grad():
        out = model(batch)
    assert len(out) == 2


def test_shufflenet_train_steps_learn():
    sn, fpn, ops, lib = _mods()
    cfg, model, opt, syn, solver = _build_model()
    d2 = importlib.import_module("3dod_amd.d2lite")
    step = solver.TrainStep(cfg, model, opt, world_size=1)
    batch = syn.make_batch(2, 7)
    bu = model.backbone.bottom_up
    conv5_0 = {k: v.detach().clone() for k, v in bu.conv5.state_dict().items()}
    totals = []
    with d2.EventStorage(0):
        for i in range(8):
            step(batch)
            rep = step.report()
            totals.append(rep["total_loss"])
            if i == 0:                                      # the step leaves this iteration's gradient in the sinks
                for name, p in bu.named_parameters():
                    gbuf = ops.grad_sink(p)
                    if name.startswith("conv5."):
                        assert gbuf is None, name
                        continue
                    assert gbuf is not None, name
                    assert bool(torch.isfinite(gbuf).all()), name
                    assert float(gbuf.abs().sum()) > 0.0, f"{name} received no gradient"
                for conv in model.backbone.lateral_convs:
                    assert float(ops.grad_sink(conv.weight).abs().sum()) > 0.0
    print("shufflenet totals", totals)
    assert all(t == t and abs(t) < 1e4 for t in totals), totals
    assert rep["iterations_explode"] == 0, rep
    assert min(totals[-3:]) < totals[0], totals
    for k, v in bu.conv5.state_dict().items():
        assert torch.equal(v, conv5_0[k]), f"conv5.{k} changed during training"


def _to_dev(batch):
    for d in batch:
        d["image"] = d["image"].to(DEV)
        d["instances"] = d["instances"].to(DEV)
    return batch


def test_graphed_step_equals_eager_step(monkeypatch):
    """one step through solver.make_train_step (dense region replayed from HIP graphs) returns the losses of the eager step
    from the same state"""
    d2 = importlib.import_module("3dod_amd.d2lite")
    reports = {}
    for mode in ("none", "dense"):
        monkeypatch.setenv("CR_GRAPHS", mode)
        cfg, model, opt, syn, solver = _build_model(seed=0)
        step = solver.make_train_step(cfg, model, opt, world_size=1)
        batch = _to_dev(syn.make_batch(2, 11, size=256))
        torch.manual_seed(5)
        with d2.EventStorage(0):
            step(batch)
            reports[mode] = step.report()
        assert (model._graphed is not None) == (mode == "dense")
    eager, graph = reports["none"], reports["dense"]
    print("eager", eager, "\ngraphed", graph)
    assert eager["iterations_explode"] == 0 and graph["iterations_explode"] == 0
    keys = [k for k in eager if not k.startswith("iterations")]
    assert keys and set(keys) == set(k for k in graph if not k.startswith("iterations"))
    for k in keys:
        assert abs(graph[k] - eager[k]) <= 1e-6 * max(abs(eager[k]), 1e-30), (k, eager[k], graph[k])


def test_bf16_step_is_finite():
    sn, fpn, ops, lib = _mods()
    d2 = importlib.import_module("3dod_amd.d2lite")
    prev = ops.set_precision("bf16")
    try:
        cfg, model, opt, syn, solver = _build_model()
        step = solver.TrainStep(cfg, model, opt, world_size=1)
        with d2.EventStorage(0):
            step(syn.make_batch(2, 7, size=256))
            rep = step.report()
        losses = {k: v for k, v in rep.items() if not k.startswith("iterations")}
        assert all(v == v and abs(v) < 1e4 for v in losses.values()), losses
    finally:
        ops.set_precision(prev)


def test_train_net_driver_with_the_shufflenet_config(tmp_path, monkeypatch):
    """the unchanged tools/train_net.py main() with configs/cubercnn_shufflenet_FPN.yaml, as test_train_net_driver_end_to_end of
    tests/test_gpu_train_loop.py does it for the default config: synthetic Omni3D files -> do_train (4 iterations, checkpoints)
    -> do_test, then --eval-only from the written checkpoint (a state dict of logical shapes) gives the same tables"""
    import types
    syn = importlib.import_module("3dod_amd.synthetic")
    D = importlib.import_module("3dod_amd.d2lite.data")
    root = tmp_path / "datasets"
    root.mkdir()
    syn.make_omni3d_dataset(str(root), name="Synth_train", n_images=10, seed=8)
    syn.make_omni3d_dataset(str(root), name="Synth_val", n_images=4, seed=9, first_image_id=3000)
    monkeypatch.chdir(tmp_path)
    for n in list(D.DatasetCatalog):
        D.DatasetCatalog.remove(n)
    for n in ("omni3d_model", "Synth_train", "Synth_val"):
        D.MetadataCatalog.pop(n, None)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    tn = importlib.import_module("train_net")
    cats = ["bed", "car", "chair", "sofa", "table", "truck"]
    opts = ["DATASETS.TRAIN", ("Synth_train",), "DATASETS.TEST", ("Synth_val",), "DATASETS.CATEGORY_NAMES", cats,
            "SOLVER.IMS_PER_BATCH", 2, "SOLVER.MAX_ITER", 4, "SOLVER.CHECKPOINT_PERIOD", 2, "SOLVER.BASE_LR", 0.001,
            "SOLVER.WARMUP_ITERS", 2, "DATALOADER.NUM_WORKERS", 0, "INPUT.MIN_SIZE_TRAIN", (256,), "INPUT.MAX_SIZE_TRAIN", 512,
            "INPUT.MIN_SIZE_TEST", 256, "INPUT.MAX_SIZE_TEST", 512, "VIS_PERIOD", 0, "log", False, "OUTPUT_DIR", str(tmp_path / "out"),
            "TEST.EVAL_PERIOD", 0, "MODEL.DEVICE", "cuda:0"]
    config = os.path.join(ROOT, "configs", "cubercnn_shufflenet_FPN.yaml")
    analysis = tn.main(types.SimpleNamespace(config_file=config, resume=False, eval_only=False, opts=opts))
    assert "Synth_val" in analysis
    ckpt = torch.load(tmp_path / "out" / "model_final.pth", map_location="cpu")
    sd = ckpt["model"] if "model" in ckpt else ckpt
    assert tuple(sd["backbone.bottom_up.stage3.1.branch2.3.weight"].shape) == (116, 1, 3, 3)
    assert tuple(sd["backbone.fpn_lateral3.weight"].shape) == (256, 116, 1, 1)
    again = tn.main(types.SimpleNamespace(config_file=config, resume=True, eval_only=True, opts=opts))
    assert set(again) == set(analysis)


# ---------------------------------------------------------------------------------------------------------------------
# 7. CR_DETERMINISTIC=1 (read once by the library, hence a child process): a stride-2 unit's backward twice, same bits
# ---------------------------------------------------------------------------------------------------------------------
DET_PROG = r'''
import hashlib, importlib, sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
t = importlib.import_module("test_gpu_shufflenet")
for run in range(2):
    unit, out, got_g, ref64, ref32 = t._run_unit("s2_24to116", "train")
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for k in sorted(got_g):
        h.update(got_g[k].contiguous().cpu().numpy().tobytes())
    print("HASH", h.hexdigest(), len(got_g))
''' % (ROOT, os.path.join(ROOT, "tests"))


def test_deterministic_unit_backward_is_bit_reproducible():
    env = dict(os.environ, CR_DETERMINISTIC="1", CR_PRECISION="fp32")
    out = subprocess.run([sys.executable, "-c", DET_PROG], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("HASH")]
    assert len(lines) == 2, out.stderr[-2000:]
    assert int(lines[0][2]) == 1 + 3 * 5                    # x and five (conv, gamma, beta) triples
    assert lines[0][1] == lines[1][1], "two runs of the unit backward differ in deterministic mode"
