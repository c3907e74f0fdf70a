"""GPU: the MNASNet-1.0 trunk (cubercnn/modeling/backbone/mnasnet.py) on the kernels of csrc/mnasnet.hip.

torchvision is absent, so the reference here is a float64 restatement of torchvision's mnasnet1_0 from plain functionals
(F.conv2d(..., groups=c), F.batch_norm, F.relu, the residual add, F.max_pool2d) over the module's own state dict ("parity
unpinned" w.r.t. torchvision).  Everything is compared in LOGICAL channels: the trunk's padded physical maps go through
mnasnet.to_logical first, and their pad channels must be exactly zero.

Bounds.  Kernels in isolation: the project's float32 module bound, 2e-5 relative L2 and 2e-4 max-norm; a bf16 output that is one
round-to-nearest of a float32 result: |got - ref| <= 2^-8 |ref| + 1e-6 max|ref|.  Blocks, trunk stages and gradients: the method of
tests/test_gpu_shufflenet.py -- the restatement also runs in float32 on the CPU, its relative L2 distance from float64 is
`ref32_err`, and the product must stay within K_FWD * ref32_err (outputs) or K_GRAD * ref32_err (gradients) with the constants of
tests/test_gpu_dla_types.py.  Running statistics: the module's momentum is 3e-4, so the float32 restatement can land on float64's
own rounding; their bound is max(K_FWD * ref32_err, 2^-23), and one block is repeated with momentum 0.1, where the plain ratio
bound holds.  Every ratio is printed.

Measured on MI355X.  Depthwise kernels (f32 outputs, weight gradients, statistics rows): relative L2 <= 1.4e-7, max-norm <= 3.2e-7;
bf16 outputs: worst |got - ref| - bound = -1.1e-6.  cr_bn_bwd_anyc against float64: relative L2 <= 1.1e-7, max-norm <= 1.3e-7, bf16
dx never above its bound; against cr_bn_bwd / cr_bn_bwd_mask at C = 64 / 128: <= 1.5e-7 / 1.6e-7; cr_colsum_wide <= 6.6e-8.  Blocks
(ratio = error / ref32_err): output 0.98 .. 1.46 in train and 0.96 .. 1.94 in frozen and eval mode (K_FWD 2.966); running
statistics 0.53 .. 0.84 (errors 1.7e-8 .. 2.9e-8, below the 2^-23 floor) and 0.59 .. 1.11 at momentum 0.1; gradients 0.30 .. 1.75
in train and 0.30 .. 1.53 in frozen mode (K_GRAD 2.31).  Trunk stages 0.99 .. 1.05 in train and 0.95 .. 1.25 in eval mode; after
load_state_dict 1.14, after an optimizer step 1.19.

The gradient of layers.7.bias is the tightest: a block ends in a BatchNorm without a ReLU, so it is the plain per-channel sum of
the cotangent over 60 pixels, which the float32 restatement sums pairwise to a single rounding (ref32_err 5e-8 .. 8e-8).  Formed
by cr_bn_bwd (at the physical width 32) or by the bias sum of cr_conv2d_bwd_weight_bias (frozen backward), which add a block's
rows one after the other in float32, it measured 1.0e-7 .. 1.7e-7: ratios 1.80 .. 2.49, above K_GRAD in three of seven runs.  The
trunk therefore takes cr_bn_bwd_anyc at every width and cr_colsum_wide in the frozen backward (wide_sums=True), which add across
threads in double: 2.0e-8 .. 3.3e-8, ratios 0.30 .. 0.50 in all ten runs."""
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
BN_MOMENTUM, EPS = 1 - 0.9997, 1e-5
STACKS = {8: (16, 24, 3, 2, 3, 3), 9: (24, 40, 5, 2, 3, 3), 10: (40, 80, 5, 2, 6, 3), 11: (80, 96, 3, 1, 6, 2),
          12: (96, 192, 5, 2, 6, 4), 13: (192, 320, 3, 1, 6, 1)}


def _mods():
    return (importlib.import_module("3dod_amd.cubercnn.modeling.backbone.mnasnet"), importlib.import_module("3dod_amd.hipops"),
            importlib.import_module("3dod_amd._lib"))


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
# the restatement: torchvision's mnasnet1_0 from functionals over a state dict `p` (any dtype).  `new` (a dict) receives the
# running statistics every train-mode BatchNorm leaves behind.
# ---------------------------------------------------------------------------------------------------------------------
def _bn(t, p, k, training, new, momentum=BN_MOMENTUM):
    rm, rv = p[k + ".running_mean"].detach().clone(), p[k + ".running_var"].detach().clone()
    y = F.batch_norm(t, rm, rv, p[k + ".weight"], p[k + ".bias"], training, momentum, EPS)
    if new is not None:
        new[k + ".running_mean"], new[k + ".running_var"] = rm, rv
    return y


def _ref_block(p, pre, x, k, stride, residual, training, new=None, momentum=BN_MOMENTUM):
    L = pre + "layers."
    t = F.relu(_bn(F.conv2d(x, p[L + "0.weight"]), p, L + "1", training, new, momentum))
    t = F.relu(_bn(F.conv2d(t, p[L + "3.weight"], None, stride, k // 2, 1, t.shape[1]), p, L + "4", training, new, momentum))
    t = _bn(F.conv2d(t, p[L + "6.weight"]), p, L + "7", training, new, momentum)
    return t + x if residual else t


STAGES = {"p2": (8,), "p3": (9,), "p4": (10, 11), "p5": (12, 13)}


def _ref_stage(p, stage, x, training, new=None):
    if stage == "p2":
        x = F.relu(_bn(F.conv2d(x, p["base.0.weight"], None, 2, 1), p, "base.1", training, new))
        x = F.relu(_bn(F.conv2d(x, p["base.3.weight"], None, 1, 1, 1, 32), p, "base.4", training, new))
        x = _bn(F.conv2d(x, p["base.6.weight"]), p, "base.7", training, new)
    for i in STAGES[stage]:
        cin, cout, k, stride, exp, repeats = STACKS[i]
        for j in range(repeats):
            x = _ref_block(p, f"base.{i}.{j}.", x, k, stride if j == 0 else 1, j > 0, training, new)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# 1. the depthwise kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("shape", [(2, 5, 7), (2, 6, 10), (1, 1, 1), (1, 2, 2)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", [8, 72, 576])
def test_depthwise_against_float64(C, shape, k, stride, dtype):
    """C = 8 is one channel group of 8 (two of 4 for the 5x5), 72 is 9 (18): a partial workgroup column, 576 is several columns;
    odd extents give stride-2 outputs of 3 x 4; 1 x 1 and 2 x 2 maps are smaller than a 5x5 window: all halo; (2, 6, 10) at
    stride 1 is M = 120 = two statistics rows, the second partial."""
    mn, ops, lib = _mods()
    N, H, W = shape
    gen = torch.Generator().manual_seed(1000 * C + 100 * k + 10 * H + stride)
    exact = (lambda t: t.to(bf16).to(f32)) if dtype == bf16 else (lambda t: t)
    x = exact(torch.randn(N, C, H, W, generator=gen))
    w = torch.randn(C, 1, k, k, generator=gen) * 0.4
    bias = torch.randn(C, generator=gen)
    x64, w64 = x.to(f64).requires_grad_(True), w.to(f64).requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, stride, k // 2, 1, C)
    Ho, Wo = y64.shape[2], y64.shape[3]
    assert (Ho, Wo) == ((H - 1) // stride + 1, (W - 1) // stride + 1)
    dy = exact(torch.randn(N, C, Ho, Wo, generator=gen))
    acc = exact(torch.randn(N, C, H, W, generator=gen))
    dx64, dw64 = torch.autograd.grad((y64 * dy.to(f64)).sum(), [x64, w64])
    M = N * Ho * Wo
    tag = f"dw C={C} {shape} k{k} s{stride} {'bf16' if dtype == bf16 else 'f32'}"

    xg, wg, dyg = _nhwc(x).to(DEV, dtype), w.to(DEV), _nhwc(dy).to(DEV, dtype)
    nparts = (M + 63) // 64
    stats = torch.full((nparts, 2, C), float("nan"), device=DEV)
    y = ops.dwconv_fwd_raw(xg, wg, k, stride, stats=stats)
    assert y.dtype == dtype and tuple(y.shape) == (N, Ho, Wo, C)
    yb = ops.dwconv_fwd_raw(xg, wg, k, stride, bias=bias.to(DEV))
    ybr = ops.dwconv_fwd_raw(xg, wg, k, stride, bias=bias.to(DEV), relu=True)
    dx = ops.dwconv_bwd_data_raw(dyg, wg, xg.shape, k, stride)
    dxa = ops.dwconv_bwd_data_raw(dyg, wg, xg.shape, k, stride, accumulate=_nhwc(acc).to(DEV, dtype))
    n_ws = ops.dwconv_wgrad_ws_floats(M, C, k)
    assert n_ws == ops.dw_wgrad_splits(M) * C * k * k
    dw_new = torch.full((C, k, k), float("nan"), device=DEV)
    lib.call("cr_dwconv_bwd_weight", dyg, xg, dw_new, N, H, W, C, k, stride, 0, int(dtype == f32), torch.empty(n_ws, device=DEV), n_ws)
    sink0 = torch.randn(C, k, k, generator=gen)
    sink = sink0.to(DEV).clone()
    assert ops.dwconv_bwd_weight_raw(dyg, xg, k, stride, sink=sink) is None
    dw_ret = ops.dwconv_bwd_weight_raw(dyg, xg, k, stride)
    assert torch.equal(dw_ret, ops.dwconv_bwd_weight_raw(dyg, xg, k, stride)), "the weight gradient is not bit-reproducible"

    y64n, dx64n = _nhwc(y64.detach()), _nhwc(dx64)
    assert torch.equal(ybr, yb.clamp_min(0)), "the ReLU epilogue is not max(out + bias, 0)"
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
    dw_ref = dw64.reshape(C, k, k)
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
    mn, ops, lib = _mods()
    with pytest.raises(lib.CrError):
        ops.dwconv_fwd_raw(torch.zeros(1, 4, 4, 12, device=DEV), torch.zeros(12, 5, 5, device=DEV), 5, 1)     # C % 8 != 0
    x, w = torch.zeros(1, 4, 4, 16, device=DEV), torch.zeros(16, 5, 5, device=DEV)
    with pytest.raises(lib.CrError):
        ops.dwconv_fwd_raw(x, w, 5, 3)                                                                       # stride
    with pytest.raises(lib.CrError):
        ops.dwconv_fwd_raw(x, torch.zeros(16, 4, 4, device=DEV), 4, 1)                                       # k
    with pytest.raises(lib.CrError):
        ops.dwconv_fwd_raw(x, torch.zeros(16, 7, 7, device=DEV), 7, 1)
    with pytest.raises(lib.CrError):
        lib.call("cr_dwconv_bwd_data", x, w, torch.zeros_like(x), 1, 4, 4, 16, 5, 3, 1, None)
    with pytest.raises(lib.CrError):
        lib.call("cr_dwconv_bwd_data", x, w, torch.zeros_like(x), 1, 4, 4, 16, 4, 1, 1, None)
    for k in (3, 5):                                                                                         # a workspace that is too small
        with pytest.raises(lib.CrError):
            lib.call("cr_dwconv_bwd_weight", x, x, torch.zeros(16, k, k, device=DEV), 1, 4, 4, 16, k, 1, 0, 1,
                     torch.zeros(8, device=DEV), 8)
    with pytest.raises(lib.CrError):
        lib.call("cr_dwconv_bwd_weight", x, x, torch.zeros(16, 2, 2, device=DEV), 1, 4, 4, 16, 2, 1, 0, 1,
                 torch.zeros(4096, device=DEV), 4096)
    with pytest.raises(lib.CrError):
        ops.dwconv_fwd_raw(torch.zeros(1, 4, 4, 16), w.cpu(), 5, 1)                                          # no CPU path


# ---------------------------------------------------------------------------------------------------------------------
# 2. the BatchNorm backward for any C % 8 == 0 against float64
# ---------------------------------------------------------------------------------------------------------------------
def _stats_rows(x):
    """[ceil(M / 64)][2][C] float32: sum and sum of squares of every 64 pixels, as the conv epilogues hand them over"""
    M, C = x.shape
    nparts = (M + 63) // 64
    xp = torch.zeros(nparts * 64, C, dtype=f64, device=x.device)
    xp[:M] = x.to(f64)
    xp = xp.view(nparts, 64, C)
    return torch.stack([xp.sum(1), (xp * xp).sum(1)], 1).to(f32).contiguous(), nparts


def _bn_inputs(C, M, dtype):
    mn, ops, lib = _mods()
    g = torch.Generator().manual_seed(1000 * C + M)
    gamma = ((torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.3).to(DEV)
    x = (torch.randn(M, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g)).to(dtype).to(DEV)
    dy = torch.randn(M, C, generator=g).to(dtype).to(DEV)
    stats, nparts = _stats_rows(x)
    out, mi = torch.empty_like(x), torch.empty(2, C, dtype=f32, device=DEV)
    lib.call("cr_bn_fwd", x, stats, nparts, gamma, beta, None, out, M, C, 1, EPS, 0.1, mi, None, None, int(dtype == f32))
    return x, gamma, beta, dy, out, mi


def _anyc(x, gamma, beta, dy, out, mi, relu):
    mn, ops, lib = _mods()
    C = x.shape[1]
    dgamma, dbeta = torch.full((C,), 0.25, device=DEV), torch.full((C,), -0.5, device=DEV)     # both are accumulated into
    dx = ops.bn_bwd_anyc_raw(dy, out, x, mi, gamma, beta, relu, dgamma, dbeta)
    return dx, dgamma, dbeta


def _bn_ref(x, gamma, dy, mask, mi):
    M = x.shape[0]
    x, gamma, mi = x.to("cpu", f64), gamma.to("cpu", f64), mi.to("cpu", f64)
    g = dy.to("cpu", f64) * mask.to("cpu", f64)
    xh = (x - mi[0]) * mi[1]
    sg, sgx = g.sum(0), (g * xh).sum(0)
    return gamma * mi[1] * (g - sg / M - xh * sgx / M), sgx, sg


def _check_bn(tag, got, ref, dtype):
    (dx, dgamma, dbeta), (dx_r, dg_r, db_r) = got, ref
    rows = [("dgamma", dgamma.cpu().to(f64) - 0.25, dg_r), ("dbeta", dbeta.cpu().to(f64) + 0.5, db_r)]
    if dtype == bf16:
        ex = _bf16_excess(dx, dx_r)
        print(f"{tag} dx: worst |got - ref| - bound = {ex:.3g}")
        assert ex <= 0.0, (tag, ex)
    else:
        rows.append(("dx", dx, dx_r))
    figs = [(n,) + _rel(a, b) for n, a, b in rows]
    for n, l2, mx in figs:
        print(f"{tag} {n}: rel L2 {l2:.3g}, max-norm {mx:.3g}")
    for n, l2, mx in figs:
        assert l2 < L2_F32 and mx < MX_F32, (tag, n, l2, mx)


@pytest.mark.parametrize("M", [1, 63, 130, 1500])
@pytest.mark.parametrize("C", [24, 48, 80, 320, 1152])
def test_bn_bwd_anyc_against_float64(C, M):
    """C = 24 is a partial slice of 32 channels, 48 and 80 one full and one partial, 320 and 1152 full slices only; M = 1 and 63
    are less than one pass of 64 pixel lanes, 130 is a partial third pass, 1500 is six pixel chunks with a partial last one.
    relu off / relu with the mask from `out` / relu with the mask from x, each in f32 and bf16; dgamma and dbeta accumulate onto
    0.25 and -0.5."""
    for dtype in (f32, bf16):
        x, gamma, beta, dy, out, mi = _bn_inputs(C, M, dtype)
        name = "bf16" if dtype == bf16 else "f32"
        got = {"norelu": _anyc(x, gamma, beta, dy, None, mi, 0), "relu_out": _anyc(x, gamma, beta, dy, out, mi, 1),
               "relu_x": _anyc(x, gamma, beta, dy, None, mi, 1)}
        torch.cuda.synchronize()
        ones = torch.ones_like(out, dtype=f32)
        for mode, res in got.items():
            mask = ones if mode == "norelu" else (out > 0).to(f32)
            _check_bn(f"bn anyc C={C} M={M} {name} {mode}", res, _bn_ref(x, gamma, dy, mask, mi), dtype)
        for a, b in zip(got["relu_out"], got["relu_x"]):     # the mask from x is the mask of the stored output, bit for bit
            assert torch.equal(a, b), (C, M, name)
        again = _anyc(x, gamma, beta, dy, None, mi, 1)
        for a, b in zip(got["relu_x"], again):
            assert torch.equal(a, b), "two runs on the same inputs differ"


@pytest.mark.parametrize("C", [64, 128])
def test_bn_bwd_anyc_agrees_with_the_power_of_two_kernels(C):
    """at widths both families take, cr_bn_bwd_anyc against cr_bn_bwd / cr_bn_bwd_mask on the same inputs: dgamma, dbeta (f32
    outputs) and f32 dx within the kernel bounds of each other.  A bf16 dx is a rounding of either kernel's f32 value; the two
    f32 values differ in their last bits (other summation orders), so the roundings may fall on neighbouring bf16 numbers: both
    are within the bf16 bound of float64, hence within twice that bound of each other."""
    mn, ops, lib = _mods()
    for dtype in (f32, bf16):
        for M in (130, 1500):
            x, gamma, beta, dy, out, mi = _bn_inputs(C, M, dtype)
            af = int(dtype == f32)
            for mode in ("norelu", "relu_out", "relu_x"):
                relu = int(mode != "norelu")
                got = _anyc(x, gamma, beta, dy, out if mode == "relu_out" else None, mi, relu)
                sums = torch.empty(1025, 2, C, device=DEV)
                dx = torch.empty_like(x)
                dgamma, dbeta = torch.full((C,), 0.25, device=DEV), torch.full((C,), -0.5, device=DEV)
                if mode == "relu_x":
                    lib.call("cr_bn_bwd_mask", dy, None, x, mi, gamma, beta, sums, dx, None, dgamma, dbeta, M, C, 1, af)
                else:
                    lib.call("cr_bn_bwd", dy, out if relu else None, x, mi, gamma, sums, dx, None, dgamma, dbeta, M, C, relu, af)
                tag = f"bn anyc vs pow2 C={C} M={M} {'f32' if af else 'bf16'} {mode}"
                rows = [("dgamma", got[1], dgamma), ("dbeta", got[2], dbeta)]
                if dtype == f32:
                    rows.append(("dx", got[0], dx))
                else:
                    mask = torch.ones_like(out, dtype=f32) if not relu else (out > 0).to(f32)
                    ref = _bn_ref(x, gamma, dy, mask, mi)[0]
                    d = (got[0].to("cpu", f64) - dx.to("cpu", f64)).abs()
                    ex = float((d - 2 * (2.0 ** -8 * ref.abs() + 1e-6 * ref.abs().max())).max())
                    print(f"{tag} dx: worst |anyc - pow2| - 2 x bound = {ex:.3g}")
                    assert ex <= 0.0, (tag, ex)
                    assert _bf16_excess(dx, ref) <= 0.0 and _bf16_excess(got[0], ref) <= 0.0, tag
                figs = [(n,) + _rel(a, b) for n, a, b in rows]
                for n, l2, mx in figs:
                    print(f"{tag} {n}: rel L2 {l2:.3g}, max-norm {mx:.3g}")
                for n, l2, mx in figs:
                    assert l2 < L2_F32 and mx < MX_F32, (tag, n, l2, mx)


@pytest.mark.parametrize("M", [1, 63, 130, 1500])
@pytest.mark.parametrize("C", [24, 32, 320])
def test_colsum_wide_against_float64(C, M):
    """cr_colsum_wide (the bias sum of the frozen backward): out += column sums, f32 and bf16 input, within the kernel bounds of
    float64; accumulates onto 0.25; two runs are bit-identical; the same partial / full slices and pixel chunks as above"""
    mn, ops, lib = _mods()
    for dtype in (f32, bf16):
        x = torch.randn(M, C, generator=torch.Generator().manual_seed(C + M)).to(dtype).to(DEV)
        outs = []
        for _ in range(2):
            out = torch.full((C,), 0.25, device=DEV)
            ops.colsum_wide_raw(x, out)
            outs.append(out)
        assert torch.equal(outs[0], outs[1])
        l2, mx = _rel(outs[0].cpu().to(f64) - 0.25, x.to("cpu", f64).sum(0))
        print(f"colsum wide C={C} M={M} {'bf16' if dtype == bf16 else 'f32'}: rel L2 {l2:.3g}, max-norm {mx:.3g}")
        assert l2 < L2_F32 and mx < MX_F32, (C, M, l2, mx)
    with pytest.raises(lib.CrError):
        ops.colsum_wide_raw(torch.zeros(4, 12, device=DEV), torch.zeros(12, device=DEV))


def test_bn_bwd_anyc_arguments_are_checked():
    mn, ops, lib = _mods()
    for C in (12, 2056):
        x = torch.zeros(4, C, device=DEV)
        v = torch.ones(C, device=DEV)
        with pytest.raises(lib.CrError):
            lib.call("cr_bn_bwd_anyc", x, None, x, torch.ones(2, C, device=DEV), v, v, torch.empty(256, 2, C, device=DEV),
                     torch.empty_like(x), v.clone(), v.clone(), 4, C, 0, 1)
    x = torch.zeros(4, 24, device=DEV)
    v = torch.ones(24, device=DEV)
    with pytest.raises(lib.CrError):                         # relu must be 0 or 1
        lib.call("cr_bn_bwd_anyc", x, None, x, torch.ones(2, 24, device=DEV), v, v, torch.empty(256, 2, 24, device=DEV),
                 torch.empty_like(x), v.clone(), v.clone(), 4, 24, 2, 1)


# ---------------------------------------------------------------------------------------------------------------------
# 3. blocks against float64
# ---------------------------------------------------------------------------------------------------------------------
BLOCK_CASES = {"16to24_k3s2": (16, 24, 3, 2, 3, (2, 9, 11)), "24_k3_res": (24, 24, 3, 1, 3, (2, 5, 6)),
               "40_k5_res": (40, 40, 5, 1, 3, (2, 5, 6)), "40to80_k5s2": (40, 80, 5, 2, 6, (2, 6, 10)),
               "192to320_k3": (192, 320, 3, 1, 6, (2, 4, 4))}


def _block_reference(blk, x, R, k, stride, residual, training, grad, dtype, momentum):
    p = {kk: v.detach().clone().to(dtype) for kk, v in blk.state_dict().items() if "num_batches" not in kk}
    names = [kk for kk in p if "running" not in kk]
    leaves = [p[kk].requires_grad_(grad) for kk in names]
    xr = x.to(dtype).requires_grad_(grad)
    new = {}
    out = _ref_block(p, "", xr, k, stride, residual, training, new, momentum)
    grads = torch.autograd.grad((out * R.to(dtype)).sum(), [xr] + leaves) if grad else ()
    return out.detach(), new, dict(zip(["x"] + names, grads)), names


def _run_block(case, mode, momentum=BN_MOMENTUM, seed=21):
    mn, ops, lib = _mods()
    inp, oup, k, stride, exp, (N, H, W) = BLOCK_CASES[case]
    training, grad = mode == "train", mode != "eval"
    torch.manual_seed(seed)
    blk = mn._InvertedResidual(inp, oup, k, stride, exp)
    assert blk.apply_residual == (inp == oup and stride == 1)
    _randomise_bn(blk, torch.Generator().manual_seed(seed + 1))
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = momentum
    gen = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(N, inp, H, W, generator=gen)
    R = torch.randn(N, oup, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=gen)
    ref64 = _block_reference(blk, x, R, k, stride, blk.apply_residual, training, grad, f64, momentum)
    ref32 = _block_reference(blk, x, R, k, stride, blk.apply_residual, training, grad, f32, momentum)
    blk = blk.to(DEV)
    blk.train(training)
    xg = mn.to_physical(_nhwc(x), inp).to(DEV).requires_grad_(grad)
    params = dict(blk.named_parameters())
    with torch.set_grad_enabled(grad):
        out = blk(xg)
    got_g = {}
    if grad:
        names = ref64[3]
        gs = torch.autograd.grad((mn.to_logical(out, oup) * _nhwc(R).to(DEV)).sum(), [xg] + [params[kk] for kk in names])
        got_g = dict(zip(["x"] + names, gs))
        gx = got_g["x"]
        assert tuple(gx.shape) == tuple(xg.shape)
        assert bool((gx[..., inp:] == 0).all()), "the input gradient's pad channels are not zero"
        got_g["x"] = _nchw(mn.to_logical(gx, inp))
    return blk, out, got_g, ref64, ref32


def _check_block(case, mode, momentum=BN_MOMENTUM):
    mn, ops, lib = _mods()
    blk, out, got_g, ref64, ref32 = _run_block(case, mode, momentum)
    oup = BLOCK_CASES[case][1]
    training = mode == "train"
    assert tuple(out.shape)[3] == mn.pad_width(oup) and out.dtype == f32
    assert bool((out[..., oup:] == 0).all()), "pad channels are not zero"
    rows = [("out", K_FWD, 0.0, _rel(_nchw(mn.to_logical(out, oup)), ref64[0])[0], _rel(ref32[0], ref64[0])[0])]
    sd = blk.state_dict()
    assert len(ref64[1]) == 6
    floor = 0.0 if momentum == 0.1 else 2.0 ** -23          # momentum 3e-4: float32 can land on float64's own rounding
    for kk, v in ref64[1].items():
        if training:
            rows.append((kk, K_FWD, floor, _rel(sd[kk], v)[0], _rel(ref32[1][kk], v)[0]))
        else:
            assert torch.equal(sd[kk].cpu().to(f64), v), f"{kk} changed in {mode} mode"
    for kk, g in got_g.items():
        assert tuple(g.shape) == tuple(ref64[2][kk].shape), (kk, g.shape)
        rows.append(("grad " + kk, K_GRAD, 0.0, _rel(g, ref64[2][kk])[0], _rel(ref32[2][kk], ref64[2][kk])[0]))
    for name, K, fl, err, r32 in rows:
        print(f"block {case} {mode} m={momentum:.1e} {name}: error {err:.3g}, ref32_err {r32:.3g}, ratio {err / max(r32, 1e-300):.3f}")
    for name, K, fl, err, r32 in rows:
        assert err <= max(K * r32, fl), (case, mode, name, err, r32, err / max(r32, 1e-300), K)


@pytest.mark.parametrize("mode", ["train", "frozen", "eval"])
@pytest.mark.parametrize("case", list(BLOCK_CASES))
def test_block_against_float64(case, mode):
    """output, every BatchNorm's running statistics after one call and the gradients of the input and every parameter under a
    random cotangent, each within K * ref32_err of float64; frozen / eval: the running statistics keep their bits"""
    _check_block(case, mode)


def test_block_running_statistics_with_momentum_0p1():
    """the statistics update itself under the plain ratio bound: at momentum 0.1 the new statistics are no rounding of the old"""
    _check_block("40_k5_res", "train", momentum=0.1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the trunk stage by stage, 5. stale compute copies
# ---------------------------------------------------------------------------------------------------------------------
ORDER = ["p2", "p3", "p4", "p5"]
W_IN = {"p3": 24, "p4": 40, "p5": 96}
W_OUT = {"p2": 24, "p3": 40, "p4": 96, "p5": 320}


def _stage_refs(sd, x):
    """per mode and stage: the float64 input, the float64 result and ref32_err of the float32 CPU restatement"""
    p64 = {k: v.to(f64) for k, v in sd.items() if "num_batches" not in k}
    p32 = {k: v.to(f32) for k, v in p64.items()}
    refs = {}
    with torch.no_grad():
        for training in (True, False):
            t = x.to(f64)
            for stage in ORDER:
                o64 = _ref_stage(p64, stage, t, training)
                o32 = _ref_stage(p32, stage, t.to(f32), training)
                refs[(training, stage)] = (t, o64, _rel(o32, o64)[0])
                t = o64
    return refs


@pytest.fixture(scope="module")
def trunk():
    mn, ops, lib = _mods()
    torch.manual_seed(31)
    net = mn.MNASNetBackbone(None, None)
    _randomise_bn(net, torch.Generator().manual_seed(32))
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(33))
    return net.to(DEV), sd0, _stage_refs(sd0, x), x


def _gpu_stage(net, stage, xin):
    """xin: the stage's logical NCHW input -> its logical NHWC output"""
    mn, ops, lib = _mods()
    x = _nhwc(xin.to(f32))
    if stage == "p2":                                    # the RGB stem reads 4 channels in float32: 3 real + a zero
        x = torch.cat([x, torch.zeros(x.shape[0], x.shape[1], x.shape[2], 1)], 3).to(DEV).contiguous()
    else:
        x = mn.to_physical(x, W_IN[stage]).to(DEV)
    out = net.stage(stage, x)
    wl = W_OUT[stage]
    assert out.shape[3] == mn.pad_width(wl)
    assert bool((out[..., wl:] == 0).all()), "pad channels are not zero"
    return mn.to_logical(out, wl)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_trunk_stage_by_stage(trunk, mode):
    net, sd0, refs, x = trunk
    training = mode == "train"
    net.load_state_dict(sd0)
    net.train(training)
    ratios = {}
    shapes = {"p2": (2, 32, 32, 24), "p3": (2, 16, 16, 40), "p4": (2, 8, 8, 96), "p5": (2, 4, 4, 320)}
    with torch.no_grad():
        for stage in ORDER:
            xin, o64, r32 = refs[(training, stage)]
            got = _gpu_stage(net, stage, xin)
            assert tuple(got.shape) == shapes[stage] == tuple(_nhwc(o64).shape), (stage, got.shape)
            err = _rel(_nchw(got), o64)[0]
            ratios[stage] = err / r32
            print(f"mnasnet {mode} {stage}: error {err:.3g}, ref32_err {r32:.3g}, ratio {ratios[stage]:.3f}")
    for stage, r in ratios.items():
        assert r <= K_FWD, (mode, stage, r, K_FWD)


def test_trunk_forward_shapes_and_p6(trunk):
    mn, ops, lib = _mods()
    net, sd0, refs, x = trunk
    net.load_state_dict(sd0)
    net.train()
    xg = torch.cat([_nhwc(x), torch.zeros(2, 128, 128, 1)], 3).to(DEV).contiguous()
    with torch.no_grad():
        phys = net(xg)
    out = net.logical_features(phys)
    assert list(out.keys()) == ["p2", "p3", "p4", "p5", "p6"]
    for name, (s, c) in {"p2": (32, 24), "p3": (16, 40), "p4": (8, 96), "p5": (4, 320), "p6": (2, 320)}.items():
        assert tuple(out[name].shape) == (2, s, s, c), (name, out[name].shape)
    assert [phys[k].shape[3] for k in phys] == [32, 48, 96, 320, 320]
    assert torch.equal(out["p6"], out["p5"][:, ::2, ::2])
    # the whole forward (one pack for all blocks) against the chained float64 stages: errors add up along the trunk, so the
    # bound is the sum of the stages' own
    err = _rel(_nchw(out["p3"]), refs[(True, "p3")][1])[0]
    assert err <= K_FWD * (refs[(True, "p2")][2] + refs[(True, "p3")][2])
    # base[14:17] is never run: its running statistics keep their bits
    sd = net.state_dict()
    assert torch.equal(sd["base.15.running_mean"].cpu(), sd0["base.15.running_mean"])
    assert torch.equal(sd["base.15.running_var"].cpu(), sd0["base.15.running_var"])
    assert not torch.equal(sd["base.9.0.layers.4.running_mean"].cpu(), sd0["base.9.0.layers.4.running_mean"])
    assert not torch.equal(sd["base.4.running_var"].cpu(), sd0["base.4.running_var"])


def test_no_stale_copies_after_load_state_dict_and_optimizer_step(trunk):
    """the padded compute copies follow the parameters: after load_state_dict with other weights and after one optimizer step
    (parameters rewritten through raw pointers in the optimizer's flat buffer) base[9] matches the restatement on the NEW weights"""
    mn, ops, lib = _mods()
    solver = importlib.import_module("3dod_amd.cubercnn.solver.build")
    net, sd0, refs, x = trunk
    net.load_state_dict(sd0)
    net.eval()
    xin = refs[(False, "p3")][0]
    with torch.no_grad():
        before = _gpu_stage(net, "p3", xin)
    gen = torch.Generator().manual_seed(77)
    sd1 = {k: (v + 0.05 * torch.randn(v.shape, generator=gen) if v.dtype == f32 and "running_var" not in k else v.clone())
           for k, v in sd0.items()}
    net.load_state_dict(sd1)
    with torch.no_grad():
        got = _gpu_stage(net, "p3", xin)
    assert _rel(got, before)[0] > 1e-3
    p = {k: v.to(f64) for k, v in sd1.items() if "num_batches" not in k}
    with torch.no_grad():
        o64 = _ref_stage(p, "p3", xin, False)
        o32 = _ref_stage({k: v.to(f32) for k, v in p.items()}, "p3", xin.to(f32), False)
    err, r32 = _rel(_nchw(got), o64)[0], _rel(o32, o64)[0]
    print(f"after load_state_dict: error {err:.3g}, ref32_err {r32:.3g}, ratio {err / r32:.3f}")
    assert err <= K_FWD * r32
    # one optimizer step
    params = [q for n, q in net.named_parameters() if q.requires_grad]
    opt = solver.FlatSGD([(q, 0.05, 0.0) for q in params], 0.9)
    net.train()
    xg = mn.to_physical(_nhwc(xin.to(f32)), 24).to(DEV)
    out = net.stage("p3", xg)
    out.square().mean().backward()
    opt.collect_grads()
    assert all(float(ops.grad_sink(q).abs().sum()) > 0 for n, q in net.base[9].named_parameters()), "a parameter got no gradient"
    opt.step()
    net.eval()
    sd2 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    assert not torch.equal(sd2["base.9.1.layers.0.weight"], sd1["base.9.1.layers.0.weight"])
    with torch.no_grad():
        got2 = _gpu_stage(net, "p3", xin)
    p = {k: v.to(f64) for k, v in sd2.items() if "num_batches" not in k}
    with torch.no_grad():
        o64 = _ref_stage(p, "p3", xin, False)
        o32 = _ref_stage({k: v.to(f32) for k, v in p.items()}, "p3", xin.to(f32), False)
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
    cfg = syn.make_cfg(os.path.join(ROOT, "configs", "cubercnn_mnasnet_FPN.yaml"),
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


def test_mnasnet_train_steps_learn():
    mn, ops, lib = _mods()
    cfg, model, opt, syn, solver = _build_model()
    d2 = importlib.import_module("3dod_amd.d2lite")
    step = solver.TrainStep(cfg, model, opt, world_size=1)
    batch = syn.make_batch(2, 7)
    bu = model.backbone.bottom_up
    head = ("base.14.", "base.15.", "base.16.")
    head0 = {k: v.detach().clone() for k, v in bu.state_dict().items() if k.startswith(head)}
    assert len(head0) == 1 + 5
    totals = []
    with d2.EventStorage(0):
        for i in range(8):
            step(batch)
            rep = step.report()
            totals.append(rep["total_loss"])
            if i == 0:                                      # the step leaves this iteration's gradient in the sinks
                for name, p in bu.named_parameters():
                    gbuf = ops.grad_sink(p)
                    if name.startswith(head):
                        assert gbuf is None, name
                        continue
                    assert gbuf is not None, name
                    assert bool(torch.isfinite(gbuf).all()), name
                    assert float(gbuf.abs().sum()) > 0.0, f"{name} received no gradient"
                for conv in model.backbone.lateral_convs:
                    assert float(ops.grad_sink(conv.weight).abs().sum()) > 0.0
    print("mnasnet totals", totals)
    assert all(t == t and abs(t) < 1e4 for t in totals), totals
    assert rep["iterations_explode"] == 0, rep
    assert min(totals[-3:]) < totals[0], totals
    sd = bu.state_dict()
    for k, v in head0.items():
        assert torch.equal(sd[k], v), f"{k} changed during training"


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
    mn, ops, lib = _mods()
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


def test_train_net_driver_with_the_mnasnet_config(tmp_path, monkeypatch):
    """the unchanged tools/train_net.py main() with configs/cubercnn_mnasnet_FPN.yaml, as test_train_net_driver_end_to_end of
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
    config = os.path.join(ROOT, "configs", "cubercnn_mnasnet_FPN.yaml")
    analysis = tn.main(types.SimpleNamespace(config_file=config, resume=False, eval_only=False, opts=opts))
    assert "Synth_val" in analysis
    ckpt = torch.load(tmp_path / "out" / "model_final.pth", map_location="cpu")
    sd = ckpt["model"] if "model" in ckpt else ckpt
    assert tuple(sd["backbone.bottom_up.base.9.0.layers.3.weight"].shape) == (72, 1, 5, 5)
    assert tuple(sd["backbone.fpn_lateral3.weight"].shape) == (256, 40, 1, 1)
    again = tn.main(types.SimpleNamespace(config_file=config, resume=True, eval_only=True, opts=opts))
    assert set(again) == set(analysis)


# ---------------------------------------------------------------------------------------------------------------------
# 7. CR_DETERMINISTIC=1 (read once by the library, hence a child process): a block's backward, same bits in two fresh processes
# ---------------------------------------------------------------------------------------------------------------------
DET_PROG = r'''
import hashlib, importlib, sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
t = importlib.import_module("test_gpu_mnasnet")
blk, out, got_g, ref64, ref32 = t._run_block("40to80_k5s2", "train")
torch.cuda.synchronize()
h = hashlib.sha256()
for k in sorted(got_g):
    h.update(got_g[k].contiguous().cpu().numpy().tobytes())
print("HASH", h.hexdigest(), len(got_g))
''' % (ROOT, os.path.join(ROOT, "tests"))


def test_deterministic_block_backward_is_bit_reproducible():
    env = dict(os.environ, CR_DETERMINISTIC="1", CR_PRECISION="fp32")
    lines = []
    for run in range(2):
        out = subprocess.run([sys.executable, "-c", DET_PROG], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        got = [l.split() for l in out.stdout.splitlines() if l.startswith("HASH")]
        assert len(got) == 1, out.stderr[-2000:]
        lines += got
    assert int(lines[0][2]) == 1 + 3 * 3                    # x and three (conv, gamma, beta) triples
    assert lines[0][1] == lines[1][1], "the block backward differs between two processes in deterministic mode"
