"""GPU: the ResNet-50 / ResNet-101 trunks (cubercnn/modeling/backbone/resnet.py, torchvision's Bottleneck) and the fused
projection-shortcut tail of csrc/resnet.hip (cr_bn_pair_fwd / cr_bn_pair_bwd).

torchvision is absent, so the references are float64 restatements from plain functionals (F.conv2d, F.batch_norm, F.relu, the
shortcut add, F.max_pool2d) over the module's own state dict ("parity unpinned" w.r.t. torchvision).

Bounds.  Kernels in isolation: the project's float32 module bound, 2e-5 relative L2 and 2e-4 max-norm; a bf16 output that is one
round-to-nearest of a float32 result: |got - ref| <= 2^-8 |ref| + 1e-6 max|ref|.  In f32 the pair forward must also have the BITS of
the two-call composition cr_bn_fwd(yb) -> cr_bn_fwd(ya, residual, relu) on the same inputs.  Blocks, trunk stages and gradients:
the ratio method of tests/test_gpu_mnasnet.py -- the restatement also runs in float32 on the CPU, its relative L2 distance from
float64 is `ref32_err`, and the product must stay within K_FWD * ref32_err (outputs, running statistics) or K_GRAD * ref32_err
(gradients) with the constants of tests/test_gpu_dla_types.py.  bf16 blocks: the yardstick is the same restatement in float32 with
the roundings of the bf16 mode written in -- weights, every convolution output and every block-level activation rounded to bf16
on the way forward, the gradients of those tensors on the way back (a straight-through rounding) -- so `ref32_err` there is the
error the number format itself causes in this block; the constants stay the same.  That bf16 yardstick is this file's own
definition (the other trunks' tests have no bf16 ratio check, so there is no project bound to take): it is built from plain
functionals only, shares no code with the product, and allows K times the error bf16 itself causes here, about 1e-2 at K = 2.3 .. 3.
Every ratio is printed.

Measured on MI355X.  Pair kernels, f32: relative L2 <= 1.6e-7 and max-norm <= 1.6e-6 of float64, <= 2.2e-7 / 2.1e-7 of the composition's
backward; forward bits equal to the composition's at all seven shapes; bf16 outputs: worst |got - ref| - bound = -6.7e-6.  Blocks
(ratio = error / ref32_err): outputs 0.52 .. 1.07, running statistics 0.36 .. 1.90 (K_FWD 2.966); gradients 0.19 .. 1.80 (K_GRAD
2.31), the largest on bn3.bias (train, composition 1.79; frozen identity block 1.77) and, in bf16, downsample.1.weight (1.80).  With
gradient sinks 0.65 .. 1.56.  Trunk stages 0.73 .. 1.00 in train and 0.65 .. 0.99 in eval mode.  Before the tail's frozen backward took
cr_colsum_wide for its bias sums, bn3.bias of the frozen f32 blocks measured 3.07 (64 -> 256) and 2.55 (256 -> 512)."""
import importlib
import os
import subprocess
import sys
import types

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
EPS, MOMENTUM = 1e-5, 0.1


def _mods():
    return (importlib.import_module("3dod_amd.cubercnn.modeling.backbone.resnet"), importlib.import_module("3dod_amd.hipops"),
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
# 1. the pair kernels in isolation
# ---------------------------------------------------------------------------------------------------------------------
# (C, M): 256 x 108 a partial statistics row; 256 x 17408 more than 256 rows: the unfused finalize; 32 x 131136 more than 2048
# rows: the lanes finalize, ragged; 512 x 4096 and 1024 x 1024 mid-range widths; 2048 x 32 one row per workgroup; 2048 x 1024 the
# real layer-4 map
PAIR_SHAPES = [(256, 108), (256, 17408), (32, 131136), (512, 4096), (1024, 1024), (2048, 32), (2048, 1024)]
SIDE_B = (1e-3, 0.03)          # eps and momentum of the second BatchNorm differ from the first's (1e-5, 0.1)


def _stats_rows(x):
    """[ceil(M / 64)][2][C] float32: sum and sum of squares of every 64 pixels, as the conv epilogues hand them over"""
    M, C = x.shape
    nparts = (M + 63) // 64
    xp = torch.zeros(nparts * 64, C, dtype=f64)
    xp[:M] = x.to(f64)
    xp = xp.view(nparts, 64, C)
    return torch.stack([xp.sum(1), (xp * xp).sum(1)], 1).to(f32).contiguous(), nparts


def _pair_inputs(C, M, dtype):
    g = torch.Generator().manual_seed(1000 * C + M)
    side = []
    for _ in range(2):
        gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
        beta = torch.randn(C, generator=g) * 0.3
        y = (torch.randn(M, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g)).to(dtype)
        rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
        stats, nparts = _stats_rows(y)
        side.append({"y": y, "gamma": gamma, "beta": beta, "rm": rm, "rv": rv, "stats": stats})
    dout = torch.randn(M, C, generator=g).to(dtype)
    return side[0], side[1], dout, nparts


def _dev(side):
    return {k: v.to(DEV) for k, v in side.items()}


def _pair_fwd(a, b, nparts):
    """-> out, mia, mib; a["rm"] ... are updated in place"""
    mn, ops, lib = _mods()
    return ops.bn_pair_fwd_raw(a["y"], b["y"], a["stats"], b["stats"], (a["gamma"], a["beta"], a["rm"], a["rv"], EPS, MOMENTUM),
                               (b["gamma"], b["beta"], b["rm"], b["rv"]) + SIDE_B)


def _composition_fwd(a, b, nparts):
    mn, ops, lib = _mods()
    M, C = a["y"].shape
    af = int(a["y"].dtype == f32)
    idn, out = torch.empty_like(b["y"]), torch.empty_like(a["y"])
    mia, mib = torch.empty(2, C, device=DEV), torch.empty(2, C, device=DEV)
    lib.call("cr_bn_fwd", b["y"], b["stats"], nparts, b["gamma"], b["beta"], None, idn, M, C, 0, SIDE_B[0], SIDE_B[1], mib, b["rm"],
             b["rv"], af)
    lib.call("cr_bn_fwd", a["y"], a["stats"], nparts, a["gamma"], a["beta"], idn, out, M, C, 1, EPS, MOMENTUM, mia, a["rm"], a["rv"],
             af)
    return out, mia, mib


def _pair_bwd(a, b, dout, out, mia, mib):
    mn, ops, lib = _mods()
    C = a["y"].shape[1]
    acc = [torch.full((C,), v, device=DEV) for v in (0.25, -0.5, 0.75, 1.5)]        # dgamma_a, dbeta_a, dgamma_b, dbeta_b
    dxa, dxb = ops.bn_pair_bwd_raw(dout, out, a["y"], b["y"], mia, mib, a["gamma"], b["gamma"], *acc)
    return [dxa, dxb] + acc


def _composition_bwd(a, b, dout, out, mia, mib):
    mn, ops, lib = _mods()
    M, C = a["y"].shape
    af = int(a["y"].dtype == f32)
    acc = [torch.full((C,), v, device=DEV) for v in (0.25, -0.5, 0.75, 1.5)]
    dxa, dres, dxb = torch.empty_like(out), torch.empty_like(out), torch.empty_like(out)
    lib.call("cr_bn_bwd", dout, out, a["y"], mia, a["gamma"], torch.empty(1025, 2, C, device=DEV), dxa, dres, acc[0], acc[1], M, C, 1,
             af)
    lib.call("cr_bn_bwd", dres, None, b["y"], mib, b["gamma"], torch.empty(1025, 2, C, device=DEV), dxb, None, acc[2], acc[3], M, C, 0,
             af)
    return [dxa, dxb] + acc


def _affine64(side, eps):
    y = side["y"].to(f64)
    mean, var = y.mean(0), y.var(0, unbiased=False)
    return (y - mean) / torch.sqrt(var + eps) * side["gamma"].to(f64) + side["beta"].to(f64), mean, var


def _running64(side, mean, var, momentum, M):
    unb = var * M / (M - 1) if M > 1 else var
    return (1 - momentum) * side["rm"].to(f64) + momentum * mean, (1 - momentum) * side["rv"].to(f64) + momentum * unb


def _check_rows(tag, rows):
    figs = [(n,) + _rel(g, r) for n, g, r in rows]
    for n, l2, mx in figs:
        print(f"{tag} {n}: rel L2 {l2:.3g}, max-norm {mx:.3g}")
    for n, l2, mx in figs:
        assert l2 < L2_F32 and mx < MX_F32, (tag, n, l2, mx)


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=lambda s: "C%dxM%d" % s)
def test_pair_kernels_against_float64_and_the_composition(shape, dtype):
    C, M = shape
    name = "bf16" if dtype == bf16 else "f32"
    tag = f"pair C={C} M={M} {name}"
    a0, b0, dout0, nparts = _pair_inputs(C, M, dtype)
    a, b, dout = _dev(a0), _dev(b0), dout0.to(DEV)
    out, mia, mib = _pair_fwd(a, b, nparts)
    ac, bc = _dev(a0), _dev(b0)
    out_c, mia_c, mib_c = _composition_fwd(ac, bc, nparts)
    torch.cuda.synchronize()

    # ---- forward against float64
    ta, mean_a, var_a = _affine64(a0, EPS)
    tb, mean_b, var_b = _affine64(b0, SIDE_B[0])
    out64 = F.relu(ta + tb)
    rows = [("mean a", mia[0], mean_a), ("invstd a", mia[1], 1 / torch.sqrt(var_a + EPS)),
            ("mean b", mib[0], mean_b), ("invstd b", mib[1], 1 / torch.sqrt(var_b + SIDE_B[0]))]
    for s0, s, mean, var, mom, nm in ((a0, a, mean_a, var_a, MOMENTUM, "a"), (b0, b, mean_b, var_b, SIDE_B[1], "b")):
        rm64, rv64 = _running64(s0, mean, var, mom, M)
        rows += [("running_mean " + nm, s["rm"], rm64), ("running_var " + nm, s["rv"], rv64)]
    if dtype == f32:
        rows.append(("out", out, out64))
        # the bits of the two-call composition
        for nm, x, y in (("out", out, out_c), ("mean_invstd a", mia, mia_c), ("mean_invstd b", mib, mib_c),
                         ("running_mean a", a["rm"], ac["rm"]), ("running_var a", a["rv"], ac["rv"]),
                         ("running_mean b", b["rm"], bc["rm"]), ("running_var b", b["rv"], bc["rv"])):
            assert torch.equal(x, y), f"{tag}: {nm} differs from the two-call composition in its bits"
    else:
        ex = _bf16_excess(out, out64)
        print(f"{tag} out: worst |got - ref| - bound = {ex:.3g}")
        assert ex <= 0.0, (tag, ex)
    _check_rows(tag, rows)

    # ---- backward against float64 (mask: the stored output; xh from the kernel's own mean / invstd, as the kernel forms it)
    got = _pair_bwd(a, b, dout, out, mia, mib)
    comp = _composition_bwd(a, b, dout, out, mia, mib)
    again = _pair_bwd(a, b, dout, out, mia, mib)
    torch.cuda.synchronize()
    g = dout0.to(f64) * (out.cpu() > 0).to(f64)
    sg = g.sum(0)
    ref = {}
    for nm, s0, mi in (("a", a0, mia), ("b", b0, mib)):
        mi = mi.to("cpu", f64)
        xh = (s0["y"].to(f64) - mi[0]) * mi[1]
        sgx = (g * xh).sum(0)
        ref["dx" + nm] = s0["gamma"].to(f64) * mi[1] * (g - sg / M - xh * sgx / M)
        ref["dgamma" + nm] = sgx
    pre = (0.25, -0.5, 0.75, 1.5)
    rows = [("dgamma a", got[2].cpu().to(f64) - pre[0], ref["dgammaa"]), ("dbeta a", got[3].cpu().to(f64) - pre[1], sg),
            ("dgamma b", got[4].cpu().to(f64) - pre[2], ref["dgammab"]), ("dbeta b", got[5].cpu().to(f64) - pre[3], sg)]
    if dtype == f32:
        rows += [("dxa", got[0], ref["dxa"]), ("dxb", got[1], ref["dxb"])]
        rows += [("dxa vs composition", got[0], comp[0]), ("dxb vs composition", got[1], comp[1])]
        rows += [(f"{nm} vs composition", got[i].cpu().to(f64) - pre[i - 2], comp[i].cpu().to(f64) - pre[i - 2])
                 for i, nm in ((2, "dgamma a"), (3, "dbeta a"), (4, "dgamma b"), (5, "dbeta b"))]
    else:
        for nm, x, r in (("dxa", got[0], ref["dxa"]), ("dxb", got[1], ref["dxb"])):
            ex = _bf16_excess(x, r)
            print(f"{tag} {nm}: worst |got - ref| - bound = {ex:.3g}")
            assert ex <= 0.0, (tag, nm, ex)
    _check_rows(tag, rows)

    # ---- two runs give identical bits (the forward too)
    a2, b2 = _dev(a0), _dev(b0)
    out2, mia2, mib2 = _pair_fwd(a2, b2, nparts)
    for x, y in [(out, out2), (mia, mia2), (mib, mib2), (a["rm"], a2["rm"]), (a["rv"], a2["rv"]), (b["rm"], b2["rm"]),
                 (b["rv"], b2["rv"])] + list(zip(got, again)):
        assert torch.equal(x, y), f"{tag}: two runs on the same inputs differ"


def test_pair_arguments_are_checked():
    """C = 24 (256 % 3 != 0), C = 4096 and a short workspace are refused, and nothing is launched: the outputs keep their fill"""
    mn, ops, lib = _mods()
    for C in (24, 4096, 12):
        M = 70
        y = torch.zeros(M, C, device=DEV)
        v = torch.ones(C, device=DEV)
        stats = torch.zeros(2, 2, C, device=DEV)
        out = torch.full((M, C), 7.0, device=DEV)
        mi = torch.full((2, C), 7.0, device=DEV)
        with pytest.raises(lib.CrError):
            lib.call("cr_bn_pair_fwd", y, y, stats, stats, 2, v, v, v, v, out, M, C, EPS, 0.1, EPS, 0.1, mi, mi.clone(), None, None,
                     None, None, 1)
        dx = torch.full((M, C), 7.0, device=DEV)
        acc = [torch.full((C,), 7.0, device=DEV) for _ in range(4)]
        n = 1025 * 3 * C
        with pytest.raises(lib.CrError):
            lib.call("cr_bn_pair_bwd", y, y, y, y, mi, mi, v, v, torch.empty(n, device=DEV), n, dx, dx.clone(), *acc, M, C, 1)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((mi == 7.0).all()) and bool((dx == 7.0).all())
        assert all(bool((t == 7.0).all()) for t in acc)
    C, M = 64, 70
    y, v, mi = torch.zeros(M, C, device=DEV), torch.ones(C, device=DEV), torch.ones(2, C, device=DEV)
    acc = [torch.zeros(C, device=DEV) for _ in range(4)]
    n = ops.bn_pair_bwd_ws_floats(M, C)
    assert n == (1 + 1) * 3 * C                                # 32 rows of 8 channel groups per workgroup, 8 rows per thread: one workgroup
    with pytest.raises(lib.CrError):                           # one float short
        lib.call("cr_bn_pair_bwd", y, y, y, y, mi, mi, v, v, torch.empty(n, device=DEV), n - 1, torch.empty_like(y),
                 torch.empty_like(y), *acc, M, C, 1)
    with pytest.raises(lib.CrError):                           # the statistics rows do not match M
        lib.call("cr_bn_pair_fwd", y, y, torch.zeros(3, 2, C, device=DEV), torch.zeros(3, 2, C, device=DEV), 3, v, v, v, v,
                 torch.empty_like(y), M, C, EPS, 0.1, EPS, 0.1, mi, mi.clone(), None, None, None, None, 1)
    for shared in ("mean_invstd", "running_mean", "running_var across"):     # a buffer of one BatchNorm handed in for the other too
        bufs = [mi.clone(), mi.clone(), v.clone(), v.clone(), v.clone(), v.clone()]  # mia, mib, rma, rva, rmb, rvb
        if shared == "mean_invstd":
            bufs[1] = bufs[0]
        elif shared == "running_mean":
            bufs[4] = bufs[2]
        else:
            bufs[5] = bufs[2]
        out = torch.full((M, C), 7.0, device=DEV)
        with pytest.raises(lib.CrError):
            lib.call("cr_bn_pair_fwd", y, y, torch.zeros(2, 2, C, device=DEV), torch.zeros(2, 2, C, device=DEV), 2, v, v, v, v, out, M,
                     C, EPS, 0.1, EPS, 0.1, *bufs, 1)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), shared
    with pytest.raises(lib.CrError):                           # one gradient buffer for both BatchNorms
        lib.call("cr_bn_pair_bwd", y, y, y, y, mi, mi, v, v, torch.empty(n, device=DEV), n, torch.empty_like(y),
                 torch.empty_like(y), acc[0], acc[1], acc[0], acc[1], M, C, 1)


# ---------------------------------------------------------------------------------------------------------------------
# 2. blocks against float64
# ---------------------------------------------------------------------------------------------------------------------
class _Q(torch.autograd.Function):
    """straight-through bf16 rounding of a tensor and of its gradient: what storing it in bf16 does in both directions"""

    @staticmethod
    def forward(ctx, t):
        return t.to(bf16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(bf16).to(g.dtype)


def _bn(t, p, k, training, new):
    rm, rv = p[k + ".running_mean"].detach().clone(), p[k + ".running_var"].detach().clone()
    y = F.batch_norm(t, rm, rv, p[k + ".weight"], p[k + ".bias"], training, MOMENTUM, EPS)
    if new is not None:
        new[k + ".running_mean"], new[k + ".running_var"] = rm, rv
    return y


def _ref_bottleneck(p, pre, x, stride, training, new=None, q=lambda t: t):
    """torchvision's Bottleneck.forward (v1.5) over the state dict p; q: identity, or the bf16 mode's roundings"""
    t = q(F.relu(_bn(q(F.conv2d(x, q(p[pre + "conv1.weight"]))), p, pre + "bn1", training, new)))
    t = q(F.relu(_bn(q(F.conv2d(t, q(p[pre + "conv2.weight"]), None, stride, 1)), p, pre + "bn2", training, new)))
    t = _bn(q(F.conv2d(t, q(p[pre + "conv3.weight"]))), p, pre + "bn3", training, new)
    idn = x
    if pre + "downsample.0.weight" in p:
        idn = _bn(q(F.conv2d(x, q(p[pre + "downsample.0.weight"]), None, stride)), p, pre + "downsample.1", training, new)
    return q(F.relu(t + idn))


# inplanes, planes, stride, downsample, input (N, H, W)
BLOCK_CASES = {"64_64_s1_ds": (64, 64, 1, True, (2, 8, 8)), "256_128_s2_ds": (256, 128, 2, True, (2, 8, 8)),
               "1024_512_s2_ds": (1024, 512, 2, True, (2, 4, 4)), "2048_512_identity": (2048, 512, 1, False, (2, 2, 2))}


def _make_block(case, seed):
    mn, ops, lib = _mods()
    inp, planes, stride, ds, _ = BLOCK_CASES[case]
    torch.manual_seed(seed)
    down = None
    if ds:
        down = torch.nn.Sequential(torch.nn.Conv2d(inp, planes * 4, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(planes * 4))
    blk = mn.Bottleneck(inp, planes, stride, down)
    for m in blk.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    _randomise_bn(blk, torch.Generator().manual_seed(seed + 1))
    return mn.to_channels_last(blk)


def _block_reference(blk, x, R, stride, training, dtype, emu):
    p = {kk: v.detach().clone().to(dtype) for kk, v in blk.state_dict().items() if "num_batches" not in kk}
    names = [kk for kk in p if "running" not in kk]
    leaves = [p[kk].requires_grad_(True) for kk in names]
    xr = x.to(dtype).requires_grad_(True)
    new = {}
    out = _ref_bottleneck(p, "", xr, stride, training, new, _Q.apply if emu else (lambda t: t))
    grads = torch.autograd.grad((out * R.to(dtype)).sum(), [xr] + leaves)
    return out.detach(), new, dict(zip(["x"] + names, grads)), names


def _run_block(case, mode, precision="fp32", fused=True, seed=41):
    """-> the block after one call, its output, its gradients, (ref64, yardstick restatement)"""
    mn, ops, lib = _mods()
    inp, planes, stride, ds, (N, H, W) = BLOCK_CASES[case]
    training = mode == "train"
    adt = bf16 if precision == "bf16" else f32
    blk = _make_block(case, seed)
    blk.fused_tail = fused
    gen = torch.Generator().manual_seed(seed + 2)
    exact = (lambda t: t.to(bf16).to(f32)) if adt == bf16 else (lambda t: t)  # bf16 mode: input and cotangent exact in bf16
    x = exact(torch.randn(N, inp, H, W, generator=gen))
    R = exact(torch.randn(N, planes * 4, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=gen))
    ref64 = _block_reference(blk, x, R, stride, training, f64, False)
    yard = _block_reference(blk, x, R, stride, training, f32, adt == bf16)
    blk = blk.to(DEV)
    blk.train(training)
    xg = _nhwc(x).to(DEV, adt).requires_grad_(True)
    params = dict(blk.named_parameters())
    prev = ops.set_precision(precision)
    try:
        out = blk(xg)
        assert out.dtype == adt
        names = ref64[3]
        gs = torch.autograd.grad((out.float() * _nhwc(R).to(DEV)).sum(), [xg] + [params[kk] for kk in names])
    finally:
        ops.set_precision(prev)
    got_g = dict(zip(["x"] + names, gs))
    got_g["x"] = _nchw(got_g["x"])
    return blk, out, got_g, ref64, yard


def _check_block(case, mode, precision, fused):
    blk, out, got_g, ref64, yard = _run_block(case, mode, precision, fused)
    training = mode == "train"
    tag = f"bottleneck {case} {mode} {precision} {'fused' if fused else 'composition'}"
    rows = [("out", K_FWD, _rel(_nchw(out), ref64[0])[0], _rel(yard[0], ref64[0])[0])]
    sd = blk.state_dict()
    assert len(ref64[1]) == (8 if BLOCK_CASES[case][3] else 6)
    for kk, v in ref64[1].items():
        if training:
            rows.append((kk, K_FWD, _rel(sd[kk], v)[0], _rel(yard[1][kk], v)[0]))
        else:
            assert torch.equal(sd[kk].cpu().to(f64), v), f"{kk} changed in {mode} mode"
    for kk, g in got_g.items():
        assert tuple(g.shape) == tuple(ref64[2][kk].shape), (kk, g.shape)
        assert g.dtype == (f32 if kk != "x" or precision == "fp32" else bf16)
        rows.append(("grad " + kk, K_GRAD, _rel(g, ref64[2][kk])[0], _rel(yard[2][kk], ref64[2][kk])[0]))
    for name, K, err, r32 in rows:
        print(f"{tag} {name}: error {err:.3g}, ref32_err {r32:.3g}, ratio {err / max(r32, 1e-300):.3f}")
    for name, K, err, r32 in rows:
        assert err <= K * r32, (tag, name, err, r32, err / max(r32, 1e-300), K)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["train", "frozen"])
@pytest.mark.parametrize("case", list(BLOCK_CASES))
def test_block_against_float64(case, mode, precision):
    """output, every BatchNorm's running statistics after one call and the gradients of the input and every parameter under a
    random cotangent, each within K * ref32_err of float64; frozen: the running statistics keep their bits.  Blocks with a
    downsample run with the fused tail and with the two-call composition."""
    _check_block(case, mode, precision, True)
    if BLOCK_CASES[case][3]:
        _check_block(case, mode, precision, False)


@pytest.mark.parametrize("case", [c for c in BLOCK_CASES if BLOCK_CASES[c][3]])
def test_fused_tail_against_the_composition(case):
    """fused_tail True against False on the same weights and input.  Train mode, f32: both are within K * ref32_err of float64
    (test_block_against_float64), hence within twice that of each other; frozen mode never reaches the pair kernels: same bits."""
    for mode in ("train", "frozen"):
        blk_f, out_f, g_f, ref64, ref32 = _run_block(case, mode, "fp32", True)
        blk_c, out_c, g_c, _, _ = _run_block(case, mode, "fp32", False)
        e32 = _rel(ref32[0], ref64[0])[0]
        d = _rel(out_f, out_c)[0]
        print(f"tail fused vs composition {case} {mode} out: {d:.3g} (ref32_err {e32:.3g}), same bits: {torch.equal(out_f, out_c)}")
        assert d <= 2 * K_FWD * e32
        if mode == "frozen":
            assert torch.equal(out_f, out_c)
        for kk in g_f:
            e32 = _rel(ref32[2][kk], ref64[2][kk])[0]
            d = _rel(g_f[kk], g_c[kk])[0]
            print(f"tail fused vs composition {case} {mode} grad {kk}: {d:.3g} (ref32_err {e32:.3g})")
            assert d <= 2 * K_GRAD * e32, (case, mode, kk, d, e32)
        sd_f, sd_c = blk_f.state_dict(), blk_c.state_dict()
        for kk in sd_f:
            if "running" in kk:
                d = _rel(sd_f[kk], sd_c[kk])[0]
                assert d <= 2 * K_FWD * max(_rel(ref32[1][kk], ref64[1][kk])[0], 1e-300) if mode == "train" else d == 0.0, (kk, d)


def test_tail_with_gradient_sinks_and_deferred_weight_gradients():
    """the route the train step takes: parameters with gradient sinks (kernels accumulate into them, autograd sees None) inside
    deferred_wgrad(), and the block input's two consumers meeting in conv1's backward-data through the gradient slot -- against
    the same block without sinks"""
    mn, ops, lib = _mods()
    case = "256_128_s2_ds"
    blk, out, g_plain, ref64, ref32 = _run_block(case, "train")
    blk2 = _make_block(case, 41).to(DEV).train()
    inp, planes, stride, ds, (N, H, W) = BLOCK_CASES[case]
    gen = torch.Generator().manual_seed(43)
    x = torch.randn(N, inp, H, W, generator=gen)               # the input and cotangent of _run_block
    R = torch.randn(N, planes * 4, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=gen)
    sinks = {}
    for n, p in blk2.named_parameters():
        sinks[n] = torch.full(p.shape, 0.5, device=DEV).contiguous(memory_format=torch.channels_last) if p.dim() == 4 \
            else torch.full(p.shape, 0.5, device=DEV)
        p._cr_grad = sinks[n]
    xg = _nhwc(x).to(DEV).requires_grad_(True)
    with ops.deferred_wgrad():
        out2 = blk2(xg)
        (gx,) = torch.autograd.grad((out2 * _nhwc(R).to(DEV)).sum(), [xg])
    assert ops.wgrad_pending() == 0
    assert all(p.grad is None for p in blk2.parameters())
    for kk, g in g_plain.items():
        got = _nchw(gx) if kk == "x" else sinks[kk] - 0.5
        e32 = _rel(ref32[2][kk], ref64[2][kk])[0]
        err = _rel(got, ref64[2][kk])[0]
        print(f"sinks {kk}: error {err:.3g}, ref32_err {e32:.3g}, ratio {err / max(e32, 1e-300):.3f}")
        # the sink holds 0.5 + g: subtracting costs up to 2^-24 * 0.5 per element on top of the gradient's own error
        floor = 2.0 ** -24 * 0.5 * (ref64[2][kk].numel() ** 0.5) / float(ref64[2][kk].norm())
        assert err <= K_GRAD * e32 + floor, (kk, err, e32)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the trunk
# ---------------------------------------------------------------------------------------------------------------------
LAYERS50 = [3, 4, 6, 3]
ORDER = ["p2", "p3", "p4", "p5"]


def _cfg(depth):
    return types.SimpleNamespace(MODEL=types.SimpleNamespace(RESNETS=types.SimpleNamespace(DEPTH=depth)))


def _ref_stage(p, stage, x, training):
    li = ORDER.index(stage) + 1
    if stage == "p2":
        x = F.relu(_bn(F.conv2d(x, p["conv1.weight"], None, 2, 3), p, "bn1", training, None))
        x = F.max_pool2d(x, 3, 2, 1)
    for b in range(LAYERS50[li - 1]):
        x = _ref_bottleneck(p, f"layer{li}.{b}.", x, 2 if (b == 0 and li > 1) else 1, training)
    return x


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
    torch.manual_seed(51)
    net = mn.ResNet(_cfg(50), None)
    _randomise_bn(net, torch.Generator().manual_seed(52))
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(53))
    return net.to(DEV), sd0, _stage_refs(sd0, x), x


def _gpu_stage(net, stage, xin):
    """xin: the stage's NCHW input -> its NHWC output"""
    mn, ops, lib = _mods()
    x = _nhwc(xin.to(f32))
    if stage == "p2":                                    # the RGB stem reads 4 channels in float32: 3 real + a zero
        x = torch.cat([x, torch.zeros(x.shape[0], x.shape[1], x.shape[2], 1)], 3).to(DEV).contiguous()
        x = ops.maxpool3x3s2(mn._conv_bn(x, net.conv1, net.bn1, relu=True))
    else:
        x = x.to(DEV)
    return getattr(net, "layer%d" % (ORDER.index(stage) + 1))(x)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_trunk_stage_by_stage(trunk, mode):
    net, sd0, refs, x = trunk
    training = mode == "train"
    net.load_state_dict(sd0)
    net.train(training)
    ratios = {}
    shapes = {"p2": (2, 16, 16, 256), "p3": (2, 8, 8, 512), "p4": (2, 4, 4, 1024), "p5": (2, 2, 2, 2048)}
    with torch.no_grad():
        for stage in ORDER:
            xin, o64, r32 = refs[(training, stage)]
            got = _gpu_stage(net, stage, xin)
            assert tuple(got.shape) == shapes[stage] == tuple(_nhwc(o64).shape), (stage, got.shape)
            err = _rel(_nchw(got), o64)[0]
            ratios[stage] = err / r32
            print(f"resnet50 {mode} {stage}: error {err:.3g}, ref32_err {r32:.3g}, ratio {ratios[stage]:.3f}")
    for stage, r in ratios.items():
        assert r <= K_FWD, (mode, stage, r, K_FWD)


def test_trunk_forward_and_load_state_dict_round_trip(trunk):
    mn, ops, lib = _mods()
    net, sd0, refs, x = trunk
    net.load_state_dict(sd0)
    net.eval()
    xg = torch.cat([_nhwc(x), torch.zeros(2, 64, 64, 1)], 3).to(DEV).contiguous()
    with torch.no_grad():
        out = net(xg)
    assert list(out.keys()) == ["p2", "p3", "p4", "p5", "p6"]
    for name, (s, c) in {"p2": (16, 256), "p3": (8, 512), "p4": (4, 1024), "p5": (2, 2048), "p6": (1, 2048)}.items():
        assert tuple(out[name].shape) == (2, s, s, c), (name, out[name].shape)
    assert torch.equal(out["p6"], out["p5"][:, ::2, ::2])
    # another initialisation gives other features; its state dict loaded back gives the first ones, bit for bit
    torch.manual_seed(99)
    other = mn.ResNet(_cfg(50), None).to(DEV).eval()
    assert list(other.state_dict().keys()) == list(sd0.keys())
    with torch.no_grad():
        assert _rel(other(xg)["p3"], out["p3"])[0] > 1e-2
        other.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
        again = other(xg)
    for k in out:
        assert torch.equal(again[k], out[k]), k


def test_resnet101_forward_shapes():
    mn, ops, lib = _mods()
    torch.manual_seed(61)
    net = mn.ResNet(_cfg(101), None).to(DEV).train()
    assert [len(getattr(net, "layer%d" % i)) for i in (1, 2, 3, 4)] == [3, 4, 23, 3]
    xg = torch.randn(2, 64, 64, 4, generator=torch.Generator().manual_seed(62)).to(DEV)
    with torch.no_grad():
        out = net(xg)
    for name, (s, c) in {"p2": (16, 256), "p3": (8, 512), "p4": (4, 1024), "p5": (2, 2048), "p6": (1, 2048)}.items():
        assert tuple(out[name].shape) == (2, s, s, c), (name, out[name].shape)
        assert bool(torch.isfinite(out[name]).all()), name


# ---------------------------------------------------------------------------------------------------------------------
# 4. whole model
# ---------------------------------------------------------------------------------------------------------------------
def _build_model(seed=0, depth=50):
    syn = importlib.import_module("3dod_amd.synthetic")
    modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
    solver = importlib.import_module("3dod_amd.cubercnn.solver")
    cfg = syn.make_cfg(os.path.join(ROOT, "configs", "cubercnn_ResNet%d_FPN.yaml" % depth),
                       overrides=["MODEL.DEVICE", "cuda:0", "VIS_PERIOD", 0, "log", False, "SOLVER.BASE_LR", 0.0025])
    torch.manual_seed(seed)
    model = modeling.build_model(cfg).to(DEV).train()
    opt = solver.build_optimizer(cfg, model)
    return cfg, model, opt, syn, solver


def test_pyramid_keys_and_shapes():
    cfg, model, opt, syn, solver = _build_model()
    batch = syn.make_batch(2, 3, with_gt=False, size=256)
    with torch.no_grad():
        images, x = model.preprocess_image(batch)
        feats = model.backbone(x)
    # detectron2 FPN + LastLevelMaxPool: "p7" = max_pool2d(k=1, s=2) of the BOTTOM-UP p5 (its in_feature exists there)
    assert list(feats.keys()) == ["p2", "p3", "p4", "p5", "p6", "p7"]
    for name, s, c in (("p2", 64, 256), ("p3", 32, 256), ("p4", 16, 256), ("p5", 8, 256), ("p6", 4, 256), ("p7", 4, 2048)):
        assert tuple(feats[name].shape) == (2, s, s, c), (name, feats[name].shape)


def test_resnet50_train_steps_learn():
    """as test_resnet_train_steps_learn of tests/test_gpu_resnet.py; after the first step every trunk parameter's gradient sink
    holds a finite, non-zero gradient (the downsample convolutions and BatchNorms included)"""
    mn, ops, lib = _mods()
    cfg, model, opt, syn, solver = _build_model()
    d2 = importlib.import_module("3dod_amd.d2lite")
    step = solver.TrainStep(cfg, model, opt, world_size=1)
    batch = syn.make_batch(2, 7, size=256)
    totals = []
    with d2.EventStorage(0):
        for i in range(8):
            step(batch)
            rep = step.report()
            totals.append(rep["total_loss"])
            if i == 0:
                for name, p in model.backbone.bottom_up.named_parameters():
                    gbuf = ops.grad_sink(p)
                    assert gbuf is not None and bool(torch.isfinite(gbuf).all()), name
                    assert float(gbuf.abs().sum()) > 0.0, f"{name} received no gradient"
    print("resnet50 totals", totals)
    assert all(t == t and abs(t) < 1e4 for t in totals), totals
    assert rep["iterations_explode"] == 0, rep
    assert min(totals[-3:]) < totals[0], totals


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


# CR_DETERMINISTIC=1 is read once by the library, hence a child process: one train step from the same state twice
DET_PROG = r'''
import hashlib, importlib, sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
t = importlib.import_module("test_gpu_resnet_bottleneck")
ops = importlib.import_module("3dod_amd.hipops")
d2 = importlib.import_module("3dod_amd.d2lite")
for run in range(2):
    cfg, model, opt, syn, solver = t._build_model(seed=0)
    step = solver.TrainStep(cfg, model, opt, world_size=1)
    with d2.EventStorage(0):
        step(syn.make_batch(2, 7, size=256))
        rep = step.report()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    n = 0
    for name, p in model.named_parameters():
        g = ops.grad_sink(p)
        if g is not None:
            h.update(g.contiguous().cpu().numpy().tobytes()); n += 1
        h.update(p.detach().contiguous().cpu().numpy().tobytes())
    for k, v in sorted(model.backbone.bottom_up.state_dict().items()):
        h.update(v.contiguous().cpu().numpy().tobytes())
    print("HASH", h.hexdigest(), n, repr(rep["total_loss"]))
''' % (ROOT, os.path.join(ROOT, "tests"))


def test_deterministic_step_is_bit_reproducible():
    env = dict(os.environ, CR_DETERMINISTIC="1", CR_PRECISION="fp32")
    out = subprocess.run([sys.executable, "-c", DET_PROG], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    got = [l.split() for l in out.stdout.splitlines() if l.startswith("HASH")]
    assert len(got) == 2, out.stderr[-2000:]
    print(got)
    assert int(got[0][2]) >= 161                              # the trunk's 161 parameters have gradient sinks
    assert got[0][1:] == got[1][1:], "one train step differs between two runs in deterministic mode"
