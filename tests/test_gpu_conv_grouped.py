"""GPU: the grouped 3x3 convolution kernels (csrc/conv_grouped.hip) against float64 ATen, element by element.

Bound (tests/f64_bound.py): |got - ref| <= C * u * sqrt(K) * absref with the project's C = 4, K = 9 * cg for the forward and the
backward-data pass, K = N * Ho * Wo for the weight and bias gradients; absref is the same contraction over magnitudes.  In bf16
mode the float64 reference is computed on the bf16-rounded activations (the weights stay f32, as in the kernels) and a
bf16-stored result gets 2^-8 * |ref| on top for its one output rounding.  Epilogue terms (bias, residual, accumulate) add
their magnitude to absref and one to K each.

Shapes: N = 2, (H, W) in {(7, 9), (8, 8)}, stride 1 and 2, every (C, groups) of the DLA-X trunks (cg = 2, 4, 8, 16, 32 at 32 groups;
4 and 32 at 64 groups), plus 2 x 40 x 40 at C = 64 (3200 output pixels: 50 forward workgroup rows, 25 pixel ranges in the weight
gradient's first pass).  M = 2 * 7 * 9 = 126 is not a multiple of 64: the tail statistics row is partial."""
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

import f64_bound as fb

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f64 = torch.float64

CHANNELS = [(64, 32), (128, 32), (256, 32), (512, 32), (1024, 32), (256, 64), (2048, 64)]
CASES = [(2, H, W, C, g, s) for (C, g) in CHANNELS for (H, W) in ((7, 9), (8, 8)) for s in (1, 2)] + [(2, 40, 40, 64, 32, 1)]


def _ops():
    return importlib.import_module("3dod_amd.hipops")


@pytest.fixture(params=["fp32", "bf16"])
def mode(request):
    ops = _ops()
    prev = ops.set_precision(request.param)
    yield request.param
    ops.set_precision(prev)


def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV).to(dtype)


def _nchw(t):
    return t.detach().permute(0, 3, 1, 2).to("cpu", f64)


def _problem(N, H, W, C, groups, stride, mode, seed=0):
    """operands as the kernels see them (activations rounded to the mode's storage type) and their float64 copies"""
    gen = torch.Generator().manual_seed(1000 * C + 10 * H + stride + seed)
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    cg = C // groups
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dt).float()
    p = {"x": rnd(N, C, H, W), "dy": rnd(N, C, Ho, Wo), "res": rnd(N, C, Ho, Wo), "acc": rnd(N, C, H, W),
         "w": torch.randn(C, cg, 3, 3, generator=gen) * math.sqrt(2.0 / (9 * cg)), "bias": torch.randn(C, generator=gen),
         "dw0": torch.randn(C, cg, 3, 3, generator=gen), "db0": torch.randn(C, generator=gen)}
    p.update(dt=dt, cg=cg, Ho=Ho, Wo=Wo, M=N * Ho * Wo)
    return p


def _check(got, ref, absref, K, what, out_dtype=torch.float32):
    if out_dtype == torch.bfloat16:                       # one rounding of the stored result: + 2^-8 |ref|
        absref = absref + 2.0 ** -8 * ref.abs() / (fb.C * fb.U * math.sqrt(K))
    r = fb.report(got, ref, absref, K)
    print(f"{what}: worst ratio {r['ratio']:.3f} of {fb.C}, normwise {r['norm']:.3g}, K {K}")
    return fb.check(got, ref, absref, K, what)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N{}_{}x{}_C{}_g{}_s{}".format(*c))
def test_three_directions_against_float64(case, mode):
    N, H, W, C, groups, stride = case
    ops = _ops()
    p = _problem(N, H, W, C, groups, stride, mode)
    dt, cg, M = p["dt"], p["cg"], p["M"]
    x64, w64, dy64 = p["x"].to(f64), p["w"].to(f64), p["dy"].to(f64)
    x, dy = _nhwc(p["x"], dt), _nhwc(p["dy"], dt)
    w = p["w"].to(DEV).contiguous(memory_format=torch.channels_last)
    tag = f"{case} {mode}"

    # forward, with the statistics rows of the plain convolution
    nparts = (M + 63) // 64
    stats = torch.full((nparts, 2, C), float("nan"), device=DEV)
    y = ops.conv_grouped_fwd_raw(x, w, groups, stride, stats=stats)
    assert y.dtype == dt and tuple(y.shape) == (N, p["Ho"], p["Wo"], C)
    ref = F.conv2d(x64, w64, None, stride, 1, groups=groups)
    absref = F.conv2d(x64.abs(), w64.abs(), None, stride, 1, groups=groups)
    _check(_nchw(y), ref, absref, 9 * cg, "forward " + tag, dt)
    rows = y.detach().to("cpu", f64).view(M, C)
    rows = torch.cat([rows, rows.new_zeros(nparts * 64 - M, C)]).view(nparts, 64, C)      # the tail row is partial
    s_ref = torch.stack([rows.sum(1), (rows * rows).sum(1)], 1)
    s_abs = torch.stack([rows.abs().sum(1), (rows * rows).sum(1)], 1)
    _check(stats.cpu(), s_ref, s_abs, 64, "statistics rows " + tag)

    # forward epilogue: bias + residual + ReLU
    res = _nhwc(p["res"], dt)
    bias = p["bias"].to(DEV)
    y2 = ops.conv_grouped_fwd_raw(x, w, groups, stride, bias=bias, residual=res, relu=True)
    b64, r64 = p["bias"].to(f64).view(1, C, 1, 1), p["res"].to(f64)
    _check(_nchw(y2), torch.relu(ref + b64 + r64), absref + b64.abs() + r64.abs(), 9 * cg + 2, "forward epilogue " + tag, dt)

    # backward-data, plain and with an accumulate tensor
    grad_in = lambda d, ww: torch.nn.grad.conv2d_input((N, C, H, W), ww, d, stride, 1, groups=groups)
    dref, dabs = grad_in(dy64, w64), grad_in(dy64.abs(), w64.abs())
    dx = ops.conv_grouped_bwd_data_raw(dy, w, (N, H, W, C), groups, stride)
    assert dx.dtype == dt
    _check(_nchw(dx), dref, dabs, 9 * cg, "backward-data " + tag, dt)
    acc = _nhwc(p["acc"], dt)
    dx2 = ops.conv_grouped_bwd_data_raw(dy, w, (N, H, W, C), groups, stride, accumulate=acc)
    a64 = p["acc"].to(f64)
    _check(_nchw(dx2), dref + a64, dabs + a64.abs(), 9 * cg + 1, "backward-data accumulate " + tag, dt)

    # weight gradient with the fused bias gradient: written, and added into a sink; twice -> bit-equal
    grad_w = lambda d, xx: torch.nn.grad.conv2d_weight(xx, (C, cg, 3, 3), d, stride, 1, groups=groups)
    wref, wabs = grad_w(dy64, x64), grad_w(dy64.abs(), x64.abs())
    bref, babs = dy64.sum((0, 2, 3)), dy64.abs().sum((0, 2, 3))
    db0 = p["db0"].to(f64)
    runs = []
    for _ in range(2):
        db = p["db0"].to(DEV)
        dw = ops.conv_grouped_bwd_weight_raw(dy, x, groups, stride, bias_acc=db)
        runs.append((dw.clone(), db.clone()))
    dw, db = runs[0]
    assert tuple(dw.shape) == (C, cg, 3, 3) and dw.is_contiguous(memory_format=torch.channels_last)
    _check(dw.cpu(), wref, wabs, M, "weight gradient " + tag)
    _check(db.cpu(), bref + db0, babs + db0.abs(), M + 1, "bias gradient " + tag)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "weight gradient differs between two runs"
    sinks = []
    for _ in range(2):
        sink = p["dw0"].to(DEV).contiguous(memory_format=torch.channels_last)
        assert ops.conv_grouped_bwd_weight_raw(dy, x, groups, stride, sink=sink) is None
        sinks.append(sink)
    d064 = p["dw0"].to(f64)
    _check(sinks[0].cpu(), wref + d064, wabs + d064.abs(), M + 1, "weight gradient into a sink " + tag)
    assert torch.equal(sinks[0], sinks[1]), "accumulated weight gradient differs between two runs"


def test_split_mode_runs_the_f32_arithmetic():
    """fp32x3 has no grouped variant: float32 tensors take the same kernels in both float32 modes, bit for bit"""
    ops = _ops()
    p = _problem(2, 7, 9, 128, 32, 2, "fp32")
    x, dy = _nhwc(p["x"], torch.float32), _nhwc(p["dy"], torch.float32)
    w = p["w"].to(DEV).contiguous(memory_format=torch.channels_last)
    outs = []
    for m in ("fp32", "fp32x3"):
        prev = ops.set_precision(m)
        try:
            outs.append((ops.conv_grouped_fwd_raw(x, w, 32, 2), ops.conv_grouped_bwd_data_raw(dy, w, x.shape, 32, 2),
                         ops.conv_grouped_bwd_weight_raw(dy, x, 32, 2)))
        finally:
            ops.set_precision(prev)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("C,groups", [(96, 32), (2048, 32), (64, 16), (192, 64)])
def test_unsupported_geometry_is_an_error_not_a_launch(C, groups):
    """cg = 3, 64, 4 at 16 groups, 3: CrError from the argument check, and the output buffers keep their contents"""
    ops = _ops()
    lib = importlib.import_module("3dod_amd._lib")
    cg = C // groups
    x = torch.randn(1, 4, 4, C, device=DEV)
    w = torch.randn(C, cg, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last)
    out = torch.full((1, 4, 4, C), 7.0, device=DEV)
    dw = torch.full((C, cg, 3, 3), 7.0, device=DEV).contiguous(memory_format=torch.channels_last)
    ws = torch.empty((C * 9 * cg + C,), device=DEV)
    with pytest.raises(lib.CrError, match="cr_conv2d_grouped_fwd"):
        lib.call("cr_conv2d_grouped_fwd", x, w, out, 1, 4, 4, C, C, groups, 3, 1, 1, None, None, 0, None, 1)
    with pytest.raises(lib.CrError, match="cr_conv2d_grouped_bwd_data"):
        lib.call("cr_conv2d_grouped_bwd_data", x, w, out, 1, 4, 4, C, C, groups, 3, 1, 1, 1, None)
    with pytest.raises(lib.CrError, match="cr_conv2d_grouped_bwd_weight"):
        lib.call("cr_conv2d_grouped_bwd_weight", x, x, dw, None, 1, 4, 4, C, C, groups, 3, 1, 1, 0, 1, ws, ws.numel())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dw == 7.0).all())


def test_other_kernel_sizes_strides_and_short_workspace_are_errors():
    lib = importlib.import_module("3dod_amd._lib")
    C, groups, cg = 64, 32, 2
    x = torch.randn(1, 4, 4, C, device=DEV)
    w = torch.randn(C, cg, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last)
    out = torch.full((1, 4, 4, C), 7.0, device=DEV)
    for ks, stride, pad, cout in ((1, 1, 0, C), (3, 3, 1, C), (3, 1, 0, C), (3, 1, 1, 2 * C)):
        with pytest.raises(lib.CrError):
            lib.call("cr_conv2d_grouped_fwd", x, w, out, 1, 4, 4, C, cout, groups, ks, stride, pad, None, None, 0, None, 1)
    dw = torch.full((C, cg, 3, 3), 7.0, device=DEV).contiguous(memory_format=torch.channels_last)
    ws = torch.empty((C * 9 * cg + C,), device=DEV)
    with pytest.raises(lib.CrError, match="workspace"):
        lib.call("cr_conv2d_grouped_bwd_weight", x, x, dw, None, 1, 4, 4, C, C, groups, 3, 1, 1, 0, 1, ws, ws.numel() - 1)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dw == 7.0).all())
