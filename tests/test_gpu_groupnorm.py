"""GPU: the GroupNorm kernels (csrc/groupnorm.hip) in isolation against float64 F.group_norm (+ F.relu) on the CPU.

G = 32, float32 and bf16, ReLU off and on.  Inputs: randn * (rand(C) + 0.5) + 3 * randn(C) (per-channel scale and an offset of
several sigma), gamma with random signs.  The gradient accumulators are pre-filled (0.25 / -0.5): the kernels add.
Bounds: float32 -- y, dx, dgamma, dbeta, mean, rstd within the project's module bound (2e-5 relative L2, 2e-4 max-norm);
bf16 (inputs exact in bf16) -- y and dx within |got - ref| <= 2^-8 |ref| + 1e-6 max|ref| (tests/test_gpu_resnet_bottleneck.py),
the float32 quantities (mean, rstd, dgamma, dbeta: the same arithmetic on exactly representable inputs) within the float32 bound.
With ReLU the reference cotangent is masked by the STORED output.  Every measured error is printed before it is asserted.

Measured on MI355X: float32 quantities at most 1.4e-6 relative L2 / 1.1e-5 max-norm (dx of 1100 x 3 x 3 x 32: 9 pixels, one
channel per group; torch's float32 CPU kernel measures 1.3e-6 / 5.0e-5 on y there), bf16 y / dx at least 1.9e-6 inside their
bound; epilogue rows against the own statistics pass: mean / rstd equal to 1.8e-7 relative."""
import importlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
EPS = 1e-5
G = 32
T_L2, T_MX = 2e-5, 2e-4

# (N, H, W, C): four full rows per sample | the RoI tile: a ragged row, the one-launch regime | many samples | two channels per
# group, 15 pixels | groups of 3 channels that straddle the vectors | 76.6 rows: the split regime with a ragged tail | 32 channels
# per group, wider than the one-launch regime takes | more samples than workgroups of the one-launch regime, one channel per group
SHAPES = [(2, 16, 16, 256), (3, 7, 7, 256), (130, 7, 7, 256), (1, 5, 3, 64), (2, 9, 11, 96), (1, 70, 70, 128), (2, 4, 4, 1024),
          (1100, 3, 3, 32)]


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("3dod_amd.hipops")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dod_amd._lib")


def _inputs(shape, dtype, seed=0):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(1000 * seed + C + N)
    x = torch.randn(N, H, W, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + 3 * torch.randn(C, generator=g)
    dy = torch.randn(N, H, W, C, generator=g)
    gamma = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    beta = torch.randn(C, generator=g)
    if dtype == bf16:                                   # inputs exact in bf16
        x, dy = x.to(bf16).float(), dy.to(bf16).float()
    return x, dy, gamma, beta


def _reference(x, dy, gamma, beta, relu, y_stored):
    """float64: y, dx, dgamma, dbeta, mean, rstd (NHWC); with relu the cotangent is masked by the stored output"""
    N, H, W, C = x.shape
    x64 = x.to(f64).permute(0, 3, 1, 2).contiguous().requires_grad_()
    ga, be = gamma.to(f64).requires_grad_(), beta.to(f64).requires_grad_()
    v = F.group_norm(x64, G, ga, be, EPS)
    y = F.relu(v) if relu else v
    g = dy.to(f64).permute(0, 3, 1, 2)
    if relu:
        g = g * (y_stored.to(f64).permute(0, 3, 1, 2) > 0)
    v.backward(g)
    xg = x64.detach().reshape(N, G, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return nhwc(y), nhwc(x64.grad), ga.grad, be.grad, mean, 1.0 / torch.sqrt(var + EPS)


def _rel(got, ref):
    got, ref = got.detach().to("cpu", f64), ref.detach().to("cpu", f64)
    return float((got - ref).norm() / (ref.norm() + 1e-300)), float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def _bf16_excess(got, ref):
    got, ref = got.detach().to("cpu", f64), ref.detach().to("cpu", f64)
    return float(((got - ref).abs() - (2.0 ** -8 * ref.abs() + 1e-6 * ref.abs().max())).max())


def _run(ops, x, dy, gamma, beta, relu, dtype):
    xd, dyd = x.to(DEV, dtype), dy.to(DEV, dtype)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    y, mr = ops.group_norm_fwd_raw(xd, gd, bd, G, EPS, relu)
    dgamma = torch.full_like(gd, 0.25)
    dbeta = torch.full_like(bd, -0.5)
    dx = ops.group_norm_bwd_raw(dyd, xd, y, mr, gd, G, relu, dgamma, dbeta)
    torch.cuda.synchronize()
    return y, mr, dx, dgamma, dbeta


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_against_float64(ops, shape, dtype, relu):
    x, dy, gamma, beta = _inputs(shape, dtype)
    y, mr, dx, dgamma, dbeta = _run(ops, x, dy, gamma, beta, relu, dtype)
    assert y.dtype == dtype and dx.dtype == dtype and mr.dtype == f32 and tuple(mr.shape) == (shape[0], G, 2)
    ry, rdx, rdg, rdb, rmean, rrstd = _reference(x, dy, gamma, beta, relu, y.float().cpu())
    # the float32 CPU kernel on the same inputs, for scale (printed only)
    y32 = F.group_norm(x.permute(0, 3, 1, 2), G, gamma, beta, EPS)
    y32 = (F.relu(y32) if relu else y32).permute(0, 2, 3, 1)
    print("\n%s %s relu=%d: float32 CPU reference y %.2e / %.2e" % ((shape, dtype, relu) + _rel(y32, ry)))
    small = {"mean": (mr[..., 0], rmean), "rstd": (mr[..., 1], rrstd), "dgamma": (dgamma - 0.25, rdg), "dbeta": (dbeta + 0.5, rdb)}
    errs = {k: _rel(a, b) for k, (a, b) in small.items()}
    if dtype == f32:
        errs["y"], errs["dx"] = _rel(y, ry), _rel(dx, rdx)
    for k, (l2, mx) in errs.items():
        print("  %-6s rel L2 %.2e  max-norm %.2e" % (k, l2, mx))
    if dtype == bf16:
        ex_y, ex_dx = _bf16_excess(y, ry), _bf16_excess(dx, rdx)
        print("  bf16 excess over 2^-8 |ref| + 1e-6 max|ref|: y %.2e  dx %.2e" % (ex_y, ex_dx))
    assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(dx.float()).all())
    for k, (l2, mx) in errs.items():
        assert l2 <= T_L2 and mx <= T_MX, (k, l2, mx)
    if dtype == bf16:
        assert ex_y <= 0.0 and ex_dx <= 0.0, (ex_y, ex_dx)


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 16, 256), (130, 7, 7, 256), (1, 70, 70, 128)], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_have_the_same_bits(ops, shape, dtype):
    x, dy, gamma, beta = _inputs(shape, dtype, seed=1)
    a = _run(ops, x, dy, gamma, beta, True, dtype)
    b = _run(ops, x, dy, gamma, beta, True, dtype)
    for name, p, q in zip(("y", "mean_rstd", "dx", "dgamma", "dbeta"), a, b):
        assert torch.equal(p, q), name


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 16, 256), (3, 7, 7, 256)], ids=lambda s: "x".join(map(str, s)))
def test_constant_group_gives_exactly_beta(ops, shape, dtype):
    """one group constant at 0.5: its sums are exact in float32, the variance is 0, y is exactly beta and dx is finite"""
    x, dy, gamma, beta = _inputs(shape, dtype, seed=2)
    cpg = shape[3] // G
    x[..., 5 * cpg:6 * cpg] = 0.5
    y, mr, dx, _, _ = _run(ops, x, dy, gamma, beta, False, dtype)
    want = beta[5 * cpg:6 * cpg].to(DEV).to(dtype).expand_as(y[..., 5 * cpg:6 * cpg])
    assert torch.equal(y[..., 5 * cpg:6 * cpg], want)
    assert bool((mr[:, 5, 0] == 0.5).all())
    assert bool(torch.isfinite(dx.float()).all())


def test_rows_from_the_convolution_epilogue_give_the_same_statistics(ops):
    """cr_groupnorm_fwd takes the convolution's per-64-pixel rows instead of reading the map; both routes on the same map
    agree on mean and rstd to 1e-6 relative.  float32, the only mode in which conv_gn_act takes this route: the epilogue sums
    the float32 accumulators, which a bf16 map no longer holds."""
    dtype = f32
    g = torch.Generator().manual_seed(3)
    N, H, W, Cin, C = 2, 16, 16, 64, 256
    xin = (torch.randn(N, H, W, Cin, generator=g) + 1.0).to(DEV, dtype)
    w = (torch.randn(C, Cin, generator=g) / 8 + 0.05).to(DEV, dtype)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), torch.randn(C, generator=g).to(DEV)
    rows = torch.full((N * H * W // 64, 2, C), float("nan"), dtype=f32, device=DEV)
    t = ops.conv_fwd_raw(xin, w, C, 1, 1, 0, stats=rows)
    y_own, mr_own = ops.group_norm_fwd_raw(t, gamma, beta, G, EPS, True)
    y_rows, mr_rows = ops.group_norm_fwd_raw(t, gamma, beta, G, EPS, True, stat_rows=rows)
    torch.cuda.synchronize()
    rel = ((mr_own - mr_rows).abs() / mr_own.abs().clamp_min(1e-30)).max(0)[0].max(0)[0]
    print("\nmean / rstd, epilogue rows against own pass, max relative difference:", rel.tolist())
    assert bool(torch.isfinite(mr_rows).all())
    assert float(rel.max()) <= 1e-6
    l2, mx = _rel(y_rows, y_own.float())
    print("y: rel L2 %.2e max-norm %.2e" % (l2, mx))
    assert mx <= (2.0 ** -7 if dtype == bf16 else 1e-5)


def _refusal_buffers(C, N=2, HW=49, fill=7.0):
    n = max(C, 4096)
    mk = lambda *s: torch.full(s, fill, dtype=f32, device=DEV)
    return dict(x=mk(N, HW, n), dy=mk(N, HW, n), y=mk(N, HW, n), dx=mk(N, HW, n), gamma=mk(n), beta=mk(n), mr=mk(N, n, 2),
                dgamma=mk(n), dbeta=mk(n), ws=mk(N * n * 16))


@pytest.mark.parametrize("case", ["C=48", "C=4096", "G=7", "short workspace", "relu without y"])
def test_refusals_leave_the_outputs_untouched(lib, case):
    N, HW, C, Gc = 2, 49, 256, 32
    if case == "C=48":
        C, Gc = 48, 16
    elif case == "C=4096":
        C = 4096
    elif case == "G=7":
        Gc = 7
    b = _refusal_buffers(C, N, HW)
    need = lib.groupnorm_ws_floats(N, HW, C)
    if case in ("C=48", "C=4096"):
        assert need == 0
        need = b["ws"].numel()
    else:
        assert need == N * C * (2 * 1 + 6)
    ws_n = need - 1 if case == "short workspace" else need
    fwd = lambda: lib.call("cr_groupnorm_fwd", b["x"], b["gamma"], b["beta"], None, b["y"], b["mr"], b["ws"], ws_n, N, HW, C, Gc,
                           EPS, 1, 1)
    bwd = lambda y: lib.call("cr_groupnorm_bwd", b["dy"], b["x"], y, b["mr"], b["gamma"], b["ws"], ws_n, b["dx"], b["dgamma"],
                             b["dbeta"], N, HW, C, Gc, 1, 1)
    if case != "relu without y":
        with pytest.raises(lib.CrError):
            fwd()
        with pytest.raises(lib.CrError):
            bwd(b["y"])
    else:
        with pytest.raises(lib.CrError):
            bwd(None)
    torch.cuda.synchronize()
    for name in ("y", "mr", "dx", "dgamma", "dbeta"):
        assert bool((b[name] == 7.0).all()), name
