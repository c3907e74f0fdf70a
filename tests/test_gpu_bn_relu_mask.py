"""GPU: cr_bn_bwd_mask (the BatchNorm backward of a ReLU layer without a residual, which recomputes the ReLU mask from the
raw conv output instead of reading the forward's output) against cr_bn_bwd given that output -- bit for bit on dx, dgamma,
dbeta and the whole partial-sum workspace -- and both against float64 autograd of the BatchNorm part of
oracle/torch_ref.conv_bn_act with the mask the GPU forward produced (the convention of test_gpu_step_shapes_f64.py;
tolerances: max-norm relative 1e-4 in float32 as there and in test_gpu_convops_f32.py, 3e-2 in bf16 storage as in
test_gpu_convops.py).

Shapes, so that every branch runs: C = 32, M = 512 and C = 64, M = 4096 (fused reduce + apply, several pixel chunks);
C = 16, M = 2048 (C % 32 != 0: unfused finalize + apply); C = 32, M = 133 120 (260 reduce blocks > 256: the unfused apply
with C % 32 == 0, and enough statistics rows for the two-launch forward finalize).

Inputs that make the mask hard, by channel (c mod 16):
  gamma exactly 0 with beta in {0, +-1e-30, +-1e-45}: the activation IS beta -- exactly 0, the smallest positive float32
    (a denormal that bf16 storage rounds to 0) and small negatives;
  whole channels equal to their mean (x = 0.5: xhat = 0, the activation is beta again, with gamma != 0): beta in
    {0, 1e-45, -1e-30, 1e-40};
  ordinary channels with gamma of both signs: seven pixels are set to the zero crossing of the activation and its
    neighbours in the storage format (0, +-1, +-2, +-3 ulp), found by iterating statistics -> forward -> crossing a few
    times; the statistics are always those of the final x."""
import importlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
lib = importlib.import_module("3dod_amd._lib")
DEV = torch.device("cuda:0")
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
EPS, SENTINEL = 1e-5, -12345.0
SHAPES = [(32, 512), (64, 4096), (16, 2048), (32, 2 * 256 * 260)]
TOL = {f32: 1e-4, bf16: 3e-2}


def _stats_rows(x):
    """[ceil(M / 64)][2][C] float32: sum and sum of squares of every 64 pixels, as the conv epilogues hand them over"""
    M, C = x.shape
    nparts = (M + 63) // 64
    xp = torch.zeros(nparts * 64, C, dtype=f64, device=x.device)
    xp[:M] = x.to(f64)
    xp = xp.view(nparts, 64, C)
    return torch.stack([xp.sum(1), (xp * xp).sum(1)], 1).to(f32).contiguous(), nparts


def _forward(x, gamma, beta):
    M, C = x.shape
    stats, nparts = _stats_rows(x)
    out, mi = torch.empty_like(x), torch.empty(2, C, dtype=f32, device=DEV)
    lib.call("cr_bn_fwd", x, stats, nparts, gamma, beta, None, out, M, C, 1, EPS, 0.1, mi, None, None, int(x.dtype == f32))
    return out, mi


def _neighbours(v, dtype, k):
    """v rounded to `dtype`, moved k steps along that format's grid (v away from 0 and from the format's limits)"""
    bits = v.to(f32).view(torch.int32) if dtype == f32 else v.to(bf16).view(torch.int16).to(torch.int32)
    bits = bits + torch.where(bits >= 0, torch.full_like(bits, k), torch.full_like(bits, -k))
    return bits.view(f32) if dtype == f32 else bits.to(torch.int16).view(bf16)


def _inputs(C, M, dtype):
    g = torch.Generator().manual_seed(1000 * C + M % 997)
    role = torch.arange(C) % 16
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    beta = torch.randn(C, generator=g) * 0.3
    gamma[(role >= 2) & (role <= 6)] = 0.0
    for r, b in ((2, 0.0), (3, 1e-30), (4, -1e-30), (5, 1e-45), (6, -1e-45), (7, 0.0), (8, 1e-45), (9, -1e-30), (10, 1e-40), (11, 0.0)):
        beta[role == r] = b
    gamma[role == 9] = -gamma[role == 9].abs()
    assert float(beta[role == 5][0]) > 0 and float(beta[role == 10][0]) > 0       # the denormals survived the host
    x = torch.randn(M, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g)
    const = (role >= 7) & (role <= 10)
    x[:, const] = 0.5
    x = x.to(dtype).to(DEV)
    gamma, beta = gamma.to(DEV), beta.to(DEV)
    cross = ((gamma != 0) & ~const.to(DEV)).nonzero().flatten()
    for _ in range(4):                     # statistics -> crossing -> insert: seven pixels move the mean by ~1 ulp at most
        _, mi = _forward(x, gamma, beta)
        x0 = mi[0].to(f64) - beta.to(f64) / (gamma.to(f64) * mi[1].to(f64))
        x[:7, cross] = torch.stack([_neighbours(x0[cross], dtype, k) for k in range(-3, 4)])
    dy = torch.randn(M, C, generator=g).to(dtype).to(DEV)
    return x, gamma, beta, dy


def _backward(entry, x, out, mi, gamma, beta, dy):
    M, C = x.shape
    sums = torch.full((1025, 2, C), SENTINEL, dtype=f32, device=DEV)
    dx = torch.empty_like(x)
    dgamma, dbeta = torch.full((C,), 0.25, device=DEV), torch.full((C,), -0.5, device=DEV)     # both are accumulated into
    af = int(x.dtype == f32)
    if entry == "cr_bn_bwd":
        lib.call("cr_bn_bwd", dy, out, x, mi, gamma, sums, dx, None, dgamma, dbeta, M, C, 1, af)
    else:
        lib.call("cr_bn_bwd_mask", dy, out, x, mi, gamma, beta, sums, dx, None, dgamma, dbeta, M, C, 1, af)
    torch.cuda.synchronize()
    return dx, dgamma, dbeta, sums


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(C, M, dtype):
        key = (C, M, dtype)
        if key not in cache:
            x, gamma, beta, dy = _inputs(C, M, dtype)
            out, mi = _forward(x, gamma, beta)
            cache[key] = {"x": x, "gamma": gamma, "beta": beta, "dy": dy, "out": out, "mi": mi,
                          "given": _backward("cr_bn_bwd", x, out, mi, gamma, beta, dy),
                          "mask": _backward("cr_bn_bwd_mask", x, None, mi, gamma, beta, dy),
                          "mask_out": _backward("cr_bn_bwd_mask", x, out, mi, gamma, beta, dy)}
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,M", SHAPES)
def test_mask_from_x_is_bit_equal(runs, C, M, dtype):
    r = runs(C, M, dtype)
    out, beta = r["out"].float(), r["beta"]
    role = torch.arange(C, device=DEV) % 16
    # the hard activations all occur: exactly 0, the smallest positive stored value, tiny negatives clipped to 0
    assert bool((out[:, role == 2] == 0).all()) and bool((out[:, role == 7] == 0).all())
    assert bool((out[:, role == 3] == beta[role == 3].to(dtype).float()).all()) and bool((out[:, role == 4] == 0).all())
    tiny = out[:, role == 5]
    assert bool((tiny > 0).all()) if dtype == f32 else bool((tiny == 0).all())
    assert bool((out[:, role == 10] > 0).all()) and bool((out[:, role == 9] == 0).all())
    first = out[:7][:, (r["gamma"] != 0) & ~((role >= 7) & (role <= 10))]
    assert bool((first > 0).any()) and bool((first == 0).any())              # the crossing pixels straddle the crossing
    for name, a, b in zip(("dx", "dgamma", "dbeta", "workspace"), r["given"], r["mask"]):
        assert torch.equal(a, b), f"{name}: out == NULL differs from cr_bn_bwd"
    for name, a, b in zip(("dx", "dgamma", "dbeta", "workspace"), r["given"], r["mask_out"]):
        assert torch.equal(a, b), f"{name}: cr_bn_bwd_mask given out differs from cr_bn_bwd"
    nb = min(1024, -(-M // (256 // (C // 8) * 8)))
    assert bool((r["mask"][3][:nb] != SENTINEL).all()) and bool((r["mask"][3][nb:1024] == SENTINEL).all())


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,M", SHAPES)
def test_against_float64_autograd(runs, C, M, dtype):
    r = runs(C, M, dtype)
    x64 = r["x"].cpu().to(f64).t().reshape(1, C, M, 1).requires_grad_(True)
    g64, b64 = r["gamma"].cpu().to(f64).requires_grad_(True), r["beta"].cpu().to(f64).requires_grad_(True)
    z = F.batch_norm(x64, None, None, g64, b64, True, 0.1, EPS)       # torch_ref.conv_bn_act after its convolution ...
    y64 = z * (r["out"].cpu().t().reshape(1, C, M, 1) > 0).to(f64)    # ... with the ReLU as the GPU forward's mask
    y64.backward(r["dy"].cpu().to(f64).t().reshape(1, C, M, 1))
    dx, dgamma, dbeta, _ = r["mask"]
    got = {"dx": dx.cpu().to(f64).t().reshape(1, C, M, 1), "dgamma": dgamma.cpu().to(f64) - 0.25,
           "dbeta": dbeta.cpu().to(f64) + 0.5}
    ref = {"dx": x64.grad, "dgamma": g64.grad, "dbeta": b64.grad}
    err = {k: float((got[k] - ref[k]).abs().max() / (ref[k].abs().max() + 1e-300)) for k in ref}
    print(f"C={C} M={M} {dtype}: {err}")
    assert all(v < TOL[dtype] for v in err.values()), err


def test_residual_layer_needs_out():
    x = torch.zeros(64, 32, device=DEV)
    v = torch.ones(32, device=DEV)
    with pytest.raises(lib.CrError):
        lib.call("cr_bn_bwd_mask", x, None, x, torch.ones(2, 32, device=DEV), v, v, torch.empty(1025, 2, 32, device=DEV),
                 torch.empty_like(x), torch.empty_like(x), v.clone(), v.clone(), 64, 32, 1, 1)
