"""CPU self-test of the element-wise float64 bound (tests/f64_bound.py): float32 ATen passes it in all three directions of
a convolution, and the same convolution fails it when one input channel is dropped in one 16x16 output tile, when the last
1/8 of the pixels is missing from the weight gradient, and when the operands are rounded to bf16.  The float32 Winograd
F(2x2, 3x3) pipeline passes its own bound, which is looser than the direct one.

The linear-layer helpers the same way: a float32 matmul passes them in every direction with a worst ratio under C / 2, and
fails when one 32-wide k stage is dropped from one 64x64 output tile, when the partial sum of one k split is added twice,
when the bias is missing from one 16-column group, and when an operand (or the stored result) is truncated to bf16
instead of rounded."""
import pytest
import torch
import torch.nn.functional as F

import f64_bound as B

N, CIN, COUT, H, W, K, STRIDE, PAD = 2, 32, 32, 48, 48, 3, 1, 1


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, CIN, H, W, generator=g)
    w = torch.randn(COUT, CIN, K, K, generator=g) * (2.0 / (K * K * CIN)) ** 0.5
    b = torch.randn(COUT, generator=g) * 0.1
    dy = torch.randn(N, COUT, H, W, generator=g)
    return x, w, b, dy


def _fails(got, ref, absref, k):
    with pytest.raises(AssertionError, match="over the bound"):
        B.check(got, ref, absref, k, "perturbed")
    return B.report(got, ref, absref, k)


def test_float32_aten_passes(case):
    x, w, b, dy = case
    r = B.check(F.conv2d(x, w, b, STRIDE, PAD), *B.conv_fwd(x, w, b, STRIDE, PAD), "forward")
    assert r["ratio"] < B.C
    B.check(torch.nn.grad.conv2d_input(x.shape, w, dy, STRIDE, PAD), *B.conv_bwd_data(dy, w, x.shape, STRIDE, PAD), "dX")
    B.check(torch.nn.grad.conv2d_weight(x, w.shape, dy, STRIDE, PAD), *B.conv_bwd_weight(dy, x, w.shape, STRIDE, PAD), "dW")
    B.check(dy.sum((0, 2, 3)), *B.bias_grad(dy), "db")
    # stride 2 and a 1x1 convolution through the same helpers
    B.check(F.conv2d(x, w, None, 2, 1), *B.conv_fwd(x, w, None, 2, 1), "forward s2")
    d2 = dy[:, :, ::2, ::2].contiguous()
    B.check(torch.nn.grad.conv2d_input(x.shape, w, d2, 2, 1), *B.conv_bwd_data(d2, w, x.shape, 2, 1), "dX s2")
    B.check(torch.nn.grad.conv2d_weight(x, w.shape, d2, 2, 1), *B.conv_bwd_weight(d2, x, w.shape, 2, 1), "dW s2")


def test_dropped_channel_in_one_tile_fails(case):
    x, w, b, _ = case
    ref, absref, k = B.conv_fwd(x, w, b, STRIDE, PAD)
    x0 = x.clone()
    x0[:, 7] = 0
    got = F.conv2d(x, w, b, STRIDE, PAD)
    got[:, :, 16:32, 16:32] = F.conv2d(x0, w, b, STRIDE, PAD)[:, :, 16:32, 16:32]
    r = _fails(got, ref, absref, k)
    assert 16 <= r["where"][2] < 32 and 16 <= r["where"][3] < 32, r
    # the normwise error of the whole tensor is what a max-norm tolerance of 2e-5 would have to see
    print(f"dropped channel in one tile: worst ratio {r['ratio']:.3g}, normwise {r['norm']:.3g}")


def test_weight_gradient_missing_last_eighth_of_pixels_fails(case):
    x, w, _, dy = case
    ref, absref, k = B.conv_bwd_weight(dy, x, w.shape, STRIDE, PAD)
    cut = dy.permute(0, 2, 3, 1).reshape(-1, COUT).clone()            # pixels in (n, h, w) order, as a reduce splits them
    cut[cut.shape[0] * 7 // 8:] = 0
    cut = cut.view(N, H, W, COUT).permute(0, 3, 1, 2)
    r = _fails(torch.nn.grad.conv2d_weight(x, w.shape, cut, STRIDE, PAD), ref, absref, k)
    print(f"weight gradient without the last 1/8 of the pixels: worst ratio {r['ratio']:.3g}, normwise {r['norm']:.3g}")
    ref, absref, k = B.bias_grad(dy)
    r = _fails(cut.sum((0, 2, 3)), ref, absref, k)


def test_bf16_operands_fail(case):
    x, w, b, dy = case
    q = lambda t: t.to(torch.bfloat16).float()
    r = _fails(F.conv2d(q(x), q(w), b, STRIDE, PAD), *B.conv_fwd(x, w, b, STRIDE, PAD))
    print(f"bf16 operands, forward: worst ratio {r['ratio']:.3g}, normwise {r['norm']:.3g}")
    _fails(torch.nn.grad.conv2d_input(x.shape, q(w), q(dy), STRIDE, PAD), *B.conv_bwd_data(dy, w, x.shape, STRIDE, PAD))
    _fails(torch.nn.grad.conv2d_weight(q(x), w.shape, q(dy), STRIDE, PAD), *B.conv_bwd_weight(dy, x, w.shape, STRIDE, PAD))


def test_winograd_pipeline_in_float32_passes_its_bound(case):
    x, w, b, dy = case
    ref, absref_direct, k = B.conv_fwd(x, w, b, 1, 1)
    absw = B.wino_fwd(x, w, b, absval=True)
    assert bool((absw >= absref_direct * (1 - 1e-12)).all()), "the Winograd absref bounds the direct one"
    B.check(B.wino_fwd(x, w, b, dtype=torch.float32), ref, absw, CIN + B.WINO_DEPTH, "winograd forward")
    assert torch.allclose(B.wino_fwd(x, w, b), ref, rtol=0, atol=1e-12), "the float64 pipeline is the convolution"
    ref, _, _ = B.conv_bwd_data(dy, w, x.shape, 1, 1)
    assert torch.allclose(B.wino_bwd_data(dy, w), ref, rtol=0, atol=1e-12)
    B.check(B.wino_bwd_data(dy, w, dtype=torch.float32), ref, B.wino_bwd_data(dy, w, absval=True), COUT + B.WINO_DEPTH,
            "winograd dX")
    ref, _, _ = B.conv_bwd_weight(dy, x, w.shape, 1, 1)
    assert torch.allclose(B.wino_wgrad(dy, x), ref, rtol=0, atol=1e-9)
    B.check(B.wino_wgrad(dy, x, dtype=torch.float32), ref, B.wino_wgrad(dy, x, absval=True),
            B.wino_tiles(dy) + B.WINO_DEPTH, "winograd dW")
    # ... and bf16 operands fail it too
    q = lambda t: t.to(torch.bfloat16).float()
    _fails(B.wino_fwd(q(x), q(w), b, dtype=torch.float32), B.conv_fwd(x, w, b, 1, 1)[0], absw, CIN + B.WINO_DEPTH)


# ---------------------------------------------------------------------------------------------------------------------
# linear layers: a float32 matmul passes linear_fwd / linear_bwd_data / linear_bwd_weight, and the errors a tiled, split-K
# GEMM can make fail them at the element where they happen
# ---------------------------------------------------------------------------------------------------------------------
LR, LK, LO = 160, 512, 128


@pytest.fixture(scope="module")
def lin():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(LR, LK, generator=g)
    w = torch.randn(LO, LK, generator=g) * LK ** -0.5
    b = torch.randn(LO, generator=g) * 0.1
    dy = torch.randn(LR, LO, generator=g)
    return x, w, b, dy


def _q(t):
    return t.to(torch.bfloat16).float()


def _trunc_bf16(t):
    """float32 -> bfloat16 by dropping the low 16 bits (what a kernel that forgets to round does)"""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def test_float32_matmul_passes_linear_bounds(lin):
    x, w, b, dy = lin
    r = B.check(F.linear(x, w, b), *B.linear_fwd(x, w, b), "linear forward")
    assert r["ratio"] < B.C / 2, r
    assert B.check(x @ w.t(), *B.linear_fwd(x, w, None), "linear forward, no bias")["ratio"] < B.C / 2
    assert B.check(dy @ w, *B.linear_bwd_data(dy, w), "linear dX")["ratio"] < B.C / 2
    assert B.check(dy.t() @ x, *B.linear_bwd_weight(dy, x), "linear dW")["ratio"] < B.C / 2
    assert B.check(dy.sum(0), *B.linear_bias_grad(dy), "linear db")["ratio"] < B.C / 2
    ref, absref, k = B.linear_fwd(x, w, b)
    assert k == LK and B.linear_bwd_data(dy, w)[2] == LO and B.linear_bwd_weight(dy, x)[2] == LR
    assert torch.equal(ref, x.double() @ w.double().t() + b.double())
    assert torch.equal(absref, x.double().abs() @ w.double().abs().t() + b.double().abs())
    # bf16 operands: rounded first, the float32 product sums keep the float32 bound; a bf16-stored result the wider one
    xq, wq = _q(x), _q(w)
    y = F.linear(xq, wq, b)
    B.check(y, *B.linear_fwd(xq, wq, b), "bf16 operands, f32 output")
    r = B.check_bf16_out(_q(y), *B.linear_fwd(xq, wq, b), "bf16 operands, bf16 output")
    assert 0.5 < r["ratio"] < B.C                       # the store's rounding dominates and is what the bound is made of
    with pytest.raises(AssertionError, match="over the bound"):
        B.check(_q(y), *B.linear_fwd(xq, wq, b), "a bf16-stored output is outside the float32 bound")


def test_k_stage_dropped_from_one_tile_fails(lin):
    x, w, b, _ = lin
    ref, absref, k = B.linear_fwd(x, w, b)
    x0 = x.clone()
    x0[:, 64:96] = 0                                                   # one 32-wide k stage
    got = F.linear(x, w, b)
    got[64:128, 64:128] = F.linear(x0, w, b)[64:128, 64:128]           # ... of one 64x64 output tile
    r = _fails(got, ref, absref, k)
    assert 64 <= r["where"][0] < 128 and 64 <= r["where"][1] < 128, r
    print(f"k stage dropped from one tile: worst ratio {r['ratio']:.3g}, normwise {r['norm']:.3g}")


def test_partial_sum_of_one_k_split_added_twice_fails(lin):
    x, w, b, dy = lin
    s = slice(3 * LK // 4, LK)                                         # the last of four k splits
    r = _fails(F.linear(x, w, b) + x[:, s] @ w[:, s].t(), *B.linear_fwd(x, w, b))
    print(f"one k split added twice: worst ratio {r['ratio']:.3g}, normwise {r['norm']:.3g}")
    s = slice(0, LR // 8)                                              # weight gradient: the first of eight row splits
    _fails(dy.t() @ x + dy[s].t() @ x[s], *B.linear_bwd_weight(dy, x))
    _fails(dy.sum(0) + dy[s].sum(0), *B.linear_bias_grad(dy))


def test_bias_missing_from_one_column_group_fails(lin):
    x, w, b, _ = lin
    got = F.linear(x, w, b)
    got[:, 32:48] -= b[32:48]
    r = _fails(got, *B.linear_fwd(x, w, b))
    assert 32 <= r["where"][1] < 48, r
    print(f"bias missing from 16 columns: worst ratio {r['ratio']:.3g}, normwise {r['norm']:.3g}")


def test_truncated_bf16_operand_fails(lin):
    x, w, b, dy = lin
    xq, wq, dq = _q(x), _q(w), _q(dy)
    xt = _trunc_bf16(x)
    assert torch.equal(_q(xt), xt) and not torch.equal(xt, xq)
    r = _fails(F.linear(xt, wq, b), *B.linear_fwd(xq, wq, b))
    print(f"operand truncated to bf16: worst ratio {r['ratio']:.3g}, normwise {r['norm']:.3g}")
    _fails(dq @ _trunc_bf16(w), *B.linear_bwd_data(dq, wq))
    _fails(_trunc_bf16(dy).t() @ xq, *B.linear_bwd_weight(dq, xq))
    # ... and a result truncated on its way to bf16 fails the bf16-output bound
    y = F.linear(xq, wq, b)
    with pytest.raises(AssertionError, match="over the bf16-output bound"):
        B.check_bf16_out(_trunc_bf16(y), *B.linear_fwd(xq, wq, b), "truncated store")
