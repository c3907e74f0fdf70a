"""CPU self-test of the element-wise float64 bound (tests/f64_bound.py): float32 ATen passes it in all three directions of
a convolution, and the same convolution fails it when one input channel is dropped in one 16x16 output tile, when the last
1/8 of the pixels is missing from the weight gradient, and when the operands are rounded to bf16.  The float32 Winograd
F(2x2, 3x3) pipeline passes its own bound, which is looser than the direct one."""
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
