"""Backward kernels of the Depth-Anything-V2 training step (csrc/vit_bwd.hip) against float64 torch autograd on the
bf16-rounded inputs the kernels see.  Every test prints its figures before it asserts."""
import importlib
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_bound as fb  # noqa: E402

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dod_amd.hipops")
lib = importlib.import_module("3dod_amd._lib")
DEV = torch.device("cuda:0")
f64, bf16 = torch.float64, torch.bfloat16
D = 64


def rb(t):
    """round a float64 tensor to bfloat16 (nearest even), back in float64"""
    return t.to(torch.float32).to(bf16).to(f64)


def attention_case(B, N, H, qscale=1.0, seed=None, base=1.5):
    g = torch.Generator().manual_seed(N * 7 + H if seed is None else seed)
    qkv = torch.randn(B * N, 3 * H * D, generator=g) * base
    qkv.view(B, N, 3, H, D)[:, :, 0] *= qscale
    return qkv.to(bf16), torch.randn(B * N, H * D, generator=g).to(bf16)


def attention_refs(qkv, dout, B, N, H):
    """float64: the exact backward, and the same backward with the roundings a bf16 MFMA kernel cannot avoid (P and dS
    rounded to bf16 before their products, dq / dk / dv rounded at the end)"""
    scale = D ** -0.5
    q, k, v = qkv.to(f64).view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)            # (B,H,N,D)
    do = dout.to(f64).view(B, N, H, D).permute(0, 2, 1, 3)
    P = torch.softmax(scale * q @ k.transpose(-2, -1), dim=-1)
    o = P @ v
    dP = do @ v.transpose(-2, -1)
    delta = (do * o).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    exact = (scale * dS @ k, scale * dS.transpose(-2, -1) @ q, P.transpose(-2, -1) @ do)
    Pb, dSb = rb(P), rb(dS)
    model = tuple(rb(t) for t in (scale * dSb @ k, scale * dSb.transpose(-2, -1) @ q, Pb.transpose(-2, -1) @ do))
    return exact, model


def unpack_dqkv(dqkv, B, N, H):
    return dqkv.cpu().to(f64).view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)


def check_attention_bwd(qkv, dout, B, N, H, what):
    qd, dd = qkv.to(DEV), dout.to(DEV)
    out, lse = ops.attention_lse(qd, B, N, H, D, D ** -0.5)
    dqkv = ops.attention_bwd(qd, dd, lse, B, N, H, D, D ** -0.5)
    assert torch.isfinite(dqkv.float()).all()
    got = unpack_dqkv(dqkv, B, N, H)
    exact, model = attention_refs(qkv, dout, B, N, H)
    for name, g_, e_, m_ in zip(("dq", "dk", "dv"), got, exact, model):
        e_model = float((m_ - e_).norm() / (e_.norm() + 1e-300))
        err = float((g_ - e_).norm())
        print(f"{what} {name}: E_model {e_model:.3e}  kernel {err / (float(e_.norm()) + 1e-300):.3e}  "
              f"max|err| {float((g_ - e_).abs().max()):.3e}  max|ref| {float(e_.abs().max()):.3e}")
        assert err <= 2 * e_model * float(e_.norm()), (name, err, e_model)
        assert float((g_ - e_).abs().max()) <= 0.05 * float(e_.abs().max()), name
    if N == 1:          # P = 1 and dP = delta: dq and dk are exactly zero, dv is dO
        assert not bool(got[0].any()) and not bool(got[1].any())
        assert torch.equal(got[2], dout.to(f64).view(B, N, H, D).permute(0, 2, 1, 3))


@pytest.mark.parametrize("B,N,H", [(1, 1, 1), (2, 17, 2), (1, 64, 3), (2, 65, 2), (1, 197, 6), (1, 1370, 2)])
def test_attention_bwd(B, N, H):
    qkv, dout = attention_case(B, N, H)
    check_attention_bwd(qkv, dout, B, N, H, f"({B},{N},{H})")


def test_attention_bwd_peaked():
    """the peaked case of the forward test (q * 12: one dominant key per row) under the same bound"""
    B, N, H = 1, 300, 2
    qkv, dout = attention_case(B, N, H, qscale=12.0, seed=3, base=1.0)
    check_attention_bwd(qkv, dout, B, N, H, "peaked")


def test_attention_train_forward_equals_inference_and_backward_repeats():
    B, N, H = 2, 197, 6
    qkv, dout = attention_case(B, N, H)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    out, lse = ops.attention_lse(qd, B, N, H, D, D ** -0.5)
    assert torch.equal(out, ops.attention(qd, B, N, H, D, D ** -0.5))
    q, k, _ = qkv.to(f64).view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    want = torch.logsumexp(D ** -0.5 * q @ k.transpose(-2, -1), dim=-1)
    assert float((lse.cpu().to(f64) - want).abs().max()) < 1e-4
    a = ops.attention_bwd(qd, dd, lse, B, N, H, D, D ** -0.5)
    b = ops.attention_bwd(qd, dd, lse, B, N, H, D, D ** -0.5)
    assert torch.equal(a, b)
    # through autograd: the same gradient reaches the packed qkv
    qa = qd.clone().requires_grad_()
    ops.attention_train(qa, B, N, H, D, D ** -0.5).backward(dd)
    assert torch.equal(qa.grad, a)


def test_attention_bwd_rejects_other_head_dims():
    z = lambda *s: torch.zeros(*s, dtype=bf16, device=DEV)
    with pytest.raises(lib.CrError):
        ops.attention_lse(z(4, 3 * 2 * 32), 1, 4, 2, 32, 1.0)
    with pytest.raises(lib.CrError):
        ops.attention_bwd(z(4, 3 * 2 * 32), z(4, 64), torch.zeros(1, 2, 4, device=DEV), 1, 4, 2, 32, 1.0)


@pytest.mark.parametrize("M,C", [(1, 64), (37, 384), (1370, 1024), (5, 1536)])
def test_layernorm_bwd(M, C):
    g = torch.Generator().manual_seed(M + C)
    x = (torch.randn(M, C, generator=g) * 3 + 1.5).to(bf16)
    dy = torch.randn(M, C, generator=g).to(bf16)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    eps = 1e-6
    dgamma, dbeta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = ops.layernorm_bwd_raw(x.to(DEV), dy.to(DEV), gamma.to(DEV), dgamma, dbeta, eps, accumulate=False)
    x64, d64, g64 = x.to(f64).requires_grad_(), dy.to(f64), gamma.to(f64).requires_grad_()
    b64 = beta.to(f64).requires_grad_()
    F.layer_norm(x64, (C,), g64, b64, eps).backward(d64)
    xd = x.to(f64)
    inv = 1.0 / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + eps)
    xh = (xd - xd.mean(1, keepdim=True)) * inv
    ga = (d64 * gamma.to(f64)).abs()
    abs_dx = inv * (ga + ga.mean(1, keepdim=True) + xh.abs() * (ga * xh.abs()).mean(1, keepdim=True))
    for name, r in (("dx", fb.report_bf16_out(dx.cpu(), x64.grad, abs_dx, C)),
                    ("dgamma", fb.report(dgamma.cpu(), g64.grad, (d64 * xh).abs().sum(0), M + C)),
                    ("dbeta", fb.report(dbeta.cpu(), b64.grad, d64.abs().sum(0), M + C))):
        print(f"layernorm_bwd ({M},{C}) {name}: worst ratio {r['ratio']:.3g} (bound {fb.C}), normwise {r['norm']:.3g}")
    fb.check_bf16_out(dx.cpu(), x64.grad, abs_dx, C, "layernorm dx")
    fb.check(dgamma.cpu(), g64.grad, (d64 * xh).abs().sum(0), M + C, "layernorm dgamma")
    fb.check(dbeta.cpu(), b64.grad, d64.abs().sum(0), M + C, "layernorm dbeta")
    # either parameter gradient may be absent (a frozen weight or bias): the other one and dx are unchanged
    only_b, only_g = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx_b = ops.layernorm_bwd_raw(x.to(DEV), dy.to(DEV), gamma.to(DEV), None, only_b, eps, accumulate=False)
    dx_g = ops.layernorm_bwd_raw(x.to(DEV), dy.to(DEV), gamma.to(DEV), only_g, None, eps, accumulate=False)
    dx_n = ops.layernorm_bwd_raw(x.to(DEV), dy.to(DEV), gamma.to(DEV), None, None, eps, accumulate=False)
    assert torch.equal(dx_b, dx) and torch.equal(dx_g, dx) and torch.equal(dx_n, dx)
    assert torch.equal(only_b, dbeta) and torch.equal(only_g, dgamma)
    # a second run gives the same bits, and accumulate adds to what is there
    dg2, db2 = dgamma.clone(), dbeta.clone()
    dx2 = ops.layernorm_bwd_raw(x.to(DEV), dy.to(DEV), gamma.to(DEV), dg2, db2, eps, accumulate=True)
    assert torch.equal(dx, dx2) and torch.equal(dg2, dgamma + dgamma) and torch.equal(db2, dbeta + dbeta)


@pytest.mark.parametrize("M,C", [(3, 64), (37, 384), (130, 1024), (5, 1536)])
def test_float32_residual_stream_kernels(M, C):
    """the training route's stream: LayerNorm of float32 rows (forward and backward) and x + gamma * y in float32"""
    g = torch.Generator().manual_seed(M * 3 + C)
    x = torch.randn(M, C, generator=g) * 3 + 1.5                     # float32: NOT rounded to bf16
    dy, y = torch.randn(M, C, generator=g).to(bf16), torch.randn(M, C, generator=g).to(bf16)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    eps = 1e-6
    x64, g64, b64 = x.to(f64).requires_grad_(), gamma.to(f64).requires_grad_(), beta.to(f64).requires_grad_()
    ref = F.layer_norm(x64, (C,), g64, b64, eps)
    ref.backward(dy.to(f64))
    xd = x.to(f64)
    inv = 1.0 / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + eps)
    xh = (xd - xd.mean(1, keepdim=True)) * inv
    out = ops.layernorm_f32in(x.to(DEV), gamma.to(DEV), beta.to(DEV), eps)
    abs_fwd = inv * (xd.abs() + xd.mean(1, keepdim=True).abs()) * gamma.to(f64).abs() + beta.to(f64).abs()   # terms by magnitude
    fb.check_bf16_out(out.cpu(), ref.detach(), abs_fwd, C, "layernorm_f32in")
    dgamma, dbeta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = ops.layernorm_bwd_raw(x.to(DEV), dy.to(DEV), gamma.to(DEV), dgamma, dbeta, eps, accumulate=False)
    ga = (dy.to(f64) * gamma.to(f64)).abs()
    abs_dx = inv * (ga + ga.mean(1, keepdim=True) + xh.abs() * (ga * xh.abs()).mean(1, keepdim=True))
    assert dx.dtype == torch.float32                                  # the stream's gradient is stored in float32
    fb.check(dx.cpu(), x64.grad, abs_dx, C, "layernorm dx (float32 x)")
    fb.check(dgamma.cpu(), g64.grad, (dy.to(f64) * xh).abs().sum(0), M + C, "layernorm dgamma (float32 x)")
    fb.check(dbeta.cpu(), b64.grad, dy.to(f64).abs().sum(0), M + C, "layernorm dbeta (float32 x)")
    got = ops.scale_residual_f32(x.to(DEV), y.to(DEV), gamma.to(DEV))
    want = x.to(f64) + gamma.to(f64) * y.to(f64)
    fb.check(got.cpu(), want, x.to(f64).abs() + (gamma.to(f64) * y.to(f64)).abs(), 2, "scale_residual_f32")
    # through autograd: the stream's gradient passes through in float32, the branch's is bf16
    xa, ya = x.to(DEV).requires_grad_(), y.to(DEV).requires_grad_()
    up = torch.randn(M, C, generator=g)
    ops.scale_residual_train(xa, ya, gamma.to(DEV)).backward(up.to(DEV))
    assert xa.grad.dtype == torch.float32 and torch.equal(xa.grad.cpu(), up) and ya.grad.dtype == bf16
    xa = x.to(DEV).requires_grad_()
    ops.layernorm_train(xa, gamma.to(DEV), beta.to(DEV), eps).backward(dy.to(DEV))
    assert xa.grad.dtype == torch.float32 and torch.equal(xa.grad, dx)
    # through autograd with a frozen weight / a frozen bias: the other gradient still arrives
    for fg, fbias in ((True, False), (False, True)):
        ga, ba = gamma.to(DEV).requires_grad_(not fg), beta.to(DEV).requires_grad_(not fbias)
        xa = x.to(DEV).requires_grad_()
        ops.layernorm_train(xa, ga, ba, eps).backward(dy.to(DEV))
        assert torch.equal(xa.grad, dx) and (ga.grad is None) == fg and (ba.grad is None) == fbias
        assert torch.equal(ba.grad if fg else ga.grad, dbeta if fg else dgamma)


def test_gelu_fwd_bwd():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(333, 128, generator=g) * 3).to(bf16)
    dy = torch.randn(333, 128, generator=g).to(bf16)
    y = ops.gelu_fwd_raw(x.to(DEV))
    assert torch.equal(y, ops.gelu_(x.to(DEV).clone()))             # the inference kernel's values, out of place
    dx = ops.gelu_bwd_raw(x.to(DEV), dy.to(DEV)).cpu().to(f64)
    x64 = x.to(f64).requires_grad_()
    F.gelu(x64).backward(dy.to(f64))
    err, bound = (dx - x64.grad).abs(), 2.0 ** -8 * x64.grad.abs() + 2.0 ** -20 * dy.to(f64).abs()
    print(f"gelu_bwd: worst err / bound {float((err / (bound + 1e-300)).max()):.3g}")
    assert bool((err <= bound).all())


def test_layerscale_bwd():
    M, C = 77, 256
    g = torch.Generator().manual_seed(1)
    up, y = torch.randn(M, C, generator=g).to(bf16), torch.randn(M, C, generator=g).to(bf16)
    gamma = torch.randn(C, generator=g)
    dgamma = torch.zeros(C, device=DEV)
    dy = ops.layerscale_bwd_raw(up.to(DEV), y.to(DEV), gamma.to(DEV), dgamma, accumulate=False)
    u64, y64, g64 = up.to(f64), y.to(f64), gamma.to(f64)
    r1 = fb.check(dgamma.cpu(), (u64 * y64).sum(0), (u64 * y64).abs().sum(0), M, "layerscale dgamma")
    r2 = fb.check_bf16_out(dy.cpu(), g64 * u64, (g64 * u64).abs(), 1, "layerscale dy")
    print(f"layerscale_bwd: dgamma ratio {r1['ratio']:.3g}, dy ratio {r2['ratio']:.3g}")
    # through autograd, with the residual: dx passes through
    xa, ya = up.to(DEV).clone().requires_grad_(), y.to(DEV).clone().requires_grad_()
    ga = gamma.to(DEV).requires_grad_()
    ops.scale_residual_train(xa, ya, ga).backward(up.to(DEV))
    assert torch.equal(xa.grad, up.to(DEV)) and torch.equal(ya.grad, dy) and torch.equal(ga.grad, dgamma)


@pytest.mark.parametrize("h,w,Ho,Wo,C", [(7, 10, 14, 20, 32), (5, 9, 13, 4, 16), (1, 1, 3, 3, 8), (37, 37, 74, 74, 64)])
def test_resize_bwd(h, w, Ho, Wo, C):
    B = 2
    g = torch.Generator().manual_seed(h * 100 + Ho)
    dy = torch.randn(B, Ho, Wo, C, generator=g).to(bf16)
    dx = ops.resize_bilinear_ac_bwd_raw(dy.to(DEV), (B, h, w, C)).cpu()

    def bwd(d):
        x = torch.zeros(B, C, h, w, dtype=f64, requires_grad=True)
        F.interpolate(x, (Ho, Wo), mode="bilinear", align_corners=True).backward(d.to(f64).permute(0, 3, 1, 2))
        return x.grad.permute(0, 2, 3, 1)
    K = 4 * math.ceil(Ho / h) * math.ceil(Wo / w)
    r = fb.report_bf16_out(dx, bwd(dy), bwd(dy.abs()), K)
    print(f"resize_bwd ({h},{w})->({Ho},{Wo}): worst ratio {r['ratio']:.3g} (bound {fb.C}), normwise {r['norm']:.3g}")
    fb.check_bf16_out(dx, bwd(dy), bwd(dy.abs()), K, "resize dx")
    xa = torch.randn(B, h, w, C, generator=g).to(bf16).to(DEV).requires_grad_()
    ops.resize_bilinear_ac_train(xa, (Ho, Wo)).backward(dy.to(DEV))
    assert torch.equal(xa.grad.cpu(), dx)


def _depth_case(name):
    g = torch.Generator().manual_seed(11)
    if name == "full":
        shape, valid = (1, 14, 14), torch.ones(1, 14, 14, dtype=torch.bool)
    else:
        shape = (2, 70, 98)
        valid = torch.rand(shape, generator=g) < 0.8
        if name == "two":
            valid[1] = False
            valid[1, 3, 5] = valid[1, 60, 97] = True
    pred = torch.rand(shape, generator=g) * 15 + 1
    target = torch.rand(shape, generator=g) * 15 + 1
    return pred, target, valid


def _eval_depth64(pred, target):
    """util/metric.py in float64 (the thresholds compare float32 values, as there)"""
    p32, t32 = pred.float(), target.float()
    thresh = torch.max(t32 / p32, p32 / t32)
    n = len(thresh)
    p, t = pred.to(f64), target.to(f64)
    diff, dl = p - t, torch.log(p) - torch.log(t)
    return {"d1": float((thresh < 1.25).sum()) / n, "d2": float((thresh < 1.25 ** 2).sum()) / n,
            "d3": float((thresh < 1.25 ** 3).sum()) / n, "abs_rel": float((diff.abs() / t).mean()),
            "sq_rel": float((diff ** 2 / t).mean()), "rmse": float((diff ** 2).mean().sqrt()),
            "rmse_log": float((dl ** 2).mean().sqrt()), "log10": float((torch.log10(p) - torch.log10(t)).abs().mean()),
            "silog": float(((dl ** 2).mean() - 0.5 * dl.mean() ** 2).sqrt())}


@pytest.mark.parametrize("name", ["full", "most", "two"])
def test_silog_loss_and_depth_metrics(name):
    pred, target, valid = _depth_case(name)
    pa = pred.to(DEV).requires_grad_()
    loss = ops.silog_loss(pa, target.to(DEV), valid.to(DEV))
    loss.backward()
    p64 = pred.to(f64).requires_grad_()
    dl = torch.log(target.to(f64)[valid]) - torch.log(p64[valid])
    ref = torch.sqrt((dl ** 2).mean() - 0.5 * dl.mean() ** 2)
    ref.backward()
    loss, ref = float(loss.detach()), float(ref.detach())
    print(f"silog {name}: loss {loss:.7f} ref {ref:.7f}")
    assert abs(loss - ref) <= 5e-5 * abs(ref)
    got = pa.grad.cpu().to(f64)
    assert bool(((got - p64.grad).abs() <= 5e-5 * p64.grad.abs() + 1e-9).all())
    assert bool((pa.grad.cpu()[~valid] == 0).all())
    for i in range(pred.shape[0]):
        m = ops.depth_metrics(pred[i].to(DEV), target[i].to(DEV), valid[i].to(DEV))
        want = _eval_depth64(pred[i][valid[i]], target[i][valid[i]])
        assert list(m) == list(ops.DEPTH_METRICS)
        for k in ("d1", "d2", "d3"):
            assert m[k] == want[k], (k, m[k], want[k])
        for k in ops.DEPTH_METRICS[3:]:
            assert abs(m[k] - want[k]) <= 5e-5 * abs(want[k]), (k, m[k], want[k])
