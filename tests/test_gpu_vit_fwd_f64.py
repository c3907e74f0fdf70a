"""The forward kernels of the depth model (csrc/vit.hip) against float64, element by element, under the bounds of
tests/vit_ref.py (derived there; tests/test_vit_ref.py shows on the CPU what they let through and what they catch), and the
two pieces of torch glue around GEMMs in the DPT head.

The entry points are called through _lib.call with outputs the test owns: filled with NaN, inside a buffer with sentinel
guards on both sides.  After the call the guards must be intact and no NaN may be left, so a row that was not written and a
store past the end both show; a result from torch.empty can hide the first behind the values of an earlier call.  The
inputs lie between NaN guards: a load past them that is weighted with 0 still gives NaN.  The ops.* wrappers are compared
bit for bit with the direct calls, once per kernel.  Every test prints its worst ratio before it asserts."""
import importlib
import types

import pytest
import torch
import torch.nn.functional as F

import f64_bound as fb
import vit_ref as vr

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dod_amd.hipops")
lib = importlib.import_module("3dod_amd._lib")
dpt = importlib.import_module("3dod_amd.depth_anything_v2.dpt")
DEV = torch.device("cuda:0")
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
D, SCALE = vr.D, vr.SCALE
GUARD = 4096            # elements on either side (a multiple of 8: the kernels' 16-byte accesses stay aligned)
SENTINEL = -7.25e7
ON_DEVICE = 1 << 20     # from this many elements the float64 reference is computed on the device with torch's own ops


def guarded(shape, dtype):
    """(buffer, view): a NaN-filled tensor of `shape` between two sentinel guards"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    out = buf[GUARD:GUARD + n].view(shape)
    out.fill_(float("nan"))
    return buf, out


def assert_written(buf, out, what):
    guard = torch.full((GUARD,), SENTINEL, dtype=buf.dtype, device=DEV)
    assert torch.equal(buf[:GUARD], guard) and torch.equal(buf[-GUARD:], guard), f"{what}: a guard was overwritten"
    left = int(torch.isnan(out).sum())
    assert left == 0, f"{what}: {left} of {out.numel()} elements were not written (or are NaN)"


def between_nans(t):
    """t on the device, with NaN before and after it in memory"""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=t.dtype, device=DEV)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def where_ref(t):
    """the tensor the float64 reference is computed from: on the CPU, or on the device for the large cases"""
    return t.to(DEV) if t.numel() >= ON_DEVICE else t.cpu()


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def run_attention(qkv, B, N, H):
    """(out, lse) of cr_attention_fwd_lse, after checking cr_attention_fwd's out against it bit for bit"""
    qd = between_nans(qkv)
    buf0, out0 = guarded((B * N, H * D), bf16)
    lib.call("cr_attention_fwd", qd, out0, B, N, H, D, SCALE)
    assert_written(buf0, out0, "cr_attention_fwd out")
    buf1, out1 = guarded((B * N, H * D), bf16)
    bufl, lse = guarded((B, H, N), f32)
    lib.call("cr_attention_fwd_lse", qd, out1, lse, B, N, H, D, SCALE)
    assert_written(buf1, out1, "cr_attention_fwd_lse out")
    assert_written(bufl, lse, "cr_attention_fwd_lse lse")
    assert torch.equal(out0, out1)
    return out1.cpu(), lse.cpu()


ATTENTION_CASES = [("randn",) + s for s in vr.ATTENTION_SHAPES] + [("peaked",) + s for s in vr.PEAKED_SHAPES] + \
                  [("dominant",) + s for s in vr.DOMINANT_SHAPES]


@pytest.mark.parametrize("kind,B,N,H", ATTENTION_CASES)
def test_attention(kind, B, N, H):
    qkv = vr.attention_input(kind, B, N, H)
    if kind == "dominant":
        print(f"dominant ({B},{N},{H}): smallest per-key maximum of P {vr.assert_dominant(qkv, B, N, H):.4f}")
    out, lse = run_attention(qkv, B, N, H)
    ref, bound = vr.attention(qkv, B, N, H, SCALE)
    lref, lbound = vr.attention_lse(qkv, B, N, H, SCALE)
    exact, e_model = vr.attention_model(qkv, B, N, H, SCALE)
    err = float((out.to(f64) - exact).norm() / (exact.norm() + 1e-300))
    r, rl = vr.report(out, ref, bound), vr.report(lse, lref, lbound)
    print(f"attention {kind} ({B},{N},{H}): out ratio {r['ratio']:.3g}, lse ratio {rl['ratio']:.3g} (bound {vr.C}); "
          f"normwise kernel {err:.3e}, E_model {e_model:.3e}")
    vr.check(out, ref, bound, "attention out")
    vr.check(lse, lref, lbound, "attention lse")
    assert err <= 2 * e_model, (err, e_model)


def test_attention_of_no_tokens_leaves_the_output_alone():
    qkv = torch.zeros(8, 3 * D, dtype=bf16, device=DEV)
    for B, N in ((0, 5), (2, 0)):
        buf, out = guarded((8, D), bf16)
        bufl, lse = guarded((8,), f32)
        before, before_l = buf.clone(), bufl.clone()
        lib.call("cr_attention_fwd", qkv, out, B, N, 1, D, SCALE)
        lib.call("cr_attention_fwd_lse", qkv, out, lse, B, N, 1, D, SCALE)
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int16), before.view(torch.int16))
        assert torch.equal(bufl.view(torch.int32), before_l.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm and the fused residual + LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def run_layernorm(x, gamma, beta):
    buf, y = guarded(tuple(x.shape), bf16)
    lib.call("cr_layernorm", x, gamma, beta, y, x.shape[0], x.shape[1], vr.LN_EPS)
    assert_written(buf, y, "cr_layernorm")
    return y


def run_residual(x, y, gamma):
    buf, out = guarded(tuple(x.shape), bf16)
    lib.call("cr_scale_residual", x, y, gamma, out, x.shape[0], x.shape[1])
    assert_written(buf, out, "cr_scale_residual")
    return out


def run_fused(x, y, ls, gamma, beta):
    bufx, xo = guarded(tuple(x.shape), bf16)
    bufh, ho = guarded(tuple(x.shape), bf16)
    lib.call("cr_scale_residual_layernorm", x, y, ls, gamma, beta, xo, ho, x.shape[0], x.shape[1], vr.LN_EPS)
    assert_written(bufx, xo, "cr_scale_residual_layernorm x_out")
    assert_written(bufh, ho, "cr_scale_residual_layernorm h_out")
    return xo, ho


@pytest.mark.parametrize("C", vr.LN_C)
def test_layernorm_and_fused_residual_layernorm(C):
    worst = {"layernorm": 0.0, "fused h": 0.0, "fused xo": 0.0}
    for M in vr.LN_M:
        for rows in vr.LN_ROWS:
            x, y, ls, gamma, beta = vr.layernorm_input(M, C, rows)
            xd, yd = between_nans(x), between_nans(y)
            lsd, gd, bd = ls.to(DEV), gamma.to(DEV), beta.to(DEV)
            what = f"{M}x{C} {rows}"
            got = run_layernorm(xd, gd, bd).cpu()
            ln_ref = vr.layernorm(x, gamma, beta, vr.LN_EPS)
            worst["layernorm"] = max(worst["layernorm"], fb.report_bf16_out(got, *ln_ref, C)["ratio"])
            fused = []
            for l, ld in ((ls, lsd), (None, None)):
                xo, ho = run_fused(xd, yd, ld, gd, bd)
                x2 = run_residual(xd, yd, ld)
                assert torch.equal(xo, x2) and torch.equal(ho, run_layernorm(x2, gd, bd)), what
                # the statistics are those of the bf16 row the kernel stored: xo is held to its own bound, then h to the
                # LayerNorm of that xo (rounding x + ls y to bf16 a second time in float64 could fall on the other side
                # of a tie)
                xo, ho = xo.cpu(), ho.cpu()
                x_ref, h_ref = vr.residual(x, y, l), vr.layernorm(xo, gamma, beta, vr.LN_EPS)
                worst["fused xo"] = max(worst["fused xo"], vr.report(xo, *x_ref, c=1)["ratio"])
                worst["fused h"] = max(worst["fused h"], fb.report_bf16_out(ho, *h_ref, C)["ratio"])
                fused.append((xo, ho, x_ref, h_ref))
            print(f"{what}: worst ratios so far {worst}")
            fb.check_bf16_out(got, *ln_ref, C, f"layernorm {what}")
            for xo, ho, x_ref, h_ref in fused:
                vr.check(xo, *x_ref, f"fused xo {what}", c=1)
                fb.check_bf16_out(ho, *h_ref, C, f"fused h {what}")
            if rows == "constant":          # x - mean is exactly 0: the rows are beta, as stored
                want = beta.to(bf16).expand(M, C)
                assert torch.equal(got, want) and all(torch.equal(f[1], want) for f in fused), what
    print(f"C = {C}: worst ratio layernorm {worst['layernorm']:.3g}, fused h {worst['fused h']:.3g} (bound {fb.C}); "
          f"fused xo {worst['fused xo']:.3g} of its bound")


@pytest.mark.parametrize("C", [12, 2056])
def test_layernorm_refuses_other_widths(C):
    z = torch.zeros(4, C, dtype=bf16, device=DEV)
    p = torch.zeros(C, device=DEV)
    with pytest.raises(lib.CrError):
        lib.call("cr_layernorm", z, p, p, torch.empty_like(z), 4, C, vr.LN_EPS)
    with pytest.raises(lib.CrError):
        lib.call("cr_scale_residual_layernorm", z, z, p, p, p, torch.empty_like(z), torch.empty_like(z), 4, C, vr.LN_EPS)


# ---------------------------------------------------------------------------------------------------------------------
# GELU and residual
# ---------------------------------------------------------------------------------------------------------------------
def run_gelu(x):
    """in place: the buffer is the input between two guards"""
    buf = torch.full((x.numel() + 2 * GUARD,), SENTINEL, dtype=bf16, device=DEV)
    y = buf[GUARD:GUARD + x.numel()]
    y.copy_(x.flatten())
    lib.call("cr_gelu_inplace", y, y.numel())
    assert_written(buf, y, "cr_gelu_inplace")
    return y


@pytest.mark.parametrize("n", ["grid"] + vr.GELU_N)
def test_gelu(n):
    x = vr.bf16_grid() if n == "grid" else vr.gelu_input(n)
    got = run_gelu(x)
    ref, bound = vr.gelu(where_ref(x))
    r = vr.report(got, ref, bound)
    print(f"gelu {n} ({x.numel()} values): worst ratio {r['ratio']:.3g} (bound {vr.C})")
    vr.check(got, ref, bound, f"gelu {n}")


def test_gelu_refuses_a_length_that_is_no_multiple_of_8():
    with pytest.raises(lib.CrError):
        lib.call("cr_gelu_inplace", torch.zeros(16, dtype=bf16, device=DEV), 12)


@pytest.mark.parametrize("M,C", vr.RESIDUAL_MC)
def test_scale_residual(M, C):
    x, y, gamma = vr.residual_input(M, C)
    xd, yd = between_nans(x), between_nans(y)
    for g in (gamma, None):
        got = run_residual(xd, yd, None if g is None else g.to(DEV))
        ref, bound = vr.residual(where_ref(x), where_ref(y), None if g is None else g.to(where_ref(x).device))
        r = vr.report(got, ref, bound, c=1)
        print(f"residual {M}x{C} {'with' if g is not None else 'without'} gamma: worst {r['ratio']:.3g} of the bound")
        vr.check(got, ref, bound, f"residual {M}x{C}", c=1)


# ---------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------
def run_resize(x, Ho, Wo):
    B, h, w, C = x.shape
    buf, y = guarded((B, Ho, Wo, C), bf16)
    lib.call("cr_resize_bilinear_ac", x, y, B, h, w, Ho, Wo, C)
    assert_written(buf, y, "cr_resize_bilinear_ac")
    return y


@pytest.mark.parametrize("B,h,w,Ho,Wo,C", vr.RESIZE_SHAPES + [vr.RESIZE_PAST_CAP])
def test_resize(B, h, w, Ho, Wo, C):
    x = vr.resize_input(B, h, w, C)
    got = run_resize(between_nans(x), Ho, Wo)
    big = B * Ho * Wo * C >= ON_DEVICE
    ref, bound = vr.resize(x.to(DEV) if big else x, Ho, Wo)
    r = vr.report(got, ref, bound, c=1)
    print(f"resize ({h},{w})->({Ho},{Wo}) C = {C}: worst {r['ratio']:.3g} of the bound")
    vr.check(got, ref, bound, f"resize ({h},{w})->({Ho},{Wo})", c=1)
    if (h, w) == (Ho, Wo):
        assert torch.equal(got.cpu(), x)


# ---------------------------------------------------------------------------------------------------------------------
# the ops.* wrappers return the bits of the direct calls
# ---------------------------------------------------------------------------------------------------------------------
def test_wrappers_equal_the_direct_calls():
    B, N, H = 2, 65, 2
    qd = vr.attention_input("randn", B, N, H).to(DEV)
    _, out = guarded((B * N, H * D), bf16)
    _, lse = guarded((B, H, N), f32)
    lib.call("cr_attention_fwd_lse", qd, out, lse, B, N, H, D, SCALE)
    assert torch.equal(ops.attention(qd, B, N, H, D, SCALE), out)
    o2, l2 = ops.attention_lse(qd, B, N, H, D, SCALE)
    assert torch.equal(o2, out) and torch.equal(l2, lse)
    x, y, ls, gamma, beta = (t.to(DEV) for t in vr.layernorm_input(5, 520, "ordinary"))
    assert torch.equal(ops.layernorm(x, gamma, beta, vr.LN_EPS), run_layernorm(x, gamma, beta))
    assert torch.equal(ops.scale_residual(x, y, ls), run_residual(x, y, ls))
    assert torch.equal(ops.scale_residual(x, y), run_residual(x, y, None))
    for l in (ls, None):
        xo, ho = ops.scale_residual_layernorm(x, y, l, gamma, beta, vr.LN_EPS)
        xo2, ho2 = run_fused(x, y, l, gamma, beta)
        assert torch.equal(xo, xo2) and torch.equal(ho, ho2)
    xg = vr.gelu_input(2400)
    assert torch.equal(ops.gelu_(xg.to(DEV).clone()), run_gelu(xg))
    xr = vr.resize_input(2, 5, 9, 16).to(DEV)
    assert torch.equal(ops.resize_bilinear_ac(xr, (13, 4)), run_resize(xr, 13, 4))


# ---------------------------------------------------------------------------------------------------------------------
# the model's glue around two GEMMs of the DPT head
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 4])
def test_deconv_ks_both_routes(k):
    """ConvTranspose2d with kernel == stride as one GEMM and a pixel shuffle: the cached inference route and the training
    route against F.conv_transpose2d in float64 (Cin != Cout, h != w; the weight holds bf16 values, which both routes
    round to)"""
    Cin, Cout, B, h, w = 32, 48, 2, 5, 7
    g = torch.Generator().manual_seed(k)
    m = torch.nn.ConvTranspose2d(Cin, Cout, kernel_size=k, stride=k)
    with torch.no_grad():
        m.weight.copy_((torch.randn(Cin, Cout, k, k, generator=g) * Cin ** -0.5).to(bf16))
        m.bias.copy_(torch.randn(Cout, generator=g))
    m = m.to(DEV)
    x = torch.randn(B, h, w, Cin, generator=g).to(bf16)
    x64, w64, b64 = x.to(f64).permute(0, 3, 1, 2), m.weight.detach().cpu().to(f64), m.bias.detach().cpu().to(f64)
    ref = F.conv_transpose2d(x64, w64, b64, stride=k).permute(0, 2, 3, 1)
    absref = F.conv_transpose2d(x64.abs(), w64.abs(), b64.abs(), stride=k).permute(0, 2, 3, 1)
    m.eval()
    with torch.no_grad():
        infer = dpt.deconv_ks(x.to(DEV), m)
    m.train()
    with torch.enable_grad():
        train = dpt.deconv_ks(x.to(DEV), m)
    for name, got in (("inference", infer), ("training", train)):
        assert got.shape == (B, h * k, w * k, Cout) and got.dtype == bf16 and got.is_contiguous()
        r = fb.report_bf16_out(got.detach().cpu(), ref, absref, Cin)
        print(f"deconv_ks k = {k} {name}: worst ratio {r['ratio']:.3g} (bound {fb.C})")
        fb.check_bf16_out(got.detach().cpu(), ref, absref, Cin, f"deconv_ks k = {k} {name}")
    assert train.requires_grad and not infer.requires_grad


def test_final_1x1():
    """the 32 -> 1 convolution in row 0 of a zero-padded 16-row weight; float32 output"""
    g = torch.Generator().manual_seed(9)
    conv = torch.nn.Conv2d(32, 1, kernel_size=1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(1, 32, 1, 1, generator=g) * 0.3)
        conv.bias.copy_(torch.randn(1, generator=g))
    conv = conv.to(DEV)
    head = types.SimpleNamespace(scratch=types.SimpleNamespace(output_conv2=[None, None, conv]))
    x = torch.relu(torch.randn(2, 9, 11, 32, generator=g)).to(bf16)
    got = dpt.DPTHead._final_1x1(head, x.to(DEV))
    assert got.shape == (2, 9, 11) and got.dtype == f32
    wv = conv.weight.detach().cpu().to(bf16)                      # the value the kernel sees
    ref, absref, K = fb.conv_fwd(x.permute(0, 3, 1, 2), wv, conv.bias.detach().cpu(), 1, 0)
    r = fb.report(got.cpu(), ref[:, 0], absref[:, 0], K)
    print(f"final 1x1: worst ratio {r['ratio']:.3g} (bound {fb.C})")
    fb.check(got.cpu(), ref[:, 0], absref[:, 0], K, "final 1x1")
