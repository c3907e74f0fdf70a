"""The bounds of tests/vit_ref.py, tested without a GPU: torch float32 emulations of the arithmetic of each forward kernel
of csrc/vit.hip (attention as 64-key tiles with the online rescale, bf16 P, bf16 stores; the resize with its float32
coordinates) must pass their bound at the inputs of tests/test_gpu_vit_fwd_f64.py, and the same emulation with one defect
of the kind such kernels have must fail it.  The emulations share no code with the float64 references."""
import math

import pytest
import torch

import f64_bound as fb
import vit_ref as vr

f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
D, TK = vr.D, 64


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def emu_attention(qkv, B, N, H, scale, defect=None):
    """the kernel's schedule in float32: keys in tiles of 64 (the last one zero-padded and masked), running maximum m and
    sum l with the rescale alpha, P rounded to bf16 for the second product only, out = o * (1 / l) stored as bf16, and
    lse = m + log l.  Returns (out (B*N, H*64) bf16, lse (B,H,N) float32)."""
    q, k, v = qkv.to(f32).view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    n_keys = N - 1 if defect == "last_key_ignored" else N
    ntiles = (N + TK - 1) // TK
    pad = ntiles * TK - N
    k = torch.nn.functional.pad(k, (0, 0, 0, pad))
    v = torch.nn.functional.pad(v, (0, 0, 0, pad))
    m = torch.full((B, H, N), -math.inf)
    l = torch.zeros(B, H, N)
    o = torch.zeros(B, H, N, D)
    for t in range(ntiles):
        ks, vs = k[:, :, t * TK:(t + 1) * TK], v[:, :, t * TK:(t + 1) * TK]
        s = (q @ ks.transpose(-2, -1)) * scale
        key = torch.arange(t * TK, (t + 1) * TK)
        valid = key < n_keys
        if defect == "tail_key_unmasked":
            valid = key < min(n_keys + 1, ntiles * TK)
        s = torch.where(valid, s, torch.full_like(s, -math.inf))
        m_new = torch.maximum(m, s.amax(-1))
        alpha = torch.exp(m - m_new)
        p = torch.exp(s - m_new[..., None])
        l = l * alpha + p.sum(-1)
        if defect == "alpha_skipped" and t == 1:
            alpha = torch.ones_like(alpha)
        o = o * alpha[..., None] + p.to(bf16).to(f32) @ vs
        m = m_new
    out = (o * (1.0 / l)[..., None]).to(bf16)
    lse = m if defect == "lse_without_log_l" else m + torch.log(l)
    return out.transpose(1, 2).reshape(B * N, H * D), lse


def attention_bad(kind, B, N, H, defect=None):
    """elements of (out, lse) over their bounds, and whether the normwise criterion holds"""
    qkv = vr.attention_input(kind, B, N, H)
    out, lse = emu_attention(qkv, B, N, H, vr.SCALE, defect)
    r_out = vr.report(out, *vr.attention(qkv, B, N, H, vr.SCALE))
    r_lse = vr.report(lse, *vr.attention_lse(qkv, B, N, H, vr.SCALE))
    exact, e_model = vr.attention_model(qkv, B, N, H, vr.SCALE)
    norm_ok = float((out.to(f64) - exact).norm()) <= 2 * e_model * float(exact.norm())
    return r_out, r_lse, norm_ok


CASES = [("randn",) + s for s in vr.ATTENTION_SHAPES] + [("peaked",) + s for s in vr.PEAKED_SHAPES] + \
        [("dominant",) + s for s in vr.DOMINANT_SHAPES]


@pytest.mark.parametrize("kind,B,N,H", CASES)
def test_clean_attention_passes(kind, B, N, H):
    r_out, r_lse, norm_ok = attention_bad(kind, B, N, H)
    print(f"attention {kind} ({B},{N},{H}): out ratio {r_out['ratio']:.3g}, lse ratio {r_lse['ratio']:.3g} (bound {vr.C})")
    assert r_out["bad"] == 0 and r_lse["bad"] == 0 and norm_ok


@pytest.mark.parametrize("B,N,H", vr.DOMINANT_SHAPES)
def test_dominant_case_precondition(B, N, H):
    least = vr.assert_dominant(vr.attention_input("dominant", B, N, H), B, N, H)
    print(f"dominant ({B},{N},{H}): smallest per-key maximum of P {least:.4f}")


def test_last_key_ignored_fails_at_the_models_length():
    """one key of 1370 changes little of the whole tensor's norm; element-wise it shows in thousands of places"""
    B, N, H = 1, 1370, 2
    qkv = vr.attention_input("randn", B, N, H)
    out, _ = emu_attention(qkv, B, N, H, vr.SCALE, "last_key_ignored")
    exact, _ = vr.attention_model(qkv, B, N, H, vr.SCALE)
    norm = float((out.to(f64) - exact).norm() / exact.norm())
    r = vr.report(out, *vr.attention(qkv, B, N, H, vr.SCALE))
    print(f"last key ignored at N = 1370: normwise {norm:.3g}, {r['bad']} elements over the bound")
    assert r["bad"] > 0
    # the dominant case: the query whose key it is loses its whole row
    r_out, r_lse, norm_ok = attention_bad("dominant", 1, 1370, 1, "last_key_ignored")
    assert r_out["bad"] >= D and r_lse["bad"] > 0 and not norm_ok


@pytest.mark.parametrize("kind,B,N,H", [("randn", 1, 1, 1), ("randn", 2, 17, 2), ("randn", 2, 65, 2)])
def test_unmasked_tail_key_fails(kind, B, N, H):
    """key N of the zero-padded last tile takes part with score 0: it adds exp(0 - m) to every row's sum (one key's worth
    of weight: below the bf16 roundings once a row has hundreds of keys, so the short sequences are the ones that show it)"""
    r_out, r_lse, _ = attention_bad(kind, B, N, H, "tail_key_unmasked")
    assert r_out["bad"] > 0 and r_lse["bad"] > 0


@pytest.mark.parametrize("kind,B,N,H", [("randn", 2, 129, 1), ("randn", 1, 197, 6), ("peaked", 1, 300, 2), ("dominant", 1, 197, 3)])
def test_skipped_rescale_fails(kind, B, N, H):
    r_out, _, norm_ok = attention_bad(kind, B, N, H, "alpha_skipped")
    assert r_out["bad"] > 0


@pytest.mark.parametrize("kind,B,N,H", [("randn", 1, 15, 1), ("randn", 1, 197, 6), ("peaked", 1, 300, 2)])
def test_lse_without_log_l_fails(kind, B, N, H):
    r_out, r_lse, norm_ok = attention_bad(kind, B, N, H, "lse_without_log_l")
    assert r_out["bad"] == 0 and norm_ok and r_lse["bad"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm, residual, GELU
# ---------------------------------------------------------------------------------------------------------------------
def emu_layernorm(x, gamma, beta, eps, defect=None):
    x = x.to(f32)
    C = x.shape[1]
    n = (C + 511) // 512 * 512 if defect == "chunk_statistics" else C
    mean = x.sum(1, keepdim=True) / n
    q = ((x - mean) ** 2).sum(1, keepdim=True)
    if defect == "chunk_statistics":
        q = q + (n - C) * mean ** 2                  # the padding lanes hold 0
    inv = torch.rsqrt(q / n + eps)
    return ((x - mean) * inv * gamma + beta).to(bf16)


def emu_residual(x, y, gamma):
    return (x.to(f32) + (y.to(f32) if gamma is None else gamma * y.to(f32))).to(bf16)


@pytest.mark.parametrize("C", vr.LN_C)
def test_clean_layernorm_and_fused_residual_pass(C):
    worst = 0.0
    for M in vr.LN_M:
        for rows in vr.LN_ROWS:
            x, y, ls, gamma, beta = vr.layernorm_input(M, C, rows)
            got = emu_layernorm(x, gamma, beta, vr.LN_EPS)
            worst = max(worst, fb.check_bf16_out(got, *vr.layernorm(x, gamma, beta, vr.LN_EPS), C, f"layernorm {M}x{C} {rows}")["ratio"])
            if rows == "constant":
                assert torch.equal(got, beta.to(bf16).expand(M, C))
            for l in (ls, None):
                xo = emu_residual(x, y, l)
                vr.check(xo, *vr.residual(x, y, l), f"residual {M}x{C} {rows}", c=1)
                h = emu_layernorm(xo, gamma, beta, vr.LN_EPS)
                fb.check_bf16_out(h, *vr.layernorm(xo, gamma, beta, vr.LN_EPS), C, f"fused h {M}x{C} {rows}")
    print(f"layernorm C = {C}: worst ratio {worst:.3g} (bound {fb.C})")


@pytest.mark.parametrize("C", [8, 520, 1032])
def test_layernorm_statistics_over_the_padded_chunk_fail(C):
    x, _, _, gamma, beta = vr.layernorm_input(5, C, "ordinary")
    got = emu_layernorm(x, gamma, beta, vr.LN_EPS, "chunk_statistics")
    assert fb.report_bf16_out(got, *vr.layernorm(x, gamma, beta, vr.LN_EPS), C)["bad"] > 0


@pytest.mark.parametrize("M,C", vr.RESIDUAL_MC)
def test_clean_residual_passes(M, C):
    x, y, gamma = vr.residual_input(M, C)
    for g in (gamma, None):
        r = vr.check(emu_residual(x, y, g), *vr.residual(x, y, g), f"residual {M}x{C}", c=1)
    print(f"residual {M}x{C}: worst fraction of the bound {r['ratio']:.3g}")
    # a gamma taken from the neighbouring channel
    assert vr.report(emu_residual(x, y, gamma.roll(1)), *vr.residual(x, y, gamma))["bad"] > 0


def emu_gelu(x, defect=None):
    x = x.to(f32)
    if defect == "tanh":
        return (0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))).to(bf16)
    return (0.5 * x * (1 + torch.erf(x * 0.70710678118654752))).to(bf16)


def test_clean_gelu_passes_and_the_tanh_form_fails():
    inputs = [vr.bf16_grid()] + [vr.gelu_input(n) for n in vr.GELU_N]
    for x in inputs:
        r = vr.check(emu_gelu(x), *vr.gelu(x), f"gelu n = {x.numel()}")
        print(f"gelu n = {x.numel()}: worst ratio {r['ratio']:.3g} (bound {vr.C})")
    x = inputs[0]
    assert float(x.float().min()) == -12 and float(x.float().max()) == 12 and x.numel() % 8 == 0
    assert vr.report(emu_gelu(x, "tanh"), *vr.gelu(x))["bad"] > 0
    # the absolute term is needed: the float32 formula itself is far over a purely relative bound at negative x
    ref, _ = vr.gelu(x)
    err = (emu_gelu(x).to(f64) - ref).abs()
    assert bool((err > vr.U_BF16 * ref.abs() + vr.TINY).any())


# ---------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------
def emu_resize(x, Ho, Wo, defect=None):
    """the kernel's arithmetic in float32 on the flat NHWC buffer, followed by NaN as the memory past it"""
    B, h, w, C = x.shape
    flat = torch.cat([x.to(f32).reshape(-1), torch.full((w * C + C,), math.nan)])
    sy = torch.tensor(float(h - 1)) / torch.tensor(float(Ho - 1)) if Ho > 1 else torch.tensor(0.0)
    sx = torch.tensor(float(w - 1)) / torch.tensor(float(Wo - 1)) if Wo > 1 else torch.tensor(0.0)
    oy, ox = torch.arange(Ho, dtype=f32), torch.arange(Wo, dtype=f32)
    if defect == "align_corners_false":
        fy = torch.clamp((oy + 0.5) * (h / Ho) - 0.5, min=0.0)
        fx = torch.clamp((ox + 0.5) * (w / Wo) - 0.5, min=0.0)
    else:
        fy, fx = sy * oy, sx * ox
    y0, x0 = torch.clamp(fy.to(torch.int64), max=h - 1), torch.clamp(fx.to(torch.int64), max=w - 1)
    y1 = y0 + 1 if defect == "y1_unclamped" else torch.clamp(y0 + 1, max=h - 1)
    x1 = torch.clamp(x0 + 1, max=w - 1)
    ly, lx = (fy - y0.to(f32)).view(1, Ho, 1, 1), (fx - x0.to(f32)).view(1, 1, Wo, 1)
    base = (torch.arange(B) * (h * w * C)).view(B, 1, 1, 1) + torch.arange(C).view(1, 1, 1, C)

    def at(yy, xx):
        return flat[base + ((yy.view(1, Ho, 1, 1) * w + xx.view(1, 1, Wo, 1)) * C)]
    t00, t01, t10, t11 = at(y0, x0), at(y0, x1), at(y1, x0), at(y1, x1)
    top, bot = t00 + (t01 - t00) * lx, t10 + (t11 - t10) * lx
    return (top + (bot - top) * ly).to(bf16)


@pytest.mark.parametrize("B,h,w,Ho,Wo,C", vr.RESIZE_SHAPES + [vr.RESIZE_PAST_CAP])
def test_clean_resize_passes(B, h, w, Ho, Wo, C):
    x = vr.resize_input(B, h, w, C)
    got = emu_resize(x, Ho, Wo)
    r = vr.check(got, *vr.resize(x, Ho, Wo), f"resize ({h},{w})->({Ho},{Wo})", c=1)
    print(f"resize ({h},{w})->({Ho},{Wo}): worst fraction of the bound {r['ratio']:.3g}")
    if (h, w) == (Ho, Wo):
        assert torch.equal(got, x)


@pytest.mark.parametrize("B,h,w,Ho,Wo,C", [(2, 7, 10, 14, 20, 32), (2, 148, 148, 518, 518, 16), (2, 20, 30, 7, 11, 8)])
def test_resize_with_align_corners_false_coordinates_fails(B, h, w, Ho, Wo, C):
    x = vr.resize_input(B, h, w, C)
    assert vr.report(emu_resize(x, Ho, Wo, "align_corners_false"), *vr.resize(x, Ho, Wo))["bad"] > 0


@pytest.mark.parametrize("B,h,w,Ho,Wo,C", [(2, 8, 8, 8, 8, 8), (2, 1, 9, 4, 30, 8), (2, 37, 37, 74, 74, 64)])
def test_resize_with_y1_not_clamped_fails(B, h, w, Ho, Wo, C):
    """row h of the last image lies past the buffer; its weight is 0 (or a rounding error), and 0 * NaN is NaN"""
    x = vr.resize_input(B, h, w, C)
    assert vr.report(emu_resize(x, Ho, Wo, "y1_unclamped"), *vr.resize(x, Ho, Wo))["bad"] > 0
