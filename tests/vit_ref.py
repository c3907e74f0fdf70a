"""Float64 references and element-wise error bounds for the forward kernels of the depth model (csrc/vit.hip): attention
and its log-sum-exp rows, LayerNorm, LayerScale + residual, GELU and the bilinear resize (a plain test module, not a
conftest; tests/test_vit_ref.py tests the bounds themselves on the CPU).

Every function takes the values the kernel sees (the bf16 inputs, after their rounding; float32 parameters as they are),
computes on the device of its inputs and returns float64 tensors (ref, bound): the kernel's result `got` must satisfy
|got - ref| <= bound at every element.  `layernorm` returns (ref, absref) for f64_bound.check_bf16_out instead.  The bounds
are built from the unit roundoffs U (float32) and U_BF16, the constant C = 4 of f64_bound and float64 magnitudes of the
terms that are added; none holds a number fitted to a case.  TINY (f64_bound's) is added to each: a unit roundoff says
nothing below the normal range, where a result may be flushed or lose its low bits."""
import math

import torch
import torch.nn.functional as F

import f64_bound as fb

U, U_BF16, C, TINY = fb.U, fb.U_BF16, fb.C, fb.TINY
f64, bf16 = torch.float64, torch.bfloat16
D = 64                  # head dimension of the attention kernel


def rb(t):
    """round a float64 tensor to bfloat16 (nearest even), back in float64"""
    return t.to(torch.float32).to(bf16).to(f64)


def report(got, ref, bound, c=C):
    """worst element of got against (ref, bound): "ratio" = c * max |got - ref| / bound, so that the bound holds exactly when
    ratio <= c (the convention of f64_bound.report); a NaN in got counts as over the bound"""
    got = got.detach().to(ref.device, f64)
    assert got.shape == ref.shape == bound.shape, (tuple(got.shape), tuple(ref.shape), tuple(bound.shape))
    if ref.numel() == 0:
        return {"ratio": 0.0, "bad": 0, "n": 0, "where": (), "got": 0.0, "ref": 0.0, "bound": 0.0, "norm": 0.0}
    err = (got - ref).abs()
    nan = torch.isnan(got)
    bad = (err > bound) | nan
    ratio = torch.where(nan, torch.full_like(err, float("inf")), c * err / bound)
    i = int(ratio.flatten().argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
    return {"ratio": float(ratio.flatten()[i]), "bad": int(bad.sum()), "n": ref.numel(), "where": idx,
            "got": float(got.flatten()[i]), "ref": float(ref.flatten()[i]), "bound": float(bound.flatten()[i]),
            "norm": float((got - ref).norm() / (ref.norm() + 1e-300))}


def check(got, ref, bound, what, c=C):
    r = report(got, ref, bound, c)
    assert r["bad"] == 0, f"{what}: {r['bad']} of {r['n']} elements over the bound; worst ratio {r['ratio']:.3g} > {c} at index " \
                          f"{r['where']} (got {r['got']:.9g}, ref {r['ref']:.9g}, bound {r['bound']:.3g}); normwise {r['norm']:.3g}"
    return r


# ---------------------------------------------------------------------------------------------------------------------
# attention, head dimension 64.  qkv (B*N, 3*H*64) bf16 in the packed layout of the qkv linear; results in the kernel's
# layouts: out (B*N, H*64), lse (B, H, N).
# ---------------------------------------------------------------------------------------------------------------------
def _qkv(qkv, B, N, H):
    return qkv.to(f64).view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)               # 3 x (B,H,N,D)


def _rows(t, B, N, H):
    return t.transpose(1, 2).reshape(B * N, H * D)


def attention_probs(qkv, B, N, H, scale):
    """P = softmax(scale q k^T), (B,H,N,N) float64"""
    q, k, _ = _qkv(qkv, B, N, H)
    return torch.softmax(scale * q @ k.transpose(-2, -1), dim=-1)


def attention(qkv, B, N, H, scale, c=C):
    """ref = P v with P = softmax(scale q k^T); absref = P |v|.

    The kernel accumulates sum_j p_j v_j with p_j = exp(s_j - m) rounded to bf16, and divides by the sum of the unrounded
    p_j.  Rounding p_j moves each term by at most U_BF16 p_j |v_j|: U_BF16 * absref after the division.  The bf16 store
    moves the quotient by at most U_BF16 times its magnitude, which is |ref| up to the other errors.  What is left is
    float32: the 64 products of a score, the exponential, and N additions each of numerator and denominator -- a random
    walk of N + 64 roundings of unit roundoff U over terms of total magnitude absref, the form of f64_bound.check.  So

        |got - ref| <= U_BF16 (absref + |ref|) + c U sqrt(N + 64) absref + TINY"""
    _, _, v = _qkv(qkv, B, N, H)
    P = attention_probs(qkv, B, N, H, scale)
    ref, absref = P @ v, P @ v.abs()
    bound = U_BF16 * (absref + ref.abs()) + c * U * math.sqrt(N + D) * absref + TINY
    return _rows(ref, B, N, H), _rows(bound, B, N, H)


def attention_model(qkv, B, N, H, scale):
    """(exact, E_model) of the normwise criterion ||got - exact|| <= 2 E_model ||exact|| (the one the backward kernels are
    held to): E_model is the normwise error of the same float64 pipeline with the two roundings a bf16 MFMA kernel cannot
    avoid, P before the second product and the output"""
    _, _, v = _qkv(qkv, B, N, H)
    P = attention_probs(qkv, B, N, H, scale)
    exact = P @ v
    model = rb(rb(P) @ v)
    return _rows(exact, B, N, H), float((model - exact).norm() / (exact.norm() + 1e-300))


def attention_lse(qkv, B, N, H, scale, c=C):
    """ref = log sum_j exp(s_j), s = scale q k^T (float32 in the kernel: m + log l).

    A score is a float32 contraction of 64 exact products: off by about U sqrt(64) s_abs, s_abs = scale max_j sum_d |q_d|
    |k_jd|, and log-sum-exp moves by at most the largest change of a score.  m + log l rounds relative to |ref| and to
    log l, which is at most |ref| + |m| <= |ref| + s_abs; the exponentials and the sum put a few U into l, i.e. a few U
    absolute into log l.  So

        |lse - ref| <= c U (8 s_abs + |ref| + 1) + TINY"""
    q, k, _ = _qkv(qkv, B, N, H)
    ref = torch.logsumexp(scale * q @ k.transpose(-2, -1), dim=-1)
    s_abs = scale * (q.abs() @ k.abs().transpose(-2, -1)).amax(-1)
    return ref, c * U * (math.sqrt(D) * s_abs + ref.abs() + 1) + TINY


# ---------------------------------------------------------------------------------------------------------------------
# row-wise and element-wise kernels on (M, C)
# ---------------------------------------------------------------------------------------------------------------------
def layernorm(x, gamma, beta, eps):
    """(ref, absref) of LayerNorm over the last dimension for f64_bound.check_bf16_out(got, ref, absref, K=C).

    The statistics are sums of C terms in float32 (K = C), and an output element is (x - mean) inv gamma + beta: absref is
    that expression with every term taken by magnitude, inv (|x| + |mean|) |gamma| + |beta| -- the one the float32-stream
    LayerNorm of the training route is held to.  For the fused residual + LayerNorm kernel x is the bf16 row it stored."""
    x, gamma, beta = x.to(f64), gamma.to(f64), beta.to(f64)
    ref = F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    mean = x.mean(-1, keepdim=True)
    inv = 1.0 / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps)
    return ref, inv * (x.abs() + mean.abs()) * gamma.abs() + beta.abs()


def residual(x, y, gamma):
    """ref = x + gamma y (gamma float32 per channel, or None = 1), stored as bf16.  Two float32 roundings, of the product and
    of the sum, each at most U times a magnitude below |x| + |gamma y|, then the bf16 store:

        |got - ref| <= U_BF16 |ref| + 2 U (|x| + |gamma y|) + TINY"""
    x, y = x.to(f64), y.to(f64)
    gy = y if gamma is None else gamma.to(f64) * y
    ref = x + gy
    return ref, U_BF16 * ref.abs() + 2 * U * (x.abs() + gy.abs()) + TINY


def gelu(x, c=C):
    """ref = x Phi(x) (the erf form), stored as bf16.  In float32 the kernel forms 0.5 x (1 + erff(x / sqrt 2)); the sum
    1 + erff cancels for negative x, so its rounding error, about U, stays absolute there while Phi(x) itself falls to 0:
    the float32 error is c U |x|, not a multiple of |ref|.

        |got - ref| <= U_BF16 |ref| + c U |x| + TINY"""
    x = x.to(f64)
    ref = F.gelu(x)
    return ref, U_BF16 * ref.abs() + c * U * x.abs() + TINY


# ---------------------------------------------------------------------------------------------------------------------
# bilinear resize, align_corners=True.  x (B, h, w, Ch) NHWC.
# ---------------------------------------------------------------------------------------------------------------------
def _axis_corners(n_in, n_out, device):
    """per output index of one axis: the two input indices the exact coordinate o (n_in - 1) / (n_out - 1) lies between, and
    the pair one below where that coordinate is an integer (integer arithmetic: no rounding).  A float32 coordinate
    cannot cross an integer otherwise: a non-integer coordinate is at least 1 / (n_out - 1) away from one."""
    o = torch.arange(n_out, device=device, dtype=torch.int64)
    num, den = o * (n_in - 1), max(n_out - 1, 1)
    i0 = torch.clamp(num // den, max=n_in - 1)
    i1 = torch.clamp(i0 + 1, max=n_in - 1)
    below = torch.where(num % den == 0, torch.clamp(i0 - 1, min=0), i0)
    return (i0, i1), (below, torch.clamp(below + 1, max=n_in - 1))


def resize_sum4(x, Ho, Wo):
    """sum of the magnitudes of the four corner values each output element is interpolated from, (B, Ho, Wo, Ch) float64.
    Where the exact source coordinate is an integer k, float32 may give k - epsilon and the kernel then reads k - 1 and k
    instead of k and k + 1: the larger of the two sums is taken there."""
    a = x.to(f64).abs()
    h, w = a.shape[1], a.shape[2]
    best = None
    for y0, y1 in _axis_corners(h, Ho, a.device):
        for x0, x1 in _axis_corners(w, Wo, a.device):
            s = sum(a[:, yy][:, :, xx] for yy in (y0, y1) for xx in (x0, x1))
            best = s if best is None else torch.maximum(best, s)
    return best


def resize(x, Ho, Wo):
    """ref = float64 F.interpolate(mode="bilinear", align_corners=True), stored as bf16.

    The kernel's source coordinate is fl(fl(s) o) with s = (h - 1) / (Ho - 1): two roundings of a value of at most h - 1,
    so it is off by at most 2 U (h - 1), and by 2 U (w - 1) on the x axis.  A weight that is off by d moves the result by
    at most d times the difference of two corner values, which is below d * sum4.  The three lerps a + (b - a) t add six
    float32 roundings of at most U sum4 each.  With B = U (2 (h + w) + 6) sum4 for the float32 value,

        |got - ref| <= B + U_BF16 (|ref| + B) + TINY

    (this bound and `residual`'s count their roundings one by one and have no free constant: report them with c = 1)"""
    xd = x.to(f64)
    h, w = xd.shape[1], xd.shape[2]
    ref = F.interpolate(xd.permute(0, 3, 1, 2), (Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    Bf = U * (2 * (h + w) + 6) * resize_sum4(x, Ho, Wo)
    return ref, Bf + U_BF16 * (ref.abs() + Bf) + TINY


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_vit_fwd_f64.py; tests/test_vit_ref.py runs its float32 emulations on the same inputs.
# Inputs are drawn on the CPU from seeded generators, so both files see the same values.
# ---------------------------------------------------------------------------------------------------------------------
ATTENTION_SHAPES = [(1, 1, 1), (1, 15, 1), (1, 16, 2), (2, 17, 2),          # a partial wave
                    (1, 63, 1), (1, 64, 3), (2, 65, 2),                     # the key-tile edge (64 keys)
                    (1, 127, 1), (1, 128, 2), (2, 129, 1),                  # the query-tile edge (128 queries)
                    (1, 197, 6),                                            # 12 blocks: renumbered body 8, remainder 4
                    (2, 200, 5),                                            # 20 blocks: 2 per XCD, remainder 4
                    (1, 300, 3),                                            # 9 blocks
                    (1, 1370, 2)]                                           # the model's own sequence length (518 x 518)
PEAKED_SHAPES = [(1, 300, 2)]
DOMINANT_SHAPES = [(2, 17, 2), (2, 65, 2), (1, 130, 2), (1, 197, 3), (1, 1370, 1)]
SCALE = D ** -0.5


def attention_input(kind, B, N, H):
    """qkv (B*N, 3*H*64) bf16.  "randn": randn * 1.5.  "peaked": randn with q * 12 (large logits).  "dominant": per batch
    and head q_i = 4 k_pi(i) for a seeded permutation pi, so that every key position -- each one of the last partial tile
    and of the MFMA key mapping among them -- carries nearly all the weight of exactly one query (`dominant_perm`
    returns pi, `assert_dominant` the precondition); 4 k is exact in bf16."""
    if kind == "randn":
        g = torch.Generator().manual_seed(N * 7 + H)
        return (torch.randn(B * N, 3 * H * D, generator=g) * 1.5).to(bf16)
    if kind == "peaked":
        g = torch.Generator().manual_seed(3)
        qkv = torch.randn(B * N, 3 * H * D, generator=g)
        qkv.view(B, N, 3, H, D)[:, :, 0] *= 12.0
        return qkv.to(bf16)
    assert kind == "dominant"
    g = torch.Generator().manual_seed(5000 + N)
    qkv = torch.randn(B * N, 3 * H * D, generator=g).to(bf16)
    v5 = qkv.view(B, N, 3, H, D)
    pi = dominant_perm(B, N, H)
    for b in range(B):
        for h in range(H):
            v5[b, :, 0, h] = 4.0 * v5[b, pi[b, h], 1, h]
    return qkv


def dominant_perm(B, N, H):
    g = torch.Generator().manual_seed(7000 + N)
    return torch.stack([torch.stack([torch.randperm(N, generator=g) for _ in range(H)]) for _ in range(B)])     # (B,H,N)


def assert_dominant(qkv, B, N, H):
    """the precondition of the dominant case, on the float64 reference: argmax_j P_ij = pi(i), and every key has a query
    with P >= 0.9.  Returns the smallest of those per-key maxima."""
    P = attention_probs(qkv, B, N, H, SCALE)
    assert torch.equal(P.argmax(-1), dominant_perm(B, N, H).to(P.device))
    least = float(P.amax(-2).min())
    assert least >= 0.9, least
    return least


LN_C = [8, 64, 384, 512, 520, 1024, 1032, 1536, 2048]      # first / last lane of each 512-channel chunk; NCH = 4 at its limit
LN_M = [1, 3, 4, 5, 37]                                    # 4 rows per block
LN_ROWS = ["ordinary", "offset", "constant"]
LN_EPS = 1e-6
LN_CONSTANT = 3.25


def layernorm_input(M, C, rows):
    """(x, y, ls, gamma, beta): x (M,C) bf16 is the LayerNorm input and the residual stream of the fused kernel, y its
    branch (zero for the constant rows, so that x + ls y stays constant)"""
    g = torch.Generator().manual_seed(M * 4099 + C)
    x = torch.randn(M, C, generator=g)
    y = torch.randn(M, C, generator=g).to(bf16)
    ls, gamma, beta = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    if rows == "ordinary":
        x = x * 3 + 1.5
    elif rows == "offset":
        x = x + 16
    else:
        x, y = torch.full((M, C), LN_CONSTANT), torch.zeros(M, C, dtype=bf16)
    return x.to(bf16), y, ls, gamma, beta


ELEMENTWISE_BLOCK_CAP = 8192 * 256          # 16-byte groups one sweep of the GELU / residual grid covers
RESIZE_BLOCK_CAP = 16384 * 256
# GELU: 8 values; 300 groups (no multiple of the 256 threads); one sweep and 77 groups
GELU_N = [8, 8 * 300, 8 * (ELEMENTWISE_BLOCK_CAP + 77)]
# residual (M, C): one group; 37 * 65 groups; one sweep and 1451 groups
RESIDUAL_MC = [(1, 8), (37, 520), (2731, 6152)]
assert 2731 * (6152 // 8) > ELEMENTWISE_BLOCK_CAP


def bf16_grid(lim=12.0):
    """every bf16 value in [-lim, lim], padded with zeros to a multiple of 8"""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    v = bits.view(bf16)
    v = v[torch.isfinite(v.float()) & (v.float().abs() <= lim)]
    return torch.cat([v, torch.zeros(-v.numel() % 8, dtype=bf16)])


def gelu_input(n):
    g = torch.Generator().manual_seed(n)
    return (torch.randn(n, generator=g) * 3).to(bf16)


def residual_input(M, C):
    g = torch.Generator().manual_seed(M + C)
    return torch.randn(M, C, generator=g).to(bf16), torch.randn(M, C, generator=g).to(bf16), torch.randn(C, generator=g)


# (B, h, w, Ho, Wo, C)
RESIZE_SHAPES = [(2, 7, 10, 14, 20, 32), (2, 37, 37, 74, 74, 64), (2, 5, 9, 13, 4, 16), (2, 1, 1, 3, 3, 8),
                 (2, 148, 148, 518, 518, 16),                                   # the model's own last resize
                 (2, 1, 9, 4, 30, 8), (2, 6, 1, 11, 1, 8), (2, 9, 9, 1, 1, 8),  # h = 1; w = Wo = 1; Ho = Wo = 1
                 (2, 8, 8, 8, 8, 8),                                            # identity
                 (2, 20, 30, 7, 11, 8)]                                         # down-scaling
RESIZE_PAST_CAP = (2, 33, 29, 1031, 1021, 16)
assert 2 * 1031 * 1021 * (16 // 8) > RESIZE_BLOCK_CAP


def resize_input(B, h, w, C):
    g = torch.Generator().manual_seed(h * w + C)
    return torch.randn(B, h, w, C, generator=g).to(bf16)
