"""Element-wise float64 error bound for the float32 contractions of the conv stack (a plain test module, not a conftest).

A float32 contraction of length K, summed in any order with one rounding per fused multiply-add, is off from the exact
result by about u * sqrt(K) times the size of the terms it adds (u = 2^-24, random rounding errors of unit roundoff u
add up like a random walk).  The size of the terms at an output element is absref = the same contraction over |x| and
|w|, so every element must satisfy

    |got - ref| <= C * u * sqrt(K) * absref + TINY

with ref and absref computed in float64 by ATen.  K is taps * Cin for the forward pass, taps * Cout for the backward-data
pass and N * Ho * Wo for the weight (and bias) gradient; for a linear layer over R rows that is K, O and R.  The bound is
local: an error confined to one tile, one channel or one split of a reduce shows at the element where it happens instead
of averaging into a norm over the whole tensor, and so does an operand that lost a few bits (tests/test_f64_bound.py shows
all three failing it).  `linear_*` are the same three directions of a linear layer, and `check_bf16_out` is the bound for
bfloat16 operands with a bfloat16-stored result.

Winograd F(2x2, 3x3) adds transforms around its contraction, and the products it sums are of transformed operands whose
magnitudes exceed those of the direct form; `wino_fwd` / `wino_wgrad` with absval=True give the matching absref (see
wino_fwd's docstring for the derivation).  Tensors here are NCHW; the tests convert from the kernels' NHWC."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24          # float32 unit roundoff
C = 4.0                 # the one constant of the bound: |got - ref| <= C * U * sqrt(K) * absref + TINY
TINY = 1e-35            # absref == 0 only where every product is 0: the kernel must then return 0 (up to a denormal)
f64 = torch.float64


def check(got, ref, absref, K, what, c=C):
    """element-wise bound on got against float64 (ref, absref) of a contraction of length K.  Returns a dict with the
    largest observed ratio |got - ref| / (U * sqrt(K) * absref) ("ratio", must stay <= c), the normwise error
    ||got - ref|| / ||ref|| ("norm") and the number of elements over the bound ("bad"); raises AssertionError if bad > 0."""
    r = report(got, ref, absref, K)
    assert r["bad"] == 0, f"{what}: {r['bad']} of {r['n']} elements over the bound; worst ratio {r['ratio']:.3g} > {c} at " \
                          f"index {r['where']} (got {r['got']:.9g}, ref {r['ref']:.9g}, absref {r['absref']:.4g}, K {K}); " \
                          f"normwise {r['norm']:.3g}"
    return r


def report(got, ref, absref, K, c=C):
    got = got.detach().to(ref.device, f64)
    assert got.shape == ref.shape == absref.shape, (tuple(got.shape), tuple(ref.shape), tuple(absref.shape))
    err = (got - ref).abs()
    scale = U * math.sqrt(K) * absref
    bad = err > c * scale + TINY
    ratio = err / (scale + TINY)
    ratio = torch.where(torch.isnan(got), torch.full_like(ratio, float("inf")), ratio)
    bad |= torch.isnan(got)
    i = int(ratio.flatten().argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
    return {"ratio": float(ratio.flatten()[i]), "bad": int(bad.sum()), "n": ref.numel(), "where": idx,
            "got": float(got.flatten()[i]), "ref": float(ref.flatten()[i]), "absref": float(absref.flatten()[i]),
            "norm": float((got - ref).norm() / (ref.norm() + 1e-300)), "K": K}


# ---------------------------------------------------------------------------------------------------------------------
# direct convolution: (ref, absref, K) of the three directions, float64
# ---------------------------------------------------------------------------------------------------------------------
def conv_fwd(x, w, b, stride, pad):
    x, w = x.to(f64), w.to(f64)
    ref = F.conv2d(x, w, None if b is None else b.to(f64), stride, pad)
    absref = F.conv2d(x.abs(), w.abs(), None if b is None else b.to(f64).abs(), stride, pad)
    return ref, absref, w.shape[1] * w.shape[2] * w.shape[3]


def conv_bwd_data(dy, w, in_shape, stride, pad):
    dy, w = dy.to(f64), w.to(f64)
    grad = lambda d, ww: torch.nn.grad.conv2d_input(tuple(in_shape), ww, d, stride, pad)
    return grad(dy, w), grad(dy.abs(), w.abs()), w.shape[0] * w.shape[2] * w.shape[3]


def conv_bwd_weight(dy, x, w_shape, stride, pad):
    dy, x = dy.to(f64), x.to(f64)
    grad = lambda d, xx: torch.nn.grad.conv2d_weight(xx, tuple(w_shape), d, stride, pad)
    return grad(dy, x), grad(dy.abs(), x.abs()), dy.shape[0] * dy.shape[2] * dy.shape[3]


def bias_grad(dy):
    dy = dy.to(f64)
    return dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3)), dy.shape[0] * dy.shape[2] * dy.shape[3]


# ---------------------------------------------------------------------------------------------------------------------
# linear layers (the GEMM family behind cr_linear_*): (ref, absref, K) of the three directions, float64, computed on the
# device of the inputs (the large cases take torch's own float64 matmul on the GPU, which shares nothing with the kernels
# under test).  x (R, K), w (O, K), dy (R, O).
# ---------------------------------------------------------------------------------------------------------------------
def linear_fwd(x, w, b):
    x, w = x.to(f64), w.to(f64)
    ref, absref = x @ w.t(), x.abs() @ w.abs().t()
    if b is not None:
        ref, absref = ref + b.to(f64), absref + b.to(f64).abs()
    return ref, absref, x.shape[1]


def linear_bwd_data(dy, w):
    dy, w = dy.to(f64), w.to(f64)
    return dy @ w, dy.abs() @ w.abs(), w.shape[0]


def linear_bwd_weight(dy, x):
    dy, x = dy.to(f64), x.to(f64)
    return dy.t() @ x, dy.abs().t() @ x.abs(), dy.shape[0]


def linear_bias_grad(dy):
    dy = dy.to(f64)
    return dy.sum(0), dy.abs().sum(0), dy.shape[0]


U_BF16 = 2.0 ** -8      # bfloat16 unit roundoff (8 significand bits, round to nearest even)


def report_bf16_out(got, ref, absref, K, c=C):
    """report() for a result that was accumulated in float32 and then stored as bfloat16; "ratio" is scaled so that the
    bound of check_bf16_out is ratio <= c, like report()'s"""
    got = got.detach().to(ref.device, f64)
    assert got.shape == ref.shape == absref.shape, (tuple(got.shape), tuple(ref.shape), tuple(absref.shape))
    err = (got - ref).abs()
    b1 = U * math.sqrt(K) * absref                                  # the float32 bound at c = 1
    scale = b1 + U_BF16 * (ref.abs() / c + b1)                      # c * scale = B + 2^-8 (|ref| + B) with B = c * b1
    bad = (err > c * scale + TINY * (1 + U_BF16)) | torch.isnan(got)
    ratio = err / (scale + TINY)
    ratio = torch.where(torch.isnan(got), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.flatten().argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
    return {"ratio": float(ratio.flatten()[i]), "bad": int(bad.sum()), "n": ref.numel(), "where": idx,
            "got": float(got.flatten()[i]), "ref": float(ref.flatten()[i]), "absref": float(absref.flatten()[i]),
            "norm": float((got - ref).norm() / (ref.norm() + 1e-300)), "K": K}


def check_bf16_out(got, ref, absref, K, what, c=C):
    """the bound for bfloat16 operands and a bfloat16-stored result.  ref / absref are computed from the operands AFTER
    their rounding to bfloat16.  A product of two bfloat16 values has 16 significand bits and is exact in float32, so the
    float32 accumulator v obeys the float32 bound unchanged: |v - ref| <= B, B = c * U * sqrt(K) * absref + TINY (which
    is what check() asks of an output kept in float32: out_f32, dw, dbias).  Storing v as bfloat16 rounds once more, to
    nearest: |got - v| <= 2^-8 |v| <= 2^-8 (|ref| + B).  Together

        |got - ref| <= B + 2^-8 * (|ref| + B)

    A ReLU between the accumulator and the store commutes with the rounding and does not increase |v - ref| when ref is
    passed through the same ReLU."""
    r = report_bf16_out(got, ref, absref, K, c)
    assert r["bad"] == 0, f"{what}: {r['bad']} of {r['n']} elements over the bf16-output bound; worst ratio {r['ratio']:.3g} > {c} " \
                          f"at index {r['where']} (got {r['got']:.9g}, ref {r['ref']:.9g}, absref {r['absref']:.4g}, K {K}); " \
                          f"normwise {r['norm']:.3g}"
    return r


# ---------------------------------------------------------------------------------------------------------------------
# Winograd F(2x2, 3x3) (stride 1, pad 1, even maps)
# ---------------------------------------------------------------------------------------------------------------------
_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
_G = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]
_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]
WINO_DEPTH = 16         # additions of the three transforms on the path of one product (<= 3 + 2 + 8, rounded up)


def _mats(dtype, device, absval):
    m = [torch.tensor(a, dtype=dtype, device=device) for a in (_BT, _G, _AT)]
    return [t.abs() for t in m] if absval else m


def wino_fwd(x, w, b=None, absval=False, dtype=f64):
    """Y = A^T [ sum_c (G g G^T) .* (B^T d B) ] A per 2x2 output tile, computed in `dtype`; x (N,C,H,W), w (O,C,3,3).

    absval=True: the same pipeline over |x|, |w| and |A|, |B|, |G| -- the Winograd route's absref.  Derivation: every value
    the route rounds is a signed sum; replacing each operand and each transform coefficient by its magnitude turns that
    sum into a bound on the magnitudes of everything that was added on the way to it.  The error of the float32 route at an
    output element is then a random walk of one rounding of unit roundoff u per addition along the paths into that element:
    Cin products of the contraction at each of the 16 transformed positions, plus the additions of the input transform (3),
    the filter transform (2) and the output transform (8).  Every one of those errors is at most u times a partial sum whose
    magnitude is bounded by the absval pipeline's value, so

        |Y - Y_exact| <= C * u * sqrt(Cin + WINO_DEPTH) * |A^T| [ sum_c (|G| |g| |G^T|) .* (|B^T| |d| |B|) ] |A|

    with the same constant C as the direct route.  This absref is larger than the direct route's (the transforms mix up to
    16 input and 9 filter values into each product), which is the precision Winograd gives up."""
    BT, G, AT = _mats(dtype, x.device, absval)
    x, w = x.to(dtype), w.to(dtype)
    if absval:
        x, w = x.abs(), w.abs()
    N, Cin, H, W = x.shape
    assert H % 2 == 0 and W % 2 == 0 and w.shape[2:] == (3, 3)
    d = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)            # (N, C, H/2, W/2, 4, 4)
    V = torch.einsum("ia,nctsab,jb->ijtsnc", BT, d, BT)                    # (4, 4, th, tw, N, C)
    Uw = torch.einsum("ia,ocab,jb->ijco", G, w, G)                         # (4, 4, C, O)
    M = torch.matmul(V.reshape(16, -1, Cin), Uw.reshape(16, Cin, -1))      # (16, th*tw*N, O)
    M = M.view(4, 4, H // 2, W // 2, N, -1)
    Y = torch.einsum("ui,ijtsno,vj->notusv", AT, M, AT)                    # (N, O, th, 2, tw, 2)
    Y = Y.reshape(N, -1, H, W)
    if b is not None:
        bb = b.to(dtype)
        Y = Y + (bb.abs() if absval else bb).view(1, -1, 1, 1)
    return Y


def wino_bwd_data(dy, w, absval=False, dtype=f64):
    """dX of a stride-1 pad-1 3x3 convolution through the forward pipeline on the flipped, transposed filter (what the
    route does: dX = conv(dY, rot180(w)^T))"""
    return wino_fwd(dy, w.flip(2, 3).transpose(0, 1), None, absval, dtype)


def wino_wgrad(dy, x, absval=False, dtype=f64):
    """dW = G^T [ sum_tiles (A dY A^T) .* (B^T d B) ] G, computed in `dtype`; absval as for wino_fwd (the contraction runs
    over the tiles, so its length is N * H * W / 4 + WINO_DEPTH)"""
    BT, G, AT = _mats(dtype, x.device, absval)
    x, dy = x.to(dtype), dy.to(dtype)
    if absval:
        x, dy = x.abs(), dy.abs()
    N, Cin, H, W = x.shape
    O = dy.shape[1]
    d = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)            # (N, C, th, tw, 4, 4)
    V = torch.einsum("ia,nctsab,jb->ijntsc", BT, d, BT).reshape(16, -1, Cin)
    t = dy.view(N, O, H // 2, 2, W // 2, 2)
    dM = torch.einsum("ui,notusv,vj->ijntso", AT, t, AT).reshape(16, -1, O)
    dU = torch.matmul(dM.transpose(1, 2), V).view(4, 4, O, Cin)           # (4, 4, O, C)
    return torch.einsum("ia,ijoc,jb->ocab", G, dU, G)


def wino_tiles(dy):
    return dy.shape[0] * (dy.shape[2] // 2) * (dy.shape[3] // 2)
