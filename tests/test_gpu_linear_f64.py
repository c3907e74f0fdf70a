"""The linear-layer GEMM family (cr_linear_fwd / cr_linear_bwd_data / cr_linear_bwd_weight: a linear layer over R rows is a
1x1 convolution over a (1, 1, R, K) map) against float64 at the edges of its dispatch, element-wise (tests/f64_bound.py),
and the kernels around it (cr_fc_weight_prepare, cr_fc_grad_accum, cr_transpose2d, cr_colsum_accum, cr_multi_seg through
linear_cat) bit-exactly where they only move or round values.

Every row of the tables names the branch of csrc/conv.hip it was derived for (launch_igemm_ks / try_launch_dma for forward
and backward-data with M = R, Cin = K, Cout = O -- backward-data runs the same code with K and O exchanged, so its cases
are the forward rows read as (R, O, K); plan_wgrad_f32 / launch_wgrad_ks / try_launch_wgrad_s3 for the weight gradient).
Inputs are seeded: randn activations, weights scaled by K^-0.5.  Cases of up to 2^24 multiply-adds take their float64
reference on the CPU, larger ones from torch's float64 matmul on the device (which shares nothing with these kernels).

A kernel trace of this module shows every instantiation those functions can choose for a 1x1 layer: k_conv_igemm at the
six f32 tiles (128x128, 64x64, 128x32, 64x32, 128x16, 64x16) and the six bf16 shapes (64x64 KG 4, 64x64 KU 4, 128x128,
128x64, 128x32, 128x16; forward with bf16 and with float32 output) in both modes, k_conv_igemm_dma at bn 64 / 128 with
one and two wave groups, its 64-row form, bf16, and k_conv_igemm_dma_s3 at both widths, in both modes,
k_splitk_epilogue<float>, k_conv_wgrad_f32 at 16 / 32 / 64 / 128, k_conv_wgrad at 16 / 32 / 64 / 128 and with 2 and 4 wave
groups, k_conv_wgrad_s3 at 64 / 128.  Not reachable from a linear layer: everything with KS = 3 or 7 (the patch kernels,
k_conv_wgrad_s3_row, the parity classes of a stride-2 backward-data) and bf16 backward-data with a float32 output (the
wrapper never asks for it).

Bounds: fp32 f64_bound.check as it is; bf16 operands are rounded first, then check for float32 outputs and
check_bf16_out for bf16-stored ones; fp32x3 may reach max(C, 2 x the worst ratio of the fp32 route on the same inputs),
the margin tests/test_gpu_convops_x3.py gives that mode.  Every check prints a "RATIO" line (run with -s to collect)."""
import contextlib
import importlib
import zlib

import pytest
import torch

import f64_bound as B

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dod_amd.hipops")
_lib = importlib.import_module("3dod_amd._lib")
DEV = torch.device("cuda:0")
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
CPU_REF_MACS = 1 << 24


@contextlib.contextmanager
def _prec(name):
    prev = ops.set_precision(name)
    try:
        yield
    finally:
        ops.set_precision(prev)


def _note(what, case, r, extra=""):
    print(f"RATIO {what} {case}: {r['ratio']:.3f}{extra}")
    return r


def _inputs(R, K, O, bf=False):
    """x (R,K), w (O,K), b (O), dy (R,O) as float32 values on the device the reference is computed on; bf: already
    rounded to bfloat16 (so that casting them is exact and the reference sees the kernels' operands)"""
    dev = DEV if R * K * O > CPU_REF_MACS else torch.device("cpu")
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(repr((R, K, O)).encode()))
    x = torch.randn(R, K, device=dev, generator=g)
    w = torch.randn(O, K, device=dev, generator=g) * K ** -0.5
    b = torch.randn(O, device=dev, generator=g) * 0.1
    dy = torch.randn(R, O, device=dev, generator=g)
    if bf:
        x, w, dy = (t.to(bf16).float() for t in (x, w, dy))
    return x, w, b, dy


def _weights(w, dt):
    """(wp (O,K), wt (K,O)) compute copies of a float32 master weight, made as ops.linear makes them"""
    return ops.prepared_fc_weight(w.to(DEV), None, dt, need_transposed=True)


# ---------------------------------------------------------------------------------------------------------------------
# forward and backward-data
# ---------------------------------------------------------------------------------------------------------------------
FWD_F32 = [  # (R, K, O): M = R, Cin = Kdim = K, Cout = O.  K % 32 != 0 keeps a row off the LDS-DMA kernels.
    ("64x16 tile, one row", (1, 16, 48)),                   # O % 32 != 0, cdiv(M,128) * O/16 = 3 < 512
    ("64x16 tile, row tail", (65, 16, 48)),
    ("128x16 tile", (21900, 16, 48)),                       # 172 * 3 = 516 >= 512
    ("64x32 tile", (130, 48, 96)),                          # O % 32 == 0, 2 * 3 < 512
    ("128x32 tile", (21900, 16, 96)),                       # 172 * 3 >= 512
    ("64x64 tile", (1024, 48, 768)),                        # b128 = 48 < 256, b64 = 16 * 12 = 192 >= 192
    ("128x128 tile", (2048, 48, 2048)),                     # b128 = 16 * 16 = 256
    ("DMA bn 64, one wave group", (2000, 64, 1024)),        # big_tiles = 128 (< 512: bn 64), grid 256 but K/32 = 2 < 4
    ("DMA bn 64, two wave groups", (2048, 128, 1024)),      # grid 256 <= 256 and K/32 = 4
    ("DMA bn 128", (4096, 64, 2048)),                       # big_tiles = 512
    ("DMA, Cout % 128 != 0", (16384, 32, 192)),             # big_tiles = 128 * 1, bn 64, grid 384
    ("split-K, 64-row tiles, 16 splits of 4 stages", (128, 2048, 128)),     # bn2 128, M >= 128: bm 64, 2 tiles
    ("split-K, row tail inside a 64-row tile", (200, 4096, 256)),           # 4 x 2 tiles, 16 splits of 8 stages
    ("split-K, 128-row tiles, bn2 64, 65 stages over 13 splits", (50, 2080, 64)),
    ("split-K, 128-row tiles, bn2 128 (M < 128), two wave groups", (50, 2048, 128)),
    ("unsplit 64x128 tiles (S < 2)", (2048, 2048, 1024)),   # 32 * 8 = 256 half-height tiles: S = 1
    # long_k (K >= 8192, >= 128 big tiles): test_gpu_convops_f32.py::test_linear_head_fc1_full_size
]
FWD_BF16 = [  # out_f32 keeps a row off the DMA kernels, as does K % 64 != 0
    ("64x64 KG 4", (100, 512, 64)),                         # 2 blocks <= 320, K >= 512
    ("64x64 KG 4, 8 blocks", (512, 1024, 64)),
    ("64x64 KU 4", (100, 80, 64)),                          # K < 512
    ("128x128 tile", (4096, 80, 2048)),                     # big_tiles = 512
    ("128x64 tile", (65500, 16, 192)),                      # big_tiles = 512 * 1, O % 128 != 0
    ("128x32 tile", (130, 16, 96)),
    ("128x16 tile", (1, 16, 48)),
    ("DMA bn 64", (2048, 64, 1024)),                        # big_tiles = 128
    ("DMA bn 128", (4096, 64, 2048)),                       # big_tiles = 512
    ("ViT qkv, 64x64 KU 4", (394, 384, 1152)),              # two images of 197 tokens; K = 384 < 512
    ("ViT proj, 64x64 KU 4", (394, 384, 384)),
    ("ViT fc1, 64x64 KU 4", (394, 384, 1536)),
    ("ViT fc2, 64x64 KG 4", (394, 1536, 384)),              # 7 * 6 blocks, K >= 512
]
# fp32x3: the rows whose K % 32 == 0 reach try_launch_dma with the split weights (k_conv_igemm_dma_s3, bm 128 always)
FWD_X3 = [c for c in FWD_F32 if c[1][1] % 32 == 0]
X3_FP32_ROUTE = (130, 48, 96)                               # K % 32 != 0: no split weights, the fp32 kernels' bits


def _fwd(x, w, b, dt, relu, out_f32=False):
    wp, _ = _weights(w, dt)
    return ops.linear_fwd_raw(x.to(DEV, dt), wp, None if b is None else b.to(DEV), out_f32=out_f32, relu=relu)


def _bwd_data(dy, w, dt):
    _, wt = _weights(w, dt)
    return ops.linear_bwd_data_raw(dy.to(DEV, dt), wt)


def _fwd_refs(x, w, b):
    base, absbase, k = B.linear_fwd(x, w, None)
    return (base, absbase, k), (torch.relu(base + b.to(f64)), absbase + b.to(f64).abs(), k)


@pytest.mark.parametrize("branch,case", FWD_F32, ids=[str(c[1]) for c in FWD_F32])
def test_forward_f32(branch, case):
    x, w, b, _ = _inputs(*case)
    plain, biased = _fwd_refs(x, w, b)
    with _prec("fp32"):
        y = _fwd(x, w, b, f32, relu=True)
        assert y.dtype == f32 and y.shape == (case[0], case[2])
        _note("fwd fp32 bias+relu", case, B.check(y, *biased, f"{branch} {case}, bias + ReLU"))
        _note("fwd fp32 no bias", case, B.check(_fwd(x, w, None, f32, relu=False), *plain, f"{branch} {case}, no bias"))


@pytest.mark.parametrize("branch,case", FWD_F32, ids=[str(c[1]) for c in FWD_F32])
def test_backward_data_f32(branch, case):
    R, O, K = case                                          # the forward row read as (R, O, K)
    _, w, _, dy = _inputs(R, K, O)
    with _prec("fp32"):
        dx = _bwd_data(dy, w, f32)
    assert dx.dtype == f32 and dx.shape == (R, K)
    _note("dx fp32", (R, K, O), B.check(dx, *B.linear_bwd_data(dy, w), f"backward-data, {branch}, (R,K,O) = {(R, K, O)}"))


@pytest.mark.parametrize("branch,case", FWD_BF16, ids=[str(c[1]) for c in FWD_BF16])
def test_forward_bf16(branch, case):
    x, w, b, _ = _inputs(*case, bf=True)
    plain, biased = _fwd_refs(x, w, b)
    y = _fwd(x, w, b, bf16, relu=True)
    assert y.dtype == bf16
    _note("fwd bf16 bias+relu", case, B.check_bf16_out(y, *biased, f"{branch} {case}, bias + ReLU"))
    _note("fwd bf16 no bias", case,
          B.check_bf16_out(_fwd(x, w, None, bf16, relu=False), *plain, f"{branch} {case}, no bias"))
    # float32 output (what linear_cat asks for): the non-DMA kernel of the shape, held to the float32 bound
    y = _fwd(x, w, b, bf16, relu=True, out_f32=True)
    assert y.dtype == f32
    _note("fwd bf16 out_f32 bias+relu", case, B.check(y, *biased, f"{branch} {case}, out_f32, bias + ReLU"))
    _note("fwd bf16 out_f32 no bias", case,
          B.check(_fwd(x, w, None, bf16, relu=False, out_f32=True), *plain, f"{branch} {case}, out_f32, no bias"))


@pytest.mark.parametrize("branch,case", FWD_BF16, ids=[str(c[1]) for c in FWD_BF16])
def test_backward_data_bf16(branch, case):
    R, O, K = case
    _, w, _, dy = _inputs(R, K, O, bf=True)
    dx = _bwd_data(dy, w, bf16)
    assert dx.dtype == bf16 and dx.shape == (R, K)
    _note("dx bf16", (R, K, O),
          B.check_bf16_out(dx, *B.linear_bwd_data(dy, w), f"backward-data, {branch}, (R,K,O) = {(R, K, O)}"))


def _x3_check(got3, got32, ref, what, case):
    r32 = B.check(got32, *ref, f"{what} {case}, fp32 route")
    c = max(B.C, 2.0 * r32["ratio"])
    r3 = B.check(got3, *ref, f"{what} {case}, fp32x3 (fp32 route: {r32['ratio']:.3f})", c=c)
    _note(f"{what} fp32x3", case, r3, f" (fp32 route {r32['ratio']:.3f})")


@pytest.mark.parametrize("branch,case", FWD_X3, ids=[str(c[1]) for c in FWD_X3])
def test_forward_x3(branch, case):
    x, w, b, _ = _inputs(*case)
    plain, biased = _fwd_refs(x, w, b)
    with _prec("fp32"):
        y32, p32 = _fwd(x, w, b, f32, relu=True), _fwd(x, w, None, f32, relu=False)
    with _prec("fp32x3"):
        y3, p3 = _fwd(x, w, b, f32, relu=True), _fwd(x, w, None, f32, relu=False)
    _x3_check(y3, y32, biased, "fwd bias+relu", case)
    _x3_check(p3, p32, plain, "fwd no bias", case)


@pytest.mark.parametrize("branch,case", FWD_X3, ids=[str(c[1]) for c in FWD_X3])
def test_backward_data_x3(branch, case):
    R, O, K = case
    _, w, _, dy = _inputs(R, K, O)
    with _prec("fp32"):
        d32 = _bwd_data(dy, w, f32)
    with _prec("fp32x3"):
        d3 = _bwd_data(dy, w, f32)
    _x3_check(d3, d32, B.linear_bwd_data(dy, w), "dx", (R, K, O))


def test_x3_without_split_weights_is_fp32_bit_for_bit():
    """a contraction length that is no multiple of 32 has no split weights: forward and backward-data run the fp32 kernels"""
    R, K, O = X3_FP32_ROUTE
    x, w, b, dy = _inputs(R, K, O)
    _, w2, _, dy2 = _inputs(R, O, K)                        # backward-data contracts over O: (R, O, K) puts 48 there
    with _prec("fp32"):
        y32, d32 = _fwd(x, w, b, f32, relu=True), _bwd_data(dy2, w2, f32)
    with _prec("fp32x3"):
        y3, d3 = _fwd(x, w, b, f32, relu=True), _bwd_data(dy2, w2, f32)
    assert torch.equal(y3, y32) and torch.equal(d3, d32)
    B.check(y3, *_fwd_refs(x, w, b)[1], "fp32x3 forward on the fp32 route")


# ---------------------------------------------------------------------------------------------------------------------
# weight and bias gradient
# ---------------------------------------------------------------------------------------------------------------------
WGRAD = [  # mode, branch, (R, K, O): M = R, Kdim = K, Cout = O; f32 pixel steps are 16 rows, bf16 / fp32x3 steps 32
    ("fp32", "TM 16", (1, 16, 16)),
    ("fp32", "TM 32, second channel tile half empty", (17, 144, 48)),
    ("fp32", "TM 64, ragged channel tile", (50, 1200, 80)),
    ("fp32", "TM 128, two splits of 10 and 7 steps", (272, 16, 144)),
    ("fp32", "Cout >= 1024: 64-row tiles", (2048, 128, 1024)),
    ("fp32", "TM 128", (300, 272, 384)),
    ("fp32", "more than 768 tiles: two splits", (512, 6272, 1024)),             # 16 x 49 = 784 tiles, 32 steps
    ("bf16", "TM 16, one row", (1, 16, 16)),
    ("bf16", "TM 32, one row past a 32-pixel step", (33, 144, 48)),
    ("bf16", "TM 64, ragged channel tile, one wave group", (200, 144, 80)),
    ("bf16", "kg 4", (1024, 256, 64)),                                          # O * K = 16384 <= 160 K
    ("bf16", "kg 2", (1024, 2048, 128)),
    ("bf16", "kg 1, TM 128", (1000, 2048, 128)),                                # M < 1024
    ("fp32x3", "s3 kernel, TM 64", (512, 64, 64)),
    ("fp32x3", "s3 kernel, TM 128, splits of 10 and 7 steps, ragged channel tile", (544, 64, 192)),
    ("fp32x3", "below the s3 threshold: the fp32 route", (500, 64, 64)),
]


def _wgrad(dy, x, dt, with_bias, accumulate):
    R, O = dy.shape
    K = x.shape[1]
    # accumulate: onto ones; otherwise the kernel has to overwrite dw (NaN-filled) -- dbias is always added to what is there
    dw = torch.ones(O, K, device=DEV) if accumulate else torch.full((O, K), float("nan"), device=DEV)
    db = (torch.ones(O, device=DEV) if accumulate else torch.zeros(O, device=DEV)) if with_bias else None
    ops.linear_bwd_weight_raw(dy.to(DEV, dt), x.to(DEV, dt), dw, db, accumulate)
    return dw, db


@pytest.mark.parametrize("mode,branch,case", WGRAD, ids=[f"{c[0]}-{c[2]}" for c in WGRAD])
def test_weight_and_bias_gradient(mode, branch, case):
    R, K, O = case
    dt = bf16 if mode == "bf16" else f32
    x, _, _, dy = _inputs(R, K, O, bf=dt == bf16)
    wref, wabs, k = B.linear_bwd_weight(dy, x)
    bref, babs, _ = B.linear_bias_grad(dy)
    for with_bias in (True, False):
        for accumulate in (False, True):
            # accumulating onto ones adds one term of magnitude 1 to every sum
            one = 1.0 if accumulate else 0.0
            refs = ((wref + one, wabs + one, k + int(one)), (bref + one, babs + one, k + int(one)))
            what = f"{mode} {branch} {case}, dbias {with_bias}, accumulate {accumulate}"
            tag = f"{'acc' if accumulate else 'set'}{'+db' if with_bias else ''}"
            with _prec(mode):
                dw, db = _wgrad(dy, x, dt, with_bias, accumulate)
            if mode == "fp32x3":
                with _prec("fp32"):
                    dw32, db32 = _wgrad(dy, x, dt, with_bias, accumulate)
                _x3_check(dw, dw32, refs[0], f"dw {tag}", case)
                if with_bias:
                    _x3_check(db, db32, refs[1], f"db {tag}", case)
                continue
            _note(f"dw {mode} {tag}", case, B.check(dw, *refs[0], "dW, " + what))
            if with_bias:
                _note(f"db {mode} {tag}", case, B.check(db, *refs[1], "dbias, " + what))


# ---------------------------------------------------------------------------------------------------------------------
# edges of the wrappers, and the ReLU path of ops.linear through autograd
# ---------------------------------------------------------------------------------------------------------------------
def test_wrapper_edges():
    w = torch.randn(48, 32, device=DEV)
    y = ops.linear_fwd_raw(torch.empty(0, 32, device=DEV), w, None)
    assert y.shape == (0, 48) and y.dtype == f32
    dx = ops.linear_bwd_data_raw(torch.empty(0, 48, device=DEV), w.t().contiguous())
    assert dx.shape == (0, 32)
    x = torch.randn(8, 32, device=DEV)
    with pytest.raises(_lib.CrError, match="multiples of 16"):
        ops.linear_fwd_raw(x, torch.randn(40, 32, device=DEV), None)                    # O % 16
    with pytest.raises(_lib.CrError, match="multiples of 16"):
        ops.linear_fwd_raw(torch.randn(8, 40, device=DEV), torch.randn(48, 40, device=DEV), None)     # K % 16
    with pytest.raises(_lib.CrError, match="multiple of 16"):
        ops.linear_bwd_data_raw(torch.randn(8, 48, device=DEV), torch.randn(40, 48, device=DEV))      # K % 16
    with pytest.raises(_lib.CrError, match="multiple of 16"):
        ops.linear_bwd_weight_raw(torch.randn(8, 40, device=DEV), x, torch.zeros(40, 32, device=DEV), None, False)   # O % 16
    with pytest.raises(_lib.CrError, match="bad row count"):
        ops.linear_bwd_weight_raw(torch.empty(0, 48, device=DEV), torch.empty(0, 32, device=DEV),
                                  torch.zeros(48, 32, device=DEV), None, False)


@pytest.mark.parametrize("mode,chw", [("fp32", (32, 7, 7)), ("fp32", None), ("bf16", (16, 3, 5)), ("bf16", None)],
                         ids=["fp32-chw", "fp32", "bf16-chw", "bf16"])
def test_linear_relu_autograd(mode, chw):
    """ops.linear(relu=True): the mask is right wherever float64 can tell, and the gradients are those of float64 under
    the kernel's own mask (so a pre-activation of ~0 that lands on either side is not compared).  With chw the weight
    is in the checkpoint's (c,h,w) column order and x in (h,w,c) order."""
    dt = bf16 if mode == "bf16" else f32
    R, O = 50, 48
    K = 96 if chw is None else chw[0] * chw[1] * chw[2]
    x, w, b, dy = _inputs(R, K, O, bf=dt == bf16)
    perm = (lambda t: t) if chw is None else (lambda t: t.view(O, chw[0], -1).permute(0, 2, 1).reshape(O, K))
    unperm = (lambda t: t) if chw is None else (lambda t: t.view(O, -1, chw[0]).permute(0, 2, 1).reshape(O, K))
    wp = perm(w)                                            # the operand the GEMM sees, columns in x's order
    xd = x.to(DEV, dt).requires_grad_()
    wd, bd = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    with _prec("fp32"):
        y = ops.linear(xd, wd, bd, chw=chw, relu=True)
        y.backward(dy.to(DEV, dt))
    pre, absref, k = B.linear_fwd(x, wp, b)
    bound = B.C * B.U * k ** 0.5 * absref + B.TINY          # of the float32 accumulator: a bf16 store keeps its sign
    yc = y.detach().cpu().double()
    assert bool((yc[pre > bound] > 0).all()) and bool((yc[pre < -bound] == 0).all()) and bool((yc >= 0).all())
    chk = B.check_bf16_out if dt == bf16 else B.check
    _note(f"linear relu y {mode}", (R, K, O), chk(y, torch.relu(pre), absref, k, "y"))
    g = dy * (yc > 0).to(dy.dtype)                          # dy under the kernel's mask (exact in either precision)
    _note(f"linear relu dx {mode}", (R, K, O), chk(xd.grad, *B.linear_bwd_data(g, wp), "dx"))
    dwref, dwabs, kr = B.linear_bwd_weight(g, x)
    _note(f"linear relu dw {mode}", (R, K, O), B.check(wd.grad, unperm(dwref), unperm(dwabs), kr, "dw"))
    _note(f"linear relu db {mode}", (R, K, O), B.check(bd.grad, *B.linear_bias_grad(g), "db"))


# ---------------------------------------------------------------------------------------------------------------------
# the kernels around the GEMMs
# ---------------------------------------------------------------------------------------------------------------------
FC_HW_MAX = 255         # 64 channels x (HW + 1) floats = the 64 KB of dynamic LDS a launch gets without an attribute
_TIES = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(2.0 + 3 * 2.0 ** -7), 65280.0 + 128.0]


@pytest.mark.parametrize("dt", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("HW", [1, 2, 49, 196, FC_HW_MAX])
def test_fc_weight_prepare_and_grad_accum(HW, dt):
    """(O, C, HW) -> (O, HW, C) with the cast, and its transpose accumulated in float32: bit-exact, ties included"""
    g = torch.Generator().manual_seed(100 + HW)
    for O in (1, 5):
        for C in (3, 64, 65, 80):
            K = C * HW
            w = torch.randn(O, K, generator=g)
            w.view(-1)[:min(len(_TIES), K)] = torch.tensor(_TIES)[:K]               # exactly between two bf16 values
            w.view(-1)[-1] = _TIES[0]
            wd = w.to(DEV)
            wp = ops.prepared_fc_weight(wd, (C, HW, 1), dt)
            want = w.view(O, C, HW).permute(0, 2, 1).reshape(O, K).to(dt)
            assert wp.dtype == dt and torch.equal(wp.cpu(), want), (O, C, HW)
            grad = torch.randn(O, HW, C, generator=g).to(dt)
            acc = torch.randn(O, C, HW, generator=g)
            accd = acc.to(DEV)
            _lib.call("cr_fc_grad_accum", grad.to(DEV), accd, O, C, HW, int(dt == f32))
            assert torch.equal(accd.cpu(), acc + grad.float().permute(0, 2, 1)), (O, C, HW)


def test_fc_hw_limit_is_checked_on_the_host():
    O, C, HW = 1, 3, FC_HW_MAX + 1
    w, out = torch.zeros(O, C * HW, device=DEV), torch.zeros(O, C * HW, device=DEV)
    for is_f32 in (0, 1):
        with pytest.raises(_lib.CrError, match="HW in 1..255"):
            _lib.call("cr_fc_weight_prepare", w, out, O, C, HW, is_f32)
        with pytest.raises(_lib.CrError, match="HW in 1..255"):
            _lib.call("cr_fc_grad_accum", w, out, O, C, HW, is_f32)
    with pytest.raises(_lib.CrError, match="HW in 1..255"):
        ops.prepared_fc_weight(torch.zeros(16, 16 * 256, device=DEV), (16, 16, 16), bf16)


@pytest.mark.parametrize("dt", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (33, 47), (32, 64), (1000, 16)])
def test_transpose2d(rows, cols, dt):
    g = torch.Generator().manual_seed(rows * 131 + cols)
    src = torch.randn(rows, cols, generator=g).to(dt)
    dst = torch.empty(cols, rows, dtype=dt, device=DEV)
    _lib.call("cr_transpose2d", src.to(DEV), dst, rows, cols, int(dt == f32))
    assert torch.equal(dst.cpu(), src.t().contiguous())


@pytest.mark.parametrize("dt", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R", [1, 7, 8, 9, 8193])
@pytest.mark.parametrize("O", [16, 272])
def test_colsum_accum(O, R, dt):
    g = torch.Generator().manual_seed(R * 977 + O)
    dy = torch.randn(R, O, generator=g).to(dt)
    sink0 = torch.randn(O, generator=g)
    sink = sink0.to(DEV)
    _lib.call("cr_colsum_accum", dy.to(DEV), int(dt == f32), R, O, torch.empty(1024, O, device=DEV), sink)
    ref, absref, k = B.linear_bias_grad(dy.float())
    _note("colsum", (R, O, str(dt)), B.check(sink, ref + sink0.double(), absref + sink0.double().abs(), k + 1, "bias sink"))
    # ... and as ops.linear reaches it: the bias wants a gradient, the weight does not
    x = torch.randn(R, 32, generator=g).to(dt).to(DEV)
    b = torch.zeros(O, device=DEV, requires_grad=True)
    b._cr_grad = sink0.to(DEV)
    ops.linear(x, torch.randn(O, 32, device=DEV), b).backward(dy.to(DEV))
    assert b.grad is None
    B.check(b._cr_grad, ref + sink0.double(), absref + sink0.double().abs(), k + 1, "bias sink through ops.linear")


@pytest.mark.parametrize("dt", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("sinks", [False, True], ids=["returned", "sinks"])
@pytest.mark.parametrize("widths", [(1, 51, 200, 4), (1, 51, 200)], ids=["256", "252-padded"])
def test_linear_cat(widths, sinks, dt):
    """stacked predictors on K = 128: (1, 51, 200, 4) fills 256 columns exactly, (1, 51, 200) leaves four padded ones"""
    R, K = 70, 128
    g = torch.Generator().manual_seed(sum(widths) + 2 * sinks)
    q = (lambda t: t.to(bf16).float()) if dt == bf16 else (lambda t: t)
    x = q(torch.randn(R, K, generator=g))
    ws = [q(torch.randn(o, K, generator=g) * K ** -0.5) for o in widths]
    bs = [torch.randn(o, generator=g) * 0.1 for o in widths]
    Op = (sum(widths) + 15) // 16 * 16
    ops.bump_weight_epoch()             # plans are keyed by parameter addresses: an earlier test's tensors may have had these
    dy = q(torch.randn(R, Op, generator=g))
    xd = x.to(DEV, dt).requires_grad_()
    wd, bd = [w.to(DEV).requires_grad_() for w in ws], [b.to(DEV).requires_grad_() for b in bs]
    if sinks:
        for t in wd + bd:
            t._cr_grad = torch.ones_like(t)
    with _prec("fp32"):
        y, offs = ops.linear_cat(xd, wd, bd)
        assert y.shape == (R, Op) and y.dtype == f32 and offs[-1] == sum(widths)
        y.backward(dy.to(DEV))
    plan = ops._cat_plan(wd, bd)
    assert plan.sinks == sinks
    if Op > offs[-1]:
        assert float(y.detach()[:, offs[-1]:].abs().max()) == 0.0
    dx_ref = [torch.zeros(R, K, dtype=f64), torch.zeros(R, K, dtype=f64)]
    for i, (w, b) in enumerate(zip(ws, bs)):
        sl = slice(offs[i], offs[i + 1])
        B.check(y[:, sl], *B.linear_fwd(x, w, b), f"predictor {i}")
        dw_ref, db_ref = B.linear_bwd_weight(dy[:, sl], x), B.linear_bias_grad(dy[:, sl])
        B.check(plan.dW[sl], *dw_ref, f"dW {i}")
        B.check(plan.db[sl], *db_ref, f"db {i}")
        if sinks:
            assert wd[i].grad is None and bd[i].grad is None
            assert torch.equal(wd[i]._cr_grad, 1.0 + plan.dW[sl]) and torch.equal(bd[i]._cr_grad, 1.0 + plan.db[sl])
        else:
            assert torch.equal(wd[i].grad, plan.dW[sl]) and torch.equal(bd[i].grad, plan.db[sl])
        r, a, _ = B.linear_bwd_data(dy[:, sl], w)
        dx_ref[0] += r
        dx_ref[1] += a
    chk = B.check_bf16_out if dt == bf16 else B.check
    chk(xd.grad, dx_ref[0], dx_ref[1], Op, "dx")
    # an in-place weight change is seen after bump_weight_epoch()
    with torch.no_grad():
        wd[1].mul_(-2.0)
        bd[1].add_(1.0)
    ops.bump_weight_epoch()
    with _prec("fp32"):
        y2, _ = ops.linear_cat(xd.detach(), wd, bd)
    B.check(y2[:, offs[1]:offs[2]], *B.linear_fwd(x, -2.0 * ws[1], bs[1] + 1.0), "predictor 1 after the update")
    B.check(y2[:, offs[0]:offs[1]], *B.linear_fwd(x, ws[0], bs[0]), "predictor 0 after the update")
