"""torch.autograd glue over the C-ABI conv / BN / pooling / ROIAlign / NMS / optimizer kernels.

PyTorch is used for device memory, streams and the autograd tape only; every
op below is one or a few calls into libcr3dod.so.  Activations are NHWC
tensors in the ACTIVATION DTYPE of the process; conv weights are float32
(Cout,Cin,k,k) parameters in channels_last memory format (physical
[Cout][k*k][Cin]).  There is no CPU path: a non-CUDA tensor raises CrError.

Precision.  The reference trains and evaluates in float32 (tools/train_net.py:184-330,
no autocast anywhere), so float32 is the default here: activations, activation
gradients and the operands of every contraction are f32 and the convolutions / FC
layers run on the f32 MFMA (v_mfma_f32_16x16x4_f32).  `set_precision("bf16")` (or
CR_PRECISION=bf16 in the environment) selects the fast mode: the same tensors are
bfloat16 and the contractions run on the bf16 MFMA with f32 accumulation.  Every op
takes its mode from the dtype of the tensor it is handed, so both modes can coexist
in one process (the parity tests run them side by side).
"""
import contextlib
import ctypes
import math
import os

import torch

from . import _lib

bf16 = torch.bfloat16
f32 = torch.float32
STAT_REPL = 32

# name -> (activation dtype, act_f32 flag of the C ABI)
_PRECISIONS = {"fp32": (f32, 1), "f32": (f32, 1), "float32": (f32, 1), "fp32x3": (f32, 2), "bf16": (bf16, 0),
               "bfloat16": (bf16, 0)}
_ACT = [_PRECISIONS[os.environ.get("CR_PRECISION", "fp32").lower()]]


def set_precision(name):
    """"fp32" (reference precision on the f32 MFMA, default), "fp32x3" (float32 storage and float32-accurate
    contractions on the bf16 matrix cores: every operand split exactly into three bf16 values, six products per term --
    include/cr3dod.h, act_f32 = 2) or "bf16" (fast mode).  Decides the dtype of the activations produced by preprocess()
    and hence of everything downstream, and which kernels f32 tensors run on.  Returns the previous setting's name."""
    prev = precision()
    _ACT[0] = _PRECISIONS[str(name).lower()]
    return prev


def precision():
    return {0: "bf16", 1: "fp32", 2: "fp32x3"}[_ACT[0][1]]


def act_dtype():
    return _ACT[0][0]


def _af(t):
    """act_f32 flag of the C ABI from a tensor's dtype (f32 tensors: 1, or 2 in the split mode)"""
    if t.dtype == f32:
        return _ACT[0][1] if _ACT[0][0] == f32 else 1
    if t.dtype == bf16:
        return 0
    raise _lib.CrError(f"activations must be float32 or bfloat16, got {t.dtype}")


def _w3(w, af):
    """split-mode companion (cr_weight_split3) of a prepared f32 weight matrix (rows, K), or None.  WeightBank views
    carry theirs (refreshed with the bank); anything else is split on first use per weight epoch and cached on the tensor."""
    if af != 2 or w.dtype != f32:
        return None
    ent = getattr(w, "_cr_w3", None)
    if ent is not None and ent[0] == "bank":
        return ent[1]
    rows = w.shape[0]                      # (rows, K) or a channels_last (Cout,Cin,k,k) weight = physical [Cout][k*k*Cin]
    K = w.numel() // rows
    if K % 32:
        return None
    tag = (_WEIGHT_EPOCH[0], w.data_ptr(), w._version)
    if ent is None or ent[0] != tag:
        out = torch.empty((rows * K * 3,), dtype=bf16, device=w.device)
        _lib.call("cr_weight_split3", w, out, rows, K)
        ent = (tag, out)
        try:
            w._cr_w3 = ent
        except Exception:
            pass
    return ent[1]


def _need_cuda(t, name):
    if not t.is_cuda:
        raise _lib.CrError(f"{name}: expected a CUDA(HIP) tensor; 3dod_amd has no CPU path")


# --------------------------------------------------------------------------
# weight preparation (cached per parameter version)
# --------------------------------------------------------------------------
_WEIGHT_EPOCH = [0]


def bump_weight_epoch():
    """call after parameters were updated outside torch's version tracking (cr_sgd_step writes through raw
    pointers): invalidates every cached bf16 weight copy."""
    _WEIGHT_EPOCH[0] += 1


def as_krsc(weight):
    """(Cout,Cin,k,k) f32 parameter whose storage is channels_last = physical [Cout][k*k*Cin]."""
    if weight.dim() != 4:
        raise ValueError("conv weight must be 4-D")
    if not weight.is_contiguous(memory_format=torch.channels_last):
        raise _lib.CrError("conv weight must be channels_last (see cubercnn.modeling.backbone.to_channels_last)")
    return weight


class WeightBank:
    """bf16 compute copies ([Cout][k*k*Cin] and the bwd-data layout [Cin][k*k*Cout]) of ALL registered conv weights,
    refreshed by ONE launch (cr_weights_prepare) the first time any of them is asked for after the weight epoch
    moved (= after an optimizer step).  The weights must be views into one flat f32 buffer (FlatSGD.flat_p).
    Activated by the training step objects; anything that changes weights outside the optimizer must call
    bump_weight_epoch() (the model's load_state_dict hook does)."""

    def __init__(self, params, flat_p, dtype=None, split=None):
        import numpy as np
        dev = flat_p.device
        self.flat_p = flat_p
        self.dtype = dtype = dtype if dtype is not None else act_dtype()
        self.split = split = (dtype == f32 and _ACT[0][1] == 2) if split is None else bool(split and dtype == f32)
        self.mode = "bf16" if dtype == bf16 else ("fp32x3" if split else "fp32")
        descs, tiles, self.shapes = [], [], []
        off = 0
        for i, p in enumerate(params):
            Cout, Cin, k, _ = p.shape
            KK, n = k * k, p.numel()
            src_off = (p.data_ptr() - flat_p.data_ptr()) // 4
            assert 0 <= src_off and src_off + n <= flat_p.numel(), "conv weight is not a view of the flat buffer"
            descs.append((src_off, off, off, Cout, KK, Cin, 1))
            for r in range(KK):
                for o0 in range(0, Cout, 32):
                    for c0 in range(0, Cin, 32):
                        tiles.append((i, r, o0, c0))
            self.shapes.append((off, n, Cout, KK, Cin))
            off += (n + 7) // 8 * 8
        dt = np.dtype([("src", "<i8"), ("dst", "<i8"), ("dstT", "<i8"), ("Cout", "<i4"), ("KK", "<i4"), ("Cin", "<i4"),
                       ("needT", "<i4")])
        assert dt.itemsize == 40
        self.descs = torch.from_numpy(np.array(descs, dtype=dt).view(np.uint8).copy()).to(dev)
        self.tiles = torch.tensor(tiles, dtype=torch.int32, device=dev)
        self.ntiles = len(tiles)
        # f32 mode: the master weights ARE the forward / weight-gradient operand; only the bwd-data layout is a copy
        self.dst = torch.empty((off,), dtype=bf16, device=dev) if dtype == bf16 else None
        self.dstT = torch.empty((off,), dtype=dtype, device=dev)
        if dtype == bf16:
            self.views = [(self.dst[o:o + n].view(Cout, KK * Cin), self.dstT[o:o + n].view(Cin, KK * Cout))
                          for (o, n, Cout, KK, Cin) in self.shapes]
        else:
            self.views = [(p.detach(), self.dstT[o:o + n].view(Cin, KK * Cout))
                          for p, (o, n, Cout, KK, Cin) in zip(params, self.shapes)]
        if split:
            # split-mode planes (6 bytes per element) of every weight whose k extent is a multiple of 32, forward layout
            # from the flat parameter buffer and backward-data layout from dstT, one launch each
            s3 = np.dtype([("src", "<i8"), ("dst", "<i8"), ("item0", "<i8"), ("rows", "<i4"), ("K", "<i4")])
            assert s3.itemsize == 32
            recs = ([], [])
            tot, o3 = [0, 0], 0
            for i, (p, (o, n, Cout, KK, Cin)) in enumerate(zip(params, self.shapes)):
                src_off = (p.data_ptr() - flat_p.data_ptr()) // 4
                for which, (soff, rows, K) in enumerate(((src_off, Cout, KK * Cin), (o, Cin, KK * Cout))):
                    if K % 32 or soff % 4:
                        continue
                    recs[which].append((soff, o3, tot[which], rows, K, i))
                    tot[which] += rows * K // 8
                    o3 += rows * K * 3
            self.w3 = torch.empty((max(o3, 8),), dtype=bf16, device=dev)
            self.s3 = []
            for which in (0, 1):
                arr = np.array([r[:5] for r in recs[which]], dtype=s3) if recs[which] else np.zeros((0,), dtype=s3)
                self.s3.append((torch.from_numpy(arr.view(np.uint8).copy()).to(dev), len(recs[which]), tot[which]))
                for (soff, d3, _, rows, K, i) in recs[which]:
                    self.views[i][which]._cr_w3 = ("bank", self.w3[d3:d3 + rows * K * 3])
        self.epoch = None
        self.params = list(params)
        self.attach()

    def attach(self):
        """make this bank the one the parameters' compute copies come from (FlatSGD keeps one bank per precision mode)"""
        for i, p in enumerate(self.params):
            p._cr_bank = (self, i)

    def get(self, i):
        if self.epoch != _WEIGHT_EPOCH[0]:
            _lib.call("cr_weights_prepare", self.flat_p, self.dst, self.dstT, self.descs, self.tiles, self.ntiles,
                      int(self.dtype == f32))
            if self.split:
                for src, (descs, nd, tot) in zip((self.flat_p, self.dstT), self.s3):
                    _lib.call("cr_weights_split3", src, self.w3, descs, nd, tot)
            self.epoch = _WEIGHT_EPOCH[0]
        return self.views[i]


def prepared_weights(weight, need_transposed, dtype=bf16):
    """compute copies of a f32 channels_last weight in the activation dtype: [Cout][k*k*Cin] and (optionally) the bwd-data
    layout [Cin][k*k*Cout].  In f32 mode the first one is the weight itself.  Weights registered in a WeightBank of the
    same dtype come from the bank (one launch per step for the whole model); others are cached ON the tensor object (so
    a new tensor at a recycled address never hits a stale entry), keyed by torch's version counter and the global
    weight epoch."""
    bk = getattr(weight, "_cr_bank", None)
    if bk is not None and bk[0].dtype == dtype and (dtype == bf16 or bk[0].split or _ACT[0][1] != 2):
        return bk[0].get(bk[1])
    attr = "_cr_wcache" if dtype == bf16 else "_cr_wcache32"
    ent = getattr(weight, attr, None)
    tag = (weight._version, _WEIGHT_EPOCH[0], weight.data_ptr())
    if ent is None or ent[0] != tag:
        Cout, Cin, k, _ = weight.shape
        if dtype == bf16:
            wb = torch.empty((Cout, k * k * Cin), dtype=bf16, device=weight.device)
            _lib.call("cr_cast_f32_to_bf16", weight.detach(), wb, weight.numel())
        else:
            wb = weight.detach()
        ent = [tag, wb, None]
        try:
            setattr(weight, attr, ent)
        except Exception:
            pass
    if need_transposed and ent[2] is None:
        Cout, Cin, k, _ = weight.shape
        wt = torch.empty((Cin, k * k * Cout), dtype=dtype, device=weight.device)
        _lib.call("cr_weight_transpose", weight.detach(), wt, Cout, k, Cin, int(dtype == f32))
        ent[2] = wt
    return ent[1], ent[2]


# --------------------------------------------------------------------------
# raw kernels
# --------------------------------------------------------------------------
def conv_fwd_raw(x, wb, Cout, k, stride, pad, bias=None, residual=None, relu=False, stats=None, out_f32=False):
    _need_cuda(x, "conv input")
    af = _af(x)
    assert x.is_contiguous() and x.dim() == 4 and wb.dtype == x.dtype and (residual is None or residual.dtype == x.dtype)
    N, H, W, Cin = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = torch.empty((N, Ho, Wo, Cout), dtype=f32 if (out_f32 or af) else bf16, device=x.device)
    _lib.call("cr_conv2d_fwd", x, wb, y, N, H, W, Cin, Cout, k, stride, pad, bias, residual, int(relu), stats, int(out_f32), af,
              _w3(wb, af))
    return y


def conv_bwd_data_raw(dy, wt, in_shape, k, stride, pad, accumulate=None):
    """accumulate: a tensor of the result's shape that is added in the kernel's epilogue (see _GradSlot)"""
    N, H, W, Cin = in_shape
    Cout = dy.shape[3]
    assert wt.dtype == dy.dtype
    dx = torch.empty((N, H, W, Cin), dtype=dy.dtype, device=dy.device)
    if accumulate is not None:
        assert tuple(accumulate.shape) == (N, H, W, Cin), "accumulate must have the input's shape"
        accumulate = accumulate.to(dy.dtype).contiguous()
    af = _af(dy)
    _lib.call("cr_conv2d_bwd_data", dy, wt, dx, N, H, W, Cin, Cout, k, stride, pad, af, _w3(wt, af), accumulate)
    return dx


# --------------------------------------------------------------------------
# grouped 3x3 convolution (DLA's BottleneckX, csrc/conv_grouped.hip): pad 1, Cin == Cout, f32 KRSC weights (Cout, 3, 3, cg) in
# every precision mode and in all three directions -- no compute copies, no weight bank, no transposed layout
# --------------------------------------------------------------------------
def _grouped_out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def conv_grouped_fwd_raw(x, w, groups, stride, bias=None, residual=None, relu=False, stats=None):
    _need_cuda(x, "conv input")
    af = _af(x)
    assert x.is_contiguous() and x.dim() == 4 and w.dtype == f32 and (residual is None or residual.dtype == x.dtype)
    N, H, W, C = x.shape
    Ho, Wo = _grouped_out_hw(H, W, stride)
    assert w.numel() == C * 9 * (C // groups) and (residual is None or tuple(residual.shape) == (N, Ho, Wo, C))
    assert stats is None or (stats.dtype == f32 and stats.numel() >= (N * Ho * Wo + 63) // 64 * 2 * C)
    y = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    _lib.call("cr_conv2d_grouped_fwd", x, w, y, N, H, W, C, w.shape[0], groups, 3, stride, 1, bias, residual, int(relu), stats, af)
    return y


def conv_grouped_bwd_data_raw(dy, w, in_shape, groups, stride, accumulate=None):
    """accumulate: as for conv_bwd_data_raw"""
    N, H, W, C = in_shape
    assert w.dtype == f32 and dy.is_contiguous() and w.numel() == C * 9 * (C // groups)
    assert tuple(dy.shape) == (N,) + _grouped_out_hw(H, W, stride) + (C,), "dy does not have the output's shape"
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    if accumulate is not None:
        assert tuple(accumulate.shape) == (N, H, W, C), "accumulate must have the input's shape"
        accumulate = accumulate.to(dy.dtype).contiguous()
    _lib.call("cr_conv2d_grouped_bwd_data", dy, w, dx, N, H, W, C, dy.shape[3], groups, 3, stride, 1, _af(dy), accumulate)
    return dx


def grouped_wgrad_splits(M):
    """pixel ranges of cr_conv2d_grouped_bwd_weight (include/cr3dod.h): its workspace holds splits * (C * 9 * cg + C) floats"""
    rng = max(128, -(-M // 256))
    return -(-M // rng)


def conv_grouped_bwd_weight_raw(dy, x, groups, stride, sink=None, bias_acc=None):
    """dW (Cout, cg, 3, 3) channels_last, or added into `sink` when given; bias_acc: f32 [Cout] that receives += sum_pixels dy.
    Never queued (deferred_wgrad): the launch happens here."""
    N, H, W, C = x.shape
    assert dy.dtype == x.dtype and dy.is_contiguous() and x.is_contiguous()
    assert tuple(dy.shape) == (N,) + _grouped_out_hw(H, W, stride) + (C,), "dy does not have the output's shape"
    cg = C // groups
    M = dy.shape[0] * dy.shape[1] * dy.shape[2]
    n_ws = grouped_wgrad_splits(M) * (C * 9 * cg + C)
    ws = torch.empty((n_ws,), dtype=f32, device=x.device)
    dw = sink if sink is not None else torch.empty((C, cg, 3, 3), dtype=f32, device=x.device).contiguous(
        memory_format=torch.channels_last)
    _lib.call("cr_conv2d_grouped_bwd_weight", dy, x, dw, bias_acc, N, H, W, C, dy.shape[3], groups, 3, stride, 1,
              int(sink is not None), _af(x), ws, n_ws)
    return None if sink is not None else dw


# --------------------------------------------------------------------------
# Fan-in of gradients without add kernels.  An activation consumed by several of the ops below would have its gradient
# contributions summed by autograd with one elementwise add per extra consumer (60 launches per train step).  Instead the
# consumers of a tensor share a _GradSlot: the FIRST consumer registered in the forward pass must be a convolution -- its
# backward runs last (autograd executes in reverse creation order, and where the later consumers feed the first one's
# output, as in a residual block, also by dependency) and adds what the others left in the slot inside its backward-data
# epilogue (`accumulate`).  The other consumers put their contribution into the slot and return None.  The order is
# CHECKED: a contribution arriving after the first consumer's backward ran raises (a registered consumer that receives no
# gradient at all simply never contributes).  Consumers that are plain torch ops do not take part (autograd adds their share
# as before).
# --------------------------------------------------------------------------
class _GradSlot:
    __slots__ = ("n_reg", "n_arr", "buf", "done", "what")

    def __init__(self, what=""):
        self.n_reg, self.n_arr, self.buf, self.done, self.what = 0, 0, None, False, what


_SLOTS_ON = [os.environ.get("CR_GRAD_SLOTS", "1") == "1"]


def _slot_register(x, accumulator):
    """called in the forward pass by a consumer of x; -> (slot, index) or (None, 0).  accumulator: this consumer can add the
    slot's content in its backward (a convolution's backward-data)"""
    if not (_SLOTS_ON[0] and torch.is_grad_enabled() and torch.is_tensor(x) and x.requires_grad):
        return None, 0
    slot = getattr(x, "_cr_slot", None)
    if slot is None:
        if not accumulator:
            return None, 0                    # the first consumer cannot accumulate: everybody returns gradients as usual
        slot = _GradSlot(f"tensor {tuple(x.shape)}")
        try:
            x._cr_slot = slot
        except Exception:
            return None, 0
    slot.n_reg += 1
    return slot, slot.n_reg


def _slot_put(slot, g):
    """a later consumer leaves its gradient contribution (backward pass); the caller returns None for that input"""
    if slot.done:
        raise RuntimeError("gradient slot: a contribution arrived after the accumulating convolution's backward had run "
                           "(set CR_GRAD_SLOTS=0 to fall back to autograd's adds)")
    slot.buf = g if slot.buf is None else slot.buf + g
    slot.n_arr += 1


def _slot_fold(slot):
    """a later consumer whose own kernel can add: takes what the slot holds so far (or None) and will put back the sum, so
    that several contributions to one slot never meet in a torch add"""
    buf, slot.buf = slot.buf, None
    return buf


def _slot_take(slot):
    """the first consumer (a convolution) collects what the others have contributed, in its backward.  A registered
    consumer whose output receives no gradient never contributes (e.g. a pooled level nobody uses): that is a zero, not an
    error; one that contributes AFTER this point raises in _slot_put -- nothing is ever dropped silently."""
    slot.done = True
    buf, slot.buf = slot.buf, None
    return buf


def grad_sink(t):
    """a persistent f32 gradient buffer attached to a parameter by the optimizer (FlatSGD): kernels accumulate
    straight into it (no per-parameter zero-fill / add kernels); the autograd grad for that input is None."""
    return getattr(t, "_cr_grad", None)


# Deferred weight gradients.  Nothing reads a weight gradient before the optimizer (with several GPUs: before the all-reduce of
# its backward segment), so inside deferred_wgrad() the fp32 calls that accumulate into a gradient sink are queued instead of
# launched, and flushed WGRAD_GROUP at a time through cr_conv2d_bwd_weight_multi: several layers share one grid, every block
# covers a longer pixel range and pays its atomics once (csrc/conv.hip).  The queue keeps dy / x alive until they are launched.
WGRAD_GROUP = 8
_WGRAD_DEPTH = [0]
_WGRAD_PENDING = []


def wgrad_pending():
    """number of queued weight gradients (0 outside deferred_wgrad())"""
    return len(_WGRAD_PENDING)


def conv_bwd_weight_multi_raw(items):
    """items: (dy, x, dw, dbias or None, k, stride, pad), fp32 mode; dw / dbias are accumulated into, in queue order"""
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    xs = [it[1] for it in items]
    _lib.call("cr_conv2d_bwd_weight_multi", len(items), cast(_ptr_table([it[0] for it in items])), cast(_ptr_table(xs)),
              cast(_ptr_table([it[2] for it in items])), cast(_ptr_table([it[3] for it in items])),
              cast(_int_table([x.shape[0] for x in xs])), cast(_int_table([x.shape[1] for x in xs])),
              cast(_int_table([x.shape[2] for x in xs])), cast(_int_table([x.shape[3] for x in xs])),
              cast(_int_table([it[0].shape[3] for it in items])), cast(_int_table([it[4] for it in items])),
              cast(_int_table([it[5] for it in items])), cast(_int_table([it[6] for it in items])), 1, device=xs[0].device)


def wgrad_flush():
    """launch what is queued.  The queue is emptied first: a failing launch raises, it never leaves entries behind."""
    if _WGRAD_PENDING:
        items = list(_WGRAD_PENDING)
        del _WGRAD_PENDING[:]
        conv_bwd_weight_multi_raw(items)


@contextlib.contextmanager
def deferred_wgrad():
    """queue the fp32 sink-accumulating weight gradients of the enclosed backward pass (conv_bwd_weight_raw) and launch them
    in groups.  Everything queued is launched before the context is left -- also when an exception passes through: a gradient
    is never dropped.  Re-entrant; an inner exit flushes too."""
    _WGRAD_DEPTH[0] += 1
    try:
        yield
    finally:
        _WGRAD_DEPTH[0] -= 1
        wgrad_flush()


def conv_bwd_weight_raw(dy, x, k, stride, pad, sink=None, bias_acc=None):
    """dW (into `sink` when given).  bias_acc: f32 [Cout] buffer that additionally receives += sum_pixels dy (fused)."""
    N, H, W, Cin = x.shape
    Cout = dy.shape[3]
    af = _af(x)
    assert dy.dtype == x.dtype
    if sink is not None and af == 1 and _WGRAD_DEPTH[0] > 0:
        _WGRAD_PENDING.append((dy, x, sink, bias_acc, k, stride, pad))
        if len(_WGRAD_PENDING) >= WGRAD_GROUP:
            wgrad_flush()
        return None
    if bias_acc is not None:
        dw = sink if sink is not None else torch.empty((Cout, Cin, k, k), dtype=f32, device=x.device).contiguous(
            memory_format=torch.channels_last)
        _lib.call("cr_conv2d_bwd_weight_bias", dy, x, dw, bias_acc, N, H, W, Cin, Cout, k, stride, pad, int(sink is not None),
                  af)
        return None if sink is not None else dw
    if sink is not None:
        _lib.call("cr_conv2d_bwd_weight", dy, x, sink, N, H, W, Cin, Cout, k, stride, pad, 1, af)
        return None
    dw = torch.empty((Cout, Cin, k, k), dtype=f32, device=x.device).contiguous(memory_format=torch.channels_last)
    _lib.call("cr_conv2d_bwd_weight", dy, x, dw, N, H, W, Cin, Cout, k, stride, pad, 0, af)
    return dw


# --------------------------------------------------------------------------
# conv + BatchNorm(train) + residual + ReLU   (dla.py BasicBlock / Root / conv levels)
# --------------------------------------------------------------------------
class _ConvBN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, gamma, beta, residual, running_mean, running_var, stride, pad, relu, eps, momentum,
                training, slots=((None, 0), (None, 0)), groups=1, wide_sums=False):
        ctx.slots = slots
        ctx.groups = groups
        # wide_sums (the MNASNet trunk): every per-channel sum of the backward is added across threads in double -- the
        # BatchNorm backward is cr_bn_bwd_anyc at every width, the frozen backward's bias sum cr_colsum_wide
        ctx.wide_sums = wide_sums
        Cout, Cin, k, _ = weight.shape
        dev = x.device
        af = _af(x)
        if training:
            if groups == 1:
                wb, _ = prepared_weights(weight, x.requires_grad, x.dtype)
            _STATS_EPOCH[0] += 1
            N_, H_, W_, _ = x.shape
            M = N_ * ((H_ + 2 * pad - k) // stride + 1) * ((W_ + 2 * pad - k) // stride + 1)
            nparts = (M + 63) // 64            # statistics rows are per 64 pixels (independent of the tile choice)
            stats = torch.empty((nparts, 2, Cout), dtype=f32, device=dev)
            if groups == 1:
                y_raw = conv_fwd_raw(x, wb, Cout, k, stride, pad, stats=stats)
            else:
                y_raw = conv_grouped_fwd_raw(x, weight.detach(), groups, stride, stats=stats)
            out = torch.empty_like(y_raw)
            mi = torch.empty((2, Cout), dtype=f32, device=dev)
            _lib.call("cr_bn_fwd", y_raw, stats, nparts, gamma.detach(), beta.detach(), residual, out, M, Cout, int(relu),
                      float(eps), float(momentum), mi, running_mean, running_var, af)
        else:
            # frozen statistics with gradients enabled (freeze_bn fine-tuning; plain inference takes conv_bn_folded): the
            # BatchNorm folded into the convolution (cr_fold_bn) and ONE convolution with bias / residual / ReLU in its
            # epilogue.  The fold is made on every call from the live parameters -- inside a graph capture it is a node of
            # the graph -- and never shares the inference fold cache (weight._cr_fold*).  The f32 folded weight is kept for
            # the backward (its transposed copy for backward-data); y_raw is never written.
            K_ = weight.numel() // Cout
            wf32 = torch.empty((Cout, K_), dtype=f32, device=dev)
            bias_f = torch.empty((Cout,), dtype=f32, device=dev)
            _lib.call("cr_fold_bn", weight.detach(), gamma.detach(), beta.detach(), running_mean, running_var, float(eps), wf32,
                      bias_f, Cout, K_, 1)
            if groups > 1:                  # the grouped kernels read f32 weights in every mode
                out = conv_grouped_fwd_raw(x, wf32, groups, stride, bias=bias_f, residual=residual, relu=relu)
            else:
                if x.dtype == bf16:
                    wf = torch.empty((Cout, K_), dtype=bf16, device=dev)
                    _lib.call("cr_cast_f32_to_bf16", wf32, wf, wf32.numel())
                else:
                    wf = wf32
                out = conv_fwd_raw(x, wf, Cout, k, stride, pad, bias=bias_f, residual=residual, relu=relu)
            y_raw, mi = wf32, None
            ctx.frozen = (running_mean, running_var, float(eps))
        ctx.cfg = (k, stride, pad, relu, training, residual is not None)
        ctx.beta_ref = beta
        # a training ReLU layer without a residual: the backward takes the mask from y_raw (cr_bn_bwd_mask), not from out
        keep_out = relu and not (training and residual is None)
        ctx.save_for_backward(x, weight, gamma, y_raw, out if keep_out else None, mi)
        return out

    @staticmethod
    def backward(ctx, dout):
        return _ConvBN._backward_impl(ctx, dout)

    @staticmethod
    def _backward_impl(ctx, dout, want_dx=None, want_dw=None):
        """want_dx / want_dw: overrides of needs_input_grad[0] / [1] (_RootConvBN computes the input gradients itself and then
        gets (dx_raw, dw, dgamma, dbeta) back instead of the argument-ordered tuple)"""
        x, weight, gamma, y_raw, out, mi = ctx.saved_tensors
        k, stride, pad, relu, training, has_res = ctx.cfg
        root = want_dx is not None
        need_dx = ctx.needs_input_grad[0] if want_dx is None else want_dx
        need_dw = ctx.needs_input_grad[1] if want_dw is None else want_dw
        if not training:
            return _ConvBN._frozen_backward(ctx, dout, need_dx, need_dw, root)
        Cout = weight.shape[0]
        dev = x.device
        dout = dout.to(x.dtype).contiguous()
        M = y_raw.numel() // Cout
        anyc = bn_needs_anyc(Cout) or (ctx.wide_sums and not (has_res and relu))
        if not anyc:
            sums = torch.empty((1025, 2, Cout), dtype=f32, device=dev)
            dx_raw = torch.empty_like(y_raw)
            dres = torch.empty_like(y_raw) if has_res else None
        gs, bs = grad_sink(gamma), grad_sink(ctx.beta_ref)
        if gs is not None and bs is not None:
            dgamma, dbeta, ret_g, ret_b = gs, bs, None, None
        else:
            dgamma = torch.zeros((Cout,), dtype=f32, device=dev)
            dbeta = torch.zeros((Cout,), dtype=f32, device=dev)
            ret_g, ret_b = dgamma, dbeta
        if anyc:
            # a width beyond cr_bn_bwd, or wide sums asked for (MNASNet): cr_bn_bwd_anyc has no dres output -- without a ReLU
            # the residual's gradient is dout itself
            if has_res and relu:
                raise _lib.CrError(f"BatchNorm backward over {Cout} channels: residual + ReLU needs 256 % (C / 8) == 0")
            dx_raw = bn_bwd_anyc_raw(dout, None, y_raw, mi, gamma.detach(), ctx.beta_ref.detach(), relu, dgamma, dbeta)
            dres = dout if has_res else None
        elif relu and not has_res:
            _lib.call("cr_bn_bwd_mask", dout, None, y_raw, mi, gamma.detach(), ctx.beta_ref.detach(), sums, dx_raw, None, dgamma,
                      dbeta, M, Cout, 1, _af(x))
        else:
            _lib.call("cr_bn_bwd", dout, out, y_raw, mi, gamma.detach(), sums, dx_raw, dres, dgamma, dbeta, M, Cout, int(relu),
                      _af(x))
        (xslot, xi), (rslot, ri) = ctx.slots
        if rslot is not None and dres is not None:          # the residual's other consumer (a convolution) adds this
            _slot_put(rslot, dres)
            dres = None
        dx = None
        groups = ctx.groups
        if need_dx:
            if groups == 1:
                _, wt = prepared_weights(weight, True, x.dtype)
                bwd_data = lambda acc: conv_bwd_data_raw(dx_raw, wt, x.shape, k, stride, pad, accumulate=acc)
            else:
                bwd_data = lambda acc: conv_grouped_bwd_data_raw(dx_raw, weight.detach(), x.shape, groups, stride, accumulate=acc)
            if xslot is not None and xi > 1:                # not the first consumer of x: leave the contribution in the slot
                _slot_put(xslot, bwd_data(_slot_fold(xslot)))
            else:
                dx = bwd_data(_slot_take(xslot) if xslot is not None else None)
        elif xslot is not None:
            raise RuntimeError("gradient slot registered for an input that needs no gradient")
        if not need_dw:
            dw = None
        elif groups == 1:
            dw = conv_bwd_weight_raw(dx_raw, x, k, stride, pad, grad_sink(weight))
        else:
            dw = conv_grouped_bwd_weight_raw(dx_raw, x, groups, stride, grad_sink(weight))
        if root:
            return dx_raw, dw, ret_g, ret_b
        return dx, dw, ret_g, ret_b, dres, None, None, None, None, None, None, None, None, None, None, None

    @staticmethod
    def _frozen_backward(ctx, dout, need_dx, need_dw, root):
        """backward of the folded forward: g = dout masked by the ReLU (= the residual's gradient), dx = conv_bwd_data(g, wf^T),
        dwf = conv_bwd_weight(g, x) and sum_p g into scratch in one launch, then cr_bn_frozen_unfold maps them to dw, dgamma
        and dbeta (into the parameters' gradient sinks when they have them).  root: _RootConvBN forms the children's
        gradients itself from g and ctx.frozen_wt."""
        x, weight, gamma, wf32, out, _ = ctx.saved_tensors
        k, stride, pad, relu, _, has_res = ctx.cfg
        running_mean, running_var, eps = ctx.frozen
        Cout, Cin = weight.shape[0], weight.shape[1]
        K_ = weight.numel() // Cout
        dev = x.device
        dout = dout.to(x.dtype).contiguous()
        g = relu_bwd(out, dout) if relu else dout
        (xslot, xi), (rslot, ri) = ctx.slots
        dres = g if has_res else None
        if rslot is not None and dres is not None:          # the residual's other consumer (a convolution) adds this
            _slot_put(rslot, dres)
            dres = None
        dx = None
        groups = ctx.groups
        if need_dx or root:
            if groups == 1:
                wt = torch.empty((Cin, k * k * Cout), dtype=x.dtype, device=dev)        # [Cin][k*k][Cout]
                assert wt.numel() == wf32.numel()
                _lib.call("cr_weight_transpose", wf32, wt, Cout, k, Cin, int(x.dtype == f32))
                bwd_data = lambda acc: conv_bwd_data_raw(g, wt, x.shape, k, stride, pad, accumulate=acc)
            else:                                           # the grouped backward-data reads the folded f32 weights as they are
                wt = None
                bwd_data = lambda acc: conv_grouped_bwd_data_raw(g, wf32, x.shape, groups, stride, accumulate=acc)
            if root:
                ctx.frozen_wt = wt
            elif xslot is not None and xi > 1:              # not the first consumer of x: leave the contribution in the slot
                _slot_put(xslot, bwd_data(_slot_fold(xslot)))
            else:
                dx = bwd_data(_slot_take(xslot) if xslot is not None else None)
        elif xslot is not None:
            raise RuntimeError("gradient slot registered for an input that needs no gradient")
        # dgamma needs <dwf, w> even when the weight itself needs no gradient; sum_p g rides on the weight-gradient launch
        sg = torch.zeros((Cout,), dtype=f32, device=dev)
        if ctx.wide_sums and groups == 1:                  # the sum in a pass of its own, added in double
            colsum_wide_raw(g, sg)
            dwf = conv_bwd_weight_raw(g, x, k, stride, pad, None)
        elif groups == 1:
            dwf = conv_bwd_weight_raw(g, x, k, stride, pad, None, bias_acc=sg)
        else:
            dwf = conv_grouped_bwd_weight_raw(g, x, groups, stride, None, bias_acc=sg)
        wsink = grad_sink(weight) if need_dw else None
        dw = None
        if need_dw and wsink is None:
            dw = dwf                                        # scaled in place
        gs, bs = grad_sink(gamma), grad_sink(ctx.beta_ref)
        if gs is not None and bs is not None:
            dgamma, dbeta, ret_g, ret_b = gs, bs, None, None
        else:
            dgamma = torch.zeros((Cout,), dtype=f32, device=dev)
            dbeta = torch.zeros((Cout,), dtype=f32, device=dev)
            ret_g, ret_b = dgamma, dbeta
        dst = wsink if wsink is not None else dw
        assert dwf.numel() == Cout * K_ and (dst is None or dst.numel() == Cout * K_) and dgamma.numel() == Cout == dbeta.numel()
        _lib.call("cr_bn_frozen_unfold", dwf, sg, weight.detach(), gamma.detach(), running_mean, running_var, eps, dst,
                  int(wsink is not None), dgamma, dbeta, Cout, K_)
        if root:
            return g, dw, ret_g, ret_b
        return dx, dw, ret_g, ret_b, dres, None, None, None, None, None, None, None, None, None, None, None


class _RootConvBN(torch.autograd.Function):
    """DLA `Root` (dla.py:156-174): 1x1 convolution + BatchNorm (+ ReLU) over the channel concatenation of its children.
    Forward: the concatenation is made inside (one cat kernel), then exactly _ConvBN.  Backward: the gradient of every child
    is its OWN backward-data GEMM on the matching row slice of the transposed weights (rows = input channels: a slice is
    contiguous) -- no gradient of the concatenation, no narrow / copy per child, and a child that another convolution
    consumed first gets its share through that convolution's gradient slot instead of an autograd add."""

    @staticmethod
    def forward(ctx, weight, gamma, beta, running_mean, running_var, relu, eps, momentum, training, slots, *children):
        with torch.no_grad():
            x = torch.cat(children, 3)
        out = _ConvBN.forward(ctx, x, weight, gamma, beta, None, running_mean, running_var, 1, 0, relu, eps, momentum, training)
        ctx.child_slots = slots
        ctx.child_ch = [c.shape[3] for c in children]
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors[0], ctx.saved_tensors[1]
        nchild = len(ctx.child_ch)
        need = ctx.needs_input_grad
        # BatchNorm backward + weight gradient exactly as _ConvBN, without a gradient for the concatenated input
        ctx.slots = ((None, 0), (None, 0))
        res = _ConvBN._backward_impl(ctx, dout, want_dx=False, want_dw=need[0])
        dx_raw, dw, ret_g, ret_b = res
        wt = ctx.frozen_wt if hasattr(ctx, "frozen_wt") else prepared_weights(weight, True, x.dtype)[1]
        outs, c0 = [], 0
        N, H, W, _ = x.shape
        for i, ci in enumerate(ctx.child_ch):
            g = None
            if need[10 + i]:
                slot, idx = ctx.child_slots[i]
                g = conv_bwd_data_raw(dx_raw, wt[c0:c0 + ci], (N, H, W, ci), 1, 1, 0,
                                      accumulate=_slot_fold(slot) if slot is not None else None)
                if slot is not None:
                    _slot_put(slot, g)                       # the child's first consumer (a convolution / pooling) adds it
                    g = None
            elif ctx.child_slots[i][0] is not None:
                raise RuntimeError("gradient slot registered for an input that needs no gradient")
            outs.append(g)
            c0 += ci
        return (dw, ret_g, ret_b, None, None, None, None, None, None, None) + tuple(outs)


def root_conv_bn_act(children, weight, gamma, beta, running_mean, running_var, relu=True, eps=1e-5, momentum=0.1, training=True):
    """conv_bn_act(torch.cat(children, 3), 1x1 weight, ...) for DLA's Root nodes with gradients (see _RootConvBN); training:
    the BatchNorm's mode (False: frozen statistics, freeze_bn)"""
    children = list(children)
    grad = torch.is_grad_enabled() and (training or weight.requires_grad or gamma.requires_grad or beta.requires_grad
                                        or any(c.requires_grad for c in children))
    if not (grad and _ROOT_FUSED[0] and all(c.dim() == 4 for c in children)
            and all(c.shape[3] % 16 == 0 for c in children) and weight.shape[2] == 1):
        return conv_bn_act(torch.cat(children, 3), weight, gamma, beta, running_mean, running_var, 1, 0, relu, None, eps,
                           momentum, training)
    slots = tuple(_slot_register(c, False) for c in children)
    return _RootConvBN.apply(as_krsc(weight), gamma, beta, running_mean, running_var, relu, eps, momentum, bool(training), slots,
                             *children)


_ROOT_FUSED = [os.environ.get("CR_ROOT_FUSED", "1") == "1"]
_STATS_EPOCH = [0]          # bumped by every eager train-mode BatchNorm forward (running statistics change through raw pointers)


_FOLD_REG = [None]          # a list while graphed.GraphedDenseEval captures: the folds the graph reads (see refresh_folds)


def refresh_folds(reg):
    """re-fold (cr_fold_bn, in place) every registered BatchNorm whose inputs changed since its buffers were written; the
    check is host-side (version counters, weight / statistics epochs, storage addresses)"""
    for e in reg:
        w, g, b, m, v = e["t"]
        tag = (w._version, g._version, b._version, m._version, v._version, _WEIGHT_EPOCH[0], _STATS_EPOCH[0], w.data_ptr(), m.data_ptr())
        if tag == e["tag"]:
            continue
        _lib.call("cr_fold_bn", w.detach(), g.detach(), b.detach(), m, v, e["eps"], e["wf"], e["b"], e["Cout"], e["K"], e["af"])
        e["tag"] = tag


def conv_bn_folded(x, weight, gamma, beta, running_mean, running_var, stride=1, pad=0, relu=True, residual=None, eps=1e-5,
                   groups=1):
    """inference: frozen BatchNorm folded into the convolution's weights and bias (cr_fold_bn), residual and ReLU in the
    conv epilogue -- one kernel per layer instead of conv + scale/shift arithmetic + a second pass over the output.
    Outside graph capture the folded copies are cached on the weight tensor (keyed by the version counters of the five
    tensors, the weight epoch and the statistics epoch); inside a capture they are recomputed, so that a replay follows
    weights that changed since."""
    _need_cuda(x, "conv input")
    weight = as_krsc(weight)
    Cout, _, k, _ = weight.shape
    K_ = weight.numel() // Cout
    capturing = torch.cuda.is_current_stream_capturing()
    attr = "_cr_fold" if x.dtype == bf16 else "_cr_fold32"
    if groups == 1:
        fold_af, fold_dtype = _af(x), x.dtype
        fwd = lambda wf, bias_f: conv_fwd_raw(x, wf, Cout, k, stride, pad, bias=bias_f, residual=residual, relu=relu)
    else:                       # grouped 3x3: the folded weights stay f32 in every mode (cr_conv2d_grouped_fwd reads f32)
        if k != 3 or pad != 1:
            raise _lib.CrError(f"grouped convolution: only 3x3 with padding 1 (got k {k}, pad {pad})")
        fold_af, fold_dtype = 1, f32
        fwd = lambda wf, bias_f: conv_grouped_fwd_raw(x, wf, groups, stride, bias=bias_f, residual=residual, relu=relu)
    warm = getattr(weight, attr, None)
    if capturing and _FOLD_REG[0] is not None and warm is not None:
        # eval-mode graph with externally refreshed folds: the graph only READS the folded copies; refresh_folds() rewrites
        # them (eagerly, before a replay) when one of the five tensors or the weight / statistics epoch has moved.  The
        # buffers are the ones the warm-up pass allocated OUTSIDE the capture: a tensor allocated during the capture may share
        # its block with an earlier intermediate of the graph, which every replay rewrites.
        _, wf, bias_f = warm
        _FOLD_REG[0].append({"t": (weight, gamma, beta, running_mean, running_var), "eps": float(eps), "wf": wf, "b": bias_f,
                             "tag": None, "af": fold_af, "K": K_, "Cout": Cout})
        try:
            delattr(weight, attr)           # the graph owns these buffers now: eager calls make their own
        except Exception:
            pass
        return fwd(wf, bias_f)
    tag = None if capturing else (weight._version, gamma._version, beta._version, running_mean._version, running_var._version,
                                  _WEIGHT_EPOCH[0], _STATS_EPOCH[0], weight.data_ptr(), running_mean.data_ptr(), float(eps))
    ent = None if capturing else warm
    if ent is None or ent[0] != tag:
        wf = torch.empty((Cout, K_), dtype=fold_dtype, device=x.device)
        bias_f = torch.empty((Cout,), dtype=f32, device=x.device)
        _lib.call("cr_fold_bn", weight.detach(), gamma.detach(), beta.detach(), running_mean, running_var, float(eps), wf, bias_f,
                  Cout, K_, fold_af)
        ent = (tag, wf, bias_f)
        if not capturing:
            try:
                setattr(weight, attr, ent)
            except Exception:
                pass
    return fwd(ent[1], ent[2])


def conv_bn_act(x, weight, gamma, beta, running_mean, running_var, stride=1, pad=0, relu=True, residual=None,
                eps=1e-5, momentum=0.1, training=True, groups=1, wide_sums=False):
    """groups > 1: the grouped 3x3 kernels (cr_conv2d_grouped_*; pad 1, Cin == Cout) in every route below.  wide_sums: as in
    conv_bn_act_live (the backward's per-channel sums are added across threads in double)"""
    if not training and not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or gamma.requires_grad
                                                          or (residual is not None and residual.requires_grad))):
        return conv_bn_folded(x, weight, gamma, beta, running_mean, running_var, stride, pad, relu, residual, eps, groups)
    if groups > 1 and (weight.shape[2] != 3 or pad != 1):
        raise _lib.CrError(f"grouped convolution: only 3x3 with padding 1 (got k {weight.shape[2]}, pad {pad})")
    xs = _slot_register(x, True)
    rs = _slot_register(residual, False) if residual is not None else (None, 0)
    return _ConvBN.apply(x, as_krsc(weight), gamma, beta, residual, running_mean, running_var, stride, pad, relu, eps,
                         momentum, training, (xs, rs), groups, bool(wide_sums))


# --------------------------------------------------------------------------
# two convolutions, each with its own BatchNorm(train), added, ReLU: the projection-shortcut tail of a ResNet Bottleneck
# (csrc/resnet.hip).  out = relu(bn_a(conv_a(xa)) + bn_b(conv_b(xb)))
# --------------------------------------------------------------------------
def bn_pair_bwd_ws_floats(M, C):
    """floats of workspace cr_bn_pair_bwd needs (include/cr3dod.h); outside its domain the library refuses the call itself"""
    return (_lib.bn_pair_bwd_blocks(M, C) + 1) * 3 * C


def bn_pair_fwd_raw(ya, yb, stats_a, stats_b, bn_a, bn_b):
    """bn_*: (gamma, beta, running_mean, running_var, eps, momentum) -> out, mean_invstd_a, mean_invstd_b"""
    C = ya.shape[-1]
    M = ya.numel() // C
    out = torch.empty_like(ya)
    mia = torch.empty((2, C), dtype=f32, device=ya.device)
    mib = torch.empty((2, C), dtype=f32, device=ya.device)
    _lib.call("cr_bn_pair_fwd", ya, yb, stats_a, stats_b, stats_a.shape[0], bn_a[0], bn_a[1], bn_b[0], bn_b[1], out, M, C,
              float(bn_a[4]), float(bn_a[5]), float(bn_b[4]), float(bn_b[5]), mia, mib, bn_a[2], bn_a[3], bn_b[2], bn_b[3],
              _af(ya))
    return out, mia, mib


def bn_pair_bwd_raw(dout, out, ya, yb, mia, mib, gamma_a, gamma_b, dgamma_a, dbeta_a, dgamma_b, dbeta_b):
    """-> dxa_raw, dxb_raw; the four parameter gradients are accumulated into"""
    C = ya.shape[-1]
    M = ya.numel() // C
    n = bn_pair_bwd_ws_floats(M, C)
    ws = torch.empty((n,), dtype=f32, device=ya.device)
    dxa, dxb = torch.empty_like(ya), torch.empty_like(yb)
    _lib.call("cr_bn_pair_bwd", dout, out, ya, yb, mia, mib, gamma_a, gamma_b, ws, n, dxa, dxb, dgamma_a, dbeta_a, dgamma_b,
              dbeta_b, M, C, _af(ya))
    return dxa, dxb


class _ConvBNPair(torch.autograd.Function):
    """side a: (xa, wa, gamma_a, beta_a), side b: (xb, wb, gamma_b, beta_b); bufs: the four running-statistics buffers;
    cfg: (stride_a, pad_a, eps_a, momentum_a, stride_b, pad_b, eps_b, momentum_b); slots: the gradient slots of xa and xb"""

    @staticmethod
    def forward(ctx, xa, wa, gamma_a, beta_a, xb, wb, gamma_b, beta_b, bufs, cfg, slots):
        sa, pa, eps_a, mom_a, sb, pb, eps_b, mom_b = cfg
        C = wa.shape[0]
        assert wb.shape[0] == C and xa.dtype == xb.dtype
        wpa, _ = prepared_weights(wa, xa.requires_grad, xa.dtype)
        wpb, _ = prepared_weights(wb, xb.requires_grad, xb.dtype)
        _STATS_EPOCH[0] += 1
        ka, kb = wa.shape[2], wb.shape[2]
        N_, H_, W_, _ = xa.shape
        M = N_ * ((H_ + 2 * pa - ka) // sa + 1) * ((W_ + 2 * pa - ka) // sa + 1)
        nparts = (M + 63) // 64                # statistics rows are per 64 pixels
        stats_a = torch.empty((nparts, 2, C), dtype=f32, device=xa.device)
        stats_b = torch.empty((nparts, 2, C), dtype=f32, device=xa.device)
        ya = conv_fwd_raw(xa, wpa, C, ka, sa, pa, stats=stats_a)
        yb = conv_fwd_raw(xb, wpb, C, kb, sb, pb, stats=stats_b)
        if ya.shape != yb.shape:
            raise _lib.CrError(f"conv_bn_pair_act: the two convolutions give {tuple(ya.shape)} and {tuple(yb.shape)}")
        out, mia, mib = bn_pair_fwd_raw(ya, yb, stats_a, stats_b,
                                        (gamma_a.detach(), beta_a.detach(), bufs[0], bufs[1], eps_a, mom_a),
                                        (gamma_b.detach(), beta_b.detach(), bufs[2], bufs[3], eps_b, mom_b))
        ctx.cfg, ctx.slots = cfg, slots
        ctx.beta_refs = (beta_a, beta_b)
        ctx.save_for_backward(xa, wa, gamma_a, xb, wb, gamma_b, ya, yb, out, mia, mib)
        return out

    @staticmethod
    def backward(ctx, dout):
        xa, wa, gamma_a, xb, wb, gamma_b, ya, yb, out, mia, mib = ctx.saved_tensors
        sa, pa, _, _, sb, pb, _, _ = ctx.cfg
        C = wa.shape[0]
        dout = dout.to(ya.dtype).contiguous()
        acc, ret = [], []
        for gamma, beta in ((gamma_a, ctx.beta_refs[0]), (gamma_b, ctx.beta_refs[1])):
            gs, bs = grad_sink(gamma), grad_sink(beta)
            if gs is not None and bs is not None:
                acc += [gs, bs]
                ret += [None, None]
            else:
                fresh = [torch.zeros((C,), dtype=f32, device=ya.device) for _ in range(2)]
                acc += fresh
                ret += fresh
        dxa_raw, dxb_raw = bn_pair_bwd_raw(dout, out, ya, yb, mia, mib, gamma_a.detach(), gamma_b.detach(), *acc)
        grads = []
        sides = ((xa, wa, dxa_raw, sa, pa, ctx.slots[0], 0), (xb, wb, dxb_raw, sb, pb, ctx.slots[1], 4))
        for x, w, dx_raw, stride, pad, (xslot, xi), at in sides:
            k = w.shape[2]
            dx = None
            if ctx.needs_input_grad[at]:
                _, wt = prepared_weights(w, True, x.dtype)
                bwd_data = lambda a: conv_bwd_data_raw(dx_raw, wt, x.shape, k, stride, pad, accumulate=a)
                if xslot is not None and xi > 1:            # not the first consumer of x: leave the contribution in the slot
                    _slot_put(xslot, bwd_data(_slot_fold(xslot)))
                else:
                    dx = bwd_data(_slot_take(xslot) if xslot is not None else None)
            elif xslot is not None:
                raise RuntimeError("gradient slot registered for an input that needs no gradient")
            dw = conv_bwd_weight_raw(dx_raw, x, k, stride, pad, grad_sink(w)) if ctx.needs_input_grad[at + 1] else None
            grads.append((dx, dw))
        return (grads[0][0], grads[0][1], ret[0], ret[1], grads[1][0], grads[1][1], ret[2], ret[3], None, None, None)


def conv_bn_pair_act(xa, weight_a, bn_a, xb, weight_b, bn_b, stride_a=1, pad_a=0, stride_b=1, pad_b=0):
    """relu(bn_a(conv(xa, weight_a)) + bn_b(conv(xb, weight_b))); bn_*: (gamma, beta, running_mean, running_var, eps, momentum,
    training).  Both BatchNorms in training mode: two convolutions with statistics rows, then cr_bn_pair_fwd -- the normalised
    shortcut is never materialised; the backward is cr_bn_pair_bwd and the convolutions' own backward kernels.  Frozen
    statistics (with or without gradients) take the folded routes of conv_bn_act: one convolution per BatchNorm with bias,
    residual and ReLU in its epilogue.  Their backward forms the bias gradients -- plain sums of the masked cotangent over the
    pixels -- with cr_colsum_wide (wide_sums): the weight gradient's own bias sum adds a block's rows one after the other in
    float32, which measured 2.5 .. 3.1 x the float32 restatement's error on bn3.bias."""
    if not (bn_a[6] and bn_b[6]):
        identity = conv_bn_act(xb, weight_b, bn_b[0], bn_b[1], bn_b[2], bn_b[3], stride_b, pad_b, False, None, bn_b[4], bn_b[5],
                               bn_b[6], wide_sums=not bn_b[6])
        return conv_bn_act(xa, weight_a, bn_a[0], bn_a[1], bn_a[2], bn_a[3], stride_a, pad_a, True, identity, bn_a[4], bn_a[5],
                           bn_a[6], wide_sums=not bn_a[6])
    slots = (_slot_register(xa, True), _slot_register(xb, True))
    return _ConvBNPair.apply(xa, as_krsc(weight_a), bn_a[0], bn_a[1], xb, as_krsc(weight_b), bn_b[0], bn_b[1],
                             (bn_a[2], bn_a[3], bn_b[2], bn_b[3]),
                             (stride_a, pad_a, bn_a[4], bn_a[5], stride_b, pad_b, bn_b[4], bn_b[5]), slots)


# --------------------------------------------------------------------------
# conv + bias (+ ReLU), bf16 or f32 output   (FPN laterals/outputs, RPN head)
# --------------------------------------------------------------------------
def relu_bwd(y, dy):
    """dy masked by the ReLU whose OUTPUT is y (one kernel); dy is cast to y's dtype first if it differs"""
    dy = _act_cast(dy, y.dtype)
    g = torch.empty_like(dy)
    _lib.call("cr_relu_bwd", y.contiguous(), dy, g, y.numel(), _af(y))
    return g


class _ConvBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, relu, out_f32, slot=(None, 0)):
        ctx.slot = slot
        Cout, Cin, k, _ = weight.shape
        wb, _ = prepared_weights(weight, False, x.dtype)
        y = conv_fwd_raw(x, wb, Cout, k, stride, pad, bias=None if bias is None else bias.detach(), relu=relu,
                         out_f32=out_f32)
        ctx.cfg = (k, stride, pad, relu, bias is not None)
        ctx.bias_ref = bias
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        k, stride, pad, relu, has_bias = ctx.cfg
        g = dy.contiguous()
        if relu:
            g = relu_bwd(y, g)
        db, acc = None, None
        want_db = has_bias and ctx.needs_input_grad[2]
        if want_db:
            C = g.shape[3]
            bsink = grad_sink(ctx.bias_ref)
            acc = bsink if bsink is not None else torch.zeros((C,), dtype=f32, device=g.device)
            db = None if bsink is not None else acc
            if not (ctx.needs_input_grad[1] and g.dtype == x.dtype):
                # no weight-gradient launch to ride on (or an f32 upstream gradient): separate column sum
                ws = torch.empty((1024, C), dtype=f32, device=g.device)
                _lib.call("cr_colsum_accum", g, int(g.dtype == f32), g.numel() // C, C, ws, acc)
                acc = None
        g = g.to(x.dtype).contiguous()
        dx = None
        xslot, xi = ctx.slot
        if ctx.needs_input_grad[0]:
            _, wt = prepared_weights(weight, True, x.dtype)
            if xslot is not None and xi > 1:
                _slot_put(xslot, conv_bwd_data_raw(g, wt, x.shape, k, stride, pad, accumulate=_slot_fold(xslot)))
            else:
                dx = conv_bwd_data_raw(g, wt, x.shape, k, stride, pad, accumulate=_slot_take(xslot) if xslot is not None else None)
        elif xslot is not None:
            raise RuntimeError("gradient slot registered for an input that needs no gradient")
        # the bias gradient (column sums of dy) is accumulated inside the weight-gradient kernel
        dw = conv_bwd_weight_raw(g, x, k, stride, pad, grad_sink(weight), bias_acc=acc) if ctx.needs_input_grad[1] else None
        return dx, dw, db, None, None, None, None, None


class _PadInputChannels(torch.autograd.Function):
    """(Cout,Cin,k,k) weight -> zero-padded to Cin8 input channels (the RGB stem: 3 -> 8).  Backward adds the slice of
    the padded gradient straight into the parameter's gradient sink when there is one."""
    @staticmethod
    def forward(ctx, w, cin_to):
        ctx.w_ref = w
        out = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, cin_to - w.shape[1]))
        return out.contiguous(memory_format=torch.channels_last)

    @staticmethod
    def backward(ctx, g):
        w = ctx.w_ref
        gs = g[:, :w.shape[1]]
        sink = grad_sink(w)
        if sink is not None:
            sink.add_(gs)
            return None, None
        return gs, None


def pad_input_channels(w, cin_to=8):
    return _PadInputChannels.apply(w, cin_to)


class _CatRows(torch.autograd.Function):
    """concatenate parameters along dim 0 (+ zero rows up to `rows`); backward routes each slice into its sink."""
    @staticmethod
    def forward(ctx, rows, *params):
        ctx.refs = params
        n = sum(p.shape[0] for p in params)
        parts = list(params)
        if rows > n:
            parts.append(params[0].new_zeros((rows - n,) + tuple(params[0].shape[1:])))
        return torch.cat(parts, 0)

    @staticmethod
    def backward(ctx, g):
        outs, off = [], 0
        for p in ctx.refs:
            gs = g[off:off + p.shape[0]]
            off += p.shape[0]
            sink = grad_sink(p)
            if sink is not None:
                sink.add_(gs)
                outs.append(None)
            else:
                outs.append(gs)
        return (None,) + tuple(outs)


def cat_rows(params, rows):
    return _CatRows.apply(rows, *params)


def conv_bias_act(x, weight, bias, stride=1, pad=0, relu=False, out_f32=False):
    return _ConvBias.apply(x, as_krsc(weight), bias, stride, pad, relu, out_f32, _slot_register(x, True))


# --------------------------------------------------------------------------
# GroupNorm over NHWC maps (csrc/groupnorm.hip): the norm "GN" of the FPN and of the conv box head.  No running statistics:
# eval mode is the same call.  Workspaces come from torch's allocator and nothing waits on the host, so the calls can be
# captured into the dense region's graph.
# --------------------------------------------------------------------------
def _gn_dims(x):
    N, C = x.shape[0], x.shape[-1]
    return N, x.numel() // max(1, N * C), C


def _gn_workspace(x):
    N, HW, C = _gn_dims(x)
    n = _lib.groupnorm_ws_floats(N, HW, C)      # 0 outside the domain: the library then refuses the call itself
    return torch.empty((max(n, 4),), dtype=f32, device=x.device), n


def group_norm_fwd_raw(x, gamma, beta, groups, eps, relu=False, stat_rows=None):
    """x (N, ..., C) NHWC -> y, mean_rstd (N, G, 2).  stat_rows: the [N * HW / 64][2][C] rows conv_fwd_raw(stats=) wrote for x
    (HW % 64 == 0), instead of a statistics pass over x"""
    _need_cuda(x, "group_norm input")
    assert x.is_contiguous() and gamma.dtype == f32 and beta.dtype == f32
    N, HW, C = _gn_dims(x)
    y = torch.empty_like(x)
    mr = torch.empty((N, max(1, groups), 2), dtype=f32, device=x.device)
    ws, n = _gn_workspace(x)
    _lib.call("cr_groupnorm_fwd", x, gamma, beta, stat_rows, y, mr, ws, n, N, HW, C, groups, float(eps), int(relu), _af(x))
    return y, mr


def group_norm_bwd_raw(dy, x, y, mean_rstd, gamma, groups, relu, dgamma, dbeta):
    """-> dx; dgamma / dbeta (C) f32 are accumulated into.  y: the stored output (read only with relu)"""
    assert dy.is_contiguous() and x.is_contiguous() and dy.dtype == x.dtype
    N, HW, C = _gn_dims(x)
    dx = torch.empty_like(x)
    ws, n = _gn_workspace(x)
    _lib.call("cr_groupnorm_bwd", dy, x, y if relu else None, mean_rstd, gamma, ws, n, dx, dgamma, dbeta, N, HW, C, groups,
              int(relu), _af(x))
    return dx


def _gn_param_acc(ctx_needs, gamma, beta, C, dev):
    """(accumulators, autograd returns) of dgamma / dbeta: the parameters' gradient sinks where both have one"""
    gs, bs = grad_sink(gamma), grad_sink(beta)
    if gs is not None and bs is not None:
        return (gs, bs), (None, None)
    fresh = tuple(torch.zeros((C,), dtype=f32, device=dev) for _ in range(2))
    return fresh, tuple(f if need else None for f, need in zip(fresh, ctx_needs))


class _GroupNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, relu):
        x = x.contiguous()
        y, mr = group_norm_fwd_raw(x, gamma.detach(), beta.detach(), groups, eps, relu)
        ctx.cfg = (groups, relu)
        ctx.beta_ref = beta
        ctx.save_for_backward(x, gamma, mr, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mr, y = ctx.saved_tensors
        groups, relu = ctx.cfg
        acc, ret = _gn_param_acc(ctx.needs_input_grad[1:3], gamma, ctx.beta_ref, x.shape[-1], x.device)
        dx = group_norm_bwd_raw(_act_cast(dy, x.dtype), x, y, mr, gamma.detach(), groups, relu, *acc)
        return dx, ret[0], ret[1], None, None, None


def group_norm(x, gamma, beta, groups, eps=1e-5, relu=False):
    """relu?(GroupNorm(groups, C)(x)) of an NHWC map in the activation dtype; gamma / beta (C) f32 parameters.  dgamma / dbeta
    go into the parameters' gradient sinks where they exist (autograd then sees None), else they are returned."""
    return _GroupNorm.apply(x, gamma, beta, groups, eps, relu)


class _ConvGN(torch.autograd.Function):
    """bias-free convolution, then GroupNorm (+ ReLU).  In float32, when a sample's output map is a multiple of 128 pixels, the
    convolution's epilogue writes the statistics rows and GroupNorm never reads the map for them.  128, not 64: the
    convolution's 128-pixel tiles put their sums into every second row, and no tile may straddle two samples.  Not in bf16:
    the epilogue sums the float32 accumulators, GroupNorm normalises the bf16-rounded map it is handed."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, groups, eps, stride, pad, relu, slot=(None, 0)):
        ctx.slot = slot
        Cout, Cin, k, _ = weight.shape
        wb, _ = prepared_weights(weight, False, x.dtype)
        N, H, W, _ = x.shape
        HWo = ((H + 2 * pad - k) // stride + 1) * ((W + 2 * pad - k) // stride + 1)
        rows = torch.empty((N * HWo // 64, 2, Cout), dtype=f32, device=x.device) if HWo % 128 == 0 and x.dtype == f32 else None
        t = conv_fwd_raw(x, wb, Cout, k, stride, pad, stats=rows)
        y, mr = group_norm_fwd_raw(t, gamma.detach(), beta.detach(), groups, eps, relu, stat_rows=rows)
        ctx.cfg = (k, stride, pad, relu, groups)
        ctx.beta_ref = beta
        ctx.save_for_backward(x, weight, gamma, t, mr, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, gamma, t, mr, y = ctx.saved_tensors
        k, stride, pad, relu, groups = ctx.cfg
        acc, ret = _gn_param_acc(ctx.needs_input_grad[2:4], gamma, ctx.beta_ref, t.shape[-1], x.device)
        g = group_norm_bwd_raw(_act_cast(dy, t.dtype), t, y, mr, gamma.detach(), groups, relu, *acc)
        dx = None
        xslot, xi = ctx.slot
        if ctx.needs_input_grad[0]:
            _, wt = prepared_weights(weight, True, x.dtype)
            if xslot is not None and xi > 1:
                _slot_put(xslot, conv_bwd_data_raw(g, wt, x.shape, k, stride, pad, accumulate=_slot_fold(xslot)))
            else:
                dx = conv_bwd_data_raw(g, wt, x.shape, k, stride, pad, accumulate=_slot_take(xslot) if xslot is not None else None)
        elif xslot is not None:
            raise RuntimeError("gradient slot registered for an input that needs no gradient")
        dw = conv_bwd_weight_raw(g, x, k, stride, pad, grad_sink(weight)) if ctx.needs_input_grad[1] else None
        return dx, dw, ret[0], ret[1], None, None, None, None, None, None


def conv_gn_act(x, weight, gn_args, stride=1, pad=0, relu=False):
    """relu?(GroupNorm(conv(x, weight))): a bias-free convolution followed by GroupNorm; gn_args = (gamma, beta, groups, eps)"""
    gamma, beta, groups, eps = gn_args
    return _ConvGN.apply(x, as_krsc(weight), gamma, beta, groups, eps, stride, pad, relu, _slot_register(x, True))


# --------------------------------------------------------------------------
# grouped convolutions: the five pyramid levels of an FPN output conv / the RPN head conv in ONE launch per direction
# --------------------------------------------------------------------------
_GROUP_ON = [os.environ.get("CR_CONV_GROUP", "1") == "1"]


def _ptr_table(tensors):
    return (ctypes.c_void_p * len(tensors))(*[0 if t is None else t.data_ptr() for t in tensors])


def _int_table(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def group_supported(xs, weights, stride=1):
    """shapes the grouped kernels take: stride 1, k in {1,3}, Cout % 128 == 0, Cin % 64 == 0, fp32 or bf16 (not the split mode)"""
    w0 = weights[0]
    Cout, Cin, k, _ = w0.shape
    return (_GROUP_ON[0] and stride == 1 and 2 <= len(xs) <= 8 and k in (1, 3) and Cout % 128 == 0 and Cin % 128 == 0
            and all(tuple(w.shape) == tuple(w0.shape) for w in weights) and all(x.is_cuda and x.dim() == 4 for x in xs)
            and not (xs[0].dtype == f32 and _ACT[0][1] == 2))


def conv_fwd_group_raw(xs, wbs, ys, Cin, Cout, k, pad, biases, relu):
    """cr_conv2d_fwd_group on prepared operands (module-level so that bench.py can bracket the launch with events)"""
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    _lib.call("cr_conv2d_fwd_group", len(xs), cast(_ptr_table(xs)), cast(_ptr_table(wbs)), cast(_ptr_table(ys)),
              cast(_int_table([x.shape[0] for x in xs])), cast(_int_table([x.shape[1] for x in xs])),
              cast(_int_table([x.shape[2] for x in xs])), Cin, Cout, k, pad, cast(_ptr_table(biases)), None, int(relu),
              _af(xs[0]), device=xs[0].device)


def conv_bwd_data_group_raw(gs, wts, outs, shapes, Cin, Cout, k, pad, accs):
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    _lib.call("cr_conv2d_bwd_data_group", len(gs), cast(_ptr_table(gs)), cast(_ptr_table(wts)), cast(_ptr_table(outs)),
              cast(_int_table([s_[0] for s_ in shapes])), cast(_int_table([s_[1] for s_ in shapes])),
              cast(_int_table([s_[2] for s_ in shapes])), Cin, Cout, k, pad, _af(gs[0]), cast(_ptr_table(accs)),
              device=gs[0].device)


def conv_bwd_weight_group_raw(gs, xs, dws, dbs, Cin, Cout, k, pad):
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    _lib.call("cr_conv2d_bwd_weight_group", len(xs), cast(_ptr_table(gs)), cast(_ptr_table(xs)), cast(_ptr_table(dws)),
              cast(_ptr_table(dbs)), cast(_int_table([x.shape[0] for x in xs])), cast(_int_table([x.shape[1] for x in xs])),
              cast(_int_table([x.shape[2] for x in xs])), Cin, Cout, k, pad, 1, device=xs[0].device)


# --------------------------------------------------------------------------
# Winograd F(2x2, 3x3) route of the grouped 3x3 convolutions (float32, stride 1, pad 1, even maps, one shared weight):
# input transform -> one kernel for the 16 GEMMs and the output transform (cr_wino_gemm_output).  2.25x fewer multiplies; the V
# planes (16 x tiles x C floats), and the dM planes of the weight gradient, are persistent per (tiles, channels) and must exist
# before a graph capture (first eager pass).
# --------------------------------------------------------------------------
_WINO_BUF = {}
_WINO_DM = {}


def winograd_on():
    return os.environ.get("CR_WINOGRAD", "1") == "1"


def _wino_buffers(T, C, O, dev):
    key = (T, C, O, str(dev))
    ent = _WINO_BUF.get(key)
    if ent is None:
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise _lib.CrError("winograd: the V planes must be allocated before the graph capture (run one eager pass first)")
        # U (16, O, C) is the head of a flat buffer whose 16 * O tail holds the partial bias gradients of the weight-gradient
        # route (one zero-fill covers both)
        ent = _WINO_BUF[key] = (torch.empty((16, T, C), dtype=f32, device=dev),
                                torch.empty((16 * O * C + 16 * O,), dtype=f32, device=dev))
    return ent


def _wino_dm_buffer(T, O, dev):
    """dM (16, T, O) = A dY A^T of the weight-gradient route (the forward and backward-data routes keep M in registers)"""
    key = (T, O, str(dev))
    ent = _WINO_DM.get(key)
    if ent is None:
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise _lib.CrError("winograd: the dM planes must be allocated before the graph capture (run one eager pass first)")
        ent = _WINO_DM[key] = torch.empty((16, T, O), dtype=f32, device=dev)
    return ent


def wino_supported(xs, weight, k, pad):
    return (winograd_on() and k == 3 and pad == 1 and xs[0].dtype == f32 and _ACT[0][1] == 1 and len(xs) <= 8
            and weight.shape[0] % 128 == 0 and weight.shape[1] % 128 == 0       # (backward-data swaps the two)
            and all(x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0 for x in xs))


WINO_MIN_TILES = int(os.environ.get("CR_WINO_MIN_TILES", "4096"))


def _wino_plan(xs, ws, bs, k, pad):
    """"shared": every map through ONE Winograd pipeline (one weight and bias object for all); else per map True / False"""
    n = len(xs)
    if not wino_supported(xs, ws[0], k, pad):
        return [False] * n
    if all(w is ws[0] for w in ws) and all(b is bs[0] for b in bs):
        return "shared"
    return [x.shape[0] * (x.shape[1] // 2) * (x.shape[2] // 2) >= WINO_MIN_TILES for x in xs]


def wino_conv3x3_group(srcs, w_krsc, dsts, bias, relu, accs, backward, keep_v=False):
    """dsts[i] = conv3x3(srcs[i], w) (+ bias, ReLU, + accs[i]) for n maps sharing ONE weight: forward (w (O,3,3,C) applied to
    (N,H,W,C) maps) or, backward = True, the backward-data of that convolution (srcs = dY with O channels, dsts = dX with C).
    keep_v: the transformed input goes to a tensor of its own, which is returned (the weight gradient multiplies the same
    planes: wino_wgrad_group(v_saved=...)), instead of the shared planes the next Winograd convolution overwrites."""
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert w_krsc.dim() == 4 and w_krsc.shape[2:] == (3, 3) and w_krsc.is_contiguous(memory_format=torch.channels_last)
    O, C = w_krsc.shape[0], w_krsc.shape[1]              # logical (O, C, 3, 3) over physical [O][3][3][C]
    cin, cout = (O, C) if backward else (C, O)          # channels of the maps going in / coming out
    dev = srcs[0].device
    T = sum(x.shape[0] * (x.shape[1] // 2) * (x.shape[2] // 2) for x in srcs)
    V, U = _wino_buffers(T, cin, cout, dev)
    U = U[:16 * O * C]
    if keep_v:
        V = torch.empty((16, T, cin), dtype=f32, device=dev)
    _lib.call("cr_wino_filter", w_krsc, U, O, C, int(backward))
    Ns, Hs, Ws = _int_table([x.shape[0] for x in srcs]), _int_table([x.shape[1] for x in srcs]), _int_table([x.shape[2] for x in srcs])
    _lib.call("cr_wino_input", len(srcs), cast(_ptr_table(srcs)), cast(Ns), cast(Hs), cast(Ws), cin, V, T)
    _lib.call("cr_wino_gemm_output", len(dsts), V, U, cast(_ptr_table(dsts)), cast(Ns), cast(Hs), cast(Ws), cin, cout, T, bias,
              int(relu), cast(_ptr_table(accs)) if accs is not None else None)
    return V if keep_v else None


def wino_wgrad_on():
    """the Winograd weight gradient (CR_WINO_WGRAD, default on); in the bit-reproducible mode (CR_DETERMINISTIC=1) its pixel
    splits are added in a fixed order (cr_wgrad_batched_f32) and the bias gradient is a fixed-order column sum"""
    return os.environ.get("CR_WINO_WGRAD", "1") != "0"


def deterministic_on():
    """CR_DETERMINISTIC=1: every weight-gradient reduce in a fixed order (read by the library at its first weight gradient)"""
    return os.environ.get("CR_DETERMINISTIC", "0") not in ("", "0")


def wino_wgrad_group(gs, xs, w_sink, b_sink, v_saved=None):
    """weight (and bias) gradient of ONE 3x3 weight applied to n maps, the Winograd way: dM = A dY A^T and V = B^T x B as for
    the forward pass, dU[k] = dM[k]^T V[k] per transformed position (cr_linear_bwd_weight), dW += G^T dU G into the flat
    gradient; db += channel sums of dY.  45.8 instead of 103 GFLOP for the five pyramid levels of 4 images."""
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    O, C = gs[0].shape[3], xs[0].shape[3]
    dev = xs[0].device
    T = sum(x.shape[0] * (x.shape[1] // 2) * (x.shape[2] // 2) for x in xs)
    V, U = _wino_buffers(T, C, O, dev)
    M = _wino_dm_buffer(T, O, dev)
    Ns, Hs, Ws = _int_table([x.shape[0] for x in xs]), _int_table([x.shape[1] for x in xs]), _int_table([x.shape[2] for x in xs])
    if v_saved is not None:                 # the forward pass kept B^T x B of exactly these maps
        assert v_saved.shape == (16, T, C)
        V = v_saved
    else:
        _lib.call("cr_wino_input", len(xs), cast(_ptr_table(xs)), cast(Ns), cast(Hs), cast(Ws), C, V, T)
    U.zero_()
    # the bias gradient rides on the dY transform (atomics over partial rows), or, deterministic, is a fixed-order column sum
    part = U[16 * O * C:] if b_sink is not None and not deterministic_on() else None
    if b_sink is not None and part is None:
        ws = torch.empty((1024, O), dtype=torch.float32, device=dev)
        for g in gs:
            _lib.call("cr_colsum_accum", g, 1, g.numel() // O, O, ws, b_sink)
    _lib.call("cr_wino_dy", len(gs), cast(_ptr_table(gs)), cast(Ns), cast(Hs), cast(Ws), O, M, T, part)
    _lib.call("cr_wgrad_batched_f32", M, V, U, T, C, O, 16, T * O, T * C, O * C)
    _lib.call("cr_wino_filter_grad", U, w_sink, O, C, part, b_sink if part is not None else None)


class _ConvBiasGroup(torch.autograd.Function):
    """y_i = act(conv(x_i, W_i) + b_i) for n same-geometry problems: cr_conv2d_fwd_group forward, cr_conv2d_bwd_data_group and
    (fp32) cr_conv2d_bwd_weight_group backward.  The W_i / b_i may be one parameter repeated (the RPN head)."""

    @staticmethod
    def forward(ctx, n, pad, relu, slots, *args):
        """slots[-1] == "stacked" (conv_bias_act_group(stacked=True)): the n outputs are the consecutive row blocks of ONE
        (1, 1, sum of pixels, Cout) tensor -- what a following 1x1 convolution treats as a single map (the RPN predictors
        over all pyramid levels at once); one gradient comes back and one ReLU backward covers all levels."""
        stacked = len(slots) == n + 1
        xs, ws, bs = args[:n], args[n:2 * n], args[2 * n:3 * n]
        Cout, Cin, k, _ = ws[0].shape
        dt = xs[0].dtype
        xs = [x.contiguous() for x in xs]
        wbs = [prepared_weights(w, False, dt)[0] for w in ws]
        shapes = [(x.shape[0], x.shape[1] + 2 * pad - k + 1, x.shape[2] + 2 * pad - k + 1, Cout) for x in xs]
        if stacked:
            rows = [s[0] * s[1] * s[2] for s in shapes]
            Y = torch.empty((1, 1, sum(rows), Cout), dtype=dt, device=xs[0].device)
            flat, off, ys = Y.view(-1, Cout), 0, []
            for s, m in zip(shapes, rows):
                ys.append(flat[off:off + m].view(s))
                off += m
        else:
            ys = [torch.empty(s, dtype=dt, device=x.device) for s, x in zip(shapes, xs)]
        bd = [None if b is None else b.detach() for b in bs]
        # float32 3x3: the Winograd route -- all maps in one pipeline when they share the weight (the RPN head), the big maps
        # one by one otherwise (the FPN output convolutions; the small levels stay one direct grouped launch)
        ctx.wino = plan = _wino_plan(xs, ws, bs, k, pad)
        # the transformed input is kept for the weight gradient when that will take the Winograd route too
        keep = lambda i: (ctx.needs_input_grad[4 + n + i] and grad_sink(ws[i]) is not None and wino_wgrad_on()
                          and os.environ.get("CR_WINO_KEEP_V", "1") != "0")
        ctx.wino_v = {}
        if plan == "shared":
            ctx.wino_v["shared"] = wino_conv3x3_group(xs, wbs[0], ys, bd[0], relu, None, False, keep(0))
        else:
            for i in range(n):
                if plan[i]:
                    ctx.wino_v[i] = wino_conv3x3_group([xs[i]], wbs[i], [ys[i]], bd[i], relu, None, False, keep(i))
            rest = [i for i in range(n) if not plan[i]]
            if rest:
                conv_fwd_group_raw([xs[i] for i in rest], [wbs[i] for i in rest], [ys[i] for i in rest], Cin, Cout, k, pad,
                                   [bd[i] for i in rest], relu)
        ctx.cfg = (n, k, pad, relu)
        ctx.slots = slots
        ctx.refs = (ws, bs)
        ctx.stacked = shapes if stacked else None
        ctx.save_for_backward(*xs, *((Y,) if stacked and relu else (ys if relu else ())))
        ctx.set_materialize_grads(False)
        return Y if stacked else tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        n, k, pad, relu = ctx.cfg
        ws, bs = ctx.refs
        saved = ctx.saved_tensors
        xs = saved[:n]
        gs = {}
        if ctx.stacked is not None:
            live = list(range(n)) if dys[0] is not None else []
            if live:
                g = dys[0].contiguous()
                if relu:
                    g = relu_bwd(saved[n], g)
                g = g.to(xs[0].dtype).contiguous().view(-1, g.shape[-1])
                off = 0
                for i, s in enumerate(ctx.stacked):
                    m = s[0] * s[1] * s[2]
                    gs[i] = g[off:off + m].view(s)
                    off += m
        else:
            ys = saved[n:] if relu else (None,) * n
            live = [i for i in range(n) if dys[i] is not None]            # an output nobody differentiated takes no part
            for i in live:
                g = dys[i].contiguous()
                if relu:
                    g = relu_bwd(ys[i], g)
                gs[i] = g.to(xs[i].dtype).contiguous()
        dt = xs[0].dtype
        Cout, Cin = ws[0].shape[0], ws[0].shape[1]
        dxs = [None] * n
        need_dx = [i for i in live if ctx.needs_input_grad[4 + i]]
        for i in range(n):
            if i not in need_dx and ctx.slots[i][0] is not None and i in live:
                raise RuntimeError("gradient slot registered for an input that needs no gradient")
        if need_dx:
            plan = ctx.wino
            outs = [torch.empty_like(xs[i]) for i in need_dx]
            accs = []
            for i in need_dx:
                slot, xi = ctx.slots[i]
                a = None if slot is None else (_slot_take(slot) if xi <= 1 else _slot_fold(slot))
                accs.append(None if a is None else a.to(dt).contiguous())
            if plan == "shared":
                wino_conv3x3_group([gs[i] for i in need_dx], prepared_weights(ws[0], False, dt)[0], outs, None, False, accs, True)
            else:
                for j, i in enumerate(need_dx):
                    if plan[i]:
                        wino_conv3x3_group([gs[i]], prepared_weights(ws[i], False, dt)[0], [outs[j]], None, False, [accs[j]], True)
                rest = [j for j, i in enumerate(need_dx) if not plan[i]]
                if rest:
                    conv_bwd_data_group_raw([gs[need_dx[j]] for j in rest], [prepared_weights(ws[need_dx[j]], True, dt)[1] for j in rest],
                                            [outs[j] for j in rest], [xs[need_dx[j]].shape for j in rest], Cin, Cout, k, pad,
                                            [accs[j] for j in rest])
            for i, o in zip(need_dx, outs):
                slot, xi = ctx.slots[i]
                if slot is not None and xi > 1:
                    _slot_put(slot, o)
                else:
                    dxs[i] = o
        # weight / bias gradients: one grouped launch in fp32 when every parameter has a sink to accumulate into; otherwise the
        # per-problem kernels (bf16 mode, parameters without sinks)
        dws, dbs = [None] * n, [None] * n
        wl = [i for i in live if ctx.needs_input_grad[4 + n + i]]
        sinks_ok = dt == f32 and all(grad_sink(ws[i]) is not None and (bs[i] is None or grad_sink(bs[i]) is not None) for i in wl)
        wplan = ctx.wino if sinks_ok and wino_wgrad_on() else None
        if wl and wplan == "shared":
            # one weight over all maps: dU[k] = dM[k]^T V[k] for the 16 transformed positions in one batched launch
            want_db = bs[0] is not None and ctx.needs_input_grad[4 + 2 * n + wl[0]]
            wino_wgrad_group([gs[i] for i in wl], [xs[i] for i in wl], grad_sink(ws[0]), grad_sink(bs[0]) if want_db else None,
                             ctx.wino_v.get("shared") if len(wl) == n else None)
            wl = []
        elif wl and wplan is not None and any(wplan[i] for i in wl):
            for i in [i for i in wl if wplan[i]]:
                want_db = bs[i] is not None and ctx.needs_input_grad[4 + 2 * n + i]
                wino_wgrad_group([gs[i]], [xs[i]], grad_sink(ws[i]), grad_sink(bs[i]) if want_db else None, ctx.wino_v.get(i))
            wl = [i for i in wl if not wplan[i]]
        if wl and sinks_ok and len(wl) > 1:
            dwt = [grad_sink(ws[i]) for i in wl]
            dbt = [None if bs[i] is None or not ctx.needs_input_grad[4 + 2 * n + i] else grad_sink(bs[i]) for i in wl]
            conv_bwd_weight_group_raw([gs[i] for i in wl], [xs[i] for i in wl], dwt, dbt, Cin, Cout, k, pad)
        else:
            for i in wl:
                bsink = None if bs[i] is None else grad_sink(bs[i])
                want_db = bs[i] is not None and ctx.needs_input_grad[4 + 2 * n + i]
                acc = None
                if want_db:
                    acc = bsink if bsink is not None else torch.zeros((Cout,), dtype=f32, device=xs[i].device)
                    if bsink is None:
                        dbs[i] = acc if dbs[i] is None else dbs[i] + acc
                dws[i] = conv_bwd_weight_raw(gs[i], xs[i], k, 1, pad, grad_sink(ws[i]), bias_acc=acc)
        return (None, None, None, None) + tuple(dxs) + tuple(dws) + tuple(dbs)


def conv_bias_act_group(xs, weights, biases, pad=0, relu=False, stacked=False):
    """[act(conv(x_i, W_i) + b_i)] -- one launch per direction when the shapes allow (group_supported), else one conv each.
    stacked=True (only when group_supported): ONE tensor (1, 1, sum_i N_i H_i W_i, Cout) whose row blocks are the outputs."""
    xs, weights, biases = list(xs), [as_krsc(w) for w in weights], list(biases)
    if not group_supported(xs, weights):
        if stacked:
            raise _lib.CrError("conv_bias_act_group(stacked=True): the problems do not form a group (see group_supported)")
        return [conv_bias_act(x, w, b, 1, pad, relu=relu) for x, w, b in zip(xs, weights, biases)]
    slots = tuple(_slot_register(x, True) for x in xs)
    if stacked:
        return _ConvBiasGroup.apply(len(xs), pad, relu, slots + ("stacked",), *xs, *weights, *biases)
    return list(_ConvBiasGroup.apply(len(xs), pad, relu, slots, *xs, *weights, *biases))


# --------------------------------------------------------------------------
# pooling / FPN top-down
# --------------------------------------------------------------------------
class _Pool2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, window, slot=(None, 0)):
        ctx.slot = slot
        _need_cuda(x, "pool input")
        N, H, W, C = x.shape
        y = torch.empty((N, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
        _lib.call("cr_pool2x_fwd", x, y, N, H, W, C, window, _af(x))
        ctx.window = window
        ctx.save_for_backward(x)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        N, H, W, C = x.shape
        xslot, xi = ctx.slot
        if dy is None:
            # every consumer of the pooled map handed its gradient on through gradient slots: nothing arrives here
            if xslot is None:
                return None, None, None
            if xi > 1:
                return None, None, None                      # what the slot holds stays for the accumulating consumer
            acc = _slot_take(xslot)
            return (None if acc is None else acc.to(x.dtype)), None, None
        dx = torch.empty_like(x)
        dy = dy.to(x.dtype).contiguous()
        # the FIRST registered consumer of x (DLA: a level's input is pooled before its first convolution sees it) collects
        # what the others left in the slot, a later one folds the slot's content into its own result: added in the kernel
        acc = None if xslot is None else (_slot_take(xslot) if xi <= 1 else _slot_fold(xslot))
        acc = None if acc is None else acc.to(x.dtype).contiguous()
        _lib.call("cr_pool2x_bwd", x, dy, dx, N, H, W, C, ctx.window, _af(x), acc)
        if xslot is not None and xi > 1:
            _slot_put(xslot, dx)
            dx = None
        return dx, None, None


class _Pool3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _need_cuda(x, "pool input")
        N, H, W, C = x.shape
        y = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=x.dtype, device=x.device)
        _lib.call("cr_maxpool3x3s2_fwd", x, y, N, H, W, C, _af(x))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        N, H, W, C = x.shape
        dx = torch.empty_like(x)
        dy = dy.to(x.dtype).contiguous()
        _lib.call("cr_maxpool3x3s2_bwd", x, dy, dx, N, H, W, C, _af(x))
        return dx


def maxpool3x3s2(x):
    """nn.MaxPool2d(3, stride=2, padding=1) -- the torchvision ResNet stem (resnet.py:33,49)."""
    return _Pool3s2.apply(x)


def maxpool2x2(x):
    """nn.MaxPool2d(2, stride=2) -- dla.py:208."""
    return _Pool2x.apply(x, 2, _slot_register(x, True))


def subsample2x(x):
    """F.max_pool2d(kernel_size=1, stride=2) -- dla.py:474."""
    return _Pool2x.apply(x, 1, _slot_register(x, True))


# --------------------------------------------------------------------------
# DenseNet (csrc/densenet.hip): a dense block as ONE autograd Function over a shared feature buffer, BatchNorm + ReLU on a
# channel slice of it, average pooling.  None of these takes part in the gradient-slot protocol: a block output that also feeds
# an FPN lateral gets its two gradients added by autograd.
# --------------------------------------------------------------------------
class _AvgPool2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _need_cuda(x, "pool input")
        N, H, W, C = x.shape
        y = torch.empty((N, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
        _lib.call("cr_avgpool2x2_fwd", x.contiguous(), y, N, H, W, C, _af(x))
        ctx.shape = (N, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
        _lib.call("cr_avgpool2x2_bwd", dy, dx, N, H, W, C, _af(dy))
        return dx


def avgpool2x2(x):
    """nn.AvgPool2d(kernel_size=2, stride=2) -- torchvision's DenseNet transitions; H and W must be even."""
    return _AvgPool2x2.apply(x)


def dense_stats(X, c0, C, tab, tab_off, eps):
    """batch mean | biased variance | inverse std of the stored values X[..., c0 : c0 + C] -> tab[:, tab_off : tab_off + C]"""
    ld = X.shape[-1]
    ws = torch.empty((256 * 2 * C,), dtype=f32, device=X.device)
    _lib.call("cr_dense_stats", X, X.numel() // ld, ld, c0, C, tab, tab.shape[1], tab_off, float(eps), ws, _af(X))


def dense_slice_store(src, X, c0):
    """X[..., c0 : c0 + C] = src (contiguous, C channels)"""
    ld, C = X.shape[-1], src.shape[-1]
    assert src.dtype == X.dtype and src.is_contiguous() and X.is_contiguous() and src.numel() // C == X.numel() // ld
    _lib.call("cr_dense_slice_store", src, X, X.numel() // ld, ld, c0, C, _af(X))


def dense_slice_gather(G, c0, C, dtype):
    """G[..., c0 : c0 + C] of the float32 gradient buffer as a contiguous tensor of the activation dtype"""
    assert G.dtype == f32 and G.is_contiguous()
    ld = G.shape[-1]
    out = torch.empty(tuple(G.shape[:-1]) + (C,), dtype=dtype, device=G.device)
    _lib.call("cr_dense_slice_gather", G, G.numel() // ld, ld, c0, C, out, _af(out))
    return out


def dense_bn_fwd(X, C, tab, bn, gamma, beta, relu, batch):
    """act(BatchNorm(X[..., :C])) contiguous; batch: statistics from tab and bn's running statistics updated, else bn's
    running statistics.  gamma / beta: bn's weight / bias as the caller's autograd inputs"""
    _need_cuda(X, "BatchNorm input")
    ld = X.shape[-1]
    out = torch.empty(tuple(X.shape[:-1]) + (C,), dtype=X.dtype, device=X.device)
    _lib.call("cr_dense_bn_fwd", X, X.numel() // ld, ld, C, tab if batch else None, tab.shape[1] if batch else 0,
              gamma.detach(), beta.detach(), bn.running_mean, bn.running_var, float(bn.eps), float(bn.momentum),
              int(batch), int(relu), out, _af(X))
    return out


def dense_bn_bwd(da, X, C, tab, bn, gamma, beta, relu, batch, G, accumulate):
    """adds (accumulate) or writes the gradient of dense_bn_fwd's input into G[..., :C]; -> (dgamma, dbeta), each None when
    the parameter's gradient sink took it"""
    gs, bs = grad_sink(gamma), grad_sink(beta)
    if gs is not None and bs is not None:
        dgamma, dbeta, ret_g, ret_b = gs, bs, None, None
    else:
        dgamma = torch.zeros((C,), dtype=f32, device=X.device)
        dbeta = torch.zeros((C,), dtype=f32, device=X.device)
        ret_g, ret_b = dgamma, dbeta
    ld = X.shape[-1]
    ws = torch.empty((257 * 2 * C,), dtype=f32, device=X.device)
    _lib.call("cr_dense_bn_bwd", da, X, X.numel() // ld, ld, C, tab if batch else None, tab.shape[1] if batch else 0,
              gamma.detach(), beta.detach(), bn.running_mean, bn.running_var, float(bn.eps), int(batch), int(relu), G,
              G.shape[-1], int(accumulate), dgamma, dbeta, ws, _af(X))
    return ret_g, ret_b


class _DenseBlock(torch.autograd.Function):
    """torchvision's _DenseBlock.  Per layer: slice BatchNorm + ReLU (cr_dense_bn_fwd) -> conv1 + norm2 + ReLU through
    conv_bn_act, run as a small nested autograd graph (train, frozen and folded-eval forms are _ConvBN's / conv_bn_folded's own)
    -> conv2 through conv_fwd_raw with statistics rows -> slice store + finalize.  The backward walks the layers in reverse over
    ONE float32 gradient buffer: by the time layer i's 32 channels are gathered, every later layer has added into them."""
    PER_LAYER = 6           # norm1.weight, norm1.bias, conv1.weight, norm2.weight, norm2.bias, conv2.weight

    @staticmethod
    def forward(ctx, x0, layers, *params):
        _need_cuda(x0, "dense block input")
        N, H, W, C0 = x0.shape
        L, growth = len(layers), layers[0].conv2.weight.shape[0]
        Ctot, M, dev = C0 + growth * L, N * H * W, x0.device
        batch = bool(layers[0].norm1.training)
        assert all(bool(l.norm1.training) == batch for l in layers), "a dense block's BatchNorms must share one mode"
        grad = any(ctx.needs_input_grad)
        X = torch.empty((N, H, W, Ctot), dtype=x0.dtype, device=dev)
        dense_slice_store(x0.contiguous(), X, 0)
        if batch:
            _STATS_EPOCH[0] += 1
            tab = torch.empty((3, Ctot), dtype=f32, device=dev)
            dense_stats(X, 0, C0, tab, 0, layers[0].norm1.eps)
            nparts = (M + 63) // 64
        else:
            tab = torch.zeros((3, Ctot), dtype=f32, device=dev)
        saved = []
        for i, layer in enumerate(layers):
            C = C0 + growth * i
            g1, b1, w1, g2, b2, w2 = params[6 * i:6 * i + 6]       # the autograd inputs: the backward asks for THESE tensors
            n2 = layer.norm2
            a = dense_bn_fwd(X, C, tab, layer.norm1, g1, b1, True, batch)
            if grad:
                a.requires_grad_(True)
            with torch.set_grad_enabled(grad):
                h = conv_bn_act(a, w1, g2, b2, n2.running_mean, n2.running_var, stride=1, pad=0, relu=True,
                                eps=n2.eps, momentum=n2.momentum, training=n2.training)
            wb, _ = prepared_weights(w2, grad, x0.dtype)
            stats = torch.empty((nparts, 2, growth), dtype=f32, device=dev) if batch else None
            y = conv_fwd_raw(h.detach(), wb, growth, 3, 1, 1, stats=stats)
            dense_slice_store(y, X, C)
            if batch:
                _lib.call("cr_dense_stats_finalize", stats, nparts, growth, M, tab, Ctot, C, float(layer.norm1.eps))
            if grad:
                saved.append((a, h, g1, b1, w1, g2, b2, w2))
        if grad:
            ctx.layers, ctx.inner, ctx.cfg = layers, saved, (C0, growth, batch)
            ctx.save_for_backward(X, tab)
        ctx.mark_non_differentiable(tab)
        return X, tab

    @staticmethod
    def backward(ctx, dX, _dtab):
        X, tab = ctx.saved_tensors
        layers, inner = ctx.layers, ctx.inner
        C0, growth, batch = ctx.cfg
        G = torch.empty(X.shape, dtype=f32, device=X.device)
        G.copy_(dX)
        grads = [None] * (_DenseBlock.PER_LAYER * len(layers))
        for i in reversed(range(len(layers))):
            layer, (a, h, g1, b1, w1, g2, b2, w2) = layers[i], inner[i]
            inner[i] = None                                    # this layer's activations die with the iteration
            C = C0 + growth * i
            dy = dense_slice_gather(G, C, growth, X.dtype)
            hd = h.detach()
            _, wt = prepared_weights(w2, True, X.dtype)
            dh = conv_bwd_data_raw(dy, wt, hd.shape, 3, 1, 1)
            if ctx.needs_input_grad[2 + 6 * i + 5]:
                grads[6 * i + 5] = conv_bwd_weight_raw(dy, hd, 3, 1, 1, grad_sink(w2))
            wanted = [(k, t) for k, t in ((2, w1), (3, g2), (4, b2)) if ctx.needs_input_grad[2 + 6 * i + k]]
            got = torch.autograd.grad([h], [a] + [t for _, t in wanted], [dh], allow_unused=True)
            for (k, _), g in zip(wanted, got[1:]):
                grads[6 * i + k] = g
            da = got[0].to(X.dtype).contiguous()
            dg, db = dense_bn_bwd(da, X, C, tab, layer.norm1, g1, b1, True, batch, G, True)
            if ctx.needs_input_grad[2 + 6 * i]:
                grads[6 * i] = dg
            if ctx.needs_input_grad[2 + 6 * i + 1]:
                grads[6 * i + 1] = db
        dx0 = dense_slice_gather(G, 0, C0, X.dtype) if ctx.needs_input_grad[0] else None
        ctx.inner = None
        return (dx0, None) + tuple(grads)


def dense_block(x0, layers):
    """x0 (N,H,W,C0) -> (X (N,H,W,C0 + 32 L), tab (3, C0 + 32 L) f32, not differentiable).  layers: modules with norm1, conv1
    (1x1), norm2, conv2 (3x3, pad 1) as parameter containers.  tab holds the batch statistics of every channel of X in train
    mode (bn_act reuses it) and zeros in running-statistics mode."""
    params = []
    for l in layers:
        params += [l.norm1.weight, l.norm1.bias, as_krsc(l.conv1.weight), l.norm2.weight, l.norm2.bias, as_krsc(l.conv2.weight)]
    return _DenseBlock.apply(x0, tuple(layers), *params)


class _BNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, bn, relu, tab):
        _need_cuda(x, "BatchNorm input")
        C = x.shape[-1]
        x = x.contiguous()
        batch = bool(bn.training)
        if batch:
            _STATS_EPOCH[0] += 1
            if tab is None:
                tab = torch.empty((3, C), dtype=f32, device=x.device)
                dense_stats(x, 0, C, tab, 0, bn.eps)
        out = dense_bn_fwd(x, C, tab, bn, gamma, beta, relu, batch)
        ctx.bn, ctx.cfg, ctx.affine = bn, (relu, batch), (gamma, beta)
        ctx.save_for_backward(x, tab if batch else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, tab = ctx.saved_tensors
        relu, batch = ctx.cfg
        G = torch.empty(x.shape, dtype=f32, device=x.device)
        dg, db = dense_bn_bwd(dout.to(x.dtype).contiguous(), x, x.shape[-1], tab, ctx.bn, *ctx.affine, relu, batch, G, False)
        dx = G if x.dtype == f32 else dense_slice_gather(G, 0, x.shape[-1], x.dtype)
        return (dx if ctx.needs_input_grad[0] else None, dg if ctx.needs_input_grad[1] else None,
                db if ctx.needs_input_grad[2] else None, None, None, None)


def bn_act(x, bn, relu, stats=None):
    """BatchNorm2d (+ ReLU) of a whole NHWC map that no convolution precedes (DenseNet's transition norm and norm5): the slice
    kernels at full width.  stats: the (3, C) table a dense_block returned for x, or None (computed here in train mode)."""
    return _BNAct.apply(x, bn.weight, bn.bias, bn, relu, stats)


# --------------------------------------------------------------------------
# ShuffleNetV2 (csrc/shufflenet.hip): depthwise 3x3 convolution + BatchNorm, the unit tail (concat + channel shuffle in one
# pass) and zero-padded compute copies of the parameters.  The trunk's activations live in a PADDED physical NHWC layout
# (every branch width rounded up to a power of two, a two-half tensor stored as [half 0 | pad | half 1 | pad]) so that the
# pointwise convolutions and BatchNorms run on the existing kernels; parameters, state dict and optimizer keep their logical
# shapes.  Pad rows / columns / gamma / beta are exactly zero, so pad channels stay exactly zero forward and backward.
# --------------------------------------------------------------------------
def _dw_out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def dwconv3x3_fwd_raw(x, w, stride, bias=None, stats=None):
    """x NHWC f32 / bf16, w f32 with C * 9 elements in (C, 3, 3) order; stats: f32 [ceil(M/64)][2][C] rows for cr_bn_fwd"""
    _need_cuda(x, "conv input")
    assert x.is_contiguous() and x.dim() == 4 and w.dtype == f32
    N, H, W, C = x.shape
    Ho, Wo = _dw_out_hw(H, W, stride) if stride in (1, 2) else (H, W)
    assert w.numel() == C * 9 and (bias is None or (bias.dtype == f32 and bias.numel() == C))
    assert stats is None or (stats.dtype == f32 and stats.numel() >= (N * Ho * Wo + 63) // 64 * 2 * C)
    y = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    _lib.call("cr_dwconv3x3_fwd", x, w, y, N, H, W, C, stride, bias, stats, _af(x))
    return y


def dwconv3x3_bwd_data_raw(dy, w, in_shape, stride, accumulate=None):
    """accumulate: as for conv_bwd_data_raw"""
    N, H, W, C = in_shape
    assert w.dtype == f32 and dy.is_contiguous() and w.numel() == C * 9
    assert tuple(dy.shape) == (N,) + _dw_out_hw(H, W, stride) + (C,), "dy does not have the output's shape"
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    if accumulate is not None:
        assert tuple(accumulate.shape) == (N, H, W, C), "accumulate must have the input's shape"
        accumulate = accumulate.to(dy.dtype).contiguous()
    _lib.call("cr_dwconv3x3_bwd_data", dy, w, dx, N, H, W, C, stride, _af(dy), accumulate)
    return dx


def dw_wgrad_splits(M):
    """pixel ranges of cr_dwconv3x3_bwd_weight (include/cr3dod.h): its workspace holds splits * C * 9 floats"""
    rng = max(64, -(-M // 128))
    return -(-M // rng)


def dwconv3x3_bwd_weight_raw(dy, x, stride, sink=None):
    """dW (C, 3, 3) f32, or added into `sink` (C * 9 floats) when given"""
    N, H, W, C = x.shape
    assert dy.dtype == x.dtype and dy.is_contiguous() and x.is_contiguous()
    assert tuple(dy.shape) == (N,) + _dw_out_hw(H, W, stride) + (C,), "dy does not have the output's shape"
    assert sink is None or (sink.dtype == f32 and sink.numel() == C * 9)
    n_ws = dw_wgrad_splits(dy.shape[0] * dy.shape[1] * dy.shape[2]) * C * 9
    ws = torch.empty((n_ws,), dtype=f32, device=x.device)
    dw = sink if sink is not None else torch.empty((C, 3, 3), dtype=f32, device=x.device)
    _lib.call("cr_dwconv3x3_bwd_weight", dy, x, dw, N, H, W, C, stride, int(sink is not None), _af(x), ws, n_ws)
    return None if sink is not None else dw


class _DwBN(torch.autograd.Function):
    """depthwise 3x3 convolution + BatchNorm2d without a ReLU (every depthwise convolution of ShuffleNetV2): the structure of
    _ConvBN -- train mode: statistics rows from the convolution, cr_bn_fwd / cr_bn_bwd; frozen statistics: the BatchNorm folded
    into the nine taps (cr_fold_bn on the (C, 9) weight, made on every call from the live parameters) and cr_bn_frozen_unfold
    in the backward."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var, stride, eps, momentum, training, slot=(None, 0)):
        ctx.slot = slot
        C = x.shape[3]
        dev = x.device
        if training:
            _STATS_EPOCH[0] += 1
            Ho, Wo = _dw_out_hw(x.shape[1], x.shape[2], stride)
            M = x.shape[0] * Ho * Wo
            nparts = (M + 63) // 64
            stats = torch.empty((nparts, 2, C), dtype=f32, device=dev)
            y_raw = dwconv3x3_fwd_raw(x, weight.detach(), stride, stats=stats)
            out = torch.empty_like(y_raw)
            mi = torch.empty((2, C), dtype=f32, device=dev)
            _lib.call("cr_bn_fwd", y_raw, stats, nparts, gamma.detach(), beta.detach(), None, out, M, C, 0, float(eps),
                      float(momentum), mi, running_mean, running_var, _af(x))
        else:
            wf32 = torch.empty((C, 9), dtype=f32, device=dev)
            bias_f = torch.empty((C,), dtype=f32, device=dev)
            _lib.call("cr_fold_bn", weight.detach(), gamma.detach(), beta.detach(), running_mean, running_var, float(eps), wf32,
                      bias_f, C, 9, 1)
            out = dwconv3x3_fwd_raw(x, wf32, stride, bias=bias_f)
            y_raw, mi = wf32, None
            ctx.frozen = (running_mean, running_var, float(eps))
        ctx.cfg = (stride, training)
        ctx.beta_ref = beta
        ctx.save_for_backward(x, weight, gamma, y_raw, mi)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, gamma, y_raw, mi = ctx.saved_tensors
        stride, training = ctx.cfg
        C = x.shape[3]
        dev = x.device
        dout = dout.to(x.dtype).contiguous()
        gs, bs = grad_sink(gamma), grad_sink(ctx.beta_ref)
        if gs is not None and bs is not None:
            dgamma, dbeta, ret_g, ret_b = gs, bs, None, None
        else:
            dgamma = torch.zeros((C,), dtype=f32, device=dev)
            dbeta = torch.zeros((C,), dtype=f32, device=dev)
            ret_g, ret_b = dgamma, dbeta
        need_dw = ctx.needs_input_grad[1]
        wsink = grad_sink(weight) if need_dw else None
        dw = None
        if training:
            M = y_raw.numel() // C
            sums = torch.empty((1025, 2, C), dtype=f32, device=dev)
            g = torch.empty_like(y_raw)
            _lib.call("cr_bn_bwd", dout, None, y_raw, mi, gamma.detach(), sums, g, None, dgamma, dbeta, M, C, 0, _af(x))
            w_bwd = weight.detach()
            if need_dw:
                dw = dwconv3x3_bwd_weight_raw(g, x, stride, wsink)
        else:
            running_mean, running_var, eps = ctx.frozen
            g, w_bwd = dout, y_raw                           # y_raw: the folded taps
            M = g.numel() // C
            sg = torch.zeros((C,), dtype=f32, device=dev)
            ws = torch.empty((1024, C), dtype=f32, device=dev)
            _lib.call("cr_colsum_accum", g, int(g.dtype == f32), M, C, ws, sg)
            dwf = dwconv3x3_bwd_weight_raw(g, x, stride)
            if need_dw and wsink is None:
                dw = dwf                                    # scaled in place
            dst = wsink if wsink is not None else dw
            _lib.call("cr_bn_frozen_unfold", dwf, sg, weight.detach(), gamma.detach(), running_mean, running_var, eps, dst,
                      int(wsink is not None), dgamma, dbeta, C, 9)
        dx = None
        xslot, xi = ctx.slot
        if ctx.needs_input_grad[0]:
            if xslot is not None and xi > 1:                # not the first consumer of x: leave the contribution in the slot
                _slot_put(xslot, dwconv3x3_bwd_data_raw(g, w_bwd, x.shape, stride, accumulate=_slot_fold(xslot)))
            else:
                dx = dwconv3x3_bwd_data_raw(g, w_bwd, x.shape, stride,
                                            accumulate=_slot_take(xslot) if xslot is not None else None)
        elif xslot is not None:
            raise RuntimeError("gradient slot registered for an input that needs no gradient")
        if dw is not None:
            dw = dw.view(weight.shape)
        return dx, dw, ret_g, ret_b, None, None, None, None, None, None, None


def dwconv_bn(x, weight, gamma, beta, running_mean, running_var, stride=1, eps=1e-5, momentum=0.1, training=True):
    """BatchNorm(depthwise_conv3x3(x)); weight: f32, C * 9 elements in (C, 3, 3) order (a (C,1,3,3) parameter or a padded
    (C, 9) compute copy)"""
    _need_cuda(x, "conv input")
    return _DwBN.apply(x, weight, gamma, beta, running_mean, running_var, stride, eps, momentum, bool(training),
                       _slot_register(x, False))


def conv_bn_act_live(x, weight, gamma, beta, running_mean, running_var, stride=1, pad=0, relu=True, eps=1e-5, momentum=0.1,
                     training=True, residual=None, wide_sums=False):
    """conv_bn_act without the inference fold cache: with frozen statistics the fold is made on every call from the tensors
    handed in.  For compute copies that a kernel rewrites in place (PaddedPack) -- their version counters never move.
    residual: added in the BatchNorm pass (train) or the convolution's epilogue (frozen); its gradient goes through the
    gradient slot of the tensor when that tensor's first consumer was a convolution.  wide_sums: the backward forms its
    per-channel sums with cr_bn_bwd_anyc / cr_colsum_wide (added across threads in double) at every width instead of
    cr_bn_bwd / the weight gradient's bias sum, which add a block's rows one after the other in float32."""
    xs = _slot_register(x, True)
    rs = _slot_register(residual, False) if residual is not None else (None, 0)
    return _ConvBN.apply(x, as_krsc(weight), gamma, beta, residual, running_mean, running_var, stride, pad, relu, eps, momentum,
                         bool(training), (xs, rs), 1, bool(wide_sums))


class _ShuffleTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, bf, slot=(None, 0)):
        N, H, W, wp = b.shape
        assert a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype and tuple(a.shape[:3]) == (N, H, W)
        y = torch.empty((N, H, W, 2 * wp), dtype=b.dtype, device=b.device)
        _lib.call("cr_shuffle_tail_fwd", a, a.shape[3], b, y, N * H * W, bf, wp, _af(b))
        ctx.cfg = (bf, a.shape[3], slot)
        return y

    @staticmethod
    def backward(ctx, dy):
        bf, aw, (slot, si) = ctx.cfg
        dy = dy.contiguous()
        N, H, W, wp2 = dy.shape
        da = torch.empty((N, H, W, aw), dtype=dy.dtype, device=dy.device)
        db = torch.empty((N, H, W, wp2 // 2), dtype=dy.dtype, device=dy.device)
        _lib.call("cr_shuffle_tail_bwd", dy, da, aw, db, N * H * W, bf, wp2 // 2, _af(dy))
        if slot is not None:                                # the unit input's first consumer (a convolution) adds this
            _slot_put(slot, da)
            da = None
        return da, db, None, None


def shuffle_tail(a, b, bf):
    """channel_shuffle(cat(a[..., :bf], b[..., :bf]), 2) of a ShuffleNetV2 unit in one pass -> (N, H, W, 2 * wp) in the
    two-half layout, pads zero.  a: the other branch (N, H, W, wp), or the unit's input (N, H, W, 2 * wp) whose first half
    passes through; b (N, H, W, wp).  The gradient of a is zero beyond its first bf channels."""
    _need_cuda(b, "unit tail input")
    return _ShuffleTail.apply(a, b, bf, _slot_register(a, False))


class _PackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pack, *tensors):
        ctx.set_materialize_grads(False)
        ctx.pack = pack
        outs = pack._forward(tensors, any(ctx.needs_input_grad))
        ctx.gflat, ctx.srcs = pack._gflat, tensors
        ctx.mark_non_differentiable(*[o for o, e in zip(outs, pack.entries) if not e["grad"]])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        return (None,) + tuple(ctx.pack._backward(ctx.gflat, ctx.srcs, grads, ctx.needs_input_grad[1:]))


class PaddedPack:
    """Zero-padded float32 compute copies of a set of parameters / buffers, made by ONE launch (cr_padded_pack) on every call
    of run() -- inside a captured graph it is a node of the graph, so replays follow the optimizer -- and their gradients
    gathered back by one launch.

    entries: dicts {"get": callable -> logical tensor, "rows": (halves, wl, wp), "cols": (halves, wl, wp[, leading halves that
    are pads altogether and have no logical columns]), "shape": shape of
    the padded view, "perm": optional permutation applied to it, "grad": bool, "T": bool (also the transposed copy, seeded as
    the f32 backward-data layout of a 1x1 convolution)}; the logical tensor is a (halves_r * wl_r, halves_c * wl_c) matrix
    in memory (include/cr3dod.h, cr_pdesc).  run() -> the padded tensors.  With gradients enabled every padded tensor of a "grad" entry carries a
    gradient sink (grad_sink) in a zeroed flat buffer; the pack's backward -- autograd runs it after every consumer --
    adds the logical part of that buffer into the logical tensors' own sinks (or returns it where they have none)."""

    def __init__(self, entries):
        self.entries = list(entries)
        off = offT = 0
        self.offs = []
        for e in self.entries:
            rp, cp = e["rows"][0] * e["rows"][2], e["cols"][0] * e["cols"][2]
            self.offs.append((off, offT if e.get("T") else -1, rp, cp))
            off += (rp * cp + 3) // 4 * 4
            if e.get("T"):
                offT += (rp * cp + 3) // 4 * 4
        self.total, self.totalT = off, max(offT, 4)
        self._ptrs = self._gptrs = None
        self._gflat = None

    def _descs(self, ptrs, idx, dev):
        import numpy as np
        dt = np.dtype([("logical", "<u8"), ("phys_off", "<i8"), ("physT_off", "<i8"), ("rows_p", "<i4"), ("cols_p", "<i4"),
                       ("cols_l", "<i4"), ("row_wl", "<i4"), ("row_wp", "<i4"), ("col_wl", "<i4"), ("col_wp", "<i4"),
                       ("col_skip", "<i4")])
        assert dt.itemsize == 56
        recs = []
        for i, ptr in zip(idx, ptrs):
            e, (off, offT, rp, cp) = self.entries[i], self.offs[i]
            skip = e["cols"][3] if len(e["cols"]) > 3 else 0
            recs.append((ptr, off, offT, rp, cp, (e["cols"][0] - skip) * e["cols"][1], e["rows"][1], e["rows"][2], e["cols"][1],
                         e["cols"][2], skip))
        if torch.cuda.is_current_stream_capturing():
            raise _lib.CrError("PaddedPack: the parameters moved; run the model once before capturing a graph")
        return torch.from_numpy(np.array(recs, dtype=dt).view(np.uint8).copy()).to(dev)

    def _check(self, t, e):
        n = e["rows"][0] * e["rows"][1] * (e["cols"][0] - (e["cols"][3] if len(e["cols"]) > 3 else 0)) * e["cols"][1]
        _need_cuda(t, "PaddedPack")
        if t.dtype != f32 or t.numel() != n:
            raise _lib.CrError(f"PaddedPack: expected {n} float32 elements, got {tuple(t.shape)} {t.dtype}")
        if not (t.is_contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.is_contiguous()):
            raise _lib.CrError("PaddedPack: conv weights must be channels_last, everything else contiguous")

    def run(self):
        tensors = [e["get"]() for e in self.entries]
        outs = _PackFn.apply(self, *tensors)
        gflat = self._gflat
        epoch = _WEIGHT_EPOCH[0]
        for o, e, (off, offT, rp, cp) in zip(outs, self.entries, self.offs):
            if gflat is not None and e["grad"]:
                o._cr_grad = self._view(gflat, off, rp, cp, e)
            if offT >= 0:                                   # the backward-data layout [Cin][Cout] of a 1x1 convolution (f32 modes)
                o._cr_wcache32 = [(o._version, epoch, o.data_ptr()), o.detach(), self.wT[offT:offT + rp * cp].view(cp, rp)]
        return outs

    @staticmethod
    def _view(flat, off, rp, cp, e):
        v = flat[off:off + rp * cp].view(e["shape"])
        return v.permute(e["perm"]) if e.get("perm") else v

    def _forward(self, tensors, grad):
        dev = tensors[0].device
        ptrs = tuple(t.data_ptr() for t in tensors)
        if ptrs != self._ptrs:
            for t, e in zip(tensors, self.entries):
                self._check(t, e)
            self.descs = self._descs(ptrs, range(len(ptrs)), dev)
            if getattr(self, "wflat", None) is None or self.wflat.device != dev:
                self.wflat = torch.zeros((self.total,), dtype=f32, device=dev)
                self.wT = torch.zeros((self.totalT,), dtype=f32, device=dev)
            self._ptrs = ptrs
        _lib.call("cr_padded_pack", self.descs, len(ptrs), self.wflat, self.wT, 0)
        self._gflat = torch.zeros((self.total,), dtype=f32, device=dev) if grad else None
        return [self._view(self.wflat, off, rp, cp, e) for e, (off, offT, rp, cp) in zip(self.entries, self.offs)]

    def _backward(self, gflat, srcs, grads, need):
        """-> the gradients of the logical tensors (None where they went into a sink)"""
        wgrad_flush()                                       # queued weight gradients (deferred_wgrad) target gflat
        idx = [i for i, e in enumerate(self.entries) if e["grad"] and need[i]]
        if gflat is None or not idx:
            return [None] * len(srcs)
        for i, g in enumerate(grads):                       # whatever came back through plain autograd
            if g is not None:
                off, _, rp, cp = self.offs[i]
                self._view(gflat, off, rp, cp, self.entries[i]).add_(g)
        sinks = [grad_sink(srcs[i]) for i in idx]
        ret = [None] * len(srcs)
        if any(s is None for s in sinks):
            tmp = torch.zeros((sum(srcs[i].numel() for i in idx),), dtype=f32, device=gflat.device)
            o = 0
            for k, i in enumerate(idx):
                n = srcs[i].numel()
                if sinks[k] is None:
                    v = tmp[o:o + n]
                    s = srcs[i]
                    ret[i] = v.view(s.shape[0], s.shape[2], s.shape[3], s.shape[1]).permute(0, 3, 1, 2) if s.dim() == 4 \
                        else v.view(s.shape)
                    sinks[k] = ret[i]
                o += n
        gptrs = tuple(s.data_ptr() for s in sinks)
        if gptrs != self._gptrs or any(r is not None for r in ret):
            gdescs = self._descs(gptrs, idx, gflat.device)
            if all(r is None for r in ret):
                self._gptrs, self._gdescs = gptrs, gdescs
        else:
            gdescs = self._gdescs
        _lib.call("cr_padded_pack", gdescs, len(idx), gflat, None, 2)
        return ret

    def unpack(self, which):
        """logical = padded for the entries `which` (indices): the running statistics the BatchNorm kernels updated in
        their padded copies"""
        key = tuple(which)
        cache = self.__dict__.setdefault("_udescs", {})
        ent = cache.get(key)
        if ent is None or ent[0] is not self._ptrs:
            ent = cache[key] = (self._ptrs, self._descs([self._ptrs[i] for i in key], key, self.wflat.device))
        _lib.call("cr_padded_pack", ent[1], len(key), self.wflat, None, 1)


# --------------------------------------------------------------------------
# MNASNet (csrc/mnasnet.hip): depthwise k x k convolution (k in {3, 5}) + BatchNorm (+ ReLU), and the BatchNorm backward for
# any C % 8 == 0 (cr_bn_bwd_anyc) that the trunk's widths (48, 80, 96, 192, 240, 320, 480, 576, 1152) need:
# cr_bn_bwd / cr_bn_bwd_mask take 256 % (C / 8) == 0 only.  The trunk's activations live in the padded physical layout of the
# ShuffleNetV2 trunk with single-half maps (every width rounded up to a multiple of 16); PaddedPack makes the compute copies.
# --------------------------------------------------------------------------
def dwconv_fwd_raw(x, w, k, stride, bias=None, stats=None, relu=False):
    """x NHWC f32 / bf16, w f32 with C * k * k elements in (C, k, k) order; stats: f32 [ceil(M/64)][2][C] rows for cr_bn_fwd"""
    _need_cuda(x, "conv input")
    assert x.is_contiguous() and x.dim() == 4 and w.dtype == f32
    N, H, W, C = x.shape
    Ho, Wo = _dw_out_hw(H, W, stride) if stride in (1, 2) else (H, W)
    assert w.numel() == C * k * k and (bias is None or (bias.dtype == f32 and bias.numel() == C))
    assert stats is None or (stats.dtype == f32 and stats.numel() >= (N * Ho * Wo + 63) // 64 * 2 * C)
    y = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    _lib.call("cr_dwconv_fwd", x, w, y, N, H, W, C, k, stride, bias, stats, int(relu), _af(x))
    return y


def dwconv_bwd_data_raw(dy, w, in_shape, k, stride, accumulate=None):
    """accumulate: as for conv_bwd_data_raw"""
    N, H, W, C = in_shape
    assert w.dtype == f32 and dy.is_contiguous() and w.numel() == C * k * k
    assert tuple(dy.shape) == (N,) + _dw_out_hw(H, W, stride) + (C,), "dy does not have the output's shape"
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    if accumulate is not None:
        assert tuple(accumulate.shape) == (N, H, W, C), "accumulate must have the input's shape"
        accumulate = accumulate.to(dy.dtype).contiguous()
    _lib.call("cr_dwconv_bwd_data", dy, w, dx, N, H, W, C, k, stride, _af(dy), accumulate)
    return dx


def dwconv_wgrad_ws_floats(M, C, k):
    """workspace of cr_dwconv_bwd_weight (include/cr3dod.h): splits * C * k * k floats for M output pixels"""
    return dw_wgrad_splits(M) * C * k * k


def dwconv_bwd_weight_raw(dy, x, k, stride, sink=None):
    """dW (C, k, k) f32, or added into `sink` (C * k * k floats) when given"""
    N, H, W, C = x.shape
    assert dy.dtype == x.dtype and dy.is_contiguous() and x.is_contiguous()
    assert tuple(dy.shape) == (N,) + _dw_out_hw(H, W, stride) + (C,), "dy does not have the output's shape"
    assert sink is None or (sink.dtype == f32 and sink.numel() == C * k * k)
    n_ws = dwconv_wgrad_ws_floats(dy.shape[0] * dy.shape[1] * dy.shape[2], C, k)
    ws = torch.empty((n_ws,), dtype=f32, device=x.device)
    dw = sink if sink is not None else torch.empty((C, k, k), dtype=f32, device=x.device)
    _lib.call("cr_dwconv_bwd_weight", dy, x, dw, N, H, W, C, k, stride, int(sink is not None), _af(x), ws, n_ws)
    return None if sink is not None else dw


def bn_needs_anyc(C):
    """whether a BatchNorm over C channels is beyond cr_bn_bwd / cr_bn_bwd_mask (256 % (C / 8) == 0) -> cr_bn_bwd_anyc"""
    return C % 8 != 0 or 256 % (C >> 3) != 0


def bn_bwd_anyc_raw(dy, out, x, mean_invstd, gamma, beta, relu, dgamma, dbeta):
    """-> dx; dgamma / dbeta (f32 [C]) are accumulated.  out None with relu: the mask is recomputed from x"""
    C = x.shape[-1]
    M = x.numel() // C
    assert dy.dtype == x.dtype and dy.is_contiguous() and x.is_contiguous() and dy.shape == x.shape
    assert out is None or (out.dtype == x.dtype and out.is_contiguous() and out.shape == x.shape)
    assert dgamma.dtype == f32 and dbeta.dtype == f32 and dgamma.numel() == C == dbeta.numel()
    ws = torch.empty((256, 2, C), dtype=f32, device=x.device)
    dx = torch.empty_like(x)
    _lib.call("cr_bn_bwd_anyc", dy, out, x, mean_invstd, gamma, beta, ws, dx, dgamma, dbeta, M, C, int(relu), _af(x))
    return dx


def colsum_wide_raw(x, out):
    """out[c] += sum over all leading dimensions of x[..., c]; out f32 [C]"""
    C = x.shape[-1]
    assert x.is_contiguous() and out.dtype == f32 and out.numel() == C
    ws = torch.empty((256, C), dtype=f32, device=x.device)
    _lib.call("cr_colsum_wide", x, x.numel() // C, C, ws, out, _af(x))


class _DwBNAct(torch.autograd.Function):
    """depthwise k x k convolution + BatchNorm2d (+ ReLU), the structure of _DwBN -- train mode: statistics rows from the
    convolution, cr_bn_fwd with its ReLU flag, cr_bn_bwd_anyc with the mask from the raw convolution output; frozen
    statistics: the BatchNorm folded into the k * k taps (cr_fold_bn on the (C, k * k) weight, made on every call from the live
    parameters), the ReLU in the convolution's epilogue, its mask from the stored output and cr_bn_frozen_unfold in the
    backward."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var, k, stride, relu, eps, momentum, training,
                slot=(None, 0)):
        ctx.slot = slot
        C = x.shape[3]
        dev = x.device
        kk = k * k
        if training:
            _STATS_EPOCH[0] += 1
            Ho, Wo = _dw_out_hw(x.shape[1], x.shape[2], stride)
            M = x.shape[0] * Ho * Wo
            nparts = (M + 63) // 64
            stats = torch.empty((nparts, 2, C), dtype=f32, device=dev)
            y_raw = dwconv_fwd_raw(x, weight.detach(), k, stride, stats=stats)
            out = torch.empty_like(y_raw)
            mi = torch.empty((2, C), dtype=f32, device=dev)
            _lib.call("cr_bn_fwd", y_raw, stats, nparts, gamma.detach(), beta.detach(), None, out, M, C, int(relu), float(eps),
                      float(momentum), mi, running_mean, running_var, _af(x))
            keep = None
        else:
            wf32 = torch.empty((C, kk), dtype=f32, device=dev)
            bias_f = torch.empty((C,), dtype=f32, device=dev)
            _lib.call("cr_fold_bn", weight.detach(), gamma.detach(), beta.detach(), running_mean, running_var, float(eps), wf32,
                      bias_f, C, kk, 1)
            out = dwconv_fwd_raw(x, wf32, k, stride, bias=bias_f, relu=relu)
            y_raw, mi = wf32, None
            keep = out if relu else None
            ctx.frozen = (running_mean, running_var, float(eps))
        ctx.cfg = (k, stride, relu, training)
        ctx.beta_ref = beta
        ctx.save_for_backward(x, weight, gamma, y_raw, mi, keep)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, gamma, y_raw, mi, out = ctx.saved_tensors
        k, stride, relu, training = ctx.cfg
        C = x.shape[3]
        dev = x.device
        dout = dout.to(x.dtype).contiguous()
        gs, bs = grad_sink(gamma), grad_sink(ctx.beta_ref)
        if gs is not None and bs is not None:
            dgamma, dbeta, ret_g, ret_b = gs, bs, None, None
        else:
            dgamma = torch.zeros((C,), dtype=f32, device=dev)
            dbeta = torch.zeros((C,), dtype=f32, device=dev)
            ret_g, ret_b = dgamma, dbeta
        need_dw = ctx.needs_input_grad[1]
        wsink = grad_sink(weight) if need_dw else None
        dw = None
        if training:
            g = bn_bwd_anyc_raw(dout, None, y_raw, mi, gamma.detach(), ctx.beta_ref.detach(), relu, dgamma, dbeta)
            w_bwd = weight.detach()
            if need_dw:
                dw = dwconv_bwd_weight_raw(g, x, k, stride, wsink)
        else:
            running_mean, running_var, eps = ctx.frozen
            g = relu_bwd(out, dout) if relu else dout
            w_bwd = y_raw                                   # the folded taps
            sg = torch.zeros((C,), dtype=f32, device=dev)
            colsum_wide_raw(g, sg)
            dwf = dwconv_bwd_weight_raw(g, x, k, stride)
            if need_dw and wsink is None:
                dw = dwf                                    # scaled in place
            dst = wsink if wsink is not None else dw
            _lib.call("cr_bn_frozen_unfold", dwf, sg, weight.detach(), gamma.detach(), running_mean, running_var, eps, dst,
                      int(wsink is not None), dgamma, dbeta, C, k * k)
        dx = None
        xslot, xi = ctx.slot
        if ctx.needs_input_grad[0]:
            if xslot is not None and xi > 1:                # not the first consumer of x: leave the contribution in the slot
                _slot_put(xslot, dwconv_bwd_data_raw(g, w_bwd, x.shape, k, stride, accumulate=_slot_fold(xslot)))
            else:
                dx = dwconv_bwd_data_raw(g, w_bwd, x.shape, k, stride,
                                         accumulate=_slot_take(xslot) if xslot is not None else None)
        elif xslot is not None:
            raise RuntimeError("gradient slot registered for an input that needs no gradient")
        if dw is not None:
            dw = dw.view(weight.shape)
        return dx, dw, ret_g, ret_b, None, None, None, None, None, None, None, None, None


def dwconv_bn_act(x, weight, gamma, beta, running_mean, running_var, k=3, stride=1, relu=True, eps=1e-5, momentum=0.1,
                  training=True):
    """relu?(BatchNorm(depthwise_conv k x k(x))), pad k // 2; weight: f32, C * k * k elements in (C, k, k) order (a (C,1,k,k)
    parameter or a padded (C, k * k) compute copy)"""
    _need_cuda(x, "conv input")
    return _DwBNAct.apply(x, weight, gamma, beta, running_mean, running_var, int(k), int(stride), bool(relu), eps, momentum,
                          bool(training), _slot_register(x, False))


class _UpsampleAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lat, top, slot=(None, 0)):
        ctx.slot = slot
        _need_cuda(lat, "upsample_add input")
        N, H, W, C = lat.shape
        assert tuple(top.shape) == (N, H // 2, W // 2, C)
        y = torch.empty_like(lat)
        assert lat.dtype == top.dtype
        _lib.call("cr_upsample2x_add", lat, top, y, N, H, W, C, _af(lat))
        ctx.shape = (N, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = ctx.shape
        dy = dy.contiguous()
        dtop = torch.empty((N, H // 2, W // 2, C), dtype=dy.dtype, device=dy.device)
        _lib.call("cr_sum2x2", dy, dtop, N, H, W, C, _af(dy))
        tslot, ti = ctx.slot
        if tslot is not None:                                # the coarser level's output convolution adds this (see _GradSlot)
            _slot_put(tslot, dtop)
            dtop = None
        return dy, dtop, None


def upsample2x_add(lat, top):
    """detectron2 FPN top-down step: lateral + F.interpolate(top, scale_factor=2, mode='nearest')."""
    return _UpsampleAdd.apply(lat, top, _slot_register(top, False))


def preprocess(images_u8, mean, std, dtype=None):
    """(N,3,H,W) uint8 -> normalised NHWC with 8 (bf16) or 4 (f32) channels (3 real + zeros) in the activation dtype of the process
    (set_precision) unless `dtype` says otherwise: this call decides the precision of everything downstream."""
    _need_cuda(images_u8, "images")
    assert images_u8.dtype == torch.uint8 and images_u8.is_contiguous()
    N, _, H, W = images_u8.shape
    dt = dtype if dtype is not None else act_dtype()
    y = torch.empty((N, H, W, 8 if dt == bf16 else 4), dtype=dt, device=images_u8.device)     # one 16-B chunk per pixel
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _lib.call("cr_preprocess", images_u8, y, N, H, W, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), _af(y))
    return y


# --------------------------------------------------------------------------
# ROIAlign over the FPN pyramid
# --------------------------------------------------------------------------
def _pyr_args(feats, scales):
    n = len(feats)
    ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in feats])
    Hs = (ctypes.c_int * n)(*[f.shape[1] for f in feats])
    Ws = (ctypes.c_int * n)(*[f.shape[2] for f in feats])
    sc = (ctypes.c_float * n)(*[float(s) for s in scales])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    return n, ptrs, Hs, Ws, sc, cast


_ROI_BWD_TILES = [os.environ.get("CR_ROI_BWD_TILES", "1") == "1"]
POOLER_TYPES = ("ROIAlignV2", "ROIAlign", "ROIPool")       # codes 0, 1, 2 of cr_roi_pool_*


def pooler_type_code(pooler_type, sampling_ratio=0):
    """(POOLER_TYPE, POOLER_SAMPLING_RATIO) -> the (pool_type, sampling_ratio) codes of cr_roi_pool_*"""
    if pooler_type not in POOLER_TYPES:
        raise ValueError("POOLER_TYPE %r is not built: the built types are %s" % (pooler_type, ", ".join(POOLER_TYPES)))
    if not isinstance(sampling_ratio, int) or isinstance(sampling_ratio, bool) or sampling_ratio < 0:
        raise ValueError("POOLER_SAMPLING_RATIO %r is not built: 0 (adaptive grid) or a positive integer, with POOLER_TYPE "
                         "one of %s" % (sampling_ratio, ", ".join(POOLER_TYPES)))
    code = POOLER_TYPES.index(pooler_type)
    return code, (0 if code == 2 else int(sampling_ratio))     # ROIPool has no sampling grid


class _ROIAlign(torch.autograd.Function):
    """Where the pyramid gradient goes (backward), per level, in this order of preference:
      * a gradient slot of the level's map (the RPN head's convolution consumed it first, in the same autograd graph: its
        backward-data adds this contribution in its epilogue -- no fan-in add kernel);
      * the static gradient buffer of a captured dense region (`_cr_grad_dst` on the region's output, GraphedDense): the
        scatter lands where the backward graph reads it -- no copy;
      * a fresh zero-filled buffer returned to autograd."""

    @staticmethod
    def forward(ctx, rois, scales, out_size, slots, geo, *feats):
        _need_cuda(rois, "rois")
        C = feats[0].shape[3]
        R = rois.shape[0]
        dt = feats[0].dtype
        assert all(f.dtype == dt and f.is_contiguous() for f in feats)
        out = torch.empty((R, out_size, out_size, C), dtype=dt, device=rois.device)
        n, ptrs, Hs, Ws, sc, cast = _pyr_args(feats, scales)
        rois = rois.contiguous()
        argmax = None
        if geo == (0, 0):
            _lib.call("cr_roi_align_fwd", cast(ptrs), cast(Hs), cast(Ws), cast(sc), n, C, rois, R, out_size, out_size, out,
                      _af(out))
        else:
            # ROIPool keeps the winning pixel of every output for its backward
            argmax = torch.empty((R, out_size, out_size, C), dtype=torch.int32, device=rois.device) if geo[0] == 2 else None
            _lib.call("cr_roi_pool_fwd", cast(ptrs), cast(Hs), cast(Ws), cast(sc), n, C, int(feats[0].shape[0]), rois, R,
                      out_size, out_size, geo[0], geo[1], out, argmax, _af(out))
        ctx.geo, ctx.argmax = geo, argmax
        ctx.cfg = (scales, out_size, [tuple(f.shape) for f in feats], dt)
        ctx.slots = slots
        # claimed (popped): a second RoIAlign over the same maps takes the ordinary path and autograd adds the two
        ctx.dsts = [f.__dict__.pop("_cr_grad_dst", None) if f.requires_grad else None for f in feats]
        ctx.save_for_backward(rois)
        return out

    @staticmethod
    def backward(ctx, dout):
        (rois,) = ctx.saved_tensors
        scales, out_size, shapes, dt = ctx.cfg
        C = shapes[0][3]
        dsts = ctx.dsts
        # tile-owner kernel (cr_roi_align_bwd_set): writes every pixel of every level once, no atomics, bit-reproducible,
        # and the maps need no zero fill.  CR_ROI_BWD_TILES=0: the separable atomic kernel (A/B).
        geo = ctx.geo
        tiles = _ROI_BWD_TILES[0] and out_size == 7 and C % 64 == 0 and len({s[0] for s in shapes}) == 1 and geo[0] != 2
        if all(d is not None and d.dtype == f32 and tuple(d.shape) == tuple(s) for d, s in zip(dsts, shapes)):
            grads = dsts
            if not tiles:
                torch._foreach_zero_(grads)
        else:
            # one buffer for the whole pyramid (the levels are views of it, each 16-B aligned); zero-filled for the atomics
            sizes = [(int(s[0] * s[1] * s[2] * s[3]) + 3) // 4 * 4 for s in shapes]
            flat = (torch.empty if tiles else torch.zeros)((sum(sizes),), dtype=f32, device=rois.device)
            grads, off = [], 0
            for s, n_ in zip(shapes, sizes):
                grads.append(flat[off:off + int(s[0] * s[1] * s[2] * s[3])].view(s))
                off += n_
        n, ptrs, Hs, Ws, sc, cast = _pyr_args(grads, scales)
        dout = dout.to(dt).contiguous()
        if geo != (0, 0):
            if tiles:
                _lib.call("cr_roi_pool_bwd_set", cast(ptrs), cast(Hs), cast(Ws), cast(sc), n, C, int(shapes[0][0]), rois,
                          rois.shape[0], out_size, out_size, geo[0], geo[1], dout, _af(dout))
            else:
                _lib.call("cr_roi_pool_bwd", cast(ptrs), cast(Hs), cast(Ws), cast(sc), n, C, int(shapes[0][0]), rois,
                          rois.shape[0], out_size, out_size, geo[0], geo[1], dout, ctx.argmax, _af(dout))
        elif tiles:
            _lib.call("cr_roi_align_bwd_set", cast(ptrs), cast(Hs), cast(Ws), cast(sc), n, C, int(shapes[0][0]), rois,
                      rois.shape[0], out_size, out_size, dout, _af(dout))
        else:
            _lib.call("cr_roi_align_bwd", cast(ptrs), cast(Hs), cast(Ws), cast(sc), n, C, rois, rois.shape[0], out_size,
                      out_size, dout, _af(dout))
        res = []
        for g, (slot, _i) in zip(grads, ctx.slots):
            g = g if dt == f32 else g.to(dt)
            if slot is not None:
                _slot_put(slot, g)
                g = None
            res.append(g)
        return (None, None, None, None, None) + tuple(res)


class _SharedPrefix(torch.autograd.Function):
    """(B*S, ...) pooled RoI features -> (the same tensor, a copy of the first kf RoIs of every image).  The 3D head pools
    exactly the foreground slots the box head already pooled, so they are pooled ONCE; backward adds the 3D head's gradient
    into the box head's gradient tile in place (one small kernel) instead of scattering 20 % more RoIs with atomics."""

    @staticmethod
    def forward(ctx, pooled, B, S, kf):
        ctx.dims = (B, S, kf)
        v = pooled.view(B, S, -1)
        return pooled.view_as(pooled), v[:, :kf].reshape((B * kf,) + tuple(pooled.shape[1:]))

    @staticmethod
    def backward(ctx, g_all, g_head):
        B, S, kf = ctx.dims
        if g_all is None:
            g_all = torch.zeros((B * S,) + tuple(g_head.shape[1:]), dtype=g_head.dtype, device=g_head.device)
        g_all = g_all.contiguous()
        if g_head is not None:
            g_all.view(B, S, -1)[:, :kf] += g_head.reshape(B, kf, -1).to(g_all.dtype)
        return g_all, None, None, None


def shared_prefix(pooled, B, S, kf):
    return _SharedPrefix.apply(pooled, B, S, kf)


def roi_align_pyramid(feats, rois, scales, out_size, *, pooler_type="ROIAlignV2", sampling_ratio=0):
    """feats: list of NHWC maps (fine -> coarse) in the activation dtype; rois (R,5) f32 [batch,x1,y1,x2,y2].
    pooler_type / sampling_ratio: POOLER_TYPES and the samples per bin and axis (0: adaptive); the defaults launch
    cr_roi_align_*, every other pair cr_roi_pool_*."""
    geo = pooler_type_code(pooler_type, sampling_ratio)
    slots = tuple(_slot_register(f, False) for f in feats)
    return _ROIAlign.apply(rois.to(f32), tuple(scales), out_size, slots, geo, *feats)


# --------------------------------------------------------------------------
# fused Cube R-CNN decode + corner losses (K15/K16)
# --------------------------------------------------------------------------
class _CubeLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dxy, zr, dr, Ra, u, consts, flags):
        _need_cuda(dxy, "cube head outputs")
        n = dxy.shape[0]
        ins = [t.contiguous().to(f32) for t in (dxy, zr, dr, Ra.reshape(n, 9), u)] + \
              [t.contiguous().to(f32) for t in consts]
        arr = (ctypes.c_void_p * 13)(*[t.data_ptr() for t in ins])
        losses = torch.empty((n, 5), dtype=f32, device=dxy.device)
        dec = torch.empty((n, 17), dtype=f32, device=dxy.device)
        _lib.call("cr_cube_loss_fwd", ctypes.cast(arr, ctypes.c_void_p), n, *flags, losses, dec)
        ctx.ins, ctx.flags = ins, flags
        ctx.set_materialize_grads(False)       # outputs nobody differentiates arrive as None, not as zero fills
        ctx.mark_non_differentiable(dec)
        return losses, dec

    @staticmethod
    def backward(ctx, gl, _gdec):
        ins, flags = ctx.ins, ctx.flags
        n = ins[0].shape[0]
        dev = ins[0].device
        arr = (ctypes.c_void_p * 13)(*[t.data_ptr() for t in ins])
        g_dxy = torch.empty((n, 2), dtype=f32, device=dev)
        g_zr = torch.empty((n,), dtype=f32, device=dev)
        g_dr = torch.empty((n, 3), dtype=f32, device=dev)
        g_Ra = torch.empty((n, 3, 3), dtype=f32, device=dev)
        g_u = torch.empty((n,), dtype=f32, device=dev)
        _lib.call("cr_cube_loss_bwd", ctypes.cast(arr, ctypes.c_void_p), n, *flags, gl.contiguous(), g_dxy, g_zr, g_dr, g_Ra,
                  g_u)
        return g_dxy, g_zr, g_dr, g_Ra, g_u, None, None


def cube_decode_loss(dxy, zr, dr, Ra, u, src_boxes, K4, v2r, prior_mean, gt2d, gtz, gtdims, gtR, allocentric=True,
                     chamfer_pose=True, use_conf=True, joint=True):
    """fused K15/K16 (see cr_cube_loss_fwd).  Returns (losses (n,5) [dims,xy,z,pose,joint], dec (n,17))."""
    consts = (src_boxes, K4, v2r, prior_mean, gt2d, gtz, gtdims, gtR.reshape(-1, 9))
    flags = (int(bool(allocentric)), int(bool(chamfer_pose)), int(bool(use_conf)), int(bool(joint)))
    return _CubeLoss.apply(dxy, zr, dr, Ra, u, consts, flags)


# --------------------------------------------------------------------------
# FC layers of the RoI heads on the hand-written implicit-GEMM kernels (cr_linear_*: a linear layer over R rows is a 1x1
# convolution over a (1,1,R,K) map), in both precision modes -- no library GEMM on the path.
# --------------------------------------------------------------------------
def prepared_fc_weight(weight, chw=None, dtype=bf16, need_transposed=False):
    """compute copies of an nn.Linear weight (O, K) f32 in `dtype`, cached per weight epoch on the tensor:
    wp (O,K) and, when asked, wt (K,O) for the backward-data GEMM.  chw = (C,H,W): the columns are re-ordered from the
    checkpoint's (c,h,w) flattening to (h,w,c) for NHWC-flattened RoI features.  f32 without a permutation: wp is the
    weight itself."""
    attr = "_cr_fccache" if dtype == bf16 else "_cr_fccache32"
    ent = getattr(weight, attr, None)
    tag = (weight._version, _WEIGHT_EPOCH[0], weight.data_ptr(), chw)
    O, K = weight.shape
    if ent is None or ent[0] != tag:
        if dtype == f32 and chw is None:
            wp = weight.detach()
        else:
            C, HW = (chw[0], chw[1] * chw[2]) if chw is not None else (K, 1)
            assert C * HW == K
            wp = torch.empty((O, K), dtype=dtype, device=weight.device)
            _lib.call("cr_fc_weight_prepare", weight.detach().contiguous(), wp, O, C, HW, int(dtype == f32))
        ent = [tag, wp, None]
        try:
            setattr(weight, attr, ent)
        except Exception:
            pass
    if need_transposed and ent[2] is None:
        wt = torch.empty((K, O), dtype=dtype, device=weight.device)
        _lib.call("cr_transpose2d", ent[1].contiguous(), wt, O, K, int(dtype == f32))
        ent[2] = wt
    return (ent[1], ent[2]) if need_transposed else ent[1]


def _act_cast(t, dtype):
    """f32 tensor -> the activation dtype (own cast kernel for bf16; no copy for f32)"""
    if t.dtype == dtype:
        return t.contiguous()
    if dtype == bf16 and t.dtype == f32:
        tc = t.contiguous()
        out = torch.empty(tc.shape, dtype=bf16, device=t.device)
        _lib.call("cr_cast_f32_to_bf16", tc, out, tc.numel())
        return out
    return t.to(dtype).contiguous()


def linear_fwd_raw(x, w, bias, out_f32=False, relu=False):
    """y (R,O) = x (R,K) @ w (O,K)^T + bias on the MFMA; x / w in the same activation dtype, bias f32 or None"""
    af = _af(x)
    R, K = x.shape
    O = w.shape[0]
    if O % 16 or K % 16:
        raise _lib.CrError(f"linear: the GEMM kernels need O and K multiples of 16 (got {O}x{K}); use linear_cat for predictors")
    assert w.dtype == x.dtype and x.is_contiguous() and w.is_contiguous()
    y = torch.empty((R, O), dtype=f32 if (out_f32 or af) else bf16, device=x.device)
    _lib.call("cr_linear_fwd", x, w, bias, y, R, K, O, int(relu), int(out_f32), af, _w3(w, af))
    return y


def linear_bwd_data_raw(dy, wt):
    R, O = dy.shape
    K = wt.shape[0]
    assert wt.dtype == dy.dtype and dy.is_contiguous() and wt.is_contiguous()
    dx = torch.empty((R, K), dtype=dy.dtype, device=dy.device)
    af = _af(dy)
    _lib.call("cr_linear_bwd_data", dy, wt, dx, R, K, O, af, _w3(wt, af))
    return dx


def linear_bwd_weight_raw(dy, x, dw, dbias, accumulate):
    """dw (O,K) f32 (+)= dy^T x; dbias (O) f32 += column sums of dy (None: not wanted)"""
    R, O = dy.shape
    K = x.shape[1]
    assert dy.dtype == x.dtype and dy.is_contiguous() and x.is_contiguous() and dw.dtype == f32
    _lib.call("cr_linear_bwd_weight", dy, x, dw, dbias, R, K, O, int(accumulate), _af(x))


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, chw, relu=False):
        _need_cuda(x, "linear input")
        dt = x.dtype
        wp = prepared_fc_weight(weight, chw, dt)
        xc = x.contiguous()
        y = linear_fwd_raw(xc, wp, None if bias is None else bias.detach(), relu=relu)
        ctx.save_for_backward(xc, y if relu else None)
        ctx.refs = (weight, bias, chw)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, yr = ctx.saved_tensors
        weight, bias, chw = ctx.refs
        dt = xc.dtype
        O, K = weight.shape
        C, HW = (chw[0], chw[1] * chw[2]) if chw is not None else (K, 1)
        dy = _act_cast(dy, dt)
        if yr is not None:
            dy = relu_bwd(yr, dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            _, wt = prepared_fc_weight(weight, chw, dt, need_transposed=True)
            dx = linear_bwd_data_raw(dy, wt)
        want_db = bias is not None and ctx.needs_input_grad[2]
        bacc = None
        if want_db:
            bacc = grad_sink(bias)
            if bacc is None:
                bacc = torch.zeros((O,), dtype=f32, device=dy.device)
                db = bacc
        if ctx.needs_input_grad[1]:
            acc = grad_sink(weight)
            if HW == 1 and acc is not None:
                # weight AND bias gradients land in the flat gradient straight from the GEMM
                linear_bwd_weight_raw(dy, xc, acc, bacc, accumulate=True)
            else:
                g = torch.empty((O, K), dtype=f32, device=dy.device)     # in the compute (h,w,c) column order
                linear_bwd_weight_raw(dy, xc, g, bacc, accumulate=False)
                if acc is None:
                    acc = torch.zeros((O, K), dtype=f32, device=dy.device)
                    dw = acc
                _lib.call("cr_fc_grad_accum", g, acc, O, C, HW, 1)
        elif want_db:
            ws = torch.empty((1024, O), dtype=f32, device=dy.device)
            _lib.call("cr_colsum_accum", dy, int(dt == f32), dy.shape[0], O, ws, bacc)
        return dx, dw, db, None, None


def linear(x, weight, bias=None, chw=None, relu=False):
    """F.linear on the MFMA in x's precision (own implicit-GEMM kernels) with the weight copies cached per optimizer step
    and the gradients accumulated straight into the optimizer's flat gradient (when the parameters carry sinks).
    chw: see prepared_fc_weight.  Needs O % 16 == 0 (see linear_cat for predictors with odd widths)."""
    return _Linear.apply(x, weight, bias, chw, relu)


class _CatPlan:
    """persistent buffers of one head's stacked predictors: W (Op,K) / b (Op) f32, refreshed from the parameters by ONE
    launch per weight epoch; the transposed / split copies for backward-data; dW / db that receive the stacked gradient;
    the segment tables that move rows between the parameters (or their gradient sinks) and the stacks."""

    def __init__(self, weights, biases):
        import numpy as np
        dev = weights[0].device
        self.sizes = [int(w.shape[0]) for w in weights]
        self.K = K = int(weights[0].shape[1])
        O = sum(self.sizes)
        self.Op = Op = (O + 15) // 16 * 16
        self.W = torch.zeros((Op, K), dtype=f32, device=dev)
        self.b = torch.zeros((Op,), dtype=f32, device=dev)
        self.dW = torch.empty((Op, K), dtype=f32, device=dev)
        self.db = torch.empty((Op,), dtype=f32, device=dev)
        self.sinks = all(grad_sink(t) is not None for t in list(weights) + list(biases))
        dt = np.dtype([("src", "<u8"), ("dst", "<u8"), ("n", "<i8"), ("item0", "<i8")])

        def table(pairs):
            recs, tot = [], 0
            for src, dst, n in pairs:
                recs.append((src, dst, n, tot))
                tot += n
            return torch.from_numpy(np.array(recs, dtype=dt).view(np.uint8).copy()).to(dev), len(recs), tot
        fw, bw, off = [], [], 0
        for w, bb, n in zip(weights, biases, self.sizes):
            fw.append((w.data_ptr(), self.W.data_ptr() + off * K * 4, n * K))
            fw.append((bb.data_ptr(), self.b.data_ptr() + off * 4, n))
            if self.sinks:
                bw.append((self.dW.data_ptr() + off * K * 4, grad_sink(w).data_ptr(), n * K))
                bw.append((self.db.data_ptr() + off * 4, grad_sink(bb).data_ptr(), n))
            off += n
        self.fwd_table, self.bwd_table = table(fw), (table(bw) if self.sinks else None)
        self.offs = [0]
        for n in self.sizes:
            self.offs.append(self.offs[-1] + n)
        self.tag, self.compute, self.wt = None, {}, {}

    def refresh(self):
        tag = _WEIGHT_EPOCH[0]
        if self.tag != tag:
            t, nd, tot = self.fwd_table
            _lib.call("cr_multi_seg", t, nd, tot, 0)
            self.tag, self.compute, self.wt = tag, {}, {}

    def weight(self, dtype):
        """the stacked weight in the activation dtype (f32: the stack itself)"""
        if dtype not in self.compute:
            self.compute[dtype] = self.W if dtype == f32 else _act_cast(self.W, dtype)
        return self.compute[dtype]

    def weight_t(self, dtype):
        if dtype not in self.wt:
            Wc = self.weight(dtype)
            wt = torch.empty((self.K, self.Op), dtype=dtype, device=Wc.device)
            _lib.call("cr_transpose2d", Wc, wt, self.Op, self.K, int(dtype == f32))
            self.wt[dtype] = wt
        return self.wt[dtype]


import collections as _collections
_CAT_PLANS = _collections.OrderedDict()      # least recently used plans are dropped beyond _CAT_PLANS_MAX
_CAT_PLANS_MAX = 64
_PLAN_KEEP = [None]     # a list while a graph capture is open (graphed.capture_guard): the plans the captured kernels point into


def _cat_plan(weights, biases):
    """plans are keyed by the parameters' addresses and shapes (not kept on the tensor objects: the whole-step graph runs
    the model on fresh leaf tensors over the same storage, and a plan must exist BEFORE a capture starts -- building one
    uploads its tables)"""
    sink_ptr = lambda t: 0 if grad_sink(t) is None else grad_sink(t).data_ptr()
    # (the gradient sinks are part of the key: a later model whose parameters land on a freed model's addresses has its own
    # flat gradient, and the plan's backward table holds raw sink pointers)
    key = tuple((w.data_ptr(), b.data_ptr(), tuple(w.shape), sink_ptr(w), sink_ptr(b)) for w, b in zip(weights, biases))
    sinks = all(grad_sink(t) is not None for t in list(weights) + list(biases))
    plan = _CAT_PLANS.get(key)
    if plan is None or plan.sinks != sinks:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.CrError("linear_cat: the stacked-predictor plan must be built before graph capture (run one eager step)")
        plan = _CAT_PLANS[key] = _CatPlan(weights, biases)
        while len(_CAT_PLANS) > _CAT_PLANS_MAX:
            _CAT_PLANS.popitem(last=False)
    else:
        _CAT_PLANS.move_to_end(key)
    if _PLAN_KEEP[0] is not None:
        _PLAN_KEEP[0].append(plan)          # the graph owner keeps the plan (its raw buffers) alive past an eviction
    return plan


class _LinearCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan, *params):
        plan.refresh()
        xc = x.contiguous()
        y = linear_fwd_raw(xc, plan.weight(xc.dtype), plan.b, out_f32=True)
        ctx.save_for_backward(xc)
        ctx.plan = plan
        return y

    @staticmethod
    def backward(ctx, dy):
        (xc,) = ctx.saved_tensors
        plan = ctx.plan
        dt = xc.dtype
        dy = _act_cast(dy, dt)
        dx = linear_bwd_data_raw(dy, plan.weight_t(dt)) if ctx.needs_input_grad[0] else None
        n = len(plan.sizes)
        if not any(ctx.needs_input_grad[2:]):
            return (dx, None) + (None,) * (2 * n)
        plan.db.zero_()
        linear_bwd_weight_raw(dy, xc, plan.dW, plan.db, accumulate=False)
        if plan.sinks:
            t, nd, tot = plan.bwd_table
            _lib.call("cr_multi_seg", t, nd, tot, 1)
            return (dx, None) + (None,) * (2 * n)
        gw = [plan.dW[plan.offs[i]:plan.offs[i + 1]].clone() for i in range(n)]
        gb = [plan.db[plan.offs[i]:plan.offs[i + 1]].clone() for i in range(n)]
        return (dx, None) + tuple(gw) + tuple(gb)


def linear_cat(x, weights, biases):
    """[x @ w.T + b for w, b in zip(weights, biases)] as ONE GEMM: the predictor layers of a head share their input, so
    their weights are stacked (rows zero-padded to a multiple of 16 for the MFMA tiles) in persistent buffers refreshed by
    one launch per optimizer step; the output is the padded (R, O_pad) f32 matrix plus the column offset of each predictor.
    The stacked gradient goes back into the parameters' gradient sinks with one launch (or as per-parameter slices)."""
    weights, biases = list(weights), list(biases)
    plan = _cat_plan(weights, biases)
    return _LinearCat.apply(x, plan, *weights, *biases), list(plan.offs)


# --------------------------------------------------------------------------
# NMS
# --------------------------------------------------------------------------
def nms_grouped(boxes, counts, thresh):
    """boxes (G,maxn,4) f32 sorted by descending score per group; counts (G,) int32 -> keep (G,maxn) bool."""
    _need_cuda(boxes, "boxes")
    G, maxn, _ = boxes.shape
    keep = torch.zeros((G, maxn), dtype=torch.uint8, device=boxes.device)
    if G == 0 or maxn == 0:
        return keep.bool()
    words = (maxn + 63) // 64
    ws = torch.empty((G * maxn * words,), dtype=torch.int64, device=boxes.device)
    _lib.call("cr_nms_grouped", boxes.contiguous(), counts.to(torch.int32).contiguous(), G, maxn, float(thresh), ws, keep)
    return keep.bool()


def det_select(logits, deltas, prop_boxes, objectness, img_hw, B, P, K, weights, scale_clamp, score_thresh, nms_thresh, detections,
               max_candidates=2048):
    """Test-time filter of the box head on B x P padded proposal slots, no host round trip (fast_rcnn.py:57-116): logits
    (B*P, >= K+1), deltas (B*P, 4K or 4), prop_boxes (B*P,4), objectness (B*P) or None, img_hw (B,2) float.
    -> boxes (B,D,4), scores (B,D), classes (B,D) int64, rows (B,D) int64 (proposal slot inside the image),
    scores_full (B,D,K), count (B,2) int32 = [detections, overflow flag]."""
    _need_cuda(logits, "box head logits")
    dev = logits.device
    # column slices of the predictor GEMM's output are taken as they are (row stride = its width): no copies
    rows_ok = lambda t: t.dtype == f32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]
    lg = logits.detach() if rows_ok(logits) else logits.detach().float().contiguous()
    dl = deltas.detach() if rows_ok(deltas) else deltas.detach().float().contiguous()
    ldl, ldd = lg.stride(0), dl.stride(0)
    pb = prop_boxes.detach().float().contiguous()
    nreg = 1 if dl.shape[1] < 4 * K else K
    S = torch.empty((B, P * K), dtype=f32, device=dev)
    ncand = torch.empty((B + 2,), dtype=torch.int32, device=dev)
    _lib.call("cr_det_scores", _lib.P(lg.data_ptr()), ldl, _lib.P(dl.data_ptr()), ldd, pb, objectness, B, P, K, nreg,
              float(score_thresh), S, ncand)
    Kc = min(int(max_candidates), P * K)
    val, idx = topk(S, Kc)
    boxes = torch.empty((B, Kc, 4), dtype=f32, device=dev)
    meta = torch.empty((3, B, Kc), dtype=torch.int32, device=dev)
    cls, row = meta[0], meta[1]
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    w4 = (_ct.c_float * 4)(*[float(w) for w in weights])
    val, idx = val.contiguous(), idx.contiguous()
    _lib.call("cr_det_gather", val, idx, _lib.P(dl.data_ptr()), ldd, pb, img_hw.float().contiguous(), B, P, K, nreg, Kc, w4,
              float(scale_clamp), boxes, cls, row, counts)
    words = (Kc + 63) // 64
    ws = torch.empty((B * Kc * words,), dtype=torch.int64, device=dev)
    keep = torch.empty((B, Kc), dtype=torch.uint8, device=dev)
    _lib.call("cr_nms_grouped_cls", boxes, cls, counts, B, Kc, float(nms_thresh), ws, keep)
    D = int(detections)
    ob = torch.empty((B, D, 4), dtype=f32, device=dev)
    osc = torch.empty((B, D), dtype=f32, device=dev)
    oi = torch.empty((2, B, D), dtype=torch.int64, device=dev)
    ofull = torch.empty((B, D, K), dtype=f32, device=dev)
    ocnt = torch.empty((B, 2), dtype=torch.int32, device=dev)
    _lib.call("cr_det_pick", keep, counts, ncand, val, boxes, cls, row, _lib.P(lg.data_ptr()), ldl, B, P, K, Kc, D, ob, osc,
              oi[0], oi[1], ofull, ocnt)
    return ob, osc, oi[0], oi[1], ofull, ocnt


# --------------------------------------------------------------------------
# static-shape RPN training glue (csrc/dense_train.hip)
# --------------------------------------------------------------------------
import ctypes as _ct


def _f4(vals):
    return (_ct.c_float * 4)(*[float(v) for v in vals])


def rpn_decode_select(anchors, deltas, idx, scores, weights, scale_clamp, img_hw, min_size):
    """anchors (A,4), deltas (B,A,4), idx (B,S) int64 (-1 = empty), scores (B,S), img_hw (B,2) ->
    boxes (B,S,4) clipped, nms_boxes (B,S,4) (zero where invalid), valid (B,S) bool."""
    _need_cuda(deltas, "deltas")
    B, A = deltas.shape[0], anchors.shape[0]
    S = idx.shape[1]
    dev = deltas.device
    boxes = torch.empty((B, S, 4), dtype=f32, device=dev)
    nmsb = torch.empty((B, S, 4), dtype=f32, device=dev)
    valid = torch.empty((B, S), dtype=torch.uint8, device=dev)
    _lib.call("cr_rpn_decode_select", anchors.contiguous(), deltas.contiguous(), idx.contiguous(), scores.contiguous(), B, A, S,
              _f4(weights), float(scale_clamp), img_hw.contiguous(), float(min_size), boxes, nmsb, valid)
    return boxes, nmsb, valid.bool()


def box_match(boxes, gt_boxes, gt_classes, want_best=False):
    """boxes (R,4) or (B,R,4); gt_boxes (B,G,4); gt_classes (B,G) int64 -> max_iou (B,R), argmax (B,R) int32,
    max_ioa (B,R), best (B,G) int64 (packed, see include/cr3dod.h) or None."""
    _need_cuda(gt_boxes, "gt_boxes")
    B, G = gt_classes.shape
    per_image = boxes.dim() == 3
    R = boxes.shape[-2]
    dev = gt_boxes.device
    mi = torch.empty((B, R), dtype=f32, device=dev)
    am = torch.empty((B, R), dtype=torch.int32, device=dev)
    ma = torch.empty((B, R), dtype=f32, device=dev)
    best = torch.empty((B, G), dtype=torch.int64, device=dev) if want_best else None
    _lib.call("cr_box_match", boxes.contiguous(), int(per_image), gt_boxes.contiguous(), gt_classes.contiguous(), B, R, G, mi,
              am, ma, best)
    return mi, am, ma, best


def rpn_label(anchors, gt_boxes, gt_classes, max_iou, best, expo, lo, hi, labels3, eps):
    B, A = max_iou.shape
    G = gt_classes.shape[1]
    dev = max_iou.device
    labels_pre = torch.empty((B, A), dtype=torch.int8, device=dev)
    out = torch.empty((B, A), dtype=torch.int32, device=dev)
    miou = torch.empty((B, A), dtype=f32, device=dev)
    keys = torch.empty((2, B, A), dtype=f32, device=dev)
    _lib.call("cr_rpn_label", anchors.contiguous(), gt_boxes.contiguous(), gt_classes.contiguous(), max_iou, best,
              expo.contiguous(), B, A, G, float(lo), float(hi), (_ct.c_int * 3)(*[int(v) for v in labels3]), float(eps),
              labels_pre, out, miou, keys)
    return labels_pre, out, miou, keys


def rpn_scatter(out, pos_idx, pos_key, neg_idx, neg_key, n_s, ioa, ignore_thresh):
    """in place on out (B,A) int32."""
    B, A = out.shape
    _lib.call("cr_rpn_scatter", pos_idx.contiguous(), pos_key.contiguous(), pos_idx.shape[1], neg_idx.contiguous(),
              neg_key.contiguous(), neg_idx.shape[1], int(n_s), ioa.contiguous(), float(ignore_thresh), B, A, out)
    return out


# MODEL.RPN.BBOX_REG_LOSS_TYPE values cr_rpn_loss_opt computes (detectron2 _dense_box_regression_loss); the IoU family only with
# OBJECTNESS_UNCERTAINTY "none" (rpn.py:271 raises for it on the IoU-weighted path)
RPN_REG_TYPES = {"smooth_l1": 0, "giou": 1, "diou": 2, "ciou": 3}
SCALE_CLAMP = math.log(1000.0 / 16)         # detectron2 Box2BoxTransform's default


def rpn_reg_type_code(box_reg_loss_type, objectness_none):
    """the reg_type code of cr_rpn_loss_opt, or the reference's ValueError (rpn.py:271 / detectron2 _dense_box_regression_loss)"""
    built = sorted(RPN_REG_TYPES) if objectness_none else ["smooth_l1"]
    if box_reg_loss_type not in built:
        raise ValueError(f"Invalid dense box regression loss type '{box_reg_loss_type}' (rpn.py:271; built with "
                         f"OBJECTNESS_UNCERTAINTY {'none' if objectness_none else 'other than none'}: {built})")
    return RPN_REG_TYPES[box_reg_loss_type]


class _RPNLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, deltas, anchors, labels, midx, gt_boxes, weights, opt=None):
        B, A = logits.shape
        G = gt_boxes.shape[1]
        dev = logits.device
        nb = (A + 255) // 256
        ws = torch.empty((B * nb * 6,), dtype=f32, device=dev)
        sums = torch.empty((6,), dtype=f32, device=dev)
        dl = torch.empty((B, A), dtype=f32, device=dev)
        dd = torch.empty((B, A, 4), dtype=f32, device=dev)
        if opt is None:
            _lib.call("cr_rpn_loss", logits.detach().float().contiguous(), deltas.detach().float().contiguous(),
                      anchors.contiguous(), labels.contiguous(), midx.contiguous(), gt_boxes.contiguous(), B, A, G, _f4(weights),
                      ws, sums, dl, dd)
        else:
            objectness, reg_type, beta, scale_clamp = opt
            _lib.call("cr_rpn_loss_opt", logits.detach().float().contiguous(), deltas.detach().float().contiguous(),
                      anchors.contiguous(), labels.contiguous(), midx.contiguous(), gt_boxes.contiguous(), B, A, G, _f4(weights),
                      int(objectness), int(reg_type), float(beta), float(scale_clamp), ws, sums, dl, dd)
        ctx.save_for_backward(dl, dd)
        ctx.set_materialize_grads(False)       # outputs nobody differentiates arrive as None, not as zero fills
        ctx.mark_non_differentiable(sums)
        return sums[0], sums[1], sums

    @staticmethod
    def backward(ctx, g_cls, g_loc, _gs):
        dl, dd = ctx.saved_tensors
        return (None if g_cls is None else dl * g_cls), (None if g_loc is None else dd * g_loc), None, None, None, None, None, None


def rpn_loss(logits, deltas, anchors, labels, midx, gt_boxes, weights, **options):
    """-> (loss_cls_sum, loss_loc_sum, sums6) unnormalised; labels (B,A) int32, midx (B,A) int32.  Without keywords: the default
    options (IoU-weighted objectness, L1) on cr_rpn_loss; any keyword of rpn_loss_opt selects cr_rpn_loss_opt."""
    if options:
        return rpn_loss_opt(logits, deltas, anchors, labels, midx, gt_boxes, weights, **options)
    return _RPNLoss.apply(logits, deltas, anchors, labels, midx, gt_boxes, tuple(weights))


def rpn_loss_opt(logits, deltas, anchors, labels, midx, gt_boxes, weights, objectness_none=False, box_reg_loss_type="smooth_l1",
                 beta=0.0, scale_clamp=SCALE_CLAMP):
    """rpn_loss for the other option sets (cr_rpn_loss_opt): objectness_none = OBJECTNESS_UNCERTAINTY "none" (rpn.py:181-197),
    box_reg_loss_type smooth_l1 (with beta) / giou / diou / ciou, scale_clamp of the Box2BoxTransform for the IoU family."""
    if not beta >= 0:
        raise ValueError(f"smooth_l1 beta {beta} < 0")
    code = rpn_reg_type_code(box_reg_loss_type, objectness_none)
    return _RPNLoss.apply(logits, deltas, anchors, labels, midx, gt_boxes, tuple(weights),
                          (1 if objectness_none else 0, code, float(beta), float(scale_clamp)))


def roi_label(max_iou, argmax, max_ioa, valid, gt_classes, expo, K, thr, ignore_thresh, eps):
    B, R = max_iou.shape
    dev = max_iou.device
    cls = torch.empty((B, R), dtype=torch.int64, device=dev)
    miou = torch.empty((B, R), dtype=f32, device=dev)
    keys = torch.empty((2, B, R), dtype=f32, device=dev)
    _lib.call("cr_roi_label", max_iou, argmax, max_ioa, valid.to(torch.uint8).contiguous(), gt_classes.contiguous(),
              expo.contiguous(), B, R, gt_classes.shape[1], int(K), float(thr), float(ignore_thresh), float(eps), cls, miou,
              keys)
    return cls, miou, keys


def roi_compact(fg_idx, fg_key, bg_idx, bg_key, n_s, boxes, cls, argmax):
    """-> boxes (B,n_s,4), valid (B,n_s) bool, classes (B,n_s) int64, gt_idx (B,n_s) int64, counts (B,2) int32."""
    B, R = cls.shape
    dev = cls.device
    ob = torch.empty((B, n_s, 4), dtype=f32, device=dev)
    ov = torch.empty((B, n_s), dtype=torch.uint8, device=dev)
    oc = torch.empty((B, n_s), dtype=torch.int64, device=dev)
    og = torch.empty((B, n_s), dtype=torch.int64, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    _lib.call("cr_roi_compact", fg_idx.contiguous(), fg_key.contiguous(), fg_idx.shape[1], bg_idx.contiguous(),
              bg_key.contiguous(), bg_idx.shape[1], int(n_s), boxes.contiguous(), cls, argmax, B, R, ob, ov, oc, og, counts)
    return ob, ov.bool(), oc, og, counts


class _BoxLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, deltas, valid, cls, pboxes, gt_idx, gt_boxes, weights, scale_clamp, opt=None):
        B, S = valid.shape
        N, C = scores.shape
        K = C - 1
        dev = scores.device
        nb = (N + 3) // 4
        KD = 1 if opt is not None and opt[1] else K          # regression classes: one when class-agnostic
        if N != B * S or tuple(deltas.shape) != (N, KD * 4):
            raise ValueError(f"box_loss: scores {tuple(scores.shape)} / valid {tuple(valid.shape)} need deltas ({B * S}, {KD * 4}) "
                             f"({'class-agnostic' if KD == 1 and K != 1 else 'class-specific'} regression), got {tuple(deltas.shape)}")
        ws = torch.empty((nb * 3,), dtype=f32, device=dev)
        sums = torch.empty((3,), dtype=f32, device=dev)
        ds = torch.empty((N, C), dtype=f32, device=dev)
        dd = torch.empty((N, KD * 4), dtype=f32, device=dev)
        pred = torch.empty((N, 4), dtype=f32, device=dev)
        if opt is None:
            _lib.call("cr_box_loss", scores.detach().float().contiguous(), deltas.detach().float().contiguous(),
                      valid.to(torch.uint8).contiguous(), cls.contiguous(), pboxes.contiguous(), gt_idx.contiguous(),
                      gt_boxes.contiguous(), B, S, gt_boxes.shape[1], K, _f4(weights), float(scale_clamp), ws, sums, ds, dd, pred)
        else:
            _lib.call("cr_box_loss_opt", scores.detach().float().contiguous(), deltas.detach().float().contiguous(),
                      valid.to(torch.uint8).contiguous(), cls.contiguous(), pboxes.contiguous(), gt_idx.contiguous(),
                      gt_boxes.contiguous(), B, S, gt_boxes.shape[1], K, _f4(weights), float(scale_clamp), float(opt[0]),
                      1 if opt[1] else 0, ws, sums, ds, dd, pred)
        ctx.save_for_backward(ds, dd)
        ctx.dt = (scores.dtype, deltas.dtype)
        ctx.set_materialize_grads(False)       # outputs nobody differentiates arrive as None, not as zero fills
        ctx.mark_non_differentiable(sums, pred)
        return sums[0], sums[1], sums, pred

    @staticmethod
    def backward(ctx, g_ce, g_l1, _gs, _gp):
        ds, dd = ctx.saved_tensors
        return (None if g_ce is None else (ds * g_ce).to(ctx.dt[0])), (None if g_l1 is None else (dd * g_l1).to(ctx.dt[1])), \
            None, None, None, None, None, None, None, None


def box_loss(scores, deltas, valid, cls, pboxes, gt_idx, gt_boxes, weights, scale_clamp, **options):
    """-> (sum CE, sum L1, sums3 = [.., .., n_valid], pred (N,4)); valid/cls/gt_idx (B,S), pboxes (B,S,4).  Without keywords: the
    default options (L1, class-specific deltas (N,K*4)) on cr_box_loss; any keyword of box_loss_opt selects cr_box_loss_opt."""
    if options:
        return box_loss_opt(scores, deltas, valid, cls, pboxes, gt_idx, gt_boxes, weights, scale_clamp, **options)
    return _BoxLoss.apply(scores, deltas, valid, cls, pboxes, gt_idx, gt_boxes, tuple(weights), scale_clamp)


def box_loss_opt(scores, deltas, valid, cls, pboxes, gt_idx, gt_boxes, weights, scale_clamp, beta=0.0, cls_agnostic=False):
    """box_loss for the other option sets (cr_box_loss_opt): smooth_l1 beta (fast_rcnn.py:245-252) and class-agnostic regression
    (deltas (N,4), fast_rcnn.py:207-208)."""
    if not beta >= 0:
        raise ValueError(f"smooth_l1 beta {beta} < 0")
    return _BoxLoss.apply(scores, deltas, valid, cls, pboxes, gt_idx, gt_boxes, tuple(weights), scale_clamp,
                          (float(beta), bool(cls_agnostic)))


# --------------------------------------------------------------------------
# 3D head on the static-shape path: class gather + fused decode/loss + reductions
# --------------------------------------------------------------------------
CUBE_OFF = (0, 2, 3, 6, 15, 16, 20, 21, 24, 26, 27, 30)      # chunk starts of buf39 (x n), see include/cr3dod.h
CUBE_DIM = (2, 1, 3, 9, 1, 4, 1, 3, 2, 1, 3, 9)
# MODEL.ROI_CUBE_HEAD.Z_TYPE values the kernels decode (roi_heads.py:2404-2410)
Z_TYPES = {"direct": 0, "sigmoid": 1, "log": 2, "clusters": 3}


def z_type_code(z_type):
    if z_type not in Z_TYPES:
        raise ValueError(f"Z_TYPE '{z_type}' is not built (built: {sorted(Z_TYPES)})")
    return Z_TYPES[z_type]


# MODEL.ROI_CUBE_HEAD.POSE_TYPE values the kernels decode (cube_head.py:180-190) and the columns each takes per class
POSE_TYPES = {"6d": 0, "quaternion": 1, "euler": 2}
POSE_WIDTH = {"6d": 6, "quaternion": 4, "euler": 3}
# MODEL.ROI_CUBE_HEAD.DIMS_PRIORS_FUNC values (roi_heads.py:2385-2390)
DIMS_FUNCS = {"exp": 0, "sigmoid": 1}


def pose_type_code(pose_type):
    if pose_type not in POSE_TYPES:
        raise ValueError(f"POSE_TYPE '{pose_type}' is not built (built: {sorted(POSE_TYPES)})")
    return POSE_TYPES[pose_type]


def dims_func_code(dims_func, priors=None, priors_std=None):
    """code of DIMS_PRIORS_FUNC for the prior tables (K,3) at hand: 'sigmoid' decodes between mean -+ 3 std and needs both;
    without priors the dimensions are exp(raw) whatever the function says (roi_heads.py:2392-2394) -> 0"""
    if dims_func not in DIMS_FUNCS:
        raise ValueError(f"DIMS_PRIORS_FUNC '{dims_func}' is not built (built: {sorted(DIMS_FUNCS)})")
    if priors is None:
        return 0
    if dims_func == "sigmoid" and priors_std is None:
        raise ValueError("DIMS_PRIORS_FUNC 'sigmoid' needs the standard deviations of the dimension priors (priors_std)")
    return DIMS_FUNCS[dims_func]


def z_config(z_type="direct", bins=1, z_scales=None, z_stats=None):
    """(code, bins, z_scales (K,bins) f32 or None, z_stats (K,bins,2) f32 or None): how a RoI's depth is read from the predictor
    output -- MODEL.ROI_CUBE_HEAD.Z_TYPE / CLUSTER_BINS with the head's priors_z_scales / priors_z_stats (roi_heads.py:2343-2436)"""
    code, bins = z_type_code(z_type), int(bins)
    if bins > 1 and z_scales is None:
        raise ValueError("CLUSTER_BINS > 1 needs priors_z_scales")
    if code == 3 and (bins <= 1 or z_stats is None):
        raise ValueError("Z_TYPE 'clusters' needs CLUSTER_BINS > 1 and priors_z_stats")
    f = lambda t: None if t is None else t.detach().float().contiguous()
    return (code, bins, f(z_scales) if bins > 1 else None, f(z_stats) if code == 3 else None)


def _chunks(buf, n):
    return [buf[o * n:(o + d) * n] for o, d in zip(CUBE_OFF, CUBE_DIM)]


def _cube_select(raw, layout, K, cls, valid, gt_idx, kf, gt3d, gtpose, priors, meta, boxes, zc, rows=39, param=None):
    """the one place that marshals a forward selection of the 3D head: raw (n, ld) into a fresh buffer of `rows` x n floats whose
    first 39 rows are buf39; with rows = 42 the last three are the `norm` rows of the non-disentangled loss.  param None: the
    default family, cr_cube_select (+ cr_cube_select_norm for the norm rows); param = (pose code, dims code, priors_std):
    cr_cube_select_param, which writes the norm rows itself.
    -> (raw32, the buffer, validf (n) uint8, clsc (n) int32, boxes f32)"""
    _need_cuda(raw, "cube head output")
    B, S = cls.shape
    n, K, kf = B * kf, int(K), int(kf)
    dev = raw.device
    raw32 = raw.detach().float().contiguous()
    buf = torch.empty((rows * n,), dtype=f32, device=dev)
    validf = torch.empty((n,), dtype=torch.uint8, device=dev)
    clsc = torch.empty((n,), dtype=torch.int32, device=dev)
    lay = (_ct.c_int * 5)(*[int(v) for v in layout])
    boxes = boxes.float().contiguous()
    norm = buf[39 * n:] if rows > 39 else None
    cls, valid, gt_idx = cls.contiguous(), valid.to(torch.uint8).contiguous(), gt_idx.contiguous()
    gt3d, gtpose, meta = gt3d.contiguous(), gtpose.contiguous(), meta.contiguous()
    if param is None:
        _lib.call("cr_cube_select", raw32, raw32.shape[1], lay, K, cls, valid, gt_idx, B, S, kf, gt3d.shape[1], gt3d, gtpose, priors,
                  meta, buf, validf, clsc, zc[0], zc[1], zc[2], zc[3], boxes)
        if norm is not None:
            _lib.call("cr_cube_select_norm", raw32, raw32.shape[1], lay, K, B, kf, clsc, zc[0], zc[1], zc[2], zc[3], boxes, norm)
    else:
        _lib.call("cr_cube_select_param", raw32, raw32.shape[1], lay, K, cls, valid, gt_idx, B, S, kf, gt3d.shape[1], gt3d, gtpose,
                  priors, meta, buf, validf, clsc, zc[0], zc[1], zc[2], zc[3], boxes, param[0], param[1], param[2], norm)
    return raw32, buf, validf, clsc, boxes


def _cube_loss_ins(buf, boxes, n):
    """-> (chunks of buf39, the 13-pointer input array of the loss kernels: the chunks with the RoI boxes after the fifth)"""
    ch = _chunks(buf, n)
    ins = ch[:5] + [boxes] + ch[5:]
    return ch, ctypes.cast((ctypes.c_void_p * 13)(*[t.data_ptr() for t in ins]), ctypes.c_void_p)


def _cube_grads(n, dev, zraw=False):
    """one buffer for what the loss backward kernels write, split: g_dxy, g_zr, g_dr, g_Ra, g_u (+ a 17th row: g_zraw, or the
    weak head's zero g_usel)"""
    cuts = (0, 2, 3, 6, 15, 16) + ((17,) if zraw else ())
    g = torch.empty((cuts[-1] * n,), dtype=f32, device=dev)
    return [g[a * n:b * n] for a, b in zip(cuts, cuts[1:])]


def _cube_select_bwd(raw32, layout, K, B, kf, validf, clsc, grads, g_usel, zc, boxes, param=None, g_zraw=None):
    """the one place that marshals a backward selection: the five decoded-quantity gradients, the selected uncertainty's and
    g_zraw (n) or None, the non-disentangled z term's gradient w.r.t. the raw depth -> g_raw like raw32.  param None: the default
    family, cr_cube_select_bwd (+ cr_cube_select_bwd_zraw for g_zraw); param = (pose code, dims code, priors, priors_std):
    cr_cube_select_param_bwd, which adds g_zraw itself and takes NULL for a missing g_usel."""
    g_dxy, g_zr, g_dr, g_Ra, g_u = grads
    g_raw = torch.empty_like(raw32)
    lay = (_ct.c_int * 5)(*layout)
    if param is None:
        _lib.call("cr_cube_select_bwd", raw32, raw32.shape[1], lay, K, B, kf, validf, clsc, g_dxy, g_zr, g_dr, g_Ra, g_u,
                  g_usel.contiguous(), g_raw, zc[0], zc[1], zc[2], zc[3], boxes)
        if g_zraw is not None:
            _lib.call("cr_cube_select_bwd_zraw", raw32.shape[1], lay, K, B, kf, validf, clsc, g_zraw, g_raw, zc[1], zc[2], boxes)
    else:
        _lib.call("cr_cube_select_param_bwd", raw32, raw32.shape[1], lay, K, B, kf, validf, clsc, g_dxy, g_zr, g_dr, g_Ra, g_u,
                  None if g_usel is None else g_usel.contiguous(), g_raw, zc[0], zc[1], zc[2], zc[3], boxes, param[0], param[1],
                  param[2], param[3], g_zraw)
    return g_raw


_CubeRoute = _collections.namedtuple("_CubeRoute", "param disentangled flags")


class _CubeHeadLoss(torch.autograd.Function):
    """raw (n, ld) -> per-RoI losses (n,5), selected uncertainty (n); saves what the two backward kernels need.  Four stages --
    select, loss, loss backward, select backward -- whose entry points the route picks (_CubeRoute, computed by cube_head_loss):
    param         an option off its default changes the predictor layout or the decode of a selected column (POSE_TYPE
                  'quaternion' / 'euler', no uncertainty block, DIMS_PRIORS_FUNC 'sigmoid'): cr_cube_select_param / _param_bwd,
                  else the default family cr_cube_select / _select_bwd
    disentangled  cr_cube_loss_fwd / _bwd on buf39; else the non-disentangled losses (roi_heads.py:2516-2560),
                  cr_cube_nondis_fwd / _bwd: three rows after the 39 carry the pre-decode depth and the cluster statistics, and the
                  z term's gradient w.r.t. the raw depth reaches the depth column through the backward selection
    flags         (allocentric, chamfer_pose, use_conf, joint, z config, pose code, dims code)"""

    @staticmethod
    def forward(ctx, raw, layout, K, cls, valid, gt_idx, kf, gt3d, gtpose, priors, priors_std, meta, boxes, route):
        allocentric, chamfer_pose, use_conf, joint, zc, pose_code, dims_code = route.flags
        B, n = cls.shape[0], cls.shape[0] * kf
        raw32, buf_all, validf, clsc, boxes = _cube_select(raw, layout, K, cls, valid, gt_idx, kf, gt3d, gtpose, priors, meta, boxes, zc,
                                                           rows=39 if route.disentangled else 42,
                                                           param=(pose_code, dims_code, priors_std) if route.param else None)
        buf, norm = buf_all[:39 * n], buf_all[39 * n:]
        ch, arr = _cube_loss_ins(buf, boxes, n)
        losses = torch.empty((n, 5), dtype=f32, device=raw.device)
        dec = torch.empty((n, 17), dtype=f32, device=raw.device)
        if route.disentangled:
            _lib.call("cr_cube_loss_fwd", arr, n, allocentric, chamfer_pose, use_conf, joint, losses, dec)
        else:
            _lib.call("cr_cube_nondis_fwd", arr, norm, n, allocentric, use_conf, joint, zc[0], losses, dec)
        ctx.keep = (raw32, buf_all, validf, clsc, boxes, priors, priors_std, layout, int(K), B, int(kf), route, raw.dtype)
        ctx.set_materialize_grads(False)       # outputs nobody differentiates arrive as None, not as zero fills
        ctx.mark_non_differentiable(dec, buf, validf)
        return losses, ch[4].clone(), dec, buf, validf

    @staticmethod
    def backward(ctx, gl, g_usel, _gd, _gb, _gv):
        raw32, buf_all, validf, clsc, boxes, priors, priors_std, layout, K, B, kf, route, dt = ctx.keep
        allocentric, chamfer_pose, use_conf, joint, zc, pose_code, dims_code = route.flags
        n = B * kf
        buf, norm = buf_all[:39 * n], buf_all[39 * n:]
        _, arr = _cube_loss_ins(buf, boxes, n)
        g_dxy, g_zr, g_dr, g_Ra, g_u, *g_zraw = _cube_grads(n, raw32.device, zraw=not route.disentangled)
        if route.disentangled:
            _lib.call("cr_cube_loss_bwd", arr, n, allocentric, chamfer_pose, use_conf, joint, gl.contiguous(), g_dxy, g_zr, g_dr, g_Ra,
                      g_u)
        else:
            _lib.call("cr_cube_nondis_bwd", arr, norm, n, allocentric, use_conf, joint, zc[0], gl.contiguous(), g_dxy, g_zr, g_dr, g_Ra,
                      g_u, g_zraw[0])
        # 'direct' has no normalised depth space: its z term went through g_zr
        g_raw = _cube_select_bwd(raw32, layout, K, B, kf, validf, clsc, (g_dxy, g_zr, g_dr, g_Ra, g_u), g_usel, zc, boxes,
                                 param=(pose_code, dims_code, priors, priors_std) if route.param else None,
                                 g_zraw=g_zraw[0] if g_zraw and zc[0] != 0 else None)
        return (g_raw.to(dt),) + (None,) * 13


def cube_head_loss(raw, layout, K, cls, valid, gt_idx, kf, gt3d, gtpose, priors, meta, boxes, allocentric=True,
                   chamfer_pose=True, use_conf=True, joint=True, z_type="direct", z_cfg=None, disentangled=True,
                   pose_type="6d", dims_func="exp", priors_std=None):
    """raw (n, ld) fused predictor output (13K columns in the default family); cls/valid/gt_idx (B,S); gt3d (B,G,9); gtpose
    (B,G,3,3); priors (K,3) or None;
    meta (B,5); boxes (n,4).  -> losses (n,5), u_sel (n), dec (n,17), buf39, validf (n) uint8.
    disentangled=False: the non-disentangled losses of MODEL.ROI_CUBE_HEAD.DISENTANGLED_LOSS False (roi_heads.py:2516-2560);
    `priors` must be None (the reference fails with the dimension priors there, :2532) and `chamfer_pose` plays no part (the
    pose term is the relative rotation angle, the joint term is L1, :2587-2591).
    pose_type '6d' | 'quaternion' | 'euler': the pose block of `raw` has 6 / 4 / 3 columns per class (cube_head.py:180-190).
    use_conf=False: USE_CONFIDENCE 0, `raw` has no uncertainty block (layout[4] is not read); u_sel is 0 and takes no gradient.
    dims_func 'exp' | 'sigmoid' with priors_std (K,3): DIMS_PRIORS_FUNC (roi_heads.py:2385-2390); only read with `priors`.
    With the default values of these three the entry points of the default family are launched, as before."""
    pose_code = pose_type_code(pose_type)
    dims_code = dims_func_code(dims_func, priors, priors_std)
    if not disentangled and priors is not None:
        raise ValueError("cube_head_loss: the non-disentangled loss is built without dimension priors "
                         "(DIMS_PRIORS_ENABLED False): the reference fails with them (roi_heads.py:2532)")
    route = _CubeRoute(pose_code != 0 or dims_code != 0 or not use_conf, bool(disentangled),
                       (int(bool(allocentric)), int(bool(chamfer_pose)), int(bool(use_conf)), int(bool(joint)),
                        z_cfg or z_config(z_type), pose_code, dims_code))
    lay = tuple(int(v) for v in layout[:4]) + (int(layout[4]) if use_conf else -1,)
    if route.param:
        f = lambda t: None if t is None else t.detach().float().contiguous()
        priors, priors_std = f(priors), f(priors_std) if dims_code else None
    else:
        priors_std = None
    return _CubeHeadLoss.apply(raw, lay, K, cls, valid, gt_idx, kf, gt3d, gtpose.reshape(gtpose.shape[0], -1, 9), priors, priors_std,
                               meta, boxes, route)


def cube_decode_infer(raw, layout, K, cls, img, boxes, meta6, priors, allocentric=True, z_type="direct", z_cfg=None,
                      pose_type="6d", use_conf=True, dims_func="exp", priors_std=None):
    """inference decode of the 3D head (no autograd) -> (n,42), see cr_cube_decode_infer.  pose_type / use_conf / dims_func /
    priors_std as in cube_head_loss; off their defaults the decode is cr_cube_decode_infer_param.  Without confidence column 8
    repeats column 7 (the reference's score merge reads the last column of its cube_3D, roi_heads.py:2693-2716)."""
    _need_cuda(raw, "cube head output")
    n, K, allocentric = raw.shape[0], int(K), int(bool(allocentric))
    out = torch.empty((n, 42), dtype=f32, device=raw.device)
    raw32 = raw.detach().float().contiguous()
    zc = z_cfg or z_config(z_type)
    pose_code = pose_type_code(pose_type)
    dims_code = dims_func_code(dims_func, priors, priors_std)
    lay = (_ct.c_int * 5)(*[int(v) for v in layout[:4]], int(layout[4]) if use_conf else -1)
    cls, img, boxes, meta6 = cls.contiguous(), img.to(torch.int32).contiguous(), boxes.float().contiguous(), meta6.contiguous()
    if pose_code != 0 or dims_code != 0 or not use_conf:
        f = lambda t: None if t is None else t.detach().float().contiguous()
        _lib.call("cr_cube_decode_infer_param", raw32, raw32.shape[1], lay, K, cls, img, boxes, meta6, f(priors), n, allocentric, out,
                  zc[0], zc[1], zc[2], zc[3], pose_code, dims_code, f(priors_std) if dims_code else None)
    else:
        _lib.call("cr_cube_decode_infer", raw32, raw32.shape[1], lay, K, cls, img, boxes, meta6, priors, n, allocentric, out, zc[0],
                  zc[1], zc[2], zc[3])
    return out


class _CubeReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, L, u_sel, buf, dec, validf, inverse_z):
        n = L.shape[0]
        dev = L.device
        out = torch.empty((16,), dtype=f32, device=dev)
        red, cnt, stats = out[:6], out[6:12], out[12:]
        Lc = L.detach().contiguous()
        _lib.call("cr_cube_reduce", Lc, buf, dec, validf, n, int(inverse_z), red, cnt, stats)
        ctx.keep = (Lc, buf, validf, cnt, int(inverse_z))
        ctx.set_materialize_grads(False)       # outputs nobody differentiates arrive as None, not as zero fills
        ctx.mark_non_differentiable(stats)
        return red, stats

    @staticmethod
    def backward(ctx, gred, _gs):
        Lc, buf, validf, cnt, inverse_z = ctx.keep
        n = Lc.shape[0]
        gL = torch.empty_like(Lc)
        gu = torch.empty((n,), dtype=f32, device=Lc.device)
        _lib.call("cr_cube_reduce_bwd", Lc, buf, validf, n, inverse_z, cnt, gred.contiguous(), gL, gu)
        return gL, gu, None, None, None, None


def cube_reduce(L, u_sel, buf, dec, validf, inverse_z=False):
    """-> red (6) = means of [dims, xy, z, pose, joint, uncert] over the valid finite entries, stats (4)."""
    return _CubeReduce.apply(L, u_sel, buf, dec, validf, inverse_z)


# --------------------------------------------------------------------------
# weakly supervised 3D head on the static-shape path: class gather + fused decode / losses / reductions
# --------------------------------------------------------------------------
WEAK_TERMS = ("iou", "pose", "normal", "z", "pseudo_gt_z", "dims_w", "dims_h", "dims_l")      # bit k of `terms`
WEAK_MAX_SLOTS = 256                                                                           # kf limit of k_weak_fwd / k_weak_bwd
_WEAK_IMG = {}


class _WeakCubeLoss(torch.autograd.Function):
    """raw (n,13K) -> red (9) = safely reduced, uncertainty-weighted terms + the mean uncertainty; see include/cr3dod.h
    (cr_weak_loss_fwd / _reduce / _bwd).  Five launches forward (select, terms, window medians, reduce), two backward."""

    @staticmethod
    def forward(ctx, raw, layout, K, cls, valid, gt_idx, kf, gt_boxes, gt3d, gtpose, prior_mean, prior_std, meta, table, normals,
                boxes, depth, terms, pgz_mode, weights, allocentric, zt):
        B, S = cls.shape
        n, G = B * kf, gt3d.shape[1]
        dev = raw.device
        cls, gt_idx = cls.contiguous(), gt_idx.contiguous()
        raw32, buf, validf, clsc, boxes = _cube_select(raw, layout, K, cls, valid, gt_idx, kf, gt3d, gtpose, prior_mean, meta, boxes, zt)
        gt_boxes, table = gt_boxes.float().contiguous(), table.contiguous()
        ch = _chunks(buf, n)
        ins = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in (ch[0], ch[1], ch[2], ch[3], ch[4], ch[6], ch[7], boxes)])
        out = torch.empty((n * (8 + 17 + 4 + 1 + 1) + 2 * B + 27,), dtype=f32, device=dev)
        o = 0
        def take(m):
            nonlocal o
            t = out[o:o + m]
            o += m
            return t
        Lraw, dec, pbox, ztgt, med, pimg = take(8 * n), take(17 * n), take(4 * n), take(n), take(n), take(2 * B)
        red, cnt, stats, aux = take(9), take(9), take(8), take(1)
        ibox = torch.empty((n, 4), dtype=torch.int32, device=dev)
        _lib.call("cr_weak_loss_fwd", ctypes.cast(ins, ctypes.c_void_p), validf, clsc, gt_idx, gt_boxes, prior_std, table, normals, B,
                  int(kf), S, G, int(bool(allocentric)), int(terms), Lraw, dec, pbox, ibox, pimg)
        H = W = 0
        if pgz_mode:
            depth = depth.float().contiguous()
            H, W = depth.shape[1], depth.shape[2]
        if pgz_mode == 1:
            img = _WEAK_IMG.get((B, kf, str(dev)))
            if img is None:
                img = _WEAK_IMG[(B, kf, str(dev))] = (torch.arange(n, device=dev) // kf).to(torch.int32)
            _lib.call("cr_box_median", depth, B, H, W, ibox, img, n, med)
        rin = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in (ch[4], ch[8], ch[9], ch[10])])
        wts = (_ct.c_float * 9)(*[float(w) for w in weights])
        _lib.call("cr_weak_loss_reduce", ctypes.cast(rin, ctypes.c_void_p), validf, table, depth if pgz_mode else None, H, W,
                  med if pgz_mode == 1 else None, gt_boxes, gt_idx, B, int(kf), S, G, int(terms), int(pgz_mode), wts, Lraw, dec,
                  pbox, ibox, pimg, ztgt, red, cnt, stats, aux)
        ctx.keep = (raw32, buf, validf, clsc, boxes, tuple(layout), int(K), B, int(kf), S, G, raw.dtype, cls, gt_idx, gt_boxes, prior_std,
                    table, normals, int(bool(allocentric)), int(terms), out, zt)
        dec2, pbox2 = dec.view(n, 17), pbox.view(n, 4)
        ctx.set_materialize_grads(False)       # outputs nobody differentiates arrive as None, not as zero fills
        ctx.mark_non_differentiable(stats, dec2, pbox2, validf)
        return red, stats, dec2, pbox2, validf

    @staticmethod
    def backward(ctx, gred, *_unused):
        (raw32, buf, validf, clsc, boxes, layout, K, B, kf, S, G, dt, cls, gt_idx, gt_boxes, prior_std, table, normals, allocentric, terms,
         out, zt) = ctx.keep
        n = B * kf
        dev = raw32.device
        ch = _chunks(buf, n)
        ins = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in (ch[0], ch[1], ch[2], ch[3], ch[4], ch[6], ch[7], boxes)])
        Lraw, dec, ztgt, pimg = out[:8 * n], out[8 * n:25 * n], out[29 * n:30 * n], out[31 * n:31 * n + 2 * B]
        tail = out[31 * n + 2 * B:]
        cnt, aux = tail[9:18], tail[26:27]
        g_dxy, g_zr, g_dr, g_Ra, g_u, zero = _cube_grads(n, dev, zraw=True)      # the 17th row: a zero g_usel
        zero.zero_()
        _lib.call("cr_weak_loss_bwd", ctypes.cast(ins, ctypes.c_void_p), validf, clsc, gt_idx, gt_boxes, prior_std, table,
                  normals, B, kf, S, G, allocentric, terms, gred.float().contiguous(), cnt, aux, Lraw, dec, ztgt, pimg, g_dxy,
                  g_zr, g_dr, g_Ra, g_u)
        g_raw = _cube_select_bwd(raw32, layout, K, B, kf, validf, clsc, (g_dxy, g_zr, g_dr, g_Ra, g_u), zero, zt, boxes)
        return (g_raw.to(dt),) + (None,) * 21


def weak_cube_loss(raw, layout, K, cls, valid, gt_idx, kf, gt_boxes, gt3d, gtpose, prior_mean, prior_std, meta, table, normals, boxes,
                   depth, terms, pgz_mode, weights, allocentric=True, z_type="direct", z_cfg=None):
    """Losses of the weakly supervised 3D head on the (B, kf) foreground slots (ROIHeads3DScore._forward_cube, training).
    raw (n,13K) fused predictor output; cls / valid / gt_idx (B,S); gt_boxes (B,G,4); gt3d (B,G,9); gtpose (B,G,3,3);
    prior_mean / prior_std (K,3) or None; meta (B,5) camera_meta(); table (B,20), normals (B,3) or None, depth (B,H,W) or
    None: see cr_weak_loss_fwd in include/cr3dod.h; terms: bit mask over WEAK_TERMS; pgz_mode 0 / 1 (window median) / 2 (depth
    under the centre); weights (9).  -> red (9), stats (8), dec (n,17), pbox (n,4), validf (n)."""
    if kf > WEAK_MAX_SLOTS:
        raise _lib.CrError(f"weak_cube_loss: {kf} foreground slots per image, the kernels take up to {WEAK_MAX_SLOTS}")
    return _WeakCubeLoss.apply(raw, tuple(layout), K, cls, valid, gt_idx, kf, gt_boxes, gt3d, gtpose.reshape(gtpose.shape[0], -1, 9),
                               prior_mean, prior_std, meta, table, normals, boxes, depth, terms, pgz_mode, tuple(weights), allocentric,
                               z_cfg or z_config(z_type))


# --------------------------------------------------------------------------
# optimizer
# --------------------------------------------------------------------------
class _RPNUnpack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, *ys):
        L, B, C = len(ys), ys[0].shape[0], ys[0].shape[-1]
        ys = [y.contiguous() for y in ys]
        cells = [y.numel() // (B * C) for y in ys]
        atot, amax = sum(cells) * A, max(cells) * A
        dev = ys[0].device
        logits = torch.empty((B, atot), dtype=f32, device=dev)
        deltas = torch.empty((B, atot, 4), dtype=f32, device=dev)
        padded = torch.empty((B, L, amax), dtype=f32, device=dev)
        yp, ca = (_ct.c_void_p * L)(*[y.data_ptr() for y in ys]), (_ct.c_int * L)(*cells)
        _lib.call("cr_rpn_unpack", yp, ca, L, B, A, C, logits, deltas, padded)
        ctx.cfg = (A, C, B, cells, [tuple(y.shape) for y in ys])
        ctx.set_materialize_grads(False)       # outputs nobody differentiates arrive as None, not as zero fills
        ctx.mark_non_differentiable(padded)
        return logits, deltas, padded

    @staticmethod
    def backward(ctx, dlogits, ddeltas, _dpad):
        A, C, B, cells, shapes = ctx.cfg
        L = len(cells)
        ref = dlogits if dlogits is not None else ddeltas
        dys = [torch.empty(s, dtype=f32, device=ref.device) for s in shapes]
        dl = None if dlogits is None else dlogits.contiguous()
        dd = None if ddeltas is None else ddeltas.contiguous()
        dp, ca = (_ct.c_void_p * L)(*[d.data_ptr() for d in dys]), (_ct.c_int * L)(*cells)
        _lib.call("cr_rpn_pack_grad", dl, dd, dp, ca, L, B, A, C)
        return (None,) + tuple(dys)


class _RPNUnpackStacked(torch.autograd.Function):
    """_RPNUnpack on ONE tensor Y (1,1,sum_l B H_l W_l,C) whose row blocks are the levels (conv_bias_act_group(stacked=True)
    followed by the 1x1 predictor convolution): same two kernels, level pointers = offsets into Y, one gradient tensor back"""

    @staticmethod
    def forward(ctx, A, cells, B, Y):
        Y = Y.contiguous()
        L, C = len(cells), Y.shape[-1]
        assert Y.numel() == B * sum(cells) * C, "stacked RPN output does not match the level sizes"
        atot, amax = sum(cells) * A, max(cells) * A
        dev = Y.device
        logits = torch.empty((B, atot), dtype=f32, device=dev)
        deltas = torch.empty((B, atot, 4), dtype=f32, device=dev)
        padded = torch.empty((B, L, amax), dtype=f32, device=dev)
        offs = [0]
        for c in cells:
            offs.append(offs[-1] + B * c * C * 4)
        yp, ca = (_ct.c_void_p * L)(*[Y.data_ptr() + o for o in offs[:-1]]), (_ct.c_int * L)(*cells)
        _lib.call("cr_rpn_unpack", yp, ca, L, B, A, C, logits, deltas, padded)
        ctx.cfg = (A, C, B, tuple(cells), tuple(Y.shape), offs)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(padded)
        return logits, deltas, padded

    @staticmethod
    def backward(ctx, dlogits, ddeltas, _dpad):
        A, C, B, cells, shape, offs = ctx.cfg
        L = len(cells)
        ref = dlogits if dlogits is not None else ddeltas
        dY = torch.empty(shape, dtype=f32, device=ref.device)
        dl = None if dlogits is None else dlogits.contiguous()
        dd = None if ddeltas is None else ddeltas.contiguous()
        dp, ca = (_ct.c_void_p * L)(*[dY.data_ptr() + o for o in offs[:-1]]), (_ct.c_int * L)(*cells)
        _lib.call("cr_rpn_pack_grad", dl, dd, dp, ca, L, B, A, C)
        return None, None, None, dY


def rpn_unpack_stacked(Y, cells, B, A):
    """rpn_unpack for the stacked head output: Y (1,1,B*sum(cells),C), cells = H_l*W_l per level"""
    return _RPNUnpackStacked.apply(int(A), tuple(int(c) for c in cells), int(B), Y)


def rpn_unpack(ys, A):
    """per-level RPN head outputs y_l (B,H,W,16) f32 [A logits | 4A deltas | pad] -> (logits (B,Atot), deltas (B,Atot,4),
    per-level logits padded with -inf (B,L,amax)) with ONE launch each way (was a slice copy per level and output, three cats,
    a fill and five copies; backward: a zero-fill, a slice copy and an add per level and output)"""
    return _RPNUnpack.apply(int(A), *ys)


def gt_pack(gt_instances, G, boxes, classes, boxes3D, poses):
    """fills the padded ground-truth tensors (B,G,...) of the static-shape training path from per-image Instances in one
    launch (include/cr3dod.h, cr_gt_pack); the outputs may be freshly allocated or the static buffers of a captured graph"""
    B = len(gt_instances)
    keep = []

    def dev(t, dt):
        t = t.to(device=boxes.device, dtype=dt).contiguous()
        keep.append(t)
        return t.data_ptr()
    PA, IA = _ct.c_void_p * B, _ct.c_int * B
    bp, cp, b3, pp, cnt = PA(), PA(), PA(), PA(), IA()
    for i, g in enumerate(gt_instances):
        n = len(g)
        cnt[i] = n
        bp[i] = dev(g.gt_boxes.tensor, f32) if n else None
        cp[i] = dev(g.gt_classes, torch.int64) if n else None
        has3 = n and g.has("gt_boxes3D")
        b3[i] = dev(g.gt_boxes3D, f32) if has3 else None
        pp[i] = dev(g.gt_poses, f32) if has3 else None
    _lib.call("cr_gt_pack", bp, cp, b3, pp, cnt, B, int(G), boxes, classes, boxes3D, poses)


def topk(x, k):
    """row-wise top-k of a 2-D float32 tensor: (values sorted descending, int64 indices), ties -> lower index first;
    own radix-select + bitonic merge (csrc/topk.hip: two launches, no memset nodes).  Shapes outside the kernel's range
    (k > 2048, too many candidates) fall back to torch.topk."""
    _need_cuda(x, "topk input")
    assert x.dim() == 2 and x.dtype == f32
    rows, n = x.shape
    nb = _lib.topk_blocks(n, k) if k >= 1 else 0
    if k < 1 or k > 2048 or k > n or nb * k > 16384:
        if torch.cuda.is_current_stream_capturing():
            # torch.topk's multi-block path zeroes its counters with hipMemsetAsync = memset NODES in the captured graph,
            # the cause of the memory faults between back-to-back replays of the whole-step graph
            raise _lib.CrError(f"topk: rows of {n} values with k = {k} are outside the range of csrc/topk.hip (k <= 2048, "
                               f"chunks x k <= 16384) and the torch.topk fallback must not be captured into a HIP graph; "
                               f"run this configuration with CR_GRAPHS=dense or none")
        return x.topk(k, dim=1)
    xc = x.contiguous()
    ws = torch.empty((rows * nb * k,), dtype=torch.int64, device=x.device)
    vals = torch.empty((rows, k), dtype=f32, device=x.device)
    idx = torch.empty((rows, k), dtype=torch.int64, device=x.device)
    _lib.call("cr_topk", xc, rows, n, k, ws, vals, idx)
    return vals, idx


def loss_guard(vals, scale, red, total, recent, stabilize, tolerance, gamma, flag):
    """divergence guard of train_net.py:202-220 in one launch (see include/cr3dod.h); all tensors on the device, in place"""
    _lib.call("cr_loss_guard", vals, vals.numel(), float(scale), red, total, recent, int(bool(stabilize)), float(tolerance),
              float(gamma), flag)


def step_counters(flag, explode, success):
    _lib.call("cr_step_counters", flag, explode, success)


def nonfinite_flag(flat_grad, flag):
    _lib.call("cr_nonfinite_flag", flat_grad, flat_grad.numel(), flag)


def sgd_step(p, g, m, lr, momentum, weight_decay, grad_scale=1.0, skip_flag=None, lr_scale_dev=None, nesterov=False):
    """lr_scale_dev: optional device float; the step uses lr * lr_scale_dev[0] (read on the device -> graph-capturable)"""
    _lib.call("cr_sgd_step_nesterov" if nesterov else "cr_sgd_step", p, g, m, p.numel(), float(lr), lr_scale_dev, float(momentum),
              float(weight_decay), float(grad_scale), skip_flag)


def grad_clip_value(g, clip_value, grad_scale=1.0):
    """SOLVER.CLIP_GRADIENTS, CLIP_TYPE 'value': g = clamp(g * grad_scale, -clip_value, clip_value) in place"""
    _lib.call("cr_grad_clip_value", g, g.numel(), float(clip_value), float(grad_scale))


def grad_clip_norm(g, starts, counts, max_norm, norm_type=2.0, grad_scale=1.0, partial=None):
    """CLIP_TYPE 'norm': every parameter (starts[i], counts[i] inside the flat gradient g) scaled on its own by
    min(1, max_norm / (||g_i * grad_scale|| + 1e-6)), grad_scale folded in; partial: (len(starts) * 16,) float scratch"""
    n = int(starts.numel())
    if partial is None:
        partial = torch.empty(n * 16, dtype=torch.float32, device=g.device)
    _lib.call("cr_grad_clip_norm", g, starts, counts, n, float(max_norm), float(norm_type), float(grad_scale), partial)


def adam_tick(step, skip_flag=None):
    """advance the device-side count of applied Adam updates unless the step is skipped (cr_adam_tick)"""
    _lib.call("cr_adam_tick", step, skip_flag)


def adam_step(p, g, exp_avg, exp_avg_sq, max_exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, skip_flag=None,
              lr_scale_dev=None, decoupled=False):
    """torch.optim.Adam (decoupled=False) / AdamW (True) on one hyper-parameter segment of the flat buffers; max_exp_avg_sq:
    the amsgrad state or None; step: device float advanced by adam_tick"""
    _lib.call("cr_adam_step", p, g, exp_avg, exp_avg_sq, max_exp_avg_sq, p.numel(), float(lr), lr_scale_dev, float(beta1),
              float(beta2), float(eps), float(weight_decay), float(grad_scale), int(bool(decoupled)), step, skip_flag)


# --------------------------------------------------------------------------
# Depth-Anything-V2 forward ops (inference only: no autograd)
# --------------------------------------------------------------------------
def attention(qkv, B, N, H, D, scale):
    """qkv (B*N, 3*H*D) bf16 = output of the qkv linear -> (B*N, H*D) bf16 (cr_attention_fwd)."""
    _need_cuda(qkv, "attention input")
    assert qkv.dtype == bf16 and qkv.is_contiguous() and qkv.shape == (B * N, 3 * H * D)
    out = torch.empty((B * N, H * D), dtype=bf16, device=qkv.device)
    _lib.call("cr_attention_fwd", qkv, out, B, N, H, D, float(scale))
    return out


def layernorm(x, gamma, beta, eps):
    _need_cuda(x, "layernorm input")
    assert x.dtype == bf16 and x.is_contiguous() and x.dim() == 2
    y = torch.empty_like(x)
    _lib.call("cr_layernorm", x, gamma.detach().float().contiguous(), beta.detach().float().contiguous(), y, x.shape[0],
              x.shape[1], float(eps))
    return y


def gelu_(x):
    _need_cuda(x, "gelu input")
    assert x.dtype == bf16 and x.is_contiguous()
    _lib.call("cr_gelu_inplace", x, x.numel())
    return x


def scale_residual(x, y, gamma=None):
    """x + gamma * y on (M,C) bf16"""
    _need_cuda(x, "residual input")
    assert x.dtype == bf16 and y.dtype == bf16 and x.is_contiguous() and y.is_contiguous() and x.shape == y.shape
    out = torch.empty_like(x)
    g = gamma.detach().float().contiguous() if gamma is not None else None
    _lib.call("cr_scale_residual", x, y, g, out, x.shape[0], x.shape[1])
    return out


def scale_residual_layernorm(x, y, ls, gamma, beta, eps):
    """(x + ls * y, LayerNorm(x + ls * y)) on (M,C) bf16 in one kernel"""
    _need_cuda(x, "residual input")
    assert x.dtype == bf16 and y.dtype == bf16 and x.is_contiguous() and y.is_contiguous() and x.shape == y.shape
    xo, ho = torch.empty_like(x), torch.empty_like(x)
    l = ls.detach().float().contiguous() if ls is not None else None
    _lib.call("cr_scale_residual_layernorm", x, y, l, gamma.detach().float().contiguous(), beta.detach().float().contiguous(),
              xo, ho, x.shape[0], x.shape[1], float(eps))
    return xo, ho


def resize_bilinear_ac(x, size):
    """F.interpolate(..., mode='bilinear', align_corners=True) on NHWC bf16"""
    _need_cuda(x, "resize input")
    assert x.dtype == bf16 and x.is_contiguous() and x.dim() == 4
    B, h, w, C = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    y = torch.empty((B, Ho, Wo, C), dtype=bf16, device=x.device)
    _lib.call("cr_resize_bilinear_ac", x, y, B, h, w, Ho, Wo, C)
    return y


# --------------------------------------------------------------------------
# Depth-Anything-V2 training ops (csrc/vit_bwd.hip): the ops above as autograd Functions, reached only by the model's
# training route.  Parameter gradients go to the optimizer's flat-gradient sinks when the parameters carry them
# (grad_sink), else to param.grad.  No float atomics: two backward passes over the same inputs give the same bits.
# --------------------------------------------------------------------------
RED_PARTS = 128          # partial rows of the two-stage column reductions (csrc/vit_bwd.hip)


def attention_lse(qkv, B, N, H, D, scale):
    """ops.attention (bit-identical output, same kernel body) plus the per-row log-sum-exp (B,H,N) f32"""
    _need_cuda(qkv, "attention input")
    assert qkv.dtype == bf16 and qkv.is_contiguous() and qkv.shape == (B * N, 3 * H * D)
    out = torch.empty((B * N, H * D), dtype=bf16, device=qkv.device)
    lse = torch.empty((B, H, N), dtype=f32, device=qkv.device)
    _lib.call("cr_attention_fwd_lse", qkv, out, lse, B, N, H, D, float(scale))
    return out, lse


def attention_bwd(qkv, dout, lse, B, N, H, D, scale):
    """dqkv in the packed layout of qkv (what the qkv linear's backward consumes)"""
    _need_cuda(qkv, "attention input")
    assert qkv.dtype == bf16 and dout.dtype == bf16 and lse.dtype == f32
    assert qkv.is_contiguous() and dout.is_contiguous() and lse.is_contiguous()
    assert qkv.shape == (B * N, 3 * H * D) and dout.shape == (B * N, H * D) and lse.shape == (B, H, N)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, H, N), dtype=f32, device=qkv.device)
    _lib.call("cr_attention_bwd", qkv, dout, lse, delta, dqkv, B, N, H, D, float(scale))
    return dqkv


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, B, N, H, D, scale):
        out, lse = attention_lse(qkv, B, N, H, D, scale)
        ctx.save_for_backward(qkv, lse)
        ctx.cfg = (B, N, H, D, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, lse = ctx.saved_tensors
        return (attention_bwd(qkv, _act_cast(dout, bf16), lse, *ctx.cfg),) + (None,) * 5


def attention_train(qkv, B, N, H, D, scale):
    return _Attention.apply(qkv, B, N, H, D, scale)


def _param_acc(p, n, dev):
    """(accumulator, grad to return): the parameter's flat-gradient sink, or a zero buffer that becomes its autograd grad"""
    sink = grad_sink(p)
    if sink is not None:
        return sink, None
    z = torch.zeros((n,), dtype=f32, device=dev)
    return z, z


def layernorm_bwd_raw(x, dy, gamma, dgamma, dbeta, eps, accumulate):
    """x (M,C) bf16 or float32 (the training route's residual stream); dx comes back in x's dtype.  dgamma / dbeta: f32
    accumulators, either may be None (not wanted)"""
    M, C = x.shape
    assert x.dtype in (bf16, f32) and x.is_contiguous() and dy.dtype == bf16 and dy.is_contiguous()
    dx = torch.empty_like(x)
    part = torch.empty((RED_PARTS * 2 * C,), dtype=f32, device=x.device)
    _lib.call("cr_layernorm_bwd", x, dy, gamma.detach().float().contiguous(), dx, dgamma, dbeta, part, M, C, float(eps),
              int(accumulate), int(x.dtype == f32))
    return dx


def layernorm_f32in(x, gamma, beta, eps):
    """LayerNorm of float32 rows -> bf16 (cr_layernorm_f32in)"""
    _need_cuda(x, "layernorm input")
    assert x.dtype == f32 and x.is_contiguous() and x.dim() == 2
    y = torch.empty(x.shape, dtype=bf16, device=x.device)
    _lib.call("cr_layernorm_f32in", x, gamma.detach().float().contiguous(), beta.detach().float().contiguous(), y, x.shape[0],
              x.shape[1], float(eps))
    return y


def scale_residual_f32(x, y, gamma=None):
    """x + gamma * y with float32 x and result, bf16 y (cr_scale_residual_f32)"""
    _need_cuda(x, "residual input")
    assert x.dtype == f32 and y.dtype == bf16 and x.is_contiguous() and y.is_contiguous() and x.shape == y.shape
    out = torch.empty_like(x)
    g = gamma.detach().float().contiguous() if gamma is not None else None
    _lib.call("cr_scale_residual_f32", x, y, g, out, x.shape[0], x.shape[1])
    return out


class _LayerNorm(torch.autograd.Function):
    """(like _Linear, the parameters ride on ctx as plain references and the backward re-reads gamma: a weight update
    between a forward and its backward is not detected -- the training loops here update after the backward)"""
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        ctx.save_for_backward(x)
        ctx.refs, ctx.eps = (gamma, beta), eps
        return layernorm_f32in(x, gamma, beta, eps) if x.dtype == f32 else layernorm(x, gamma, beta, eps)

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        gamma, beta = ctx.refs
        C = x.shape[1]
        ag, gg = _param_acc(gamma, C, x.device) if ctx.needs_input_grad[1] else (None, None)
        ab, gb = _param_acc(beta, C, x.device) if ctx.needs_input_grad[2] else (None, None)
        dx = layernorm_bwd_raw(x, _act_cast(dy, bf16), gamma, ag, ab, ctx.eps, accumulate=True)
        return dx, gg, gb, None


def layernorm_train(x, gamma, beta, eps):
    return _LayerNorm.apply(x, gamma, beta, eps)


def gelu_fwd_raw(x):
    y = torch.empty_like(x)
    _lib.call("cr_gelu_fwd", x, y, x.numel())
    return y


def gelu_bwd_raw(x, dy):
    dx = torch.empty_like(x)
    _lib.call("cr_gelu_bwd", x, dy, dx, x.numel())
    return dx


class _Gelu(torch.autograd.Function):
    """exact GELU that keeps the pre-activation (the inference path's gelu_ works in place)"""
    @staticmethod
    def forward(ctx, x):
        _need_cuda(x, "gelu input")
        assert x.dtype == bf16 and x.is_contiguous()
        ctx.save_for_backward(x)
        return gelu_fwd_raw(x)

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        return gelu_bwd_raw(x, _act_cast(dy, bf16))


def gelu_train(x):
    return _Gelu.apply(x)


def layerscale_bwd_raw(g, y, gamma, dgamma, accumulate):
    M, C = g.shape
    dy = torch.empty_like(g)
    part = torch.empty((RED_PARTS * C,), dtype=f32, device=g.device)
    _lib.call("cr_layerscale_bwd", g, y, gamma.detach().float().contiguous(), dy, dgamma, part, M, C, int(accumulate))
    return dy


class _ScaleResidual(torch.autograd.Function):
    """(gamma rides on ctx as a plain reference and is re-read in the backward, like _Linear's weight)"""
    @staticmethod
    def forward(ctx, x, y, gamma):
        ctx.save_for_backward(y)
        ctx.gamma = gamma
        return scale_residual_f32(x, y, gamma) if x.dtype == f32 else scale_residual(x, y, gamma)

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        gamma = ctx.gamma
        gb = _act_cast(g, bf16)                 # the branch's gradient is bf16; the stream's passes through in its own dtype
        if gamma is None:
            return g, gb, None
        acc, gg = _param_acc(gamma, gamma.numel(), g.device)
        return g, layerscale_bwd_raw(gb, y, gamma, acc, accumulate=True), gg


def scale_residual_train(x, y, gamma=None):
    return _ScaleResidual.apply(x, y, gamma)


def resize_bilinear_ac_bwd_raw(dy, in_shape):
    B, h, w, C = in_shape
    assert dy.dtype == bf16 and dy.is_contiguous() and dy.shape[0] == B and dy.shape[3] == C
    dx = torch.empty((B, h, w, C), dtype=bf16, device=dy.device)
    _lib.call("cr_resize_bilinear_ac_bwd", dy, dx, B, h, w, dy.shape[1], dy.shape[2], C)
    return dx


class _ResizeBilinearAC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size):
        ctx.in_shape = tuple(x.shape)
        return resize_bilinear_ac(x, size)

    @staticmethod
    def backward(ctx, dy):
        return resize_bilinear_ac_bwd_raw(_act_cast(dy, bf16), ctx.in_shape), None


def resize_bilinear_ac_train(x, size):
    return _ResizeBilinearAC.apply(x, size)


def _depth_args(pred, target, valid):
    _need_cuda(pred, "depth prediction")
    assert pred.shape == target.shape == valid.shape and pred.dim() == 3, "pred / target / valid are (B,H,W)"
    assert pred.dtype == f32 and target.dtype == f32
    v = valid.contiguous()
    v = v.view(torch.uint8) if v.dtype == torch.bool else (v != 0).view(torch.uint8)
    return pred.contiguous(), target.contiguous(), v


def depth_reduce(pred, target, valid):
    """(B,10) float64 per-image masked sums (cr_depth_reduce): count, sum dl, sum dl^2, sum |d|/t, sum d^2/t, sum d^2,
    sum |log10 p - log10 t|, and the counts of max(t/p, p/t) < 1.25, 1.25^2, 1.25^3"""
    p, t, v = _depth_args(pred, target, valid)
    sums = torch.empty((p.shape[0], 10), dtype=torch.float64, device=p.device)
    _lib.call("cr_depth_reduce", p, t, v, sums, p.shape[0], p.shape[1] * p.shape[2])
    return sums


class _SiLog(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, valid, lambd):
        p, t, v = _depth_args(pred, target, valid)
        s = depth_reduce(p, t, v).sum(0)
        n, s1, s2 = s[0], s[1], s[2]
        loss = torch.sqrt(s2 / n - lambd * (s1 / n) ** 2)
        ctx.save_for_backward(p, t, v, torch.stack((1.0 / (n * loss), lambd * s1 / (n * n * loss))))
        return loss.to(f32)

    @staticmethod
    def backward(ctx, gout):
        p, t, v, coef = ctx.saved_tensors
        dpred = torch.empty_like(p)
        _lib.call("cr_silog_bwd", p, t, v, (coef * gout.double()).to(f32), dpred, p.numel())
        return dpred, None, None, None


def silog_loss(pred, target, valid, lambd=0.5):
    """SiLogLoss of the reference (util/loss.py) over the valid pixels of the whole batch: sqrt(mean dl^2 - lambd mean(dl)^2),
    dl = log target - log pred; differentiable in pred (closed-form gradient, one element-wise kernel; exactly 0 on invalid
    pixels).  pred / target (B,H,W) f32, valid (B,H,W) bool."""
    return _SiLog.apply(pred, target, valid, float(lambd))


DEPTH_METRICS = ("d1", "d2", "d3", "abs_rel", "sq_rel", "rmse", "rmse_log", "log10", "silog")


def depth_metrics(pred, target, valid):
    """eval_depth of the reference (util/metric.py) over the valid pixels of ONE image: pred / target / valid (H,W) or
    (1,H,W) -> dict of the nine values (python floats)"""
    if pred.dim() == 2:
        pred, target, valid = pred[None], target[None], valid[None]
    assert pred.shape[0] == 1, "depth_metrics takes one image (the reference validates at batch 1)"
    s = depth_reduce(pred, target, valid)[0]
    n = s[0]
    vals = torch.stack((s[7] / n, s[8] / n, s[9] / n, s[3] / n, s[4] / n, torch.sqrt(s[5] / n), torch.sqrt(s[2] / n), s[6] / n,
                        torch.sqrt(s[2] / n - 0.5 * (s[1] / n) ** 2))).tolist()
    return dict(zip(DEPTH_METRICS, vals))
