"""The fused Winograd product + output-transform kernel (cr_wino_gemm_output, reached through ops.wino_conv3x3_group) against the
unfused arithmetic it replaces, bit for bit: cr_wino_filter, cr_wino_input and cr_gemm_batched_f32 into the M planes, then the
output transform y = A^T M A (+ bias, ReLU, + acc) in torch float32 on the device, written in the association the kernel
documents (torch's elementwise add / sub / max are plain IEEE operations, so torch.equal is the bound).

Cases (N = 2): maps [(16,24), (4,6), (2,2)] -- T = 206, a multiple of no row tile, one row tile spans three maps; [(2,6)] --
T = 6, less than one row tile; [(32,32)] -- T = 512, an exact multiple; each with (C, O) giving one and two channel tiles on
either side.  Float32 only."""
import ctypes
import functools
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dod_amd.hipops")
lib = importlib.import_module("3dod_amd._lib")
DEV = "cuda:0"
f32 = torch.float32

MAPS = {"three_maps": [(16, 24), (4, 6), (2, 2)], "below_one_tile": [(2, 6)], "exact_multiple": [(32, 32)]}
CHANNELS = [(128, 128), (256, 128), (128, 256)]
GUARD = 4096            # floats around a destination map (a multiple of 4: the stores are 16-byte aligned)
SENTINEL = -7.25e7


def _cast(a):
    return ctypes.cast(a, ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def problem(case, C, O, backward):
    """inputs of one call and the M planes of the unfused pipeline (computed once per case, shared, never modified)"""
    sizes = MAPS[case]
    g = torch.Generator().manual_seed(1000 * len(sizes) + C + 3 * O + int(backward))
    cin, cout = (O, C) if backward else (C, O)
    srcs = [(torch.randn(2, h, w, cin, generator=g) * 0.7).to(DEV) for h, w in sizes]
    w = (torch.randn(O, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(DEV).contiguous(memory_format=torch.channels_last)
    bias = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    accs = [torch.randn(2, h, w_, cout, generator=g).to(DEV) for h, w_ in sizes]
    T = sum(2 * (h // 2) * (w_ // 2) for h, w_ in sizes)
    U = torch.empty(16 * O * C, dtype=f32, device=DEV)
    V = torch.empty((16, T, cin), dtype=f32, device=DEV)
    M = torch.empty((16, T, cout), dtype=f32, device=DEV)
    Ns, Hs, Ws = ops._int_table([2] * len(sizes)), ops._int_table([h for h, _ in sizes]), ops._int_table([w_ for _, w_ in sizes])
    lib.call("cr_wino_filter", w, U, O, C, int(backward))
    lib.call("cr_wino_input", len(srcs), _cast(ops._ptr_table(srcs)), _cast(Ns), _cast(Hs), _cast(Ws), cin, V, T)
    lib.call("cr_gemm_batched_f32", V, U, M, T, cin, cout, 16, T * cin, cout * cin, T * cout)
    torch.cuda.synchronize()
    return srcs, w, bias, accs, M, T


def reference(case, C, O, backward, bias, relu, accs):
    """A^T M A per 2 x 2 tile in the kernel's association, + bias, ReLU, + acc, laid out per map"""
    sizes = MAPS[case]
    M = problem(case, C, O, backward)[4]
    q = M.view(4, 4, M.shape[1], M.shape[2])                     # q[i][j]: position k = 4 i + j
    s = [(q[0] + q[1]) + q[2], (q[1] - q[2]) - q[3]]             # s[r][j] over all tiles
    y = [[(s[r][0] + s[r][1]) + s[r][2], (s[r][1] - s[r][2]) - s[r][3]] for r in range(2)]
    outs, tb = [], 0
    for mi, (h, w_) in enumerate(sizes):
        th, tw = h // 2, w_ // 2
        n = 2 * th * tw
        rows = [torch.stack([y[r][c][tb:tb + n].view(2, th, tw, -1) for c in range(2)], dim=3) for r in range(2)]   # (2,th,tw,2,O)
        o = torch.stack(rows, dim=2).reshape(2, h, w_, -1)       # (2, th, 2, tw, 2, O)
        if bias is not None:
            o = o + bias
        if relu:
            o = torch.maximum(o, torch.zeros((), device=DEV))
        if accs is not None and accs[mi] is not None:
            o = o + accs[mi]
        outs.append(o)
        tb += n
    return outs


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("C,O", CHANNELS)
@pytest.mark.parametrize("case", list(MAPS))
def test_forward_bit_equal_to_unfused(case, C, O, with_bias, relu):
    srcs, w, bias, _, _, _ = problem(case, C, O, False)
    b = bias if with_bias else None
    ys = [torch.full((x.shape[0], x.shape[1], x.shape[2], O), SENTINEL, device=DEV) for x in srcs]
    ops.wino_conv3x3_group(srcs, w, ys, b, relu, None, False)
    for y, r in zip(ys, reference(case, C, O, False, b, relu, None)):
        assert torch.equal(y, r)


@pytest.mark.parametrize("last_acc", [True, False])
@pytest.mark.parametrize("C,O", CHANNELS)
@pytest.mark.parametrize("case", list(MAPS))
def test_backward_data_bit_equal_to_unfused(case, C, O, last_acc):
    gs, w, _, accs, _, _ = problem(case, C, O, True)
    accs = list(accs)
    if not last_acc:
        accs[-1] = None
    dxs = [torch.full((g.shape[0], g.shape[1], g.shape[2], C), SENTINEL, device=DEV) for g in gs]
    ops.wino_conv3x3_group(gs, w, dxs, None, False, accs, True)
    for dx, r in zip(dxs, reference(case, C, O, True, None, False, accs)):
        assert torch.equal(dx, r)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("C,O", CHANNELS)
def test_nothing_outside_the_maps_is_written(C, O, backward):
    """every destination map sits inside a larger sentinel-filled buffer: tail rows of the last row tile and a wrong map
    decode would land in the guards (or in a neighbouring map, which the equality catches)"""
    case = "three_maps"
    srcs, w, bias, accs, _, _ = problem(case, C, O, backward)
    cout = C if backward else O
    bufs, dsts = [], []
    for x in srcs:
        n = x.shape[0] * x.shape[1] * x.shape[2] * cout
        buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
        bufs.append(buf)
        dsts.append(buf[GUARD:GUARD + n].view(x.shape[0], x.shape[1], x.shape[2], cout))
    if backward:
        ops.wino_conv3x3_group(srcs, w, dsts, None, False, accs, True)
        refs = reference(case, C, O, True, None, False, accs)
    else:
        ops.wino_conv3x3_group(srcs, w, dsts, bias, True, None, False)
        refs = reference(case, C, O, False, bias, True, None)
    guard = torch.full((GUARD,), SENTINEL, device=DEV)
    for buf, d, r in zip(bufs, dsts, refs):
        assert torch.equal(buf[:GUARD], guard) and torch.equal(buf[-GUARD:], guard)
        assert torch.equal(d, r)
