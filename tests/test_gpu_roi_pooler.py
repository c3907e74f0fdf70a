"""GPU: the RoI pooler's other types and a fixed sampling ratio -- cr_roi_pool_fwd / cr_roi_pool_bwd / cr_roi_pool_bwd_set
(csrc/detection.hip: the five RoIAlign kernels instantiated on the sample geometry, k_roi_pool_fwd / k_roi_pool_bwd).

The file carries its own restatement of torchvision's roi_align / roi_pool and detectron2's level assignment (the call sites of
the reference are roi_heads.py:2071-2080,2178,2273): sample and bin coordinates in float32 in the kernels' expression order, as
torchvision computes them for float32 input; weights, products and sums in float64.

  1. RoIAlign variants (ROIAlignV2 / ROIAlign x sampling ratio 0, 1, 2, 3): forward, atomic backward and tile-owner backward
     against the restatement at normwise 1e-5 per tensor, tile-owner against atomic at 2e-6, tile-owner bit-reproducible; the old
     entry points against the restatement in its default mode (which pins the restatement's coordinate arithmetic).
     Measured on the MI355X (worst over the cases; also in DESIGN.md section 4): forward 1.6e-6, atomic and tile-owner backward
     1.6e-6 at 306 RoIs and 2.3e-6 at 2048, tile-owner against atomic 1.2e-7, the old entry points 1.1e-6; ROIPool backward 2e-7.
  2. (ROIAlignV2, ratio 0) through the new entry points is bit-equal to cr_roi_align_fwd / cr_roi_align_bwd_set and within 2e-6
     of cr_roi_align_bwd.
  3. ROIPool: output and argmax equal the restatement exactly in f32 and bf16 storage, backward within 2e-6 of a float64 scatter,
     empty bins give 0 and no gradient, the first maximum wins, a NaN never wins.
  4. default keywords launch the old entry points; equal non-default poolers pool once per step, different ones twice.
  5. a model with each setting trains two steps through solver.make_train_step with the graph cache on, and infers."""
import ctypes
import importlib
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dod_amd.hipops")
_lib = importlib.import_module("3dod_amd._lib")
DEV = torch.device("cuda:0")
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
SCALES = [1 / 4, 1 / 8, 1 / 16, 1 / 32, 1 / 64]
F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


def _rois(n_img, R, size, g, clustered=True):
    """Omni3D-shaped RoIs (the generator of tests/test_gpu_roi_bwd_tiles.py): clusters of near-duplicate proposals around a few
    centres per image, all pyramid levels"""
    img = torch.randint(0, n_img, (R,), generator=g).float()
    k = 12
    centres = torch.rand(n_img, k, 2, generator=g) * size
    which = torch.randint(0, k, (R,), generator=g)
    ctr = centres[img.long(), which] + torch.randn(R, 2, generator=g) * (8 if clustered else size / 4)
    wh = torch.exp(torch.rand(R, 2, generator=g) * 3.2 + 2.5)                  # 12 ... 300 px
    b = torch.cat([ctr - wh / 2, ctr + wh / 2], 1).clamp(0, size - 1)
    return torch.cat([img[:, None], b], 1)


NAN = float("nan")
# the edge-case list of tests/test_gpu_roi_bwd_tiles.py (192^2 images: 48 x 48 ... 3 x 3 maps, partial tiles on every level)
EDGE_ROIS = torch.tensor([[0, 10., 10, 60, 70], [1, -300, -300, -200, -250],      # far outside: no sample
                          [0, -20, -30, 40, 50], [1, 150, 160, 400, 420],         # crossing the border
                          [0, 50, 50, 50, 50], [1, 30, 40, 30.5, 41],            # empty / sub-pixel
                          [0, NAN, 0, 50, 50], [1, 0, 0, 191, 191],              # NaN box; whole image (top level, one tile)
                          [0, 0, 0, 191, 191], [1, 96, 0, 97, 191]])             # very elongated


# ------------------------------------------------------------------------------------------------ the restatement
def roi_level(b, nlev, min_level=2):
    """detectron2 assign_boxes_to_levels in float32: floor(4 + log2(sqrt(area) / 224 + 1e-8)) clamped to the pyramid"""
    with np.errstate(invalid="ignore"):
        area = F(F(b[2] - b[0]) * F(b[3] - b[1]))
        lv = np.floor(F(4.0) + np.log2(F(np.sqrt(area) / F(224.0)) + F(1e-8)))
    lv = min(max(lv, F(min_level)), F(min_level + nlev - 1)) if lv == lv else F(min_level)
    return int(lv) - min_level


def axis_weights(a1, a2, sc, P, L, ptype, ratio):
    """(L, P) float64: column p = the weights of the samples of bin p on the L pixels of the axis, averaged over the grid.
    Coordinates in float32: start = a1 sc - 0.5 (ROIAlignV2) | a1 sc (ROIAlign); extent = (a2 - a1) sc, >= 1 for ROIAlign;
    bin = extent / P; grid = ratio or ceil(extent / P); sample = start + p bin + (i + 0.5) bin / grid."""
    A = np.zeros((L, P), dtype=np.float64)
    a1, a2, sc = F(a1), F(a2), F(sc)
    start = F(F(a1 * sc) - F(0.5)) if ptype == 0 else F(a1 * sc)
    ext = F(F(a2 - a1) * sc)
    if ptype == 1 and ext < F(1.0):
        ext = F(1.0)
    bsz = F(ext / F(P))
    if not np.isfinite(bsz) or not np.isfinite(start):
        return A
    grid = ratio if ratio > 0 else int(np.ceil(F(ext / F(P))))
    for p in range(P):
        for i in range(grid):
            y = F(F(start + F(F(p) * bsz)) + F(F(F(i + 0.5) * bsz) / F(grid)))
            if not (y >= -1.0 and y <= L):
                continue
            y = max(y, F(0.0))
            lo = int(y)
            if lo >= L - 1:
                lo = hi = L - 1
                y = F(lo)
            else:
                hi = lo + 1
            l = float(F(y - F(lo)))
            A[lo, p] += (1.0 - l) / grid
            A[hi, p] += l / grid
    return A


def _span(A):
    nz = np.nonzero(A.any(1))[0]
    return (0, 0) if len(nz) == 0 else (int(nz[0]), int(nz[-1]) + 1)


def align_reference(shapes, feats, rois, dout, P, ptype, ratio):
    """feats: list of (N,H,W,C) float64 maps | None (backward only); dout (R,P,P,C) float64 -> (out (R,P,P,C) | None, list
    of gradient maps)"""
    N, C = shapes[0][0], shapes[0][3]
    R = rois.shape[0]
    out = None if feats is None else torch.zeros(R, P, P, C, dtype=f64)
    grads = [torch.zeros(s, dtype=f64) for s in shapes]
    rn = rois.numpy()
    for r in range(R):
        n = rn[r, 0]
        if not (n >= 0 and n < N):
            continue
        n = int(n)
        lv = roi_level(rn[r, 1:], len(shapes))
        H, W = shapes[lv][1], shapes[lv][2]
        Ay = axis_weights(rn[r, 2], rn[r, 4], SCALES[lv], P, H, ptype, ratio)
        Ax = axis_weights(rn[r, 1], rn[r, 3], SCALES[lv], P, W, ptype, ratio)
        (y0, y1), (x0, x1) = _span(Ay), _span(Ax)
        if y1 == y0 or x1 == x0:
            continue
        ay, ax = torch.from_numpy(Ay[y0:y1]), torch.from_numpy(Ax[x0:x1])
        if feats is not None:
            out[r] = torch.einsum("yp,yxc,xq->pqc", ay, feats[lv][n, y0:y1, x0:x1], ax)
        grads[lv][n, y0:y1, x0:x1] += torch.einsum("yp,pqc,xq->yxc", ay, dout[r], ax)
    return out, grads


def c_round(v):
    """C roundf of a float32 (half away from zero), computed exactly in float64"""
    v = float(v)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def pool_reference(feats, rois, P):
    """torchvision roi_pool per RoI on its level's map.  feats: list of (N,H,W,C) float32 numpy maps (the stored values).
    -> out (R,P,P,C) float32, argmax (R,P,P,C) int32 (y W + x, -1 where nothing won), levels, images"""
    N, C = feats[0].shape[0], feats[0].shape[3]
    R = rois.shape[0]
    out = np.zeros((R, P, P, C), dtype=np.float32)
    arg = np.full((R, P, P, C), -1, dtype=np.int32)
    lvs, ns = np.zeros(R, dtype=np.int64), np.full(R, -1, dtype=np.int64)
    rn = rois.numpy()
    for r in range(R):
        lv = lvs[r] = roi_level(rn[r, 1:], len(feats))
        n = rn[r, 0]
        if not (n >= 0 and n < N) or not np.isfinite(rn[r, 1:]).all():
            continue
        n = ns[r] = int(n)
        H, W = feats[lv].shape[1:3]
        sc = F(SCALES[lv])
        sw, sh, ew, eh = (c_round(F(F(rn[r, k]) * sc)) for k in (1, 2, 3, 4))
        rw, rh = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
        bh, bw = F(F(rh) / F(P)), F(F(rw) / F(P))
        for ph in range(P):
            hs, he = int(np.floor(F(F(ph) * bh))), int(np.ceil(F(F(ph + 1) * bh)))
            hs, he = min(max(hs + sh, 0), H), min(max(he + sh, 0), H)
            for pw in range(P):
                ws, we = int(np.floor(F(F(pw) * bw))), int(np.ceil(F(F(pw + 1) * bw)))
                ws, we = min(max(ws + sw, 0), W), min(max(we + sw, 0), W)
                if he <= hs or we <= ws:
                    continue                                                 # empty bin: 0, argmax -1
                v = feats[lv][n, hs:he, ws:we].reshape(-1, C)                # row-major scan
                v = np.where(np.isnan(v), -np.inf, v)                        # a NaN never wins
                k = v.argmax(0)                                              # the first maximum
                best = v[k, np.arange(C)]
                won = best > -FLT_MAX                                        # strict > from -FLT_MAX
                out[r, ph, pw] = np.where(won, best, F(-FLT_MAX))
                arg[r, ph, pw] = np.where(won, (hs + k // (we - ws)) * W + ws + k % (we - ws), -1)
    return out, arg, lvs, ns


# ------------------------------------------------------------------------------------------------ the entry points
def _pyr(ts):
    n = len(ts)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    Hs = (ctypes.c_int * n)(*[t.shape[1] for t in ts])
    Ws = (ctypes.c_int * n)(*[t.shape[2] for t in ts])
    sc = (ctypes.c_float * n)(*SCALES[:n])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    return n, cast(ptrs), cast(Hs), cast(Ws), cast(sc), (ptrs, Hs, Ws, sc)


def run_fwd(feats, rois, P, ptype, ratio, old=False):
    """feats on the device; -> (out, argmax | None)"""
    n, ptrs, Hs, Ws, sc, keep = _pyr(feats)
    N, C = feats[0].shape[0], feats[0].shape[3]
    R = rois.shape[0]
    out = torch.full((R, P, P, C), 7.0, dtype=feats[0].dtype, device=DEV)
    arg = torch.full((R, P, P, C), -7, dtype=torch.int32, device=DEV) if ptype == 2 else None
    af = 1 if feats[0].dtype == f32 else 0
    if old:
        _lib.call("cr_roi_align_fwd", ptrs, Hs, Ws, sc, n, C, rois, R, P, P, out, af)
    else:
        _lib.call("cr_roi_pool_fwd", ptrs, Hs, Ws, sc, n, C, N, rois, R, P, P, ptype, ratio, out, arg, af)
    torch.cuda.synchronize()
    return out, arg


def run_bwd(kind, shapes, rois, dout, P, ptype, ratio, argmax=None, old=False):
    """kind 'tiles' (overwrites: the maps start as garbage) | 'atomic' (adds: the maps start as zeros)"""
    grads = [torch.full(s, 7.0, dtype=f32, device=DEV) if kind == "tiles" else torch.zeros(s, dtype=f32, device=DEV) for s in shapes]
    n, ptrs, Hs, Ws, sc, keep = _pyr(grads)
    N, C = shapes[0][0], shapes[0][3]
    R = rois.shape[0]
    af = 1 if dout.dtype == f32 else 0
    if kind == "tiles":
        if old:
            _lib.call("cr_roi_align_bwd_set", ptrs, Hs, Ws, sc, n, C, N, rois, R, P, P, dout, af)
        else:
            _lib.call("cr_roi_pool_bwd_set", ptrs, Hs, Ws, sc, n, C, N, rois, R, P, P, ptype, ratio, dout, af)
    elif old:
        _lib.call("cr_roi_align_bwd", ptrs, Hs, Ws, sc, n, C, rois, R, P, P, dout, af)
    else:
        _lib.call("cr_roi_pool_bwd", ptrs, Hs, Ws, sc, n, C, N, rois, R, P, P, ptype, ratio, dout, argmax, af)
    torch.cuda.synchronize()
    return grads


def _rel(a, b):
    """normwise error of `a` against the reference `b` (float64, on the device)"""
    a, b = a.detach().to(DEV).double(), b.detach().to(DEV).double()
    return float((a - b).norm() / (b.norm() + 1e-20))


_CASES = {}


def case(name):
    """inputs made once per process and shared (never modified): maps, RoIs, upstream gradient"""
    if name not in _CASES:
        N, size, R, C, seed = {"c64": (2, 256, 300, 64, 300), "c128": (2, 256, 300, 128, 301), "edge": (2, 192, 0, 64, 3),
                               "big": (4, 512, 2048, 256, 2048)}[name]
        g = torch.Generator().manual_seed(seed)
        shapes = [(N, size // s, size // s, C) for s in (4, 8, 16, 32, 64)]
        rois = EDGE_ROIS.clone() if name == "edge" else _rois(N, R, size, g)
        if name in ("c64", "c128"):
            # the generator's boxes end at the image border (levels 0-2 at 256^2): a few larger ones reach the two top levels
            rois = torch.cat([rois, torch.tensor([[0, -200.0, -180, 450, 430], [1, -100, -300, 500, 390], [0, -500, -480, 700, 760],
                                                  [1, -400, -600, 800, 610], [1, 0, 0, 255, 255], [0, 100, -700, 180, 900]])])
        feats = None if name == "big" else [torch.randn(s, generator=g) for s in shapes]      # (big: backward only)
        dout = {P: torch.randn(rois.shape[0], P, P, C, generator=g) for P in ((7,) if name == "big" else (7, 14))}
        for d in dout.values():
            d[::7] = 0                                                       # masked (padding) RoI slots carry zero gradient
        _CASES[name] = dict(N=N, C=C, shapes=shapes, rois=rois, feats=feats, dout=dout,
                            feats_dev=None if feats is None else [f.to(DEV) for f in feats], rois_dev=rois.to(DEV))
    return _CASES[name]


_REFS = {}


def align_ref(name, P, ptype, ratio, forward=True):
    key = (name, P, ptype, ratio)
    if key not in _REFS:
        c = case(name)
        feats = [f.double() for f in c["feats"]] if forward else None
        _REFS[key] = align_reference(c["shapes"], feats, c["rois"], c["dout"][P].double(), P, ptype, ratio)
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ 1. the RoIAlign variants
def check_align(name, P, ptype, ratio, old=False, forward=True):
    c = case(name)
    ref_out, ref_g = align_ref(name, P, ptype, ratio, forward)
    rois, dout = c["rois_dev"], c["dout"][P].to(DEV)
    errs = {}
    if forward:
        out, _ = run_fwd(c["feats_dev"], rois, P, ptype, ratio, old=old)
        assert torch.isfinite(out).all()
        errs["fwd"] = _rel(out, ref_out)
    b = run_bwd("atomic", c["shapes"], rois, dout, P, ptype, ratio, old=old)
    errs["atomic"] = max(_rel(x, y) for x, y in zip(b, ref_g))
    if P == 7:
        a = run_bwd("tiles", c["shapes"], rois, dout, P, ptype, ratio, old=old)
        a2 = run_bwd("tiles", c["shapes"], rois, dout, P, ptype, ratio, old=old)
        for x, y in zip(a, a2):
            assert torch.equal(x, y), "the tile-owner backward must be bit-reproducible"
        assert all(torch.isfinite(x).all() for x in a)
        errs["tiles"] = max(_rel(x, y) for x, y in zip(a, ref_g))
        errs["tiles_vs_atomic"] = max(_rel(x, y) for x, y in zip(a, b))
    print("roi pooler %s P=%d type=%d ratio=%d%s: %s" % (name, P, ptype, ratio, " (old entry points)" if old else "",
                                                       " ".join("%s %.3g" % kv for kv in errs.items())))
    for k, v in errs.items():
        assert v < (2e-6 if k == "tiles_vs_atomic" else 1e-5), (k, v)
    return errs


@pytest.mark.parametrize("ratio", [0, 1, 2, 3])
@pytest.mark.parametrize("ptype", [0, 1])
@pytest.mark.parametrize("name", ["c64", "c128"])
def test_roialign_variants_match_float64(name, ptype, ratio):
    """all five levels, whole and partial tiles (64^2 ... 4^2 maps), C = 64 (the separable kernel's one-block form) and 128"""
    check_align(name, 7, ptype, ratio)


def test_old_entry_points_match_the_restatement():
    """the default kernels through cr_roi_align_* against the restatement in its default mode: pins the restatement itself"""
    check_align("c64", 7, 0, 0, old=True)
    check_align("edge", 7, 0, 0, old=True)


def test_roialign_p14_takes_the_atomic_route():
    check_align("c64", 14, 1, 2)


@pytest.mark.parametrize("ptype,ratio", [(0, 0), (0, 2), (1, 0), (1, 2), (1, 3)])
def test_roialign_variants_on_the_edge_cases(ptype, ratio):
    """boxes outside the map, crossing its border, empty, sub-pixel, NaN, the whole image, very elongated; and no RoI at all"""
    c = case("edge")
    check_align("edge", 7, ptype, ratio)
    out, _ = run_fwd(c["feats_dev"], c["rois_dev"], 7, ptype, ratio)
    assert float(out[6].abs().max()) == 0.0 and float(out[1].abs().max()) == 0.0          # NaN box, far outside: zeros
    # no RoI at all: every map is written with zeros by the tile-owner kernel, nothing is added by the atomic one
    none = torch.zeros(0, 5, device=DEV)
    z = run_bwd("tiles", c["shapes"], none, torch.zeros(0, 7, 7, c["C"], device=DEV), 7, ptype, ratio)
    assert all(float(m.abs().max()) == 0.0 for m in z)
    z = run_bwd("atomic", c["shapes"], none, torch.zeros(0, 7, 7, c["C"], device=DEV), 7, ptype, ratio)
    assert all(float(m.abs().max()) == 0.0 for m in z)
    assert run_fwd(c["feats_dev"], none, 7, ptype, ratio)[0].shape[0] == 0
    # an image index outside the batch: zeros and no gradient
    bad = c["rois_dev"][:3].clone()
    bad[:, 0] = torch.tensor([2.0, -1.0, 1.0], device=DEV)
    out, _ = run_fwd(c["feats_dev"], bad, 7, ptype, ratio)
    assert float(out[:2].abs().max()) == 0.0 and float(out[2].abs().max()) > 0.0
    d = torch.ones(3, 7, 7, c["C"], device=DEV)
    g_all = run_bwd("atomic", c["shapes"], bad, d, 7, ptype, ratio)
    g_one = run_bwd("atomic", c["shapes"], bad[2:], d[2:], 7, ptype, ratio)
    t_all = run_bwd("tiles", c["shapes"], bad, d, 7, ptype, ratio)
    for x, y, z in zip(g_all, g_one, t_all):
        assert _rel(x, y) < 2e-6 and _rel(z, y) < 2e-6


def test_tile_kernel_with_several_queue_chunks():
    """N = 4, 512^2, C = 256, R = 2048 at ratio 2: the tile-owner kernel's RoI scan runs several 256-RoI chunks per block and
    the separable kernel takes its 8-blocks-per-RoI form"""
    check_align("big", 7, 1, 2, forward=False)


# ------------------------------------------------------------------------------------------------ 2. the default options
@pytest.mark.parametrize("dt", [f32, bf16])
def test_new_entry_points_on_the_default_options_are_the_old_kernels(dt):
    c = case("c128")
    feats = [f.to(dt) for f in c["feats_dev"]]
    rois = c["rois_dev"]
    dout = c["dout"][7].to(DEV).to(dt)
    new, _ = run_fwd(feats, rois, 7, 0, 0)
    old, _ = run_fwd(feats, rois, 7, 0, 0, old=True)
    assert torch.equal(new, old)
    tn = run_bwd("tiles", c["shapes"], rois, dout, 7, 0, 0)
    to = run_bwd("tiles", c["shapes"], rois, dout, 7, 0, 0, old=True)
    an = run_bwd("atomic", c["shapes"], rois, dout, 7, 0, 0)
    ao = run_bwd("atomic", c["shapes"], rois, dout, 7, 0, 0, old=True)
    for a, b, x, y in zip(tn, to, an, ao):
        assert torch.equal(a, b)
        assert _rel(x, y) < 2e-6                                             # the atomics fix no order
    # and the generic instantiation agrees with the default one where both state the same grid (ratio 2 on 2 x 2 grids is
    # covered by test 1 against float64)


# ------------------------------------------------------------------------------------------------ 3. ROIPool
def check_pool(feats_cpu, rois, dout, P):
    """feats_cpu: float32 or bfloat16 CPU maps (the stored values)"""
    dt = feats_cpu[0].dtype
    shapes = [tuple(f.shape) for f in feats_cpu]
    C = shapes[0][3]
    ref_out, ref_arg, lvs, ns = pool_reference([f.float().numpy() for f in feats_cpu], rois, P)
    out, arg = run_fwd([f.to(DEV) for f in feats_cpu], rois.to(DEV), P, 2, 0)
    assert torch.equal(arg.cpu(), torch.from_numpy(ref_arg))
    assert torch.equal(out.float().cpu(), torch.from_numpy(ref_out))
    # backward: float64 scatter of dY to the argmax pixel
    d = dout.to(dt)
    g = run_bwd("atomic", shapes, rois.to(DEV), d.to(DEV), P, 2, 0, argmax=arg)
    ref_g = [torch.zeros(s, dtype=f64) for s in shapes]
    a = torch.from_numpy(ref_arg).long()
    dd = d.double()
    for r in range(rois.shape[0]):
        if ns[r] < 0:
            continue
        m = a[r] >= 0
        cc = torch.arange(C).expand_as(a[r])[m]
        ref_g[lvs[r]][ns[r]].view(-1, C).index_put_((a[r][m], cc), dd[r][m], accumulate=True)
    err = max(_rel(x, y) for x, y in zip(g, ref_g))
    print("roi pool P=%d %s: backward %.3g, %d empty bins" % (P, dt, err, int((ref_arg < 0).sum()) // C))
    assert err < 2e-6, err
    # empty bins: 0 out, and a gradient map that ignores their dY
    empty = torch.from_numpy((ref_arg < 0) & (ref_out == 0))                # (a bin of NaNs only is not empty: it keeps -FLT_MAX)
    if bool(empty.any()):
        assert float(out.cpu().float()[empty].abs().max()) == 0.0
        d2 = d.clone()
        d2[empty] = 1000.0
        g2 = run_bwd("atomic", shapes, rois.to(DEV), d2.to(DEV), P, 2, 0, argmax=arg)
        for x, y in zip(g2, ref_g):
            assert _rel(x, y) < 2e-6
    return ref_arg


@pytest.mark.parametrize("dt", [f32, bf16])
@pytest.mark.parametrize("name", ["c64", "c128"])
def test_roipool_matches_the_restatement_exactly(name, dt):
    c = case(name)
    check_pool([f.to(dt) for f in c["feats"]], c["rois"], c["dout"][7], 7)


def test_roipool_edge_cases_and_p14():
    c = case("edge")
    ref_arg = check_pool(c["feats"], c["rois"], c["dout"][7], 7)
    assert int((ref_arg[1] >= 0).sum()) == 0 and int((ref_arg[6] >= 0).sum()) == 0     # far outside / NaN: every bin empty
    assert int((ref_arg[3] < 0).sum()) > 0 and int((ref_arg[3] >= 0).sum()) > 0         # crossing the border: some bins empty
    check_pool(c["feats"], c["rois"], c["dout"][14], 14)
    # no RoI, and an image index outside the batch
    none = torch.zeros(0, 5, device=DEV)
    assert run_fwd(c["feats_dev"], none, 7, 2, 0)[0].shape[0] == 0
    bad = c["rois"][:3].clone()
    bad[:, 0] = torch.tensor([2.0, -1.0, 1.0])
    check_pool(c["feats"], bad, c["dout"][7][:3], 7)
    out, arg = run_fwd(c["feats_dev"], bad.to(DEV), 7, 2, 0)
    assert float(out[:2].abs().max()) == 0.0 and int((arg[:2] >= 0).sum()) == 0 and int((arg[2] >= 0).sum()) > 0


def test_roipool_first_maximum_wins_and_nan_never_wins():
    """maps of a few repeated values: every bin holds ties, the row-major first one is the argmax; NaN pixels are skipped"""
    g = torch.Generator().manual_seed(11)
    N, size, C = 2, 128, 64
    shapes = [(N, size // s, size // s, C) for s in (4, 8, 16, 32, 64)]
    feats = [torch.randint(0, 3, s, generator=g).float() for s in shapes]
    for f in feats:
        f[torch.rand(f.shape, generator=g) < 0.1] = NAN
    feats[0][0, :8, :8] = NAN                                                # whole bins of NaN: nothing wins, argmax -1
    rois = _rois(N, 120, size, g)
    rois = torch.cat([rois, torch.tensor([[0, 0.0, 0.0, 27.0, 27.0]])])      # level 0, bins of 1 px inside the NaN block
    dout = torch.randn(rois.shape[0], 7, 7, C, generator=g)
    ref_arg = check_pool(feats, rois, dout, 7)
    assert int((ref_arg[-1, :1, :1] >= 0).sum()) == 0


# ------------------------------------------------------------------------------------------------ 4. what is launched
@pytest.fixture()
def calls(monkeypatch):
    seen = []
    real = _lib.call

    def spy(name, *a, **k):
        seen.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(_lib, "call", spy)
    return seen


def _through_ops(c, **kw):
    feats = [f.clone().requires_grad_(True) for f in c["feats_dev"]]
    y = ops.roi_align_pyramid(feats, c["rois_dev"], SCALES, 7, **kw)
    y.backward(c["dout"][7].to(DEV))
    return y.detach(), [f.grad for f in feats]


def test_default_keywords_launch_the_old_entry_points(calls, monkeypatch):
    c = case("c64")
    monkeypatch.setattr(ops, "_ROI_BWD_TILES", [True])
    a = _through_ops(c)
    assert calls == ["cr_roi_align_fwd", "cr_roi_align_bwd_set"]
    del calls[:]
    b = _through_ops(c, pooler_type="ROIAlignV2", sampling_ratio=0)
    assert calls == ["cr_roi_align_fwd", "cr_roi_align_bwd_set"]
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    monkeypatch.setattr(ops, "_ROI_BWD_TILES", [False])
    del calls[:]
    _through_ops(c)
    assert calls == ["cr_roi_align_fwd", "cr_roi_align_bwd"]
    # the new modes: the same tile / atomic choice, ROIPool always atomic with its argmax
    for tiles, kw, want in ((True, dict(sampling_ratio=2), "cr_roi_pool_bwd_set"), (False, dict(sampling_ratio=2), "cr_roi_pool_bwd"),
                            (True, dict(pooler_type="ROIAlign"), "cr_roi_pool_bwd_set"), (True, dict(pooler_type="ROIPool"), "cr_roi_pool_bwd")):
        monkeypatch.setattr(ops, "_ROI_BWD_TILES", [tiles])
        del calls[:]
        y, grads = _through_ops(c, **kw)
        assert calls == ["cr_roi_pool_fwd", want], (kw, calls)
        ptype, ratio = ops.pooler_type_code(kw.get("pooler_type", "ROIAlignV2"), kw.get("sampling_ratio", 0))
        if ptype != 2:
            ref_out, ref_g = align_ref("c64", 7, ptype, ratio)
            assert _rel(y, ref_out) < 1e-5 and max(_rel(x, z) for x, z in zip(grads, ref_g)) < 1e-5
        else:
            assert all(bool(torch.isfinite(x).all()) for x in grads) and float(grads[0].abs().max()) > 0
    with pytest.raises(ValueError, match="ROIAlignV2.*ROIAlign.*ROIPool"):
        ops.roi_align_pyramid(c["feats_dev"], c["rois_dev"], SCALES, 7, pooler_type="ROIAlignRotated")
    with pytest.raises(ValueError, match="ROIAlignV2.*ROIAlign.*ROIPool"):
        ops.roi_align_pyramid(c["feats_dev"], c["rois_dev"], SCALES, 7, sampling_ratio=-1)


def test_equal_poolers_pool_once_and_different_ones_twice(calls):
    rhm = importlib.import_module("3dod_amd.cubercnn.modeling.roi_heads.roi_heads")
    dt = importlib.import_module("3dod_amd.cubercnn.modeling.dense_train")
    c = case("c64")
    names = ["p2", "p3", "p4", "p5", "p6"]
    features = dict(zip(names, c["feats_dev"]))
    g = torch.Generator().manual_seed(4)
    B, S, kf = c["N"], 24, 6
    boxes = _rois(1, B * S, 256, g)[:, 1:].reshape(B, S, 4).to(DEV)
    samp = {"valid": torch.ones(B, S, dtype=torch.bool, device=DEV), "k_fg": kf, "boxes": boxes}

    def heads(box, cube, scale_roi_boxes=0.0):
        mk = lambda t: rhm.ROIPooler(7, SCALES, t[1], t[0])
        return types.SimpleNamespace(box_pooler=mk(box), cube_pooler=mk(cube), loss_w_3d=1.0, box_in_features=names, in_features=names,
                                     scale_roi_boxes=scale_roi_boxes)
    for box, cube, scale, want in ((("ROIAlignV2", 0), ("ROIAlignV2", 0), 0.0, ["cr_roi_align_fwd"]),
                                   (("ROIAlignV2", 2), ("ROIAlignV2", 2), 0.0, ["cr_roi_pool_fwd"]),
                                   (("ROIPool", 0), ("ROIPool", 2), 0.0, ["cr_roi_pool_fwd"]),       # ROIPool ignores the ratio
                                   (("ROIAlign", 0), ("ROIAlign", 0), 1.2, ["cr_roi_pool_fwd"]),      # rescaled 3D boxes: one launch
                                   (("ROIAlignV2", 0), ("ROIAlignV2", 2), 0.0, ["cr_roi_align_fwd", "cr_roi_pool_fwd"]),
                                   (("ROIAlign", 0), ("ROIPool", 0), 0.0, ["cr_roi_pool_fwd", "cr_roi_pool_fwd"])):
        del calls[:]
        b, cu = dt.pool_roi_features(heads(box, cube, scale), features, samp)
        assert [n for n in calls if "roi" in n] == want, (box, cube, calls)
        assert tuple(b.shape) == (B * S, 7, 7, c["C"]) and tuple(cu.shape) == (B * kf, 7, 7, c["C"])
        # the 3D head's features are those of its own pooler on the foreground slots
        rois = torch.cat([torch.arange(B, device=DEV).repeat_interleave(kf)[:, None].float(), boxes[:, :kf].reshape(-1, 4)], 1)
        if not scale > 0:
            pt, ra = ops.pooler_type_code(*cube)
            want_cu = ops.roi_align_pyramid(c["feats_dev"], rois, SCALES, 7, pooler_type=cube[0], sampling_ratio=ra)
            assert torch.equal(cu, want_cu)


# ------------------------------------------------------------------------------------------------ 5. end to end
B_, C_ = "MODEL.ROI_BOX_HEAD.", "MODEL.ROI_CUBE_HEAD."
E2E = {
    "ratio2": [B_ + "POOLER_SAMPLING_RATIO", 2, C_ + "POOLER_SAMPLING_RATIO", 2],
    "roialign": [B_ + "POOLER_TYPE", "ROIAlign", C_ + "POOLER_TYPE", "ROIAlign"],
    "roipool": [B_ + "POOLER_TYPE", "ROIPool", C_ + "POOLER_TYPE", "ROIPool"],
    "cube_ratio2": [C_ + "POOLER_SAMPLING_RATIO", 2],
}


@pytest.mark.parametrize("name", list(E2E))
def test_model_trains_and_infers_with_the_pooler(monkeypatch, calls, name):
    """2 x 128^2 images, two steps of solver.make_train_step with the per-shape graph cache on, then inference on the same model"""
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    monkeypatch.setenv("CR_GRAPHS", "dense")
    cfg, model, opt, syn, solver = bt.build(DEV, seed=0, lr=0.0025, extra=E2E[name])
    rh = model.roi_heads
    step = solver.make_train_step(cfg, model, opt, world_size=1)
    torch.manual_seed(5)
    with d2.EventStorage(0):
        for i in range(2):
            b = syn.make_batch(2, 900 + i, size=128)
            for d in b:
                d["image"], d["instances"] = d["image"].to(DEV), d["instances"].to(DEV)
            step(b)
        rep = step.report()
    assert model._graphed is not None
    assert rep["iterations_explode"] == 0 and math.isfinite(rep["total_loss"]), rep
    assert all(math.isfinite(v) for k, v in rep.items() if k.startswith("Cube/") or k.startswith("BoxHead/")), rep
    assert "cr_roi_pool_fwd" in calls and ("cr_roi_pool_bwd" in calls or "cr_roi_pool_bwd_set" in calls)
    assert ("cr_roi_align_fwd" in calls) == (name == "cube_ratio2")
    first = [rh.box_head.fc1, rh.cube_head.feature_generator.fc1 if hasattr(rh.cube_head, "feature_generator")
             else rh.cube_head.feature_generator_XY.fc1]
    for fc in first:
        gw = fc.weight._cr_grad                              # the parameter's view of the optimizer's flat gradient (last step)
        assert gw.numel() == fc.weight.numel()
        assert bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0.0
    model.eval()
    rh.box_predictor.test_score_thresh = 0.0
    with torch.no_grad():
        out = model(syn.make_batch(2, 5, size=128, with_gt=False))
    total = 0
    for o in out:
        inst = o["instances"]
        m = len(inst)
        total += m
        assert tuple(inst.pred_bbox3D.shape) == (m, 8, 3) and tuple(inst.pred_pose.shape) == (m, 3, 3)
        assert tuple(inst.pred_center_cam.shape) == (m, 3) and tuple(inst.pred_center_2D.shape) == (m, 2)
        assert tuple(inst.pred_dimensions.shape) == (m, 3) and tuple(inst.scores.shape) == (m,)
        assert tuple(inst.pred_boxes.tensor.shape) == (m, 4)
        for f in ("pred_bbox3D", "pred_pose", "pred_center_cam", "pred_center_2D", "pred_dimensions", "scores"):
            assert bool(torch.isfinite(inst.get(f)).all()), f
    assert total > 0
