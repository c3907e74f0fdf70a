"""GPU: cr_box3d_overlap (float32, one thread per pair) against the float64 oracle (oracle/iou3d.py), the reference's
known-answer fixture (0.9944) and the corners produced by the product's own get_cuboid_verts_faces kernel; and, with the
grouped evaluation kernel (cr_eval_iou_groups, the second copy of the pair body), against the independent tolerance-free
reference tests/iou3d_ref.py on the families of tests/iou3d_families.py: nearly coinciding, nearly parallel and touching
faces, thin, tiny and very unequal boxes, at depths where a float32 ulp of a coordinate is as large as the clipper's tolerance.

Worst error / bound per family on the MI355X (both kernels, both argument orders, before and after the rigid motion):
two_routes 0.037, shifted 0.058, concentric 0.107, yaw_only 0.036, grown 0.011, contained 0.000, touching 0.006, thin 0.244,
tiny 0.030, large_small 0.000, general 0.060.  With the clips of the previous kernels (no split by one function; the same
tests, the same GPU): two_routes 1085, shifted 1354, concentric 320 (0.0003 degree) and 1.10 (5 degrees), yaw_only 103 (80 m,
after the motion); DESIGN.md, "IoU3D on crossing and nearly coinciding faces"."""
import importlib

import numpy as np
import pytest
import torch

from oracle import iou3d as O
from tests import iou3d_families as F
from tests import iou3d_ref as REF
from tests.eval_device_helpers import grouped_iou3d
from tests.test_iou3d import REF_C1, REF_C2, REF_IOU, box, rot

pytestmark = pytest.mark.gpu
geo = importlib.import_module("3dod_amd.geometry")
DEV = torch.device("cuda:0")


def test_known_answer_and_analytic():
    vol, iou = geo.box3d_overlap(torch.tensor([REF_C1], device=DEV), torch.tensor([REF_C2], device=DEV))
    assert abs(float(iou[0, 0]) - REF_IOU) < 1e-3
    a = box([10, -3, 20], [2, 2, 2])
    bs = [box([11, -3, 20], [2, 2, 2]), box([11, -2, 21], [2, 2, 2]), box([10, -3, 20], [1, 1, 1]), box([13, -3, 20], [2, 2, 2]),
          box([12, -3, 20], [2, 2, 2]), a, box([10, -3, 20], [2, 2, 2], rot([0, 0, 1], np.pi / 4))]
    want = [4.0, 1.0, 1.0, 0.0, 0.0, 8.0, 16 * (np.sqrt(2) - 1)]
    vol, iou = geo.box3d_overlap(torch.tensor(a[None], dtype=torch.float32, device=DEV),
                                 torch.tensor(np.stack(bs), dtype=torch.float32, device=DEV))
    assert np.allclose(vol.cpu().numpy()[0], want, rtol=2e-5, atol=2e-4), vol
    assert abs(float(iou[0, 5]) - 1.0) < 1e-5


def test_random_pairs_vs_oracle():
    rng = np.random.default_rng(5)
    A = np.stack([box(rng.normal(size=3) + [0, 0, 8], rng.uniform(0.4, 3, 3), rot(rng.normal(size=3), rng.uniform(0, 3))) for _ in range(24)])
    B = np.stack([box(A[i % 24].mean(0) + rng.normal(size=3) * 0.6, rng.uniform(0.4, 3, 3), rot(rng.normal(size=3), rng.uniform(0, 3)))
                  for i in range(40)])
    vol, iou = geo.box3d_overlap(torch.tensor(A, dtype=torch.float32, device=DEV), torch.tensor(B, dtype=torch.float32, device=DEV))
    rvol, riou = O.box3d_overlap(A, B)
    assert np.abs(iou.cpu().numpy() - riou).max() < 2e-4, np.abs(iou.cpu().numpy() - riou).max()
    P = F.family("general")[0][1]                                        # the same boxes, from their parameters
    assert np.array_equal(P.c1, A.astype(np.float32)) and np.array_equal(P.c2, B.astype(np.float32))
    assert np.abs(iou.cpu().numpy() - P.iou.reshape(24, 40)).max() < 2e-4 and np.abs(riou - P.iou.reshape(24, 40)).max() < 2e-4
    assert (riou > 0.05).sum() > 20 and (riou == 0).sum() > 20           # both regimes covered


def test_on_cuboid_corners_kernel():
    """corners from cr_cuboid_corners (math_util.get_cuboid_verts_faces order) feed box3d_overlap like iou_3d does."""
    g = torch.Generator().manual_seed(3)
    n = 16
    box6 = torch.cat([torch.randn(n, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 6.0]), torch.rand(n, 3, generator=g) + 0.5], 1)
    util = importlib.import_module("3dod_amd.cubercnn.util.math_util")
    R = util.rotation_6d_to_matrix(torch.randn(n, 6, generator=g))
    verts = geo.cuboid_corners(box6.to(DEV), R.to(DEV))
    vol, iou = geo.box3d_overlap(verts, verts)
    assert torch.allclose(torch.diagonal(iou).cpu(), torch.ones(n), atol=1e-4)
    assert torch.allclose(torch.diagonal(vol).cpu(), box6[:, 3:].prod(1), rtol=1e-4)
    rvol, riou = O.box3d_overlap(verts.cpu().numpy(), verts.cpu().numpy())
    assert np.abs(iou.cpu().numpy() - riou).max() < 2e-4
    params = [(box6[i, :3].double().numpy(), box6[i, [5, 4, 3]].double().numpy(), R[i].double().numpy()) for i in range(n)]
    want = np.array([[REF.iou3d(a, b)[1] for b in params] for a in params])    # local axes carry (l, h, w)
    assert np.abs(iou.cpu().numpy() - want).max() < 2e-4 and np.abs(riou - want).max() < 2e-4


def test_ap3d_same_through_kernel_and_oracle():
    """SURVEY 8(d) "AP3D parity": the same detections scored with the HIP IoU3D kernel and with the float64 oracle give
    the same AP3D (1e-3)."""
    ev = importlib.import_module("3dod_amd.cubercnn.evaluation")
    rng = np.random.default_rng(11)
    gts, dts = [], []
    for img in range(6):
        for k in range(5):
            ctr = rng.normal(size=3) * [3, 1, 4] + [0, 0, 18]
            dims = rng.uniform(0.5, 3, 3)
            R = rot([0, 1, 0], rng.uniform(0, 3))
            cat = int(rng.integers(0, 3))
            c = box(ctr, dims, R)
            gts.append({"image_id": img, "category_id": cat, "id": len(gts) + 1, "bbox": [0, 0, 10, 10], "area": 100.0,
                        "bbox3D": c.tolist(), "depth": float(ctr[2]), "ignore2D": 0, "ignore3D": int(rng.random() < 0.1)})
            for j in range(2):                       # a good and a sloppy detection per object
                c2 = box(ctr + rng.normal(size=3) * (0.1 + 0.5 * j), dims * rng.uniform(0.8, 1.2, 3), R @ rot([0, 1, 0], rng.normal() * 0.2))
                dts.append({"image_id": img, "category_id": cat, "bbox": [0, 0, 10, 10], "area": 100.0, "bbox3D": c2.tolist(),
                            "depth": float(ctr[2]), "score": float(rng.random())})
    a = ev.Omni3Deval(gts, dts, "3D").evaluate().accumulate().summarize()              # cr_box3d_overlap
    b = ev.Omni3Deval(gts, dts, "3D", iou3d_fn=lambda d, g: O.box3d_overlap(np.asarray(d), np.asarray(g))[1]).evaluate().accumulate().summarize()
    assert 0.05 < b[0] < 0.95
    assert np.abs(a - b).max() < 1e-3, (a, b)


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).reshape(-1, 8, 3)


def _both_kernels(S, swap):
    """the pairs of S through cr_box3d_overlap and the grouped kernel (boxes2 against boxes1 when swap): per pair
    (vol, iou) and iou"""
    a, b, i, j = (S.c2, S.c1, S.j, S.i) if swap else (S.c1, S.c2, S.i, S.j)
    assert len(a) <= 64 and len(b) <= 64
    vol, iou = geo.box3d_overlap(_t(a), _t(b))
    grp = grouped_iou3d(a, b)
    return vol.cpu().numpy().astype(np.float64)[i, j], iou.cpu().numpy().astype(np.float64)[i, j], grp[i, j]


@pytest.mark.parametrize("name,variant", [(n, v) for n in F.NAMES for v in F.variants(n)])
def test_family_against_the_independent_reference(name, variant):
    """every pair, both kernels, both argument orders, before and after a common rigid motion:
    |IoU - IoU_ref| <= 2e-4 + 4 eps (S1 + S2) / (V1 + V2 - V), eps = the largest error of a given corner (Pairs.bound)"""
    P = dict(F.family(name))[variant]
    Q = P.moved(*F.motion(name))
    worst, got = {}, {}
    for tag, S in (("", P), ("moved ", Q)):
        bound = S.bound()
        # the volume of the boxes the kernel is given (float64 from the float32 corners) bounds the intersection
        vmin = np.minimum([O.box_volume(c.astype(np.float64)) for c in S.c1[S.i]], [O.box_volume(c.astype(np.float64)) for c in S.c2[S.j]])
        for swap in (False, True):
            vol, iou, grp = _both_kernels(S, swap)
            got[tag, swap] = (iou, grp)
            for kern, val in (("box3d_overlap", iou), ("grouped", grp)):
                assert np.isfinite(val).all() and (val >= 0).all() and (val <= 1).all(), (name, variant, tag, kern, swap)
                worst[tag + kern] = max(worst.get(tag + kern, 0.0), float((np.abs(val - S.iou) / bound).max()))
            assert (vol >= 0).all() and (vol <= vmin * (1 + 1e-6)).all(), (name, variant, tag, swap, (vol / vmin).max())
            worst[tag + "kernels"] = max(worst.get(tag + "kernels", 0.0), float((np.abs(iou - grp) / bound).max()))
        for k in (0, 1):
            worst[tag + "orders"] = max(worst.get(tag + "orders", 0.0), float((np.abs(got[tag, False][k] - got[tag, True][k]) / (2 * bound)).max()))
    both = P.bound(np.maximum(P.eps, Q.eps))
    for swap in (False, True):
        for k in (0, 1):
            worst["motion"] = max(worst.get("motion", 0.0), float((np.abs(got["", swap][k] - got["moved ", swap][k]) / both).max()))
    print("%s %s: worst error / bound %s (eps %.1e, moved %.1e)" % (name, variant, " ".join("%s %.3f" % kv for kv in sorted(worst.items())),
                                                                     P.eps.max(), Q.eps.max()))
    assert max(worst.values()) <= 1.0, (name, variant, worst)


def test_launch_edges():
    """N * M = 65 (a partly filled second block of cr_box3d_overlap), N = 0, M = 0"""
    P = F.family("general")[0][1]
    a, b = P.c1[:5], P.c2[:13]
    vol, iou = geo.box3d_overlap(_t(a), _t(b))
    want = P.iou.reshape(24, 40)[:5, :13]
    assert vol.shape == iou.shape == (5, 13) and np.abs(iou.cpu().numpy() - want).max() < 2e-4
    assert np.abs(grouped_iou3d(a, b) - want).max() < 2e-4
    for n, m in ((0, 13), (5, 0), (0, 0)):
        vol, iou = geo.box3d_overlap(_t(a[:n]), _t(b[:m]))
        torch.cuda.synchronize()
        assert vol.shape == iou.shape == (n, m)
        assert grouped_iou3d(a[:n], b[:m]).shape == (n, m)


def test_zero_volume_boxes():
    """two boxes of zero volume give NaN (0 / 0) and nothing else does; a zero-volume box against a solid one gives IoU 0"""
    solid = [box([0, 0, 8], [2, 1, 3], rot([1, 2, 3], 0.4)), box([0.3, 0, 8], [1, 1, 1])]
    flat = [box([0, 0, 8], [2, 0, 3], rot([1, 2, 3], 0.4)), box([0, 0, 8], [0, 0, 0]), box([0.2, 0.1, 8], [2, 1, 0])]   # a plate, a point, a plate
    allb = np.stack(solid + flat).astype(np.float32)
    zero = np.array([False, False, True, True, True])
    vol, iou = geo.box3d_overlap(_t(allb), _t(allb))
    for val in (iou.cpu().numpy(), grouped_iou3d(allb, allb)):
        both = zero[:, None] & zero[None, :]
        assert np.isnan(val[both]).all() and np.isfinite(val[~both]).all()
        assert (val[zero[:, None] ^ zero[None, :]] == 0).all()
        assert abs(val[0, 0] - 1) < 1e-5 and abs(val[1, 1] - 1) < 1e-5 and 0 < val[0, 1] < 1
    assert (vol.cpu().numpy()[zero[:, None] | zero[None, :]] == 0).all()
