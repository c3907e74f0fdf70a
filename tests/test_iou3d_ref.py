"""CPU: the independent float64 IoU3D reference (tests/iou3d_ref.py) against qhull's half-space intersection on every family
of tests/iou3d_families.py (1e-9 of the smaller box volume) and against the analytic cases of tests/test_iou3d.py."""
import numpy as np
import pytest

from tests import iou3d_families as F
from tests import iou3d_ref as REF
from tests.iou3d_families import rot


def qhull_volume(b1, b2):
    """volume of the intersection by scipy (Chebyshev centre by a linear program, qhull's HalfspaceIntersection, ConvexHull);
    None where the Chebyshev radius is below 1e-9 (the expected volume is 0)"""
    from scipy.optimize import linprog
    from scipy.spatial import ConvexHull, HalfspaceIntersection
    origin = np.asarray(b1[0], REF.LD)
    n1, o1 = REF.half_spaces(*b1, origin)
    n2, o2 = REF.half_spaces(*b2, origin)
    n, off = np.concatenate([n1, n2]).astype(np.float64), np.concatenate([o1, o2]).astype(np.float64)
    res = linprog([0, 0, 0, -1], A_ub=np.hstack([n, np.ones((12, 1))]), b_ub=off, bounds=[(None, None)] * 3 + [(0, None)])
    if res.status != 0 or res.x[3] < 1e-9:
        return None
    hs = HalfspaceIntersection(np.hstack([n, -off[:, None]]), res.x[:3])
    return ConvexHull(hs.intersections).volume


@pytest.mark.parametrize("name,variant", [(n, v) for n in F.NAMES for v in F.variants(n)])
def test_reference_against_qhull(name, variant):
    pytest.importorskip("scipy")
    worst, checked, empty = 0.0, 0, 0
    for label, P in F.family(name):
        if label != variant:
            continue
        for k, (i, j) in enumerate(P.index):
            want = qhull_volume(P.boxes1[i], P.boxes2[j])
            if want is None:
                empty += 1
                assert P.vol[k] <= 1e-6 * min(P.v1[k], P.v2[k]), (name, label, k, P.vol[k])
                continue
            checked += 1
            err = abs(P.vol[k] - want) / min(P.v1[k], P.v2[k])
            worst = max(worst, err)
            assert err <= 1e-9, (name, label, k, P.vol[k], want)
    print("%s %s: %d pairs against qhull, %d empty, worst error %.2e of the smaller box" % (name, variant, checked, empty, worst))
    assert checked > 0 or name == "touching"


@pytest.mark.parametrize("degrees", [1e-5, 1e-4, 3e-4])
def test_reference_small_rotation_first_order(degrees):
    """equal concentric boxes, one turned by the vector w (|w| <= 5e-6 rad): every face loses the half on which the other
    box's face lies inside it, V - sum over faces of 1/2 * integral |(w x x) . n| dA, up to O(|w|^2) V < 3e-11 V: a
    check that needs no other program, where the split of two nearly parallel faces is most delicate."""
    P = dict(F.family("concentric"))[str(degrees)]
    m = 1000
    g = (np.arange(m) + 0.5) / m * 2 - 1                                  # midpoints of [-1, 1]
    for k in range(F.PAIRS):
        (c, e, R1), (_, _, R2) = P.boxes1[k], P.boxes2[k]
        T = R2 @ R1.T                                                     # the relative rotation; its vector, in box 1's frame
        w = R1.T @ (np.array([T[2, 1] - T[1, 2], T[0, 2] - T[2, 0], T[1, 0] - T[0, 1]]) / 2)
        h, loss = e / 2, 0.0
        for a in range(3):
            b, c_ = (a + 1) % 3, (a + 2) % 3                              # face +-e_a: (w x x) . e_a = w_b x_c - w_c x_b
            val = np.abs(w[b] * h[c_] * g[None, :] - w[c_] * h[b] * g[:, None]).mean() * (4 * h[b] * h[c_])
            loss += 2 * 0.5 * val
        assert abs(P.vol[k] - (P.v1[k] - loss)) <= 1e-10 * P.v1[k], (degrees, k, P.vol[k], P.v1[k] - loss)


def test_reference_analytic_cases():
    a = (np.zeros(3), np.full(3, 2.0), np.eye(3))
    cases = [(([1, 0, 0], [2, 2, 2]), 4.0), (([1, 1, 1], [2, 2, 2]), 1.0), (([0, 0, 0], [1, 1, 1]), 1.0), (([3, 0, 0], [2, 2, 2]), 0.0),
             (([2, 0, 0], [2, 2, 2]), 0.0), (([0, 0, 0], [2, 2, 2]), 8.0), (([0, 0, 0], [4, 0.5, 0.5]), 0.5),
             (([0.5, 0.25, -0.5], [1, 3, 2]), 3.0)]
    for (c, e), v in cases:
        b = (np.array(c, float), np.array(e, float), np.eye(3))
        assert abs(REF.intersection_volume(a, b) - v) < 1e-12, v
        assert abs(REF.intersection_volume(b, a) - v) < 1e-12, v
    b = (np.zeros(3), np.full(3, 2.0), rot([0, 0, 1], np.pi / 4))
    assert abs(REF.intersection_volume(a, b) - 16 * (np.sqrt(2) - 1)) < 1e-12
    v, iou, s1, s2 = REF.iou3d(a, (np.array([1.0, 0, 0]), np.array([2.0, 2, 2]), np.eye(3)))
    assert abs(iou - 4 / 12) < 1e-14 and s1 == 24.0 and s2 == 24.0
    T, t = rot([1, 2, 3], 0.7), np.array([3.0, -40.0, 20.0])          # rigid motion
    m = F.moved(b, T, t)
    assert abs(REF.intersection_volume(F.moved(a, T, t), m) - 16 * (np.sqrt(2) - 1)) < 1e-12
