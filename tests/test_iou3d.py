"""CPU: the exact IoU3D oracle (oracle/iou3d.py) against the reference's own known-answer test
(ProposalNetwork/utils/tests/test_iou.py:4-27: IoU = 0.9944, 4 digits), analytic cases, and the independent tolerance-free
reference (tests/iou3d_ref.py) on the float32 corners of every family of tests/iou3d_families.py."""
import numpy as np
import pytest

from oracle import iou3d as O
from tests import iou3d_families as F
from tests.iou3d_families import box, rot          # noqa: F401  (other tests import them from here)

# fixture data of the reference's test (corner coordinates and the expected value printed there)
REF_C1 = [[0.2411, -0.1752, 1.2247], [0.1951, -0.4194, 1.7741], [0.2036, 0.4826, 2.1757], [0.2495, 0.7267, 1.6263],
          [-0.2920, -0.1549, 1.1903], [-0.3380, -0.3991, 1.7396], [-0.3295, 0.5029, 2.1412], [-0.2835, 0.7471, 1.5919]]
REF_C2 = [[0.2390, -0.1764, 1.2246], [0.1930, -0.4205, 1.7740], [0.2055, 0.4813, 2.1759], [0.2515, 0.7254, 1.6265],
          [-0.2940, -0.1536, 1.1901], [-0.3400, -0.3978, 1.7395], [-0.3274, 0.5040, 2.1414], [-0.2815, 0.7482, 1.5920]]
REF_IOU = 0.9944


def test_reference_known_answer():
    vol, iou = O.box3d_overlap([REF_C1], [REF_C2])
    # the fixture's corners are rounded to 1e-4 on ~0.5 m edges (the quads are not exactly planar), which moves the IoU
    # by up to ~6e-4 depending on how an algorithm reads planes off the corners: 3 digits are pinned
    assert abs(iou[0, 0] - REF_IOU) < 1e-3, iou


def test_analytic_cases():
    a = box([0, 0, 0], [2, 2, 2])
    assert abs(O.box_volume(a) - 8) < 1e-12
    cases = [(box([1, 0, 0], [2, 2, 2]), 4.0), (box([1, 1, 1], [2, 2, 2]), 1.0), (box([0, 0, 0], [1, 1, 1]), 1.0),
             (box([3, 0, 0], [2, 2, 2]), 0.0), (box([2, 0, 0], [2, 2, 2]), 0.0), (a, 8.0),
             (box([0, 0, 0], [4, 0.5, 0.5]), 0.5), (box([0.5, 0.25, -0.5], [1, 3, 2]), 1 * 2 * 1.5)]
    for b, v in cases:
        assert abs(O.intersection_volume(a, b) - v) < 1e-4, v        # the coplanarity tolerance is 2e-6 * scale
        assert abs(O.intersection_volume(b, a) - v) < 1e-4, v        # symmetric
    # rotation by 45 deg about z: octagonal prism, area = 8 (sqrt(2) - 1) * (s/2)^2 * ... for s = 2 -> 8(sqrt2-1)
    b = box([0, 0, 0], [2, 2, 2], rot([0, 0, 1], np.pi / 4))
    assert abs(O.intersection_volume(a, b) - 2 * 8 * (np.sqrt(2) - 1)) < 1e-4


def test_invariances_and_bounds():
    rng = np.random.default_rng(0)
    for _ in range(30):
        R1, R2 = rot(rng.normal(size=3), rng.uniform(0, 3)), rot(rng.normal(size=3), rng.uniform(0, 3))
        a = box(rng.normal(size=3), rng.uniform(0.5, 2, 3), R1)
        b = box(rng.normal(size=3) * 0.7, rng.uniform(0.5, 2, 3), R2)
        v = O.intersection_volume(a, b)
        assert -1e-12 <= v <= min(O.box_volume(a), O.box_volume(b)) + 1e-9
        assert abs(v - O.intersection_volume(b, a)) < 1e-4
        T, t = rot(rng.normal(size=3), rng.uniform(0, 3)), rng.normal(size=3) * 5      # rigid motion invariance
        assert abs(v - O.intersection_volume(a @ T.T + t, b @ T.T + t)) < 1e-4
        perm = rng.permutation(8)                         # a relabelled but consistent corner order is NOT supported:
        # the face table assumes the pytorch3d order -> only check that the documented order works
    vol, iou = O.box3d_overlap([box([0, 0, 0], [2, 2, 2])], [box([1, 0, 0], [2, 2, 2]), box([0, 0, 0], [2, 2, 2])])
    assert np.allclose(iou, [[4 / 12, 1.0]])


@pytest.mark.parametrize("name,variant", [(n, v) for n in F.NAMES for v in F.variants(n)])
def test_family_against_the_independent_reference(name, variant):
    """the CPU counterpart of tests/test_gpu_iou3d.py: the oracle on the float32 corners a kernel is given, both argument
    orders, |IoU - IoU_ref| <= 2e-4 + 4 eps (S1 + S2) / (V1 + V2 - V) (Pairs.bound).  Before faces of equal orientation that
    cross or nearly coincide were split by one function the worst error / bound was 778 (two_routes 90 m), 706 (shifted 3e-6),
    116 (concentric 0.0003 degree) and 1.11 (concentric 5 degrees)."""
    P = dict(F.family(name))[variant]
    bound, worst = P.bound(), 0.0
    for k, (i, j) in enumerate(P.index):
        a, b = P.c1[i].astype(np.float64), P.c2[j].astype(np.float64)
        va, vb = O.box_volume(a), O.box_volume(b)
        v12, v21 = O.intersection_volume(a, b), O.intersection_volume(b, a)
        i12, i21 = v12 / (va + vb - v12), v21 / (va + vb - v21)
        worst = max(worst, abs(i12 - P.iou[k]) / bound[k], abs(i21 - P.iou[k]) / bound[k], abs(i12 - i21) / (2 * bound[k]))
        assert i12 >= 0 and i21 >= 0, (name, variant, k, i12, i21)     # (the oracle does not clamp to the smaller box)
    print("%s %s: worst error / bound %.3f" % (name, variant, worst))
    assert worst <= 1.0, (name, variant, worst)
