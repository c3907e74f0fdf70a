"""Shared by tests/test_iou3d_ref.py, tests/test_iou3d.py (CPU) and tests/test_gpu_iou3d.py (GPU): seeded families of box
pairs around the places where a clipper with a coplanarity tolerance goes wrong (nearly coincident, nearly parallel and
touching faces, at depths where one float32 ulp of a coordinate is as large as the tolerance), and the error bound they
are held to.

A box is its generating parameters (centre (3,), extents (3,), rotation (3,3)) in float64; the float32 corners a kernel is
given are made from them by one of two routes: "f64" (float64 corners rounded to float32) or "f32" (the float32 product
`corners @ R.T + c`, what a float32 producer computes).  The reference value (tests/iou3d_ref.py) comes from the parameters."""
import functools

import numpy as np

from tests import iou3d_ref as REF

SIGNS = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], float)
PAIRS = 20                      # pairs per variant of a family


def box(center, dims, R=np.eye(3)):
    """corners in the pytorch3d order from centre, (dx,dy,dz) extents and a rotation."""
    return (SIGNS * (np.asarray(dims, float) / 2)) @ np.asarray(R, float).T + np.asarray(center, float)


def rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def corners32(b, route="f64"):
    """the float32 corners (8,3) of box b by `route`"""
    c, e, R = b
    if route == "f64":
        return box(c, e, R).astype(np.float32)
    assert route == "f32"
    return (SIGNS.astype(np.float32) * (np.asarray(e, np.float32) / np.float32(2))) @ np.asarray(R, np.float32).T + np.asarray(c, np.float32)


def corner_error(b, c32):
    """largest distance between a given corner and its exact position"""
    return float(np.linalg.norm(c32.astype(np.float64) - box(*b), axis=1).max())


def moved(b, T, t):
    """box b after the rigid motion x -> T x + t"""
    return T @ b[0] + t, b[1], T @ b[2]


def _rand_rot(rng):
    return rot(rng.normal(size=3), rng.uniform(0, 3))


def _rand_box(rng, depth, lo=0.5, hi=3.0):
    return np.array([rng.normal() * 2, rng.normal(), depth]), rng.uniform(lo, hi, 3), _rand_rot(rng)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _two_routes(rng, depth):
    b = _rand_box(rng, depth)
    return b, b, "f64", "f32"


def _shifted(rng, length):
    b = _rand_box(rng, 10.0)
    return b, (b[0] + _unit(rng) * length, b[1], b[2]), "f64", "f64"


def _concentric(rng, degrees):
    b = _rand_box(rng, 10.0)
    return b, (b[0], b[1], rot(rng.normal(size=3), np.deg2rad(degrees)) @ b[2]), "f64", "f64"


def _yaw_only(rng, depth):
    y, h = rng.normal() * 0.3, rng.uniform(1.0, 2.0)               # common floor and ceiling
    mk = lambda ctr: (np.array([ctr[0], y, ctr[1]]), np.array([rng.uniform(0.5, 3), h, rng.uniform(0.5, 3)]),
                      rot([0, 1, 0], rng.uniform(0, np.pi)))
    ctr = np.array([rng.normal() * 2, depth])
    return mk(ctr), mk(ctr + rng.normal(size=2) * 0.5), "f64", "f64"


def _grown(rng, _):
    c, e, R = _rand_box(rng, 10.0)
    a, g = int(rng.integers(0, 3)), rng.uniform(0.1, 1.0)
    e2 = e.copy()
    e2[a] += g
    return (c, e, R), (c + R[:, a] * g / 2, e2, R), "f64", "f64"     # five face planes shared


def _contained(rng, _):
    c, e, R = _rand_box(rng, 10.0, 2.0, 3.0)
    return (c, e, R), (c + rng.uniform(-0.2, 0.2, 3), rng.uniform(0.3, 0.8, 3), _rand_rot(rng)), "f64", "f64"


def _touching(rng, _):
    c, e, R = _rand_box(rng, 10.0)
    e2 = rng.uniform(0.5, 3, 3)
    a, s = int(rng.integers(0, 3)), rng.choice([-1.0, 1.0])
    lateral = rng.uniform(-0.4, 0.4, 3)
    lateral[a] = s * (e[a] + e2[a]) / 2                             # opposite faces in contact
    return (c, e, R), (c + R @ lateral, e2, R), "f64", "f64"


def _thin(rng, _):
    c, e, R = _rand_box(rng, 10.0)
    e[int(rng.integers(0, 3))] = 0.01
    return (c, e, R), (c + rng.normal(size=3) * 0.002, e * rng.uniform(0.9, 1.1, 3), rot(rng.normal(size=3), rng.uniform(0, 0.2)) @ R), "f64", "f64"


def _tiny(rng, _):
    c = np.array([rng.normal(), rng.normal() * 0.5, 3.0])
    return (c, np.full(3, 0.02), _rand_rot(rng)), (c + rng.uniform(-0.008, 0.008, 3), np.full(3, 0.02), _rand_rot(rng)), "f64", "f64"


def _large_small(rng, k):
    c, R = np.array([rng.normal() * 2, rng.normal(), 15.0]), _rand_rot(rng)
    a, s = int(rng.integers(0, 3)), rng.choice([-1.0, 1.0])
    at = rng.uniform(-4, 4, 3)
    at[a] = s * 5.0 + rng.uniform(-0.05, 0.05)                      # the small box straddles a face of the large one
    return (c, np.full(3, 10.0), R), (c + R @ at, np.full(3, 0.2), R if k % 2 else _rand_rot(rng)), "f64", "f64"


# family -> (pair builder, its variants, seed)
FAMILIES = {
    "two_routes": (_two_routes, [6.0, 30.0, 60.0, 90.0], 101),
    "shifted": (_shifted, [1e-7, 1e-6, 3e-6, 1e-5, 1e-4], 102),
    "concentric": (_concentric, [1e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 1.0, 2.5, 2.6, 5.0, 12.0, 25.0, 27.0], 103),
    # 2.5 / 2.6 straddle dot = 0.999 and 25 / 27 dot = 0.9, the two orientation tests of the clipper
    "yaw_only": (_yaw_only, [5.0, 40.0, 80.0], 104),
    "grown": (_grown, [None], 105),
    "contained": (_contained, [None], 106),
    "touching": (_touching, [None], 107),
    "thin": (_thin, [None], 108),
    "tiny": (_tiny, [None], 109),
    "large_small": (_large_small, [None], 110),
}
NAMES = list(FAMILIES) + ["general"]


class Pairs:
    """boxes1[i] against boxes2[j] for (i, j) in `index`: the parameters, the float32 corners and, per pair, eps (the largest
    corner error of the two boxes), the reference volume and IoU, and S1 + S2, V1, V2 of the exact boxes"""

    def __init__(self, boxes1, boxes2, routes1, routes2, index, ref=None):
        self.boxes1, self.boxes2, self.routes1, self.routes2, self.index = boxes1, boxes2, routes1, routes2, index
        self.c1 = np.stack([corners32(b, r) for b, r in zip(boxes1, routes1)])
        self.c2 = np.stack([corners32(b, r) for b, r in zip(boxes2, routes2)])
        e1 = np.array([corner_error(b, c) for b, c in zip(boxes1, self.c1)])
        e2 = np.array([corner_error(b, c) for b, c in zip(boxes2, self.c2)])
        self.i, self.j = np.array([p[0] for p in index]), np.array([p[1] for p in index])
        self.eps = np.maximum(e1[self.i], e2[self.j])
        if ref is None:
            ref = np.array([REF.iou3d(boxes1[i], boxes2[j]) for i, j in index])
        self.ref = ref
        self.vol, self.iou, self.surf = ref[:, 0], ref[:, 1], ref[:, 2] + ref[:, 3]
        self.v1 = np.array([REF.box_volume(boxes1[i]) for i in self.i])
        self.v2 = np.array([REF.box_volume(boxes2[j]) for j in self.j])

    def bound(self, eps=None):
        """2e-4, the figure granted on general pairs, plus how far corners displaced by eps can move the true IoU (dV <= eps * S;
        the factor 4 covers the two boxes and the quotient)"""
        eps = self.eps if eps is None else eps
        return 2e-4 + 4 * eps * self.surf / (self.v1 + self.v2 - self.vol)

    def moved(self, T, t):
        """the same pairs after a common rigid motion: the reference values are those of this set"""
        return Pairs([moved(b, T, t) for b in self.boxes1], [moved(b, T, t) for b in self.boxes2], self.routes1, self.routes2,
                     self.index, self.ref)


@functools.lru_cache(maxsize=None)
def family(name):
    """-> list of (variant label, Pairs); built once per process"""
    if name == "general":                                        # the 24 x 40 pairs of test_random_pairs_vs_oracle
        rng = np.random.default_rng(5)
        A = [(rng.normal(size=3) + [0, 0, 8], rng.uniform(0.4, 3, 3), rot(rng.normal(size=3), rng.uniform(0, 3))) for _ in range(24)]
        B = [(box(*A[i % 24]).mean(0) + rng.normal(size=3) * 0.6, rng.uniform(0.4, 3, 3), rot(rng.normal(size=3), rng.uniform(0, 3)))
             for i in range(40)]
        return [("24x40", Pairs(A, B, ["f64"] * 24, ["f64"] * 40, [(i, j) for i in range(24) for j in range(40)]))]
    make, variants, seed = FAMILIES[name]
    rng = np.random.default_rng(seed)
    out = []
    for v in variants:
        rows = [make(rng, v if v is not None else k) for k in range(PAIRS)]
        out.append((str(v), Pairs([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows],
                                  [(k, k) for k in range(PAIRS)])))
    return out


def variants(name):
    return ["24x40"] if name == "general" else [str(v) for v in FAMILIES[name][1]]


def motion(name):
    """the seeded rigid motion of a family: a random rotation and a translation of up to 50 m"""
    rng = np.random.default_rng(1000 + NAMES.index(name))
    return _rand_rot(rng), _unit(rng) * rng.uniform(10, 50)
