"""TEST INFRASTRUCTURE ONLY -- an independent statement of the IoU of two oriented 3D boxes (numpy float64), for the tests of
oracle/iou3d.py, cr_box3d_overlap and the grouped evaluation kernel.

It shares neither the input nor the method of oracle/iou3d.py.  The input is the GENERATING PARAMETERS of the two boxes in
float64 (centre, extents, rotation), never rounded corners, so its 12 half-spaces are exact planes; and it has no tolerance:
in a frame centred on box 1 the planes that coincide (to 1e-12) are merged (of opposite orientation: both lose their face,
the two pieces cancel), every remaining plane carries a large quad that
is clipped by all other half-spaces with a plain `d <= 0`, and the volume is 1/3 * sum (n . p0) * area.  Two nearly parallel
faces are split along the line where each crosses the other's plane, found once from either side, and the two findings differ
by (distance of a quad's points from their own plane) / (relative tilt): the arithmetic is therefore done in numpy's long
double (1e-19 on x86-64; float64 quads lie 1e-16 m off their planes, which at a tilt of 1e-5 degree moved the lines by 1e-9 m
and the volume by 4e-9).  Inputs and results are float64.  tests/test_iou3d_ref.py checks it against qhull's half-space
intersection on every family of tests/iou3d_families.py (worst 1.3e-12 of the smaller box volume; the bound is 1e-9) and
against the first-order volume of slightly rotated boxes."""
import numpy as np

MERGE = 1e-12
LD = np.longdouble


def half_spaces(centre, dims, R, origin):
    """the 6 half-spaces n.x <= off of a box (columns of R are its axes), relative to `origin`: (6,3), (6,)"""
    R = np.asarray(R, LD)
    n = np.concatenate([R.T, -R.T])
    h = np.asarray(dims, LD) / 2
    off = n @ (np.asarray(centre, LD) - origin) + np.concatenate([h, h])
    return n, off


def _clip(poly, n, off):
    """the part of the polygon (k,3) with n.x <= off"""
    if len(poly) == 0:
        return poly
    d = poly @ n - off
    out = []
    for i in range(len(poly)):
        j = (i + 1) % len(poly)
        if d[i] <= 0:
            out.append(poly[i])
        if (d[i] <= 0) != (d[j] <= 0):
            out.append(poly[i] + (poly[j] - poly[i]) * (d[i] / (d[i] - d[j])))
    return np.array(out, LD).reshape(-1, 3)


def intersection_volume(box1, box2):
    """box = (centre (3,), extents (3,), rotation (3,3)) in float64 -> volume of the intersection"""
    origin = np.asarray(box1[0], LD)
    n1, o1 = half_spaces(*box1, origin)
    n2, o2 = half_spaces(*box2, origin)
    n, off = np.concatenate([n1, n2]), np.concatenate([o1, o2])
    keep = []
    for i in range(12):                                   # one plane of every coinciding set
        if not any(np.abs(n[i] - n[k]).max() <= MERGE and abs(off[i] - off[k]) <= MERGE for k in keep):
            keep.append(i)
    n, off = n[keep], off[keep]
    # two coinciding planes of opposite orientation (touching faces) bound pieces that cancel: neither carries a quad
    cancel = [any(np.abs(n[i] + n[k]).max() <= MERGE and abs(off[i] + off[k]) <= MERGE for k in range(len(n))) for i in range(len(n))]
    big = 4.0 * (np.abs(off).max() + 1.0)
    vol = LD(0)
    for i in range(len(n)):
        if cancel[i]:
            continue
        a = np.eye(3, dtype=LD)[np.argmin(np.abs(n[i]))]
        u = np.cross(n[i], a)
        u /= np.sqrt(u @ u)
        v = np.cross(n[i], u)
        poly = n[i] * (off[i] / (n[i] @ n[i])) + big * np.array([u + v, u - v, -u - v, -u + v])     # on the plane whatever |n|
        others = [k for k in range(len(n)) if k != i]
        for k in sorted(others, key=lambda k: abs(n[i] @ n[k])):     # transversal planes first: the quad is small by the
            poly = _clip(poly, n[k], off[k])                        # time a nearly parallel plane cuts it
        if len(poly) >= 3:
            s = np.cross(poly[1:-1] - poly[0], poly[2:] - poly[0]).sum(0)
            vol += (n[i] @ poly[0]) * 0.5 * abs(s @ n[i])
    return max(float(vol / 3), 0.0)


def box_volume(box):
    return float(np.prod(box[1]))


def box_surface(box):
    a, b, c = box[1]
    return float(2 * (a * b + b * c + c * a))


def iou3d(box1, box2):
    """-> (intersection volume, IoU, surface of box 1, surface of box 2)"""
    v = intersection_volume(box1, box2)
    return v, v / (box_volume(box1) + box_volume(box2) - v), box_surface(box1), box_surface(box2)
