"""TEST INFRASTRUCTURE ONLY -- input cases of the weak-loss tests (tests/test_weak_loss_ref.py on the CPU,
tests/test_gpu_weak_loss_f64.py on the GPU), built so that every discrete decision of every valid slot is DECIDED: the builder
evaluates the float64 reference (tests/weak_loss_ref.py), redraws the random slots whose decision margin is under its threshold
and asserts that this hit at most 3 % of the slots.  Constructed slots carry exact ties on purpose and are exempt.

Small scenes: two image sizes (96 x 128 and 120 x 100) inside 120 x 128 padded depth maps, every odd image without a ground map,
K = 50 classes, G = 6 objects per image.  Numbers that the product rounds to float32 on the host (K / ratio) are exact."""
import torch

import weak_loss_ref as ref

SIZES = [(96, 128), (120, 100)]
KS = [[[110.0, 0.0, 64.0], [0.0, 110.0, 48.0], [0.0, 0.0, 1.0]], [[137.5, 0.0, 62.5], [0.0, 137.5, 75.0], [0.0, 0.0, 1.0]]]
RATIOS = [1.0, 1.25]
HP, WP = 120, 128
G = 6
VFOCAL = 512.0
REDRAW_CAP = 0.03
BITS = {"iou": 1, "pose_alignment": 2, "pose_ground": 4, "z": 8, "z_pseudo_gt_patch": 16, "z_pseudo_gt_center": 16, "dims": 32 | 64 | 128}
PRODUCTION = ["dims", "pose_alignment", "pose_ground", "iou", "z", "z_pseudo_gt_patch"]


def terms_of(loss_functions):
    t = 0
    for name in loss_functions:
        t |= BITS[name]
    pgz = 1 if "z_pseudo_gt_patch" in loss_functions else (2 if "z_pseudo_gt_center" in loss_functions else 0)
    return t, pgz


def _draw_rows(g, rows, c):
    """fresh random head outputs and proposals for the given slots (flat indices)"""
    K, kf = c["K"], c["kf"]
    m = len(rows)
    if m == 0:
        return
    rows = torch.as_tensor(rows)
    b, j = rows // kf, rows % kf
    raw = torch.zeros(m, c["raw"].shape[1], dtype=torch.float64)
    raw[:, :2 * K] = torch.randn(m, 2 * K, generator=g, dtype=torch.float64) * 0.1
    raw[:, 2 * K:5 * K] = torch.randn(m, 3 * K, generator=g, dtype=torch.float64) * 0.4
    raw[:, 5 * K:11 * K] = torch.randn(m, 6 * K, generator=g, dtype=torch.float64)
    v2r = torch.tensor([KS[i % 2][1][1] / (VFOCAL * RATIOS[i % 2]) for i in b.tolist()], dtype=torch.float64)
    raw[:, 11 * K:12 * K] = (torch.rand(m, K, generator=g, dtype=torch.float64) * 4.5 + 1.5) / v2r[:, None]      # 1.5 .. 6 m
    raw[:, 12 * K:13 * K] = torch.rand(m, K, generator=g, dtype=torch.float64) * 2 - 0.2                         # some under the clip
    c["raw"][rows] = raw.float().double()                                        # float32 values: the kernels see the same numbers
    gb = c["gt_boxes"][b, c["gt_idx"][b, j]]
    c["boxes"][b, j] = (gb + torch.randn(m, 4, generator=g, dtype=torch.float64) * 1.5).float().double()


def make_case(B, kf, S, seed, loss_functions=PRODUCTION, valid="most", allocentric=True, priors=True, constructed=False, redraw=True):
    """valid: 'all' | 'most' (random 3 of 4) | 'interleaved' | 'none' | 'one_each' | a list of per-image slot lists"""
    g = torch.Generator().manual_seed(seed)
    K = 50
    terms, pgz = terms_of(loss_functions)
    sizes = [SIZES[b % 2] for b in range(B)]
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    span = torch.tensor([[[s[1] - 40.0, s[0] - 40.0]] for s in sizes], dtype=torch.float64)
    ctr = rnd(B, G, 2) * span + 20
    wh = rnd(B, G, 2) * 34 + 16
    gt_boxes = torch.cat((ctr - wh / 2, ctr + wh / 2), -1).float().double()
    gt3d = torch.cat((ctr, rnd(B, G, 1) * 4.5 + 1.5, rnd(B, G, 3) + 0.4, torch.randn(B, G, 3, generator=g, dtype=torch.float64)), -1)
    gt3d = gt3d.float().double()
    gt_poses = torch.eye(3, dtype=torch.float64).expand(B, G, 3, 3).contiguous()
    gt_idx = torch.randint(0, G, (B, S), generator=g)
    cls = torch.randint(0, K, (B, S), generator=g)
    v = torch.zeros(B, S, dtype=torch.bool)
    if valid == "all":
        v[:, :kf] = True
    elif valid == "most":
        v[:, :kf] = torch.rand(B, kf, generator=g) < 0.75
        v[:, 0] = True
        v[:, min(1, kf - 1)] = True
    elif valid == "interleaved":
        v[:, 0:kf:2] = True
    elif valid == "one_each":
        for b in range(B):
            v[b, (5 * b + 3) % kf] = True
    elif valid != "none":
        for b, pat in enumerate(valid):
            v[b, torch.tensor(pat, dtype=torch.long)] = True
    v[:, kf:] = True                                                            # background slots: never part of the cube branch
    pri = (rnd(K, 2, 3) * 0.8 + 0.4).float().double()
    pri[:, 1] *= 0.25
    depth = (rnd(B, HP, WP) * 6 + 0.8).float().double()
    nrm = torch.nn.functional.normalize(torch.tensor([[0.05, 0.99, 0.1], [-0.1, 0.97, 0.2]], dtype=torch.float64), dim=1)
    c = dict(B=B, kf=kf, S=S, G=G, K=K, layout=(0, 2 * K, 5 * K, 11 * K, 12 * K), raw=torch.zeros(B * kf, 13 * K + 3, dtype=torch.float64),
             classes=cls, valid=v, gt_idx=gt_idx, boxes=torch.zeros(B, S, 4, dtype=torch.float64), gt_boxes=gt_boxes, gt3d=gt3d,
             gt_poses=gt_poses, prior_mean=pri[:, 0].contiguous() if priors else None, prior_std=pri[:, 1].contiguous() if priors else None,
             Ks=torch.tensor([KS[b % 2] for b in range(B)], dtype=torch.float64), ratios=[RATIOS[b % 2] for b in range(B)],
             image_sizes=sizes, ground_sizes=[sizes[b] if b % 2 == 0 else (1, 1) for b in range(B)], depth=depth, depth_sizes=sizes,
             normals=torch.stack([nrm[b % 2] for b in range(B)]).float().double(), terms=terms, pgz_mode=pgz, allocentric=allocentric,
             virtual_focal=VFOCAL, loss_functions=list(loss_functions),
             weights=dict(iou=1.0, pose=7.0, normal=20.0, z=1.0, dims=20.0, w3d=1.0, conf=1.0))
    # proposals of the background slots too (never read by the cube branch)
    bb = torch.arange(B)[:, None].expand(B, S)
    c["boxes"] = (gt_boxes[bb, gt_idx] + torch.randn(B, S, 4, generator=g, dtype=torch.float64) * 1.5).float().double()
    n = B * kf
    _draw_rows(g, list(range(n)), c)
    exempt = torch.zeros(n, dtype=torch.bool)
    if constructed:
        exempt = _construct(c)
    # ---- redraw the undecided random slots
    redrawn = set()
    for _ in range(8 if redraw else 0):
        out = ref.run(c, torch.float64, want_grad=False)
        bad = torch.nonzero(ref.undecided(out, exempt)).squeeze(1).tolist()
        if not bad:
            break
        redrawn.update(bad)
        _draw_rows(g, bad, c)
    else:
        assert not redraw, "the case builder did not settle"
    c["redrawn"], c["exempt"] = len(redrawn), exempt
    assert len(redrawn) <= REDRAW_CAP * n, (len(redrawn), n)
    return c


def _set(c, slot, cls_cols, value):
    """write `value` into the selected class's columns of a slot's row"""
    b, j = divmod(slot, c["kf"])
    k = int(c["classes"][b, j])
    o, wd = cls_cols
    c["raw"][slot, o + k * wd:o + (k + 1) * wd] = torch.as_tensor(value, dtype=torch.float64)


def _construct(c):
    """constructed slots among the random ones (kf >= 24, B >= 2); returns the exemption mask.  Every number written is exact in
    float32."""
    kf, K, n = c["kf"], c["K"], c["B"] * c["kf"]
    assert kf >= 24 and c["B"] >= 2
    ex = torch.zeros(n, dtype=torch.bool)
    D2, DIMS, Z, UNC = (0, 2), (2 * K, 3), (11 * K, 1), (12 * K, 1)
    # image 0: valid and invalid slots interleaved; slots 2, 6, 10 pushed far to the right, so that every corner clamps to the
    # upper x bound: windows without area among windows with area -> the window-median targets are permuted
    c["valid"][0, :kf] = False
    c["valid"][0, 0:kf:2] = True
    # (their area is 0 at every step of the depth search: the 1e7 rule, and an argmin over equal numbers)
    for j in (2, 6, 10):
        _set(c, j, D2, [32.0, 0.0])
        ex[j] = True
    # a cuboid the camera sits in (corners behind the image plane), and a proposal that sticks out of the image
    _set(c, 4, Z, [0.25])
    ex[4] = True
    c["boxes"][0, 8] = torch.tensor([-30.0, 40.0, 10.0, 80.0], dtype=torch.float64)
    # dims: a raw value over the clip at 5 (no gradient)
    _set(c, 12, DIMS, [5.5, 0.0, -0.25])
    ex[12] = True
    # a projected box EQUAL to its 2D box: an axis-aligned slab around the camera, 148 times as long and high as it is wide, sends
    # corners past all four clamp bounds, and object 5 of the image is given those bounds as its box (exact in both precisions)
    _set(c, 16, DIMS, [0.0, 5.5, 5.5])
    _set(c, 16, (5 * K, 6), [1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    _set(c, 16, Z, [0.25])
    _set(c, 16, D2, [0.0, 0.0])
    c["boxes"][0, 16] = torch.tensor([48.0, 32.0, 80.0, 64.0], dtype=torch.float64)      # centred on the principal point: no turn
    H, Wd = c["image_sizes"][0]
    c["gt_boxes"][0, 5] = torch.tensor(ref.int_bounds(H)[:1] + ref.int_bounds(Wd)[:1] + ref.int_bounds(H)[1:] + ref.int_bounds(Wd)[1:],
                                       dtype=torch.float64)
    c["gt_idx"][0][c["gt_idx"][0] == 5] = 4                                      # the object is this slot's alone
    c["gt_idx"][0, 16] = 5
    ex[16] = True
    # uncertainty under its clip at 0.01
    _set(c, 14, UNC, [-0.5])
    # image 1 (no ground map: confidence 0.1): object 5 lies left of the image with x2 + 50 < 1 -> the centre test of the depth
    # search fails (loss 2.5) and the projected box is disjoint from it
    c["gt_boxes"][1, 5] = torch.tensor([-90.0, 20.0, -60.0, 50.0], dtype=torch.float64)
    for j in (1, 3):
        c["valid"][1, j] = True
        c["gt_idx"][1, j] = 5
        c["boxes"][1, j] = torch.tensor([30.0, 30.0, 60.0, 70.0], dtype=torch.float64)
    return ex


SWEEP = [(1, 1, 1), (1, 7, 7), (2, 63, 70), (2, 64, 64), (3, 65, 80), (4, 128, 512), (5, 65, 65), (3, 255, 256), (3, 256, 256)]
VALIDITY = {
    "all": "all",
    "one_image_empty": [list(range(0, 65, 2)), [], list(range(1, 40))],
    "one_image_single": [list(range(0, 65, 3)), [17], list(range(5, 64))],
    "one_each": "one_each",
    "none": "none",
    "interleaved": "interleaved",
}

CENTER = PRODUCTION[:-1] + ["z_pseudo_gt_center"]
ISOLATED = {"iou": ["iou"], "pose": ["pose_alignment"], "normal": ["pose_ground"], "z": ["z"], "pgz_patch": ["z_pseudo_gt_patch"],
            "pgz_center": ["z_pseudo_gt_center"], "dims": ["dims"], "production": PRODUCTION}


def sweep_seed(B, kf, S):
    """seeds of the shape sweep (3 % of fewer than 34 slots is no slot: there the seed is one that needs no redraw)"""
    return {(1, 1, 1): 101, (1, 7, 7): 102}.get((B, kf, S), 100 + B * 1000 + kf)
