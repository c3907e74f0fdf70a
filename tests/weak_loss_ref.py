"""TEST INFRASTRUCTURE ONLY -- an independent plain-torch statement of the training branch of the weakly supervised 3D head
(ROIHeads3DScore._forward_cube of the reference, cubercnn/modeling/roi_heads/roi_heads.py) on the static (B, kf) slot layout of
the fused kernels (csrc/weak_loss.hip), for tests/test_weak_loss_ref.py and tests/test_gpu_weak_loss_f64.py.

Restated from the definitions: roi_heads.py:1055-1074 (pose alignment), :1151-1194 (depth search), :1196-1232 and :1256-1277
(pseudo depth), :1233-1254 (dimension hinge), :1470-1552 (decode), :1593-1726 (terms, logged statistics, uncertainty), :2843-2851
(safely_reduce_losses); ProposalNetwork/utils/conversions.py:25-48 (hull); Cubes.get_bube_corners (projection and clamp);
util.R_from_allocentric with pytorch3d's axis_angle_to_matrix; pytorch3d's rotation_6d_to_matrix; torchvision's
generalized_box_iou_loss; detectron2's Boxes.clip / pairwise_iou.  It imports nothing from the package: K / ratio, the integer
clamp bounds, the ground confidence and virtual-to-real are derived here from Ks, the ratios and the image / map sizes.

dtype-generic: `run(case, torch.float64)` is the truth, `run(case, torch.float32)` (CPU) the yardstick of what float32 arithmetic
can give.  Quirks of the reference are kept: the `(a <= c) <= b` test of the depth search, torch.argmin (first minimum, NaN
wins), torch.linspace(0, 4.9, 50), the ground confidence squared in total_3D_loss, the [windows with area..., windows without...]
order of the window-median targets, the skip-and-count of one-box images in the pose alignment (an image WITHOUT boxes adds the
mean of nothing, NaN), the lower median.

A case is a dict of CPU tensors / numbers:
  raw (n, ld) head output, layout (o_deltas, o_dims, o_pose, o_z, o_uncert), K classes
  classes, valid, gt_idx (B,S); kf; boxes (B,S,4) proposals (the first kf of every image are the slots)
  gt_boxes (B,G,4), gt3d (B,G,9) [x2d y2d z w h l ...], gt_poses (B,G,3,3; the weak losses do not read them)
  prior_mean, prior_std (K,3) or None
  Ks (B,3,3), ratios (B), image_sizes [(H,W)], ground_sizes [(h,w)] ((1,1): no ground map) or None
  depth (B,Hp,Wp) padded maps, depth_sizes [(h,w)]; normals (B,3)
  terms (bit k = term k: 0 iou 1 pose 2 normal 3 z 4 pseudo_gt_z 5 dims_w 6 dims_h 7 dims_l), pgz_mode (0 none, 1 window median,
  2 depth under the centre), weights dict(iou, pose, normal, z, dims, w3d, conf), allocentric, virtual_focal (None: no virtual depth)
"""
import math

import torch

STEPS = 50
NAMES = ("iou", "pose", "normal", "z", "pseudo_gt_z", "dims_w", "dims_h", "dims_l")
# sign pattern of the 8 cuboid vertices along the box axes (x: length, y: height, z: width), get_cuboid_verts_faces
_SX = (-1, 1, 1, -1, -1, 1, 1, -1)
_SY = (-1, -1, 1, 1, -1, -1, 1, 1)
_SZ = (-1, -1, -1, -1, 1, 1, 1, 1)


def term_weights(w):
    """weight of red[k] in the trained total (roi_heads.py:1728-1761, :1725): 8 terms, then the uncertainty"""
    w3 = w["w3d"]
    return [w["iou"] * w3, w["pose"] * w3, w["normal"] * w3, w["z"] * w3, w["z"] * w3, w["dims"] * w3, w["dims"] * w3, w["dims"] * w3,
            w["conf"]]


def rot6d(a):
    """pytorch3d rotation_6d_to_matrix: Gram-Schmidt on the two 3-vectors, rows b1, b2, b1 x b2"""
    a1, a2 = a[:, :3], a[:, 3:]
    b1 = a1 / a1.norm(dim=1, keepdim=True).clamp(min=1e-12)
    b2 = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    b2 = b2 / b2.norm(dim=1, keepdim=True).clamp(min=1e-12)
    return torch.stack((b1, b2, torch.linalg.cross(b1, b2, dim=1)), 1)


def axis_angle_to_matrix(aa):
    """pytorch3d: axis-angle -> quaternion -> matrix"""
    ang = aa.norm(dim=1, keepdim=True)
    half = ang * 0.5
    small = ang.abs() < 1e-6
    s = torch.where(small, 0.5 - ang * ang / 48, torch.sin(half) / torch.where(small, torch.ones_like(ang), ang))
    q = torch.cat((torch.cos(half), aa * s), 1)
    r, i, j, k = q.unbind(1)
    two_s = 2.0 / (q * q).sum(1)
    return torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                        two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                        two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), 1).view(-1, 3, 3)


def from_allocentric(Km, Ra, u, v):
    """util.R_from_allocentric: rotate by the turn that takes the optical axis onto the ray through (u, v)"""
    ray = torch.stack(((u - Km[:, 0, 2]) / Km[:, 0, 0], (v - Km[:, 1, 2]) / Km[:, 1, 1], torch.ones_like(u)), 1)
    ray = ray / ray.norm(dim=1, keepdim=True)
    angle = torch.acos(ray[:, 2])
    axis = torch.stack((-ray[:, 1], ray[:, 0], torch.zeros_like(u)), 1)
    M = axis_angle_to_matrix(angle[:, None] * axis / axis.norm(dim=1, keepdim=True))
    turn = (angle > 0)[:, None, None]                    # on the optical axis the reference leaves the row alone (0 / 0 in M there)
    return torch.where(turn, torch.bmm(torch.where(turn, M, torch.eye(3, dtype=M.dtype).expand_as(M)), Ra), Ra)


def int_bounds(c):
    """Cubes.get_bube_corners: the corners are clamped to [int(-c/2+1), int(c-1+c)]"""
    return float(int(-c / 2 + 1)), float(int(c - 1 + c))


def project(centre, dims, R, Km, bnd):
    """8 corners of the cuboids -> (unclamped u, v (m,8), depth along the axis (m,8), clamped XYXY hull (m,4))"""
    dt = centre.dtype
    sx, sy, sz = (torch.tensor(s, dtype=dt) for s in (_SX, _SY, _SZ))
    loc = torch.stack((dims[:, 2:3] * sx / 2, dims[:, 1:2] * sy / 2, dims[:, 0:1] * sz / 2), 1)          # (m,3,8)
    verts = torch.bmm(R, loc) + centre[:, :, None]
    p = torch.bmm(Km, verts)
    fu, fv = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    cu = torch.clamp(fu, bnd[:, 0:1], bnd[:, 1:2])
    cv = torch.clamp(fv, bnd[:, 2:3], bnd[:, 3:4])
    box = torch.stack((cu.min(1).values, cv.min(1).values, cu.max(1).values, cv.max(1).values), 1)
    return fu, fv, p[:, 2], cu, cv, box


def giou_loss(b1, b2, eps=1e-7):
    """torchvision.ops.generalized_box_iou_loss of paired XYXY boxes, reduction 'none'"""
    x1, y1, x2, y2 = b1.unbind(-1)
    x1g, y1g, x2g, y2g = b2.unbind(-1)
    xk1, yk1, xk2, yk2 = torch.max(x1, x1g), torch.max(y1, y1g), torch.min(x2, x2g), torch.min(y2, y2g)
    inter = torch.where((yk2 > yk1) & (xk2 > xk1), (xk2 - xk1) * (yk2 - yk1), torch.zeros_like(x1))
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter
    iou = inter / (union + eps)
    xc1, yc1, xc2, yc2 = torch.min(x1, x1g), torch.min(y1, y1g), torch.max(x2, x2g), torch.max(y2, y2g)
    area_c = (xc2 - xc1) * (yc2 - yc1)
    return 1 - (iou - (area_c - union) / (area_c + eps))


def safe_reduce(loss):
    """safely_reduce_losses: mean over the finite entries; none finite: mean * 0"""
    ok = ~loss.isinf() & ~loss.isnan()
    if bool(ok.any()):
        return loss[ok].mean()
    return loss.mean() * 0.0


def _frac_margin(x):
    """distance of x to the next integer"""
    return (x - torch.round(x)).abs()


def run(case, dtype=torch.float64, want_grad=True):
    """-> dict: dec (n,17), pbox (n,4), L (n,8) raw terms, ztgt (n) depth targets, validf (n), red (9), stats (8), total, grad (n,ld),
    margins {name: (n)} of the discrete decisions (what they are relative to is said at each; +inf where none is taken)"""
    c, dt = case, dtype
    f = lambda t: torch.as_tensor(t, dtype=torch.float64).to(dt)
    B, S = c["classes"].shape
    kf, K, n = int(c["kf"]), int(c["K"]), int(c["classes"].shape[0]) * int(c["kf"])
    o_d2, o_dims, o_pose, o_z, o_unc = (int(v) for v in c["layout"])
    terms, pgz_mode, w = int(c["terms"]), int(c["pgz_mode"]), c["weights"]
    inf = torch.full((n,), float("inf"), dtype=torch.float64)
    marg = {}

    raw = f(c["raw"]).clone().requires_grad_(want_grad)
    cls0 = c["classes"][:, :kf].reshape(n)
    validf = c["valid"][:, :kf].reshape(n).bool() & (cls0 >= 0) & (cls0 < K)
    cls = cls0.clamp(0, K - 1)
    img = torch.arange(n) // kf
    gidx = torch.where(validf, c["gt_idx"][:, :kf].reshape(n), torch.zeros_like(cls))
    ar = torch.arange(n)
    cols = lambda o, wd: raw[ar[:, None], (o + cls * wd)[:, None] + torch.arange(wd)[None, :]]
    dxy, zr, dr, a6 = cols(o_d2, 2), cols(o_z, 1)[:, 0], cols(o_dims, 3), cols(o_pose, 6)
    u = cols(o_unc, 1)[:, 0].clamp(min=0.01)                                   # CubeHead: uncertainty clipped at 0.01
    # the reference only ever sees the valid RoIs: empty slots are given harmless numbers (their results mean nothing and no
    # gradient reaches them)
    keep = lambda t, fill: torch.where(validf.view(-1, *[1] * (t.dim() - 1)), t, torch.tensor(fill, dtype=dt).expand_as(t))
    dxy, zr, dr, u = keep(dxy, 0.0), keep(zr, 20.0), keep(dr, 0.0), keep(u, 1.0)
    a6 = keep(a6, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    Ra = rot6d(a6)

    # ---- per-image constants (:1369-1404)
    Ks, ratios = f(c["Ks"]), f(c["ratios"])
    Kimg = Ks / ratios[:, None, None]
    Kimg[:, 2, 2] = 1
    Km = Kimg[img]
    Himg = f([s[0] for s in c["image_sizes"]])
    Wimg = f([s[1] for s in c["image_sizes"]])
    if c.get("virtual_focal") is not None:
        v2r_img = (Himg * Ks[:, 1, 1]) / (float(c["virtual_focal"]) * (Himg * ratios))
    else:
        v2r_img = torch.ones(B, dtype=dt)
    # the reference hands (H, W) of the image to the clamp, whose first entry bounds x (:1422-1427, :1580)
    bnd = f([int_bounds(s[0]) + int_bounds(s[1]) for s in c["image_sizes"]])[img]
    gconf_img = f([1.0 if (c.get("ground_sizes") is None or tuple(g) != (1, 1)) else 0.1 for g in
                   (c["ground_sizes"] if c.get("ground_sizes") is not None else c["image_sizes"])])
    dsz = c["depth_sizes"] if c.get("depth_sizes") is not None else c["image_sizes"]
    ih, iw = f([s[0] for s in dsz])[img], f([s[1] for s in dsz])[img]
    extent = torch.maximum(Himg, Wimg)[img].double()

    # ---- decode (:1406-1526)
    sb = keep(f(c["boxes"])[:, :kf].reshape(n, 4), [10.0, 10.0, 40.0, 40.0])
    sw, sh = sb[:, 2] - sb[:, 0], sb[:, 3] - sb[:, 1]
    cux = sb[:, 0] + 0.5 * sw + sw * dxy[:, 0]
    cuy = sb[:, 1] + 0.5 * sh + sh * dxy[:, 1]
    pm = f(c["prior_mean"])[cls] if c.get("prior_mean") is not None else torch.ones(n, 3, dtype=dt)
    ps = f(c["prior_std"])[cls] if c.get("prior_std") is not None else torch.ones(n, 3, dtype=dt)
    dims = torch.exp(dr.clamp(max=5)) * pm
    R = from_allocentric(Km, Ra, cux.detach(), cuy.detach()) if c["allocentric"] else Ra
    z = zr * v2r_img[img]
    x3d = z * (cux - Km[:, 0, 2]) / Km[:, 0, 0]
    y3d = z * (cuy - Km[:, 1, 2]) / Km[:, 1, 1]
    centre = torch.stack((x3d, y3d, z), 1)
    fu, fv, pz, cu, cv, pbox = project(centre, dims, R, Km, bnd)
    gtb = f(c["gt_boxes"])[img, gidx]
    g3 = f(c["gt3d"])[img, gidx]

    # margins of the projection: for each hull side the extreme corner, if the clamp lets it through, must beat the runner-up and
    # stay off the clamp bounds; relative to the image extent
    with torch.no_grad():
        m_hull, m_clamp = inf.clone(), inf.clone()
        for vals, raws, lo, hi, smallest in ((cu, fu, bnd[:, 0], bnd[:, 1], True), (cv, fv, bnd[:, 2], bnd[:, 3], True),
                                             (cu, fu, bnd[:, 0], bnd[:, 1], False), (cv, fv, bnd[:, 2], bnd[:, 3], False)):
            srt = torch.sort(vals.double(), dim=1, descending=not smallest)
            gap = (srt.values[:, 0] - srt.values[:, 1]).abs() / extent
            first = torch.gather(raws.double(), 1, srt.indices[:, :1])[:, 0]
            off = torch.minimum((first - lo.double()).abs(), (first - hi.double()).abs()) / extent
            passes = (first >= lo.double()) & (first <= hi.double())
            m_hull = torch.minimum(m_hull, torch.where(passes, gap, inf))
            m_clamp = torch.minimum(m_clamp, torch.where(torch.isfinite(first), off, inf))
        bad = ~torch.isfinite(pbox.double()).all(1)
        marg["hull"], marg["clamp"] = torch.where(bad, inf, m_hull), torch.where(bad, inf, m_clamp)
        marg["behind"] = pz.double().abs().min(1).values / (z.double().abs() + 1.0)       # a corner on the camera plane

    L = [None] * 8
    zero_steps = torch.zeros(n, dtype=torch.long)
    # ---- terms (:1593-1650)
    if terms & 1:
        L[0] = giou_loss(gtb, pbox)
        with torch.no_grad():
            g, p = gtb.double(), pbox.double()
            d = torch.stack(((g[:, 0] - p[:, 0]).abs(), (g[:, 1] - p[:, 1]).abs(), (g[:, 2] - p[:, 2]).abs(), (g[:, 3] - p[:, 3]).abs(),
                             (torch.min(g[:, 2], p[:, 2]) - torch.max(g[:, 0], p[:, 0])).abs(),
                             (torch.min(g[:, 3], p[:, 3]) - torch.max(g[:, 1], p[:, 1])).abs()), 1).min(1).values / extent
            # a box whose four sides sit on clamp bounds takes no gradient: its comparisons decide nothing
            frozen = ((cu.double() <= bnd[:, 0:1].double()) | (cu.double() >= bnd[:, 1:2].double())).all(1) & \
                     ((cv.double() <= bnd[:, 2:3].double()) | (cv.double() >= bnd[:, 3:4].double())).all(1)
            marg["giou"] = torch.where(frozen | bad, inf, d)
    vidx = [torch.nonzero(validf[b * kf:(b + 1) * kf]).squeeze(1) + b * kf for b in range(B)]
    if terms & 2:
        # pose_loss (:1055-1074) over the valid slots of every image, in slot order
        total, fail = torch.zeros(1, dtype=dt), 0
        m_pose = inf.clone()
        for b in range(B):
            Rb = R[vidx[b]].reshape(-1, 9)
            m = Rb.shape[0]
            if m == 1:
                fail += 1
                continue
            ij = torch.tril_indices(m, m, -1)
            cosang = ((Rb[ij[0]] * Rb[ij[1]]).sum(1) - 1) * 0.5                # cos of the relative angle from the trace
            total = total + torch.mean(1 - cosang.abs())                        # no box at all: the mean of nothing, NaN
            if m > 1:
                with torch.no_grad():
                    full = torch.full((m, m), float("inf"), dtype=torch.float64)
                    full[ij[0], ij[1]] = cosang.double().abs()
                    full = torch.minimum(full, full.t())
                    m_pose[vidx[b]] = full.min(1).values
        pose = None if fail == B else total * 1 / (fail + 1)
        marg["pose"] = m_pose
        if pose is not None:
            L[1] = pose.repeat(n)
    nrm = f(c["normals"])[img] if c.get("normals") is not None else None
    if terms & 4:
        cs = torch.nn.functional.cosine_similarity(nrm, R[:, 1, :], dim=1)
        L[2] = (1 - cs.abs()) * gconf_img[img]
        marg["normal"] = cs.detach().double().abs()
    if terms & 8:
        with torch.no_grad():
            gt_area = (gtb[:, 2] - gtb[:, 0]) * (gtb[:, 3] - gtb[:, 1])
            pcx, pcy = (pbox[:, 0] + pbox[:, 2]) / 2, (pbox[:, 1] + pbox[:, 3]) / 2
            pred_area = (pbox[:, 2] - pbox[:, 0]) * (pbox[:, 3] - pbox[:, 1])
            # as in the reference: `(a <= c) <= b` compares a boolean with b
            within = ((gtb[:, 0] - STEPS <= pcx).to(dt) <= gtb[:, 2] + STEPS) & ((gtb[:, 1] - STEPS <= pcy).to(dt) <= gtb[:, 3] + STEPS)
            values = torch.linspace(0.0, (STEPS - 1) / 10, STEPS, dtype=dt)
            sign = torch.where(gt_area < pred_area, 1.0, -1.0).to(dt)
            mod_z = z.detach()[:, None] + sign[:, None] * values[None, :]
            rep = lambda t: t.detach()[:, None].expand(n, STEPS, *t.shape[1:]).reshape(n * STEPS, *t.shape[1:])
            cen = torch.stack((rep(x3d), rep(y3d), mod_z.reshape(-1)), 1)
            _, _, spz, _, _, sbox = project(cen, rep(dims), rep(R), rep(Km), rep(bnd))
            areas = ((sbox[:, 2] - sbox[:, 0]) * (sbox[:, 3] - sbox[:, 1])).view(n, STEPS)
            zero_steps = (areas == 0).sum(1)
            areas = areas + (areas == 0) * 10000000
            dist = (gt_area[:, None] - areas).abs()
            idx = torch.argmin(dist, dim=1)
            srt = torch.sort(dist.double(), dim=1).values
            ga = gt_area.double().abs().clamp(min=1e-30)
            m_search = torch.minimum((srt[:, 1] - srt[:, 0]) / ga, (gt_area.double() - pred_area.double()).abs() / ga)
            m_search = torch.where(torch.isnan(m_search), inf, m_search)
            m_search = torch.minimum(m_search, (spz.double().abs().view(n, -1).min(1).values / (z.double().abs() + 1.0)) * 10)
            marg["search"] = torch.where(within, m_search, inf)
        found = (z - (z + sign * values[idx])).abs()                         # both carry z: a constant for the network
        L[3] = torch.where(within, found, torch.full_like(found, 0.1 * STEPS)) / 2
    ztgt = torch.zeros(n, dtype=dt)
    if pgz_mode:
        depth = f(c["depth"])
        with torch.no_grad():
            def at(xx, yy, rows):
                xx, yy = torch.nan_to_num(xx, nan=10.0), torch.nan_to_num(yy, nan=10.0)      # (the reference fails on a NaN centre)
                x = torch.minimum(torch.maximum(xx, torch.full_like(xx, 10.0)), iw[rows] - 11)
                y = torch.minimum(torch.maximum(yy, torch.full_like(yy, 10.0)), ih[rows] - 11)
                m = torch.minimum(torch.where((x == 10) | (x == iw[rows] - 11), inf[rows], _frac_margin(x.double()) / extent[rows]),
                                  torch.where((y == 10) | (y == ih[rows] - 11), inf[rows], _frac_margin(y.double()) / extent[rows]))
                return depth[img[rows], y.long(), x.long()], m
            m_pix = inf.clone()
            if pgz_mode == 2:                                                  # pseudo_gt_z_point_loss
                ztgt, m_pix = at(cux.detach(), cuy.detach(), ar)
            else:                                                              # pseudo_gt_z_box_loss on the valid slots of every image
                pb = pbox.detach()
                q = torch.stack((pb[:, 0].clamp(min=0).minimum(iw), pb[:, 1].clamp(min=0).minimum(ih),
                                 pb[:, 2].clamp(min=0).minimum(iw), pb[:, 3].clamp(min=0).minimum(ih)), 1)     # Boxes.clip
                area = (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1]) > 0
                edge = torch.stack((iw, ih, iw, ih), 1)
                fr = torch.where((q == 0) | (q == edge) | (q == torch.round(q)), inf[:, None], _frac_margin(q.double()) / extent[:, None])
                for b in range(B):
                    vi = vidx[b]
                    if vi.numel() == 0:
                        continue
                    tin, tout = [], []
                    for i in vi[area[vi]].tolist():
                        x1, y1, x2, y2 = (int(v) for v in q[i].long().tolist())
                        win = depth[b, y1:y2, x1:x2]
                        tin.append(torch.median(win) if win.numel() else torch.full((), float("nan"), dtype=dt))
                        m_pix[i] = float(fr[i].min()) if win.numel() else 0.0      # an empty integer window: the reference fails
                    out = vi[~area[vi]]
                    if out.numel():
                        tz, mo = at((q[out, 0] + q[out, 2]) / 2, (q[out, 1] + q[out, 3]) / 2, out)
                        tout, m_pix[out] = list(tz), mo
                    # the targets of the image in the reference's order, against the predictions in slot order
                    ztgt[vi] = torch.stack(tin + tout) if (tin or tout) else ztgt[vi]
                    # float area > 0 decides the group: its smaller side against the extent
                    side = torch.minimum(q[vi, 2] - q[vi, 0], q[vi, 3] - q[vi, 1]).double() / extent[vi]
                    m_pix[vi] = torch.minimum(m_pix[vi], torch.where(side == 0, inf[vi], side))
            marg["pixel"] = m_pix
        L[4] = (z - ztgt).abs()
        marg["pgz_sign"] = (z.detach().double() - ztgt.double()).abs() / (z.detach().double().abs() + 1.0)
    if terms & (32 | 64 | 128):
        if not (c.get("prior_std") is not None and bool(torch.isnan(ps).any())):      # dim_loss: a NaN deviation drops the terms
            s = torch.max((dims - pm).abs() / ps - 1.0, torch.zeros_like(dims))
            for k in range(3):
                if terms & (32 << k):
                    L[5 + k] = s[:, k]
            with torch.no_grad():
                a = ((dims - pm).abs() / ps - 1.0).double().abs()
                a = torch.minimum(a, ((dims - pm).double().abs() / ps.double()))
                on = torch.tensor([bool(terms & (32 << k)) for k in range(3)])
                marg["hinge"] = torch.where(on[None, :], a, inf[:, None]).min(1).values

    # ---- logged statistics over the valid slots (:1652-1694)
    V = torch.nonzero(validf).squeeze(1)
    nv = V.numel()
    stats = torch.zeros(8, dtype=dt)
    with torch.no_grad():
        if nv:
            tot = torch.zeros(nv, dtype=dt)
            wk = (w["iou"], w["pose"], None, w["z"], w["z"], w["dims"], w["dims"], w["dims"])
            for k in range(8):
                if L[k] is None:
                    continue
                tot = tot + (L[k][V] * w["normal"] * gconf_img[img][V] if k == 2 else L[k][V] * wk[k])      # the confidence, again
            zerr = (z[V] - g3[V, 2]).abs()
            stats[0] = zerr.mean()
            stats[1] = (dims[V] - g3[V, 3:6]).abs().mean()
            stats[2] = (torch.stack((cux, cuy), 1)[V] - g3[V, :2]).abs().mean()
            stats[3] = (zerr < 0.20).to(dt).mean()
            g, p = gtb[V], pbox[V]
            wh = (torch.min(g[:, 2:], p[:, 2:]) - torch.max(g[:, :2], p[:, :2])).clamp(min=0)
            inter = wh[:, 0] * wh[:, 1]
            un = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) + (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]) - inter
            stats[4] = torch.where(inter > 0, inter / un, torch.zeros_like(inter)).mean()
            stats[5] = torch.exp(-u[V]).mean()
            stats[6] = safe_reduce(tot) if any(t is not None for t in L) else 0.0
            marg["z_close"] = inf.clone()
            marg["z_close"][V] = (zerr.double() - 0.20).abs()
        stats[7] = nv

    # ---- uncertainty weighting and reduction (:1696-1765)
    sf = math.sqrt(2.0) * torch.exp(-u)
    red = []
    for k in range(8):
        if L[k] is None or nv == 0:
            red.append(torch.zeros((), dtype=dt))
        else:
            red.append(safe_reduce((L[k] * sf)[V]))
    red.append(safe_reduce(u[V]) if nv else torch.zeros((), dtype=dt))
    red = torch.stack(red)
    total = (red * torch.tensor(term_weights(w), dtype=dt)).sum()
    grad = None
    if want_grad:
        grad = torch.autograd.grad(total, raw)[0] if total.requires_grad else torch.zeros_like(raw)
    Lm = torch.stack([t.detach() if t is not None else torch.zeros(n, dtype=dt) for t in L], 1)
    dec = torch.cat((cux[:, None], cuy[:, None], z[:, None], dims, R.reshape(n, 9), x3d[:, None], y3d[:, None]), 1).detach()
    return dict(dec=dec, pbox=pbox.detach(), L=Lm, ztgt=ztgt, validf=validf, red=red.detach(), stats=stats, total=total.detach(),
                grad=grad, margins=marg, zero_area_steps=zero_steps, pose_dropped=bool(terms & 2) and L[1] is None)


# thresholds of the decision margins.  Area and coordinate comparisons (depth search, clamp pass-through, hull extreme, GIoU):
# relative 1e-4 (of the gt area / of the image extent).  The integer truncation of window and pixel coordinates: 1e-5 of the
# extent -- at 1e-4 a window with four free edges in a 128 px image is within reach of an integer with probability
# 4 * 2 * 0.0128 = 10 % (7.9 % measured), more than any redraw cap allows, while float32 leaves a coordinate below 128 within a few
# ulp = 1.5e-5 px of its float64 value: 1e-5 * 128 px is still a factor of 50 to 100 (tests/test_weak_loss_ref.py asserts that both
# precisions look up the same depth targets on every case).  The others from float32 rounding: a cosine or a trace of unit vectors
# is off by a few 1e-7, so 4e-6 leaves a factor of ten; the hinge and the depth signs are differences of numbers of size one.
THRESH = {"hull": 1e-4, "clamp": 1e-4, "giou": 1e-4, "search": 1e-4, "pixel": 1e-5, "behind": 1e-5, "pose": 4e-6, "normal": 4e-6,
          "pgz_sign": 1e-5, "hinge": 1e-5, "z_close": 1e-5}


def undecided(out, exempt=None):
    """(n) bool: valid slots with a decision margin under its threshold; exempt (n) bool: constructed slots whose ties are exact"""
    n = out["validf"].shape[0]
    badm = torch.zeros(n, dtype=torch.bool)
    for k, m in out["margins"].items():
        badm |= m < THRESH[k]
    badm &= out["validf"]
    if exempt is not None:
        badm &= ~exempt
    return badm
