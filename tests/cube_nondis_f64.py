"""float64 restatement of the NON-disentangled losses of the 3D head (MODEL.ROI_CUBE_HEAD.DISENTANGLED_LOSS False,
roi_heads.py:2516-2560 and :2587-2591 of the reference), written from their description, in numpy, for the fixtures
tests/golden/cubehead_train_nondis*.npz.  Shared by tests/test_cube_nondis.py (which pins it to the reference's recorded
losses) and by the fixture generator (which uses it to refuse data whose gradient signs would hang on a rounding).

Per RoI, columns [dims, xy, z, pose, joint]:
  xy     mean_2 |delta - (gt centre - proposal centre) / (proposal width, height)|
  dims   mean_3 |raw dims - log(gt dims)|                              (no dimension priors; raw = before the clip at 5)
  pose   1 - (trace(P T^T) - 1) / 2;  allocentric: P = the head's matrix, T = M^T gt pose, M = rotation of the optical axis
         onto the ray through the predicted centre (where its angle > 0); else P = the head's matrix, T = gt pose
  z      direct |z v2r - gt z| ; sigmoid |sigmoid(raw) - clip(gt z r2v / 100, 0, 1)| ; log |raw - log(max(gt z r2v, 0.01))| ;
         clusters |raw - (gt z r2v - mean) / std| of the RoI's (class, bin);  r2v = 1 / v2r
  joint  mean_24 |corners(predicted cuboid) - corners(gt cuboid)|
then x sqrt(2) exp(-u), optionally x 1 / log(max(gt z, e)), mean over the RoIs, x the loss weight.
"""
import numpy as np

# the nine fixtures: suffix -> (z_type, options that differ from allocentric / no inverse-z / joint weight 1)
CASES = {
    "": ("direct", {}),
    "_zsigmoid": ("sigmoid", {}),
    "_zlog": ("log", {}),
    "_bins3_direct": ("direct", {}),
    "_bins3_clusters": ("clusters", {}),
    "_egocentric": ("direct", {"allocentric": False}),
    "_inverse_z": ("direct", {"inverse_z": True}),
    "_nojoint": ("direct", {"w_joint": 0.0}),
    "_l1pose": ("direct", {"chamfer_pose": False}),
}
WEIGHTS = {"dims": 20.0, "xy": 1.0, "z": 1.0, "pose": 7.0, "joint": 1.0, "uncert": 1.0}     # make_golden_cubehead.py


def rot6d(a):
    b1 = a[:, :3] / np.linalg.norm(a[:, :3], axis=1, keepdims=True)
    u = a[:, 3:] - (b1 * a[:, 3:]).sum(1, keepdims=True) * b1
    b2 = u / np.linalg.norm(u, axis=1, keepdims=True)
    return np.stack((b1, b2, np.cross(b1, b2)), axis=1)


def ray_rotation(u, v, K4):
    """(n,3,3) rotation taking the optical axis to the ray through pixel (u, v) (Rodrigues), identity where the angle is 0"""
    ray = np.stack(((u - K4[:, 2]) / K4[:, 0], (v - K4[:, 3]) / K4[:, 1], np.ones_like(u)), axis=1)
    ray /= np.linalg.norm(ray, axis=1, keepdims=True)
    angle = np.arccos(ray[:, 2])
    M = np.tile(np.eye(3), (len(u), 1, 1))
    for i in np.nonzero(angle > 0)[0]:
        ax = np.array([-ray[i, 1], ray[i, 0], 0.0])
        ax /= np.linalg.norm(ax)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        M[i] = np.eye(3) + np.sin(angle[i]) * Kx + (1 - np.cos(angle[i])) * (Kx @ Kx)
    return M


def corners(c, dims, R):
    """(n,8,3): centre + R @ (+-l/2, +-h/2, +-w/2), dims = (w, h, l)"""
    s = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], dtype=np.float64) * 0.5
    loc = s[None] * dims[:, None, ::-1]
    return np.einsum("nab,nvb->nva", R, loc) + c[:, None, :]


def terms(g, z_type, allocentric=True, inverse_z=False, w_joint=1.0, chamfer_pose=True):
    """g: the fixture (np.load).  -> dict: per-RoI unweighted terms `L` (n,5), residuals of the absolute differences
    (`res_xy`, `res_dims`, `res_z`, `res_joint`), `trace` (n), and `losses` = the six reduced, weighted entries."""
    f = lambda k: np.asarray(g[k], dtype=np.float64)
    cls = np.asarray(g["gt_classes"]).astype(np.int64)
    n = len(cls)
    idx = np.arange(n)
    img = np.repeat(np.arange(len(g["n_per"])), np.asarray(g["n_per"]))
    ratios, Ks = f("ratios"), f("Ks")
    K4 = np.stack([np.array([Ks[b][0, 0], Ks[b][1, 1], Ks[b][0, 2], Ks[b][1, 2]]) / ratios[b] for b in img])
    v2r = np.array([(512.0 * Ks[b][1, 1]) / (512.0 * (512.0 * ratios[b])) for b in img])      # (H0 f) / (f0 H)
    box = f("proposal_boxes")
    sw, sh = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    cx, cy = box[:, 0] + 0.5 * sw, box[:, 1] + 0.5 * sh
    d = f("in_deltas")[idx, cls]
    dr = f("in_dims")[idx, cls]
    Ra = rot6d(f("in_pose6")[idx, cls])
    u = np.maximum(f("in_uncert")[idx, cls], 0.01)
    zin = f("in_z")
    mu = sd = None
    if zin.ndim == 4:                                                      # CLUSTER_BINS > 1: (n, bins, K, 1)
        scales = f("priors_z_scales")[cls]                                 # (n, bins)
        bin_ = np.argmin(np.abs(scales - np.sqrt(sh * sh + sw * sw)[:, None]), axis=1)
        zraw = zin[idx, bin_, cls, 0]
        st = f("priors_z_stats")[cls, bin_]
        mu, sd = st[:, 0], st[:, 1]
    else:
        zraw = zin[idx, cls, 0]
    sig = 1.0 / (1.0 + np.exp(-zraw))
    if z_type == "sigmoid":
        zdec = 100.0 * sig
    elif z_type == "log":
        zdec = np.exp(zraw)
    elif z_type == "clusters":
        mn, mx = np.maximum(mu - 3 * sd, 0.0), mu + 3 * sd
        zdec = mn + (mx - mn) * sig
    else:
        zdec = zraw
    z = zdec * v2r
    gt = f("gt_boxes3D")
    g2, gz, gd, gR = gt[:, :2], gt[:, 2], gt[:, 3:6], f("gt_poses")
    r2v = 1.0 / v2r
    cux, cuy = cx + sw * d[:, 0], cy + sh * d[:, 1]
    dims = np.exp(np.minimum(dr, 5.0))
    res_xy = d - (g2 - np.stack((cx, cy), 1)) / np.stack((sw, sh), 1)
    res_dims = dr - np.log(gd)
    if z_type == "sigmoid":
        res_z = sig - np.clip(gz * r2v / 100.0, 0.0, 1.0)
    elif z_type == "log":
        res_z = zraw - np.log(np.maximum(gz * r2v, 0.01))
    elif z_type == "clusters":
        res_z = zraw - (gz * r2v - mu) / sd
    else:
        res_z = z - gz
    if allocentric:
        M = ray_rotation(cux, cuy, K4)
        R = M @ Ra
        T = np.transpose(M, (0, 2, 1)) @ gR
    else:
        R, T = Ra, gR
    trace = np.einsum("nab,nab->n", Ra, T)
    gc = np.stack((gz * (g2[:, 0] - K4[:, 2]) / K4[:, 0], gz * (g2[:, 1] - K4[:, 3]) / K4[:, 1], gz), 1)
    pc = np.stack((z * (cux - K4[:, 2]) / K4[:, 0], z * (cuy - K4[:, 3]) / K4[:, 1], z), 1)
    res_joint = corners(pc, dims, R) - corners(gc, gd, gR)
    L = np.stack((np.abs(res_dims).mean(1), np.abs(res_xy).mean(1), np.abs(res_z), 1.0 - (trace - 1.0) / 2.0,
                  np.abs(res_joint).reshape(n, -1).mean(1)), 1)
    w = np.sqrt(2.0) * np.exp(-u)
    if inverse_z:
        w = w / np.log(np.maximum(gz, np.e))
    red = (L * w[:, None]).mean(0)
    losses = {"loss_dims": red[0] * WEIGHTS["dims"], "loss_xy": red[1] * WEIGHTS["xy"], "loss_z": red[2] * WEIGHTS["z"],
              "loss_pose": red[3] * WEIGHTS["pose"], "uncert": u.mean() * WEIGHTS["uncert"]}
    if w_joint > 0:
        losses["loss_joint"] = red[4] * w_joint
    return dict(L=L, res_xy=res_xy, res_dims=res_dims, res_z=res_z, res_joint=res_joint, trace=trace, losses=losses)


def check_conditions(t):
    """(a) no absolute-difference residual within 1e-5 of its kink, (b) every trace inside [-1 - 1e-4, 3 + 1e-4]"""
    for k in ("res_xy", "res_dims", "res_z", "res_joint"):
        m = float(np.abs(t[k]).min())
        assert m > 1e-5, "%s: smallest residual %.3g is within 1e-5 of the kink of |.|" % (k, m)
    assert float(t["trace"].min()) >= -1.0 - 1e-4 and float(t["trace"].max()) <= 3.0 + 1e-4, "trace outside [-1, 3]"
