"""GPU: the fused weak-loss kernels (k_weak_fwd, k_weak_zsearch, k_weak_reduce, k_weak_bwd of csrc/weak_loss.hip) through the
product path -- dense_train.weak_cube_losses_fused for the loss dictionary, the logged scalars and the gradient, ops.weak_cube_loss
for dec, pbox, stats and validf -- against the float64 run of the independent reference tests/weak_loss_ref.py.

Tolerance of a compared quantity q of a case: E32(q) = largest deviation of the reference's own float32 CPU run from its float64
run, scale(q) = max |q64|; the kernel must be within max(8 * E32, 32 * 2^-23 * scale), and never beyond the project's 2e-4 * scale.
Nothing is left out of a comparison near a discrete decision: the case builder (tests/weak_loss_cases.py) makes every slot decided.
Selections are compared for equality: validf, the step the depth search picks, the looked-up depth targets."""
import importlib
import os

import pytest
import torch

import weak_loss_cases as cases
import weak_loss_ref as ref
from test_weak_loss_ref import GPU_CASES, built

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
d2 = importlib.import_module("3dod_amd.d2lite")
syn = importlib.import_module("3dod_amd.synthetic")
modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
dense = importlib.import_module("3dod_amd.cubercnn.modeling.dense_train")
ops = importlib.import_module("3dod_amd.hipops")
lib = importlib.import_module("3dod_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("loss_iou", "loss_pose", "loss_normal_vec", "loss_z", "loss_pseudo_gt_z", "loss_dims_w", "loss_dims_h", "loss_dims_l", "uncert")
LOGGED = ("z_error", "dims_error", "xy_error", "z_close", "2D IoU", "conf", "total_3D_loss")
_HEAD = []


def head():
    if not _HEAD:
        cfg = syn.make_cfg(os.path.join(ROOT, "configs", "Omni_combined.yaml"), ["MODEL.DEVICE", "cuda:0", "VIS_PERIOD", 0])
        shapes = {f"p{l}": d2.ShapeSpec(channels=256, stride=2 ** l) for l in range(2, 7)}
        _HEAD.append(modeling.build_roi_heads(cfg, shapes).to(DEV).train())
    return _HEAD[0]


class _Gt:
    def __init__(self, c):
        self.boxes, self.boxes3D, self.poses = c["gt_boxes"].float().to(DEV), c["gt3d"].float().to(DEV), c["gt_poses"].float().to(DEV)


def run_gpu(c):
    """the case through the product path -> dict like the reference's (float32 tensors on the CPU) + the loss dictionary and the
    logged scalars"""
    rh = head()
    w = c["weights"]
    assert rh.num_classes == c["K"] and rh.use_confidence == w["conf"] and rh.pose_type == "6d"
    rh.loss_functions, rh.allocentric_pose = list(c["loss_functions"]), bool(c["allocentric"])
    rh.loss_w_iou, rh.loss_w_pose, rh.loss_w_normal_vec, rh.loss_w_z, rh.loss_w_dims, rh.loss_w_3d = (
        w["iou"], w["pose"], w["normal"], w["z"], w["dims"], w["w3d"])
    rh.virtual_depth, rh.virtual_focal = c["virtual_focal"] is not None, c["virtual_focal"]
    rh.dims_priors_enabled, rh.dims_priors_func = c["prior_mean"] is not None, "exp"
    if c["prior_mean"] is not None:
        rh.priors_dims_per_cat = torch.nn.Parameter(torch.stack((c["prior_mean"], c["prior_std"]), 1)[None].float().to(DEV))
    B, kf = c["B"], c["kf"]
    assert dense.weak_fusable(rh, kf, DEV)
    samp = {"valid": c["valid"].to(DEV), "classes": c["classes"].to(DEV), "gt_idx": c["gt_idx"].to(DEV),
            "boxes": c["boxes"].float().to(DEV), "k_fg": kf}
    depth = d2.ImageList(c["depth"].float().to(DEV), [tuple(s) for s in c["depth_sizes"]])
    ground = d2.ImageList(torch.zeros(B, c["depth"].shape[1], c["depth"].shape[2], dtype=torch.bool, device=DEV),
                          [tuple(s) for s in c["ground_sizes"]])
    seen = []
    orig = ops.weak_cube_loss
    ops.weak_cube_loss = lambda *a, **k: (seen.append(orig(*a, **k)), seen[-1])[1]
    try:
        with d2.EventStorage(0) as st:
            raw = c["raw"].float().to(DEV).requires_grad_(True)
            losses = dense.weak_cube_losses_fused(rh, samp, _Gt(c), None, c["Ks"].tolist(), c["image_sizes"], c["ratios"], ground, depth,
                                                  raw_layout=(raw, c["layout"]), normals=c["normals"].float().to(DEV))
            sum(losses.values()).backward()
            logged = st.latest()
    finally:
        ops.weak_cube_loss = orig
    red, stats, dec, pbox, validf = seen[0]
    n = B * kf
    buf = red.grad_fn.keep[20]                     # what the backward pass keeps: the raw terms and the depth targets per slot
    L, ztgt = buf[:8 * n].view(n, 8), buf[29 * n:30 * n]
    cpu = lambda t: t.detach().cpu()
    return dict(dec=cpu(dec), pbox=cpu(pbox), red=cpu(red), stats=cpu(stats), validf=cpu(validf).bool(), grad=cpu(raw.grad), L=cpu(L),
                ztgt=cpu(ztgt), losses={k: float(v) for k, v in losses.items()}, logged=logged)


def bound(e32, scale):
    return min(max(8.0 * e32, 32.0 * 2.0 ** -23 * scale), 2e-4 * scale)


def dev_of(a64, b):
    """(largest deviation over the entries where the float64 value is a number, scale); the NaN of the truth must be NaN"""
    a, b = a64.double(), b.double()
    ok = torch.isfinite(a)
    if not bool(ok.any()):
        return 0.0, 0.0
    return float((a[ok] - b[ok]).abs().max()), float(a[ok].abs().max())


def quantities(c, o, v):
    """the compared quantities of a run, each on its own scale: the decoded cuboid by kind (valid slots), the projected box, every
    reduced term, every logged statistic, the gradient by head output"""
    K, lay = c["K"], c["layout"]
    dec, g = o["dec"][v], o["grad"]
    q = {"dec.xy": dec[:, 0:2], "dec.z": dec[:, 2], "dec.dims": dec[:, 3:6], "dec.R": dec[:, 6:15], "dec.xyz3d": dec[:, 15:17],
         "pbox": o["pbox"][v]}
    for k, name in enumerate(ref.NAMES + ("uncert",)):
        q["red." + name] = o["red"][k]
    for k, name in enumerate(LOGGED + ("valid",)):
        q["stats." + name] = o["stats"][k]
    for name, e, wd in (("deltas", 0, 2), ("dims", 1, 3), ("pose6", 2, 6), ("z", 3, 1), ("uncert", 4, 1)):
        q["grad." + name] = g[:, lay[e]:lay[e] + K * wd]
    return q


def compare(c, o64, o32, got, label, nan_grad_ok=False):
    """every quantity against float64 under the E32-based bound; figures are printed before they are asserted"""
    v = o64["validf"]
    assert torch.equal(got["validf"], v)
    q64, q32, qk = quantities(c, o64, v), quantities(c, o32, v), quantities(c, got, v)
    fails = []
    for q in q64:
        a64, a32, k = q64[q], q32[q], qk[q]
        if a64.numel() == 0:
            continue
        e32, scale = dev_of(a64, a32)
        err, _ = dev_of(a64, k)
        lim = bound(e32, scale)
        print(f"{label} {q}: scale {scale:.3e} E32 {e32:.3e} kernel {err:.3e} bound {lim:.3e} kernel/E32 {err / e32 if e32 else float('inf'):.2f}")
        nan64 = torch.isnan(a64)
        if q.startswith("grad") and nan_grad_ok:
            assert torch.isfinite(k).all()         # where the reference's own gradient is NaN the kernels send a number
        else:
            assert torch.equal(torch.isnan(k), nan64), (label, q, "NaN pattern")
        if err > lim:
            fails.append((q, err, lim, e32, scale))
    assert not fails, (label, fails)
    # empty slots: a gradient of exactly 0
    assert float(got["grad"][~v].abs().max() if (~v).any() else 0.0) == 0.0
    # selections: the step of the depth search, the depth target that was looked up
    if (c["terms"] & 8) and v.any():
        ok = torch.isfinite(o64["L"][v, 3])
        assert torch.equal(torch.round(got["L"][v, 3][ok].double() * 20), torch.round(o64["L"][v, 3][ok] * 20)), (label, "depth-search step")
    if c["pgz_mode"] and v.any():
        assert torch.equal(got["ztgt"][v], o64["ztgt"][v].float()), (label, "depth targets")
    # the loss dictionary and the logged scalars are the reduced vector, weighted
    wts = ref.term_weights(c["weights"])
    for k, key in enumerate(KEYS):
        on = k == 8 or (c["terms"] >> k) & 1
        assert (("Cube/" + key) in got["losses"]) == bool(on), key
        if on:
            a, b = got["losses"]["Cube/" + key], float(got["red"][k]) * wts[k]
            assert (a != a and b != b) or abs(a - b) <= 1e-6 * max(1.0, abs(b)), (key, a, b)
    for k, key in enumerate(LOGGED):
        a, b = got["logged"]["Cube/" + key], float(got["stats"][k]) * (c["weights"]["w3d"] if k == 6 else 1.0)
        assert (a != a and b != b) or abs(a - b) <= 1e-6 * max(1.0, abs(b)), (key, a, b)


def check(name, **kw):
    c, o64, o32 = built(name)
    got = run_gpu(c)
    compare(c, o64, o32, got, name, **kw)
    return c, o64, got


# ------------------------------------------------------------------------------------------------------------ a. shapes
@pytest.mark.parametrize("tag", ["patch", "center"])
@pytest.mark.parametrize("B,kf,S", cases.SWEEP)
def test_shape_sweep(B, kf, S, tag):
    """all fused terms with both depth targets: one slot; one ragged search workgroup; under, at and over one wave; the training
    shape; n > 256 (strided reduce); under and at the slot limit"""
    check(f"sweep-{B}-{kf}-{S}-{tag}")


# ------------------------------------------------------------------------------------------------------------ b. terms
@pytest.mark.parametrize("pri", [True, False])
@pytest.mark.parametrize("allo", [True, False])
@pytest.mark.parametrize("term", sorted(cases.ISOLATED))
def test_terms_in_isolation(term, allo, pri):
    """each loss of the fused set alone (the three dimension terms come together: one loss function), then the production set;
    allocentric on / off, dimension priors on / off (prior_std given / NULL)"""
    check(f"term-{term}-allo{int(allo)}-pri{int(pri)}")


# ------------------------------------------------------------------------------------------------------------ c. validity
@pytest.mark.parametrize("pattern", sorted(cases.VALIDITY))
def test_validity_patterns(pattern):
    c, o64, got = check(f"valid-{pattern}", nan_grad_ok=pattern == "one_image_empty")
    if pattern == "one_each":                       # no pair anywhere: the reference drops the key, here it is 0 without gradient
        assert got["losses"]["Cube/loss_pose"] == 0.0 and float(got["red"][1]) == 0.0
    if pattern == "none":
        assert float(got["red"].abs().max()) == 0.0 and float(got["grad"].abs().max()) == 0.0
    if pattern == "one_image_empty":                # the pose alignment takes the mean of nothing there: NaN, as in the reference
        assert got["red"][1] != got["red"][1] and o64["red"][1] != o64["red"][1]


def test_image_without_valid_slot_without_the_pose_term():
    """the same pattern with a finite total: every gradient entry is compared"""
    check("valid-one_image_empty-nopose")


# ------------------------------------------------------------------------------------------------------------ d. constructed
@pytest.mark.parametrize("tag", ["patch", "center"])
def test_constructed_slots(tag):
    """windows with and without area interleaved with empty slots (the permuted window-median targets), a failed centre test
    (loss 2.5) with a disjoint box, searches over zero area (the 1e7 rule) and in both directions, the camera inside the cuboid, a proposal sticking out of
    the image, a clipped dimension, an uncertainty under its clip, ground confidence 0.1, a projected box equal to its 2D box.
    (Not built: a dimension exactly one sigma from its prior -- exp() of the raw value times the prior mean cannot land on
    mean + sigma in float32 and in float64 at once, and off the tie the hinge is an ordinary decided slot.)"""
    c, o64, got = check(f"constructed-{tag}")
    kf, K = c["kf"], c["K"]
    v = o64["validf"]
    # the constructions are what they claim to be (float64 reference)
    pb = o64["pbox"]
    assert all(float(pb[j, 0]) == float(pb[j, 2]) == 2 * 96 - 1 for j in (2, 6, 10))                 # every corner on the upper x bound
    if tag == "patch":
        perm = o64["ztgt"][:kf][v[:kf]]
        inside = ((pb[:kf, 2].clamp(0, 128) - pb[:kf, 0].clamp(0, 128)) * (pb[:kf, 3].clamp(0, 96) - pb[:kf, 1].clamp(0, 96)) > 0)[v[:kf]]
        assert not bool(inside[1]) and bool(inside[2:].any()) and not bool(inside.all())  # targets permuted against slots
        assert perm.numel() == inside.numel()
    ga = (c["gt_boxes"][:, :, 2] - c["gt_boxes"][:, :, 0]) * (c["gt_boxes"][:, :, 3] - c["gt_boxes"][:, :, 1])
    img = torch.arange(v.numel()) // kf
    closer = ga[img, c["gt_idx"][:, :kf].reshape(-1)] < (pb[:, 2] - pb[:, 0]) * (pb[:, 3] - pb[:, 1])
    assert bool(closer[v].any()) and not bool(closer[v].all())                                       # the search walks both ways
    assert all(int(o64["zero_area_steps"][j]) > 0 for j in (2, 6, 10))                               # the 1e7 rule is met
    assert float(o64["L"][kf + 1, 3]) == 2.5 and float(o64["L"][kf + 3, 3]) == 2.5                  # centre test failed
    assert float(o64["L"][kf + 1, 0]) > 1.0                                                          # GIoU of disjoint boxes
    assert torch.equal(pb[16], c["gt_boxes"][0, 5]) and abs(float(o64["L"][16, 0])) < 1e-6            # box equal to its 2D box: GIoU loss 0
    assert float(o64["dec"][4, 2]) < 0.1 and float(o64["dec"][12, 3]) > 50                           # camera inside; exp(5) x prior
    cls12 = int(c["classes"][0, 12])
    assert float(got["grad"][12, 2 * K + 3 * cls12]) == 0.0                                          # clipped: no gradient
    cls14 = int(c["classes"][0, 14])
    assert float(got["grad"][14, 12 * K + cls14]) == 0.0 and float(o64["grad"][14, 12 * K + cls14]) == 0.0      # under the clip at 0.01


def test_nan_row_is_dropped_and_leaves_the_others_alone():
    """a NaN depth in one slot: its iou / z / pseudo-depth terms are dropped by the safe reduction, its gradient is finite, the
    per-slot results of every other slot are bit-identical to the run without the NaN, and losses and gradients still agree with
    float64.  (With the depth under the centre as target: the window-median targets of an image are, as in the reference, permuted
    when one of its windows loses its area.)"""
    c, o64, _ = built("sweep-3-65-80-center")
    base = run_gpu(c)
    slot = int(torch.nonzero(o64["validf"])[5])
    c2 = dict(c)
    c2["raw"] = c["raw"].clone()
    c2["raw"][slot, 11 * c["K"] + int(c["classes"][slot // c["kf"], slot % c["kf"]])] = float("nan")
    got = run_gpu(c2)
    n64, n32 = ref.run(c2, torch.float64), ref.run(c2, torch.float32)
    assert torch.isfinite(got["grad"]).all() and torch.isfinite(got["red"]).all()
    others = torch.ones(c["B"] * c["kf"], dtype=torch.bool)
    others[slot] = False
    for q in ("dec", "pbox", "ztgt"):
        assert torch.equal(got[q][others], base[q][others]), q
    assert torch.equal(got["L"][others][:, (0, 2, 3, 4, 5, 6, 7)], base["L"][others][:, (0, 2, 3, 4, 5, 6, 7)])
    v = n64["validf"]
    q64, q32, qk = quantities(c2, n64, v), quantities(c2, n32, v), quantities(c2, got, v)
    for q in q64:
        if not (q.startswith("red") or q.startswith("grad")):
            continue
        a64, a32, k = q64[q], q32[q], qk[q]
        if q.startswith("grad"):                     # the reference's own gradient of the NaN row is NaN
            a64, a32, k = a64[others], a32[others], k[others]
        e32, scale = dev_of(a64, a32)
        err, _ = dev_of(a64, k)
        print(f"nan-row {q}: scale {scale:.3e} E32 {e32:.3e} kernel {err:.3e} bound {bound(e32, scale):.3e}")
        assert torch.isfinite(a64).all() and err <= bound(e32, scale), (q, err, bound(e32, scale))
    assert abs(float(got["red"][0]) - float(base["red"][0])) > 0            # one entry fewer in the means


# ------------------------------------------------------------------------------------------------------------ e. repeats
def test_repeats_are_bit_identical():
    c, _, _ = built("sweep-4-128-512-patch")
    a, b = run_gpu(c), run_gpu(c)
    for q in ("red", "stats", "grad", "dec", "pbox"):
        assert torch.equal(a[q].view(torch.int32), b[q].view(torch.int32)), q


# ------------------------------------------------------------------------------------------------------------ f. limits
def test_slot_limit_of_the_batch_is_accepted():
    """B * kf = 8192 = WR_MAXN: accepted, and the reduced terms agree with float64"""
    c = cases.make_case(32, 256, 256, 7, loss_functions=cases.CENTER)
    o64, o32 = ref.run(c, torch.float64, want_grad=False), ref.run(c, torch.float32, want_grad=False)
    got = run_gpu(c)
    assert torch.equal(got["validf"], o64["validf"])
    for k, name in enumerate(ref.NAMES + ("uncert",)):
        e32, scale = dev_of(o64["red"][k], o32["red"][k])
        err, _ = dev_of(o64["red"][k], got["red"][k])
        print(f"8192 slots red.{name}: scale {scale:.3e} E32 {e32:.3e} kernel {err:.3e} bound {bound(e32, scale):.3e}")
        assert err <= bound(e32, scale), (name, err, bound(e32, scale))


def test_sizes_over_the_limits_are_refused():
    """argument checks on the host: nothing is launched, nothing is returned, outputs stay as they were"""
    c = cases.make_case(2, 64, 64, 3, loss_functions=cases.CENTER, redraw=False)
    big = dict(c)
    big.update(kf=257, valid=torch.ones(2, 257, dtype=torch.bool), classes=torch.zeros(2, 257, dtype=torch.long),
               gt_idx=torch.zeros(2, 257, dtype=torch.long), boxes=torch.zeros(2, 257, 4, dtype=torch.float64),
               raw=torch.zeros(2 * 257, c["raw"].shape[1], dtype=torch.float64))
    rh = head()
    rh.loss_functions = list(c["loss_functions"])
    assert not dense.weak_fusable(rh, 257, DEV)
    t = lambda x: x.to(DEV)
    args = lambda k: (t(k["raw"].float()), k["layout"], k["K"], t(k["classes"]), t(k["valid"]), t(k["gt_idx"]), k["kf"],
                      t(k["gt_boxes"].float()), t(k["gt3d"].float()), t(k["gt_poses"].float()), None, None,
                      torch.tensor([[110.0, 110.0, 64.0, 48.0, 0.2]] * k["classes"].shape[0], device=DEV),
                      torch.zeros(k["classes"].shape[0], 20, device=DEV), None, t(k["boxes"].float()[:, :k["kf"]].reshape(-1, 4)),
                      t(k["depth"].float()[:1].expand(k["classes"].shape[0], -1, -1)), c["terms"] & ~4, 2, (1.0,) * 9)
    with pytest.raises(lib.CrError):
        ops.weak_cube_loss(*args(big))
    with pytest.raises(lib.CrError):                  # 33 x 256 slots: the reduction refuses them, nothing comes back
        run_gpu(cases.make_case(33, 256, 256, 3, loss_functions=cases.CENTER, redraw=False))
    # the C entries called directly: over WK_MAXT slots per image, over WR_MAXN slots per batch
    n = 64
    f = lambda *s: torch.full(s, 7.0, device=DEV)
    import ctypes
    z = torch.zeros(4096, device=DEV)
    ins = ctypes.cast((ctypes.c_void_p * 8)(*[z.data_ptr()] * 8), ctypes.c_void_p)
    vf, cl, gi = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(2, 300, dtype=torch.long, device=DEV)
    outs = [f(n * 8), f(n * 17), f(n * 4), torch.full((n * 4,), 7, dtype=torch.int32, device=DEV), f(4)]
    with pytest.raises(lib.CrError):
        lib.call("cr_weak_loss_fwd", ins, vf, cl, gi, z, None, z, None, 2, 257, 300, 1, 1, 1, outs[0], outs[1], outs[2], outs[3], outs[4])
    rin = ctypes.cast((ctypes.c_void_p * 4)(*[z.data_ptr()] * 4), ctypes.c_void_p)
    wts = (ctypes.c_float * 9)(*[1.0] * 9)
    outs2 = [f(n), f(9), f(9), f(8), f(1)]
    with pytest.raises(lib.CrError):
        lib.call("cr_weak_loss_reduce", rin, vf, z, None, 0, 0, None, z, gi, 33, 256, 300, 1, 1, 0, wts, outs[0], outs[1], outs[2], outs[3],
                 outs[4], outs2[0], outs2[1], outs2[2], outs2[3], outs2[4])
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs + outs2)
