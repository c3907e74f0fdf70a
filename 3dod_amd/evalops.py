"""Device backend of the AP2D / AP3D evaluator (cubercnn/evaluation/omni3d_evaluation.py, Omni3Deval(backend="device")):
every IoU of a dataset in one launch (cr_eval_iou_groups), every greedy match in one launch (cr_eval_match_groups).

Three separable steps, so that each can be tested on its own:
  pack(ev)            records -> NumPy arrays (no GPU): the group table, detections in stable descending score order cut to
                      maxDets[-1], boxes, range values, ignore flags, scores, ground-truth ids
  run(packed, ...)    one host -> device copy, the two launches, one device -> host copy
  unpack(ev, ...)     the kernels' outputs -> ev.evalImgs in the layout of Omni3Deval._evaluate_img (no GPU)

A group is one (image, category) pair with at least one detection or ground-truth box; groups are ordered category-major in
the order of params.catIds / params.imgIds.  Output layout of group g with D detections and G ground truths (T thresholds,
4 ranges), as csrc/eval.hip writes it:
  match     int32  [4][T][D] at 4 T dt_off[g]      ground-truth index within the group (original order) or -1
  dt_ignore uint8  [4][T][D] at 4 T dt_off[g]
  gt_ignore uint8  [4][G]    at 4 gt_off[g]        original ground-truth order
  nonfinite int32  [n_groups]                      the group has a NaN / infinite IoU: it is evaluated by the host route
"""
import numpy as np

from . import _lib

N_RANGES = 4          # one wave of a 256-thread workgroup per range


def _records(table, img_rank, cat_rank):
    """(records, group key) of every record of the selected images / categories, in the order the evaluator stored them"""
    recs, keys, n_img = [], [], len(img_rank)
    for (img, cat), lst in table.items():
        if lst and img in img_rank and cat in cat_rank:
            recs.extend(lst)
            keys.extend([cat_rank[cat] * n_img + img_rank[img]] * len(lst))
    return recs, np.asarray(keys, dtype=np.int64)


def pack(ev):
    """Omni3Deval -> dict of NumPy arrays.  Honours params.imgIds / catIds / maxDets[-1] like Omni3Deval.evaluate()."""
    p = ev.params
    mode3d = ev.mode == "3D"
    f_rng, f_ign = ("depth", "ignore3D") if mode3d else ("area", "ignore2D")
    img_ids, cat_ids = list(p.imgIds), list(p.catIds)
    img_rank, cat_rank = {v: i for i, v in enumerate(img_ids)}, {v: i for i, v in enumerate(cat_ids)}
    g_recs, g_key = _records(ev._gts, img_rank, cat_rank)
    d_recs, d_key = _records(ev._dts, img_rank, cat_rank)
    # ground truth: grouped, original order inside a group
    g_order = np.argsort(g_key, kind="stable")
    g_key = g_key[g_order]
    g_recs = [g_recs[i] for i in g_order]
    # detections: one lexsort = per group a stable descending sort by score (the host's mergesort argsort of -score), then the cut
    score = np.asarray([d["score"] for d in d_recs], dtype=np.float64)
    d_order = np.lexsort((np.arange(len(d_recs)), -score, d_key))
    d_key = d_key[d_order]
    first = np.searchsorted(d_key, d_key, side="left")                 # start of each detection's group
    keep = (np.arange(len(d_key)) - first) < int(p.maxDets[-1])
    d_order, d_key = d_order[keep], d_key[keep]
    d_recs = [d_recs[i] for i in d_order]
    score = score[d_order]

    groups = np.union1d(g_key, d_key)
    n_groups = len(groups)
    dt_off = np.searchsorted(d_key, np.append(groups, np.iinfo(np.int64).max), side="left").astype(np.int32)
    gt_off = np.searchsorted(g_key, np.append(groups, np.iinfo(np.int64).max), side="left").astype(np.int32)
    iou_off = np.zeros(n_groups + 1, dtype=np.int64)
    np.cumsum(np.diff(dt_off).astype(np.int64) * np.diff(gt_off).astype(np.int64), out=iou_off[1:])
    if 4 * len(p.iouThrs) * max(len(d_recs), len(g_recs)) >= 2 ** 31:
        raise ValueError("too many detections / ground truths for one evaluation launch")

    f64 = lambda recs, key, shape: np.asarray([r[key] for r in recs], dtype=np.float64).reshape(shape)
    out = {
        "mode": ev.mode, "n_groups": n_groups, "n_img": len(img_ids),
        "grp_cat": [cat_ids[k] for k in (groups // max(len(img_ids), 1)).tolist()],
        "grp_img": [img_ids[k] for k in (groups % max(len(img_ids), 1)).tolist()],
        "dt_off": dt_off, "gt_off": gt_off, "iou_off": iou_off,
        "dt_score": score, "dt_val": f64(d_recs, f_rng, (-1,)), "gt_val": f64(g_recs, f_rng, (-1,)),
        "gt_flag": np.asarray([bool(g.get(f_ign, 0)) for g in g_recs], dtype=np.uint8),
        "gt_id": np.asarray([g["id"] for g in g_recs], dtype=np.float64),
        "dt_bbox": None, "gt_bbox": None, "dt_box3d": None, "gt_box3d": None,
    }
    if not mode3d or ev.eval_prox:
        out["dt_bbox"], out["gt_bbox"] = f64(d_recs, "bbox", (-1, 4)), f64(g_recs, "bbox", (-1, 4))
    if mode3d:
        out["dt_box3d"] = np.asarray([d["bbox3D"] for d in d_recs], dtype=np.float32).reshape(-1, 8, 3)
        out["gt_box3d"] = np.asarray([g["bbox3D"] for g in g_recs], dtype=np.float32).reshape(-1, 8, 3)
    return out


# ------------------------------------------------------------------------------------------------------------ the two launches
def eval_iou_groups(mode3d, dt_off, gt_off, iou_off, n_pairs, dt_bbox, gt_bbox, dt_box3d, gt_box3d, prox_thresh, eval_prox):
    """device tensors in, (iou f64 (n_pairs), prox uint8 (n_pairs) or None, nonfinite int32 (n_groups)) out; no sync"""
    import torch
    if not dt_off.is_cuda:
        raise _lib.CrError("eval_iou_groups: expected CUDA(HIP) tensors; 3dod_amd has no CPU path")
    dev, n_groups = dt_off.device, dt_off.numel() - 1
    iou = torch.empty(n_pairs, dtype=torch.float64, device=dev)
    prox = torch.empty(n_pairs, dtype=torch.uint8, device=dev) if eval_prox else None
    nonfinite = torch.empty(n_groups, dtype=torch.int32, device=dev)
    _lib.call("cr_eval_iou_groups", int(bool(mode3d)), n_groups, dt_off, gt_off, iou_off, n_pairs, dt_bbox, gt_bbox, dt_box3d,
              gt_box3d, float(prox_thresh), iou, prox, nonfinite)
    return iou, prox, nonfinite


def eval_match_groups(dt_off, gt_off, iou_off, iou, prox, dt_val, gt_val, gt_flag, rng, thrs, match, dt_ignore, gt_ignore):
    """device tensors in; writes match / dt_ignore / gt_ignore (caller-owned, see the module docstring) and returns gt_match
    int32 [4][T][G] per group at 4 T gt_off[g] (the detection matched to each ground truth, or -1); no sync"""
    import torch
    if not dt_off.is_cuda:
        raise _lib.CrError("eval_match_groups: expected CUDA(HIP) tensors; 3dod_amd has no CPU path")
    n_groups, T = dt_off.numel() - 1, thrs.numel()
    assert rng.numel() == 2 * N_RANGES and rng.dtype == torch.float64 and thrs.dtype == torch.float64
    assert match.numel() == N_RANGES * T * dt_val.numel() == dt_ignore.numel() and gt_ignore.numel() == N_RANGES * gt_val.numel()
    gt_match = torch.empty(N_RANGES * T * gt_val.numel(), dtype=torch.int32, device=dt_off.device)
    _lib.call("cr_eval_match_groups", n_groups, dt_off, gt_off, iou_off, iou, prox, dt_val, gt_val, gt_flag, rng, thrs, T,
              match, dt_ignore, gt_ignore, gt_match)
    return gt_match


def _align(n, a=16):
    return (n + a - 1) // a * a


def run(packed, area_rng, iou_thrs, eval_prox=False, prox_thresh=0.3, device="cuda:0", keep_device=False):
    """one host -> device copy of the packed arrays, the two launches, one device -> host copy.  Returns the outputs as NumPy
    arrays (module docstring) plus "iou_ms" / "match_ms" (device events around each launch); keep_device=True also returns
    the device tensors "iou", "prox" and "gt_match"."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.CrError(f"evalops.run: the evaluation kernels run on the GPU only (got device '{dev}'); there is no CPU path")
    area_rng = np.asarray(area_rng, dtype=np.float64).reshape(-1)
    if area_rng.size != 2 * N_RANGES:
        raise ValueError("the device backend evaluates exactly %d ranges" % N_RANGES)
    n_groups, mode3d = packed["n_groups"], packed["mode"] == "3D"
    ND, NG, T = len(packed["dt_val"]), len(packed["gt_val"]), len(iou_thrs)
    host = {"dt_off": packed["dt_off"], "gt_off": packed["gt_off"], "iou_off": packed["iou_off"], "dt_val": packed["dt_val"],
            "gt_val": packed["gt_val"], "gt_flag": packed["gt_flag"], "rng": area_rng,
            "thrs": np.asarray(iou_thrs, dtype=np.float64)}
    for k in ("dt_bbox", "gt_bbox", "dt_box3d", "gt_box3d"):
        if packed[k] is not None:
            host[k] = packed[k]
    # ---- one staging buffer, one copy
    offs, total = {}, 0
    for k, a in host.items():
        offs[k] = total
        total = _align(total + a.nbytes)
    stage = np.zeros(max(total, 16), dtype=np.uint8)
    for k, a in host.items():
        stage[offs[k]:offs[k] + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    dbuf = torch.from_numpy(stage).to(dev)
    tdt = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.float64): torch.float64,
           np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8}
    d = {k: dbuf[offs[k]:offs[k] + a.nbytes].view(tdt[a.dtype]) for k, a in host.items()}
    # ---- one output buffer: match | dt_ignore | gt_ignore | nonfinite
    n_m = N_RANGES * T * ND
    o_di, o_gi = 4 * n_m, _align(4 * n_m + n_m)
    o_nf = _align(o_gi + N_RANGES * NG)
    obuf = torch.empty(o_nf + 4 * n_groups, dtype=torch.uint8, device=dev)
    match, dt_ignore = obuf[:4 * n_m].view(torch.int32), obuf[o_di:o_di + n_m]
    gt_ignore = obuf[o_gi:o_gi + N_RANGES * NG]
    ev0, ev1, ev2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    ev0.record()
    iou, prox, nonfinite = eval_iou_groups(mode3d, d["dt_off"], d["gt_off"], d["iou_off"], int(packed["iou_off"][-1]),
                                           d.get("dt_bbox"), d.get("gt_bbox"), d.get("dt_box3d"), d.get("gt_box3d"),
                                           prox_thresh, eval_prox)
    ev1.record()
    gt_match = eval_match_groups(d["dt_off"], d["gt_off"], d["iou_off"], iou, prox, d["dt_val"], d["gt_val"], d["gt_flag"],
                                 d["rng"], d["thrs"], match, dt_ignore, gt_ignore)
    ev2.record()
    obuf[o_nf:].view(torch.int32).copy_(nonfinite)
    h = obuf.cpu().numpy()                                              # the one device -> host copy (synchronises)
    out = {"match": h[:4 * n_m].view(np.int32), "dt_ignore": h[o_di:o_di + n_m], "gt_ignore": h[o_gi:o_gi + N_RANGES * NG],
           "nonfinite": h[o_nf:].view(np.int32), "iou_ms": ev0.elapsed_time(ev1), "match_ms": ev1.elapsed_time(ev2)}
    if keep_device:
        out.update(iou=iou, prox=prox, gt_match=gt_match)
    return out


# ------------------------------------------------------------------------------------------------------------ back to evalImgs
def unpack(ev, packed, out):
    """fills ev.evalImgs[cat, a, img] from the kernels' outputs with the dict layout and dtypes of Omni3Deval._evaluate_img:
    dtMatches float64 (T,D) holding ground-truth ids (0 = unmatched), dtIgnore bool (T,D), gtIgnore int64 (G) ignored last,
    dtScores (D).  (category, image) pairs without detections and ground truth get None.  Groups whose nonfinite flag is set
    go through the host's _ious / _evaluate_img: NaN comparisons of the sequential scan depend on its order."""
    p = ev.params
    T, n_groups = len(p.iouThrs), packed["n_groups"]
    dt_off, gt_off = packed["dt_off"].astype(np.int64), packed["gt_off"].astype(np.int64)
    Dg, Gg = np.diff(dt_off), np.diff(gt_off)
    ev.evalImgs = {(cat, a, img): None for cat in p.catIds for a in range(N_RANGES) for img in p.imgIds}
    # ground-truth ids of the matches, for every group at once
    match = out["match"].astype(np.int64)
    base = np.repeat(gt_off[:-1], N_RANGES * T * Dg)
    gt_id = np.append(packed["gt_id"], 0.0)                              # index -1 (unmatched) reads the appended 0
    dtm = gt_id[np.where(match >= 0, base + match, -1)]
    dti = out["dt_ignore"].astype(bool)
    # gtIgnore: a stable sort by the flag inside every (group, range) segment = the segment's flags, sorted
    seg = np.repeat(np.arange(N_RANGES * n_groups), np.repeat(Gg, N_RANGES))
    gti = out["gt_ignore"].astype(np.int64)
    gti = gti[np.lexsort((gti, seg))]
    scores = packed["dt_score"]
    flagged = out["nonfinite"] != 0
    for g in range(n_groups):
        cat, img = packed["grp_cat"][g], packed["grp_img"][g]
        if flagged[g]:
            dt_sorted, ious, prox = ev._ious(img, cat)
            for a, rng in enumerate(p.areaRng):
                ev.evalImgs[cat, a, img] = ev._evaluate_img(img, cat, rng, p.maxDets[-1], dt_sorted, ious, prox)
            continue
        D, G, d0, g0 = int(Dg[g]), int(Gg[g]), int(dt_off[g]), int(gt_off[g])
        m = dtm[N_RANGES * T * d0:N_RANGES * T * (d0 + D)].reshape(N_RANGES, T, D)
        i = dti[N_RANGES * T * d0:N_RANGES * T * (d0 + D)].reshape(N_RANGES, T, D)
        gi = gti[N_RANGES * g0:N_RANGES * (g0 + G)].reshape(N_RANGES, G)
        s = scores[d0:d0 + D]
        for a in range(N_RANGES):
            ev.evalImgs[cat, a, img] = {"dtMatches": m[a], "dtIgnore": i[a], "gtIgnore": gi[a], "dtScores": s}
    return ev
