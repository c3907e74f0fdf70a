"""Seconds per Omni3Deval.evaluate() of the host and the device backend (3dod_amd/evalops.py, csrc/eval.hip) on a synthetic
detection set of Omni3D test-split proportions: 2 000 images x 50 categories, ~10 ground truths and 100 detections per image
(random cuboids from the test helpers' generator, fixed seed).  Both backends, 2D and 3D mode, run alternately in one session;
medians of --reps.  Also: the device events around the two launches, and the maximum |difference| between the grouped IoU3D
kernel and cr_box3d_overlap on the same pairs.  Writes profiles/eval_bench.json.

    python scripts/eval_bench.py [--images 2000] [--reps 5] [--out profiles/eval_bench.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import eval_device_helpers as H          # noqa: E402

ev_mod, evalops = H.ev_mod, H.evalops
geo = importlib.import_module("3dod_amd.geometry")


def bench_set(n_img, n_cat=50, seed=0):
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for img in range(n_img):
        objs = []
        for _ in range(int(rng.integers(8, 13))):
            cat = int(rng.integers(0, n_cat))
            z = float(rng.choice([6.0, 20.0, 50.0]))
            c = H.cuboid(rng, (0.0, 0.0, z), 2.0)
            b = [rng.uniform(0, 400), rng.uniform(0, 300), rng.uniform(10, 150), rng.uniform(10, 150)]
            gts.append(H.gt_rec(img, cat, len(gts) + 1, c, b, z, b[2] * b[3], ignore=rng.random() < 0.05))
            objs.append((cat, c, b, z))
        for k in range(100):
            if k < 50:                                   # jittered copies of the image's objects, in their categories
                cat, c, b, z = objs[k % len(objs)]
                c = c + rng.normal(size=3) * 0.1 * (1 + k // len(objs))
                b = [v + rng.normal() * 3 * (1 + k // len(objs)) for v in b]
            else:                                        # false positives in random categories
                cat, z = int(rng.integers(0, n_cat)), float(rng.choice([6.0, 20.0, 50.0]))
                c = H.cuboid(rng, (0.0, 0.0, z), 2.0)
                b = [rng.uniform(0, 400), rng.uniform(0, 300), rng.uniform(10, 150), rng.uniform(10, 150)]
            dts.append(H.dt_rec(img, cat, c, b, z, max(b[2], 0) * max(b[3], 0), rng.random()))
    return gts, dts


def timed(ev):
    torch.cuda.synchronize()
    t = time.perf_counter()
    ev.evaluate()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    args = ap.parse_args()
    gts, dts = bench_set(args.images)
    res = {"images": args.images, "categories": 50, "ground_truths": len(gts), "detections": len(dts), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "rows": {}}
    stats = {}
    for mode in ("2D", "3D"):
        evs = {b: ev_mod.Omni3Deval(gts, dts, mode, backend=b) for b in ("host", "device")}
        timed(evs["device"])                                         # warm-up: context, first launch
        secs, kern = {"host": [], "device": []}, {"iou": [], "match": []}
        for _ in range(args.reps):                                    # alternate the two backends
            for b in ("host", "device"):
                secs[b].append(timed(evs[b]))
                print("%s %-6s %.3f s" % (mode, b, secs[b][-1]), flush=True)
            for k in kern:
                kern[k].append(evs["device"].device_ms[k])
        for b in ("host", "device"):
            stats[mode, b] = evs[b].accumulate().summarize()
            res["rows"]["%s_%s" % (mode, b)] = {"seconds_median": float(np.median(secs[b])), "seconds": secs[b]}
        res["rows"]["%s_device" % mode].update(iou_kernel_ms_median=float(np.median(kern["iou"])),
                                               match_kernel_ms_median=float(np.median(kern["match"])),
                                               speedup_over_host=float(np.median(secs["host"]) / np.median(secs["device"])))
        res["rows"]["%s_device" % mode]["max_abs_stats_diff_to_host"] = float(np.abs(stats[mode, "host"] - stats[mode, "device"]).max())
    # grouped IoU3D against cr_box3d_overlap on the same pairs
    ev = ev_mod.Omni3Deval(gts, dts, "3D", backend="device")
    packed = evalops.pack(ev)
    out = evalops.run(packed, ev.params.areaRng, ev.params.iouThrs, keep_device=True)
    iou = out["iou"].cpu().numpy()
    dev = torch.device("cuda:0")
    dbox, gbox = torch.as_tensor(packed["dt_box3d"], device=dev), torch.as_tensor(packed["gt_box3d"], device=dev)
    worst, n = 0.0, 0
    for g in range(packed["n_groups"]):
        o, o1 = int(packed["iou_off"][g]), int(packed["iou_off"][g + 1])
        if o1 > o:
            d0, d1, g0, g1 = packed["dt_off"][g], packed["dt_off"][g + 1], packed["gt_off"][g], packed["gt_off"][g + 1]
            ref = geo.box3d_overlap(dbox[d0:d1], gbox[g0:g1])[1].cpu().numpy().astype(np.float64).reshape(-1)
            worst, n = max(worst, float(np.abs(ref - iou[o:o1]).max())), n + (o1 - o)
    res["iou3d_grouped_vs_box3d_overlap"] = {"pairs": n, "max_abs_diff": worst, "groups": packed["n_groups"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
