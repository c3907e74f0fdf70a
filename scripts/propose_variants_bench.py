"""BoxNet on GT boxes with each of the six ablation proposal samplers ('random', 'xy', 'z', 'dim', 'aspect', 'rotation') at the
boxnet workload's size (64 images x 16 objects x 1000 cubes, as `bench.py --workload boxnet`), timed through two routes:

  batched     ProposalNetwork.proposals.propose_variant_batched -> cr_propose_sampler_batched, one launch for the batch (the
              route ROIHeads_Boxer._forward_cube takes)
  per_image   the per-image loop over ROIHeads_Boxer.predict_cubes and the host samplers that _forward_cube ran before, which
              this script puts in the proposal stage's place itself

The two alternate in one session; medians of the synchronised wall time per batch go to profiles/propose_variants_bench.json.

    python scripts/propose_variants_bench.py [--reps 7] [--out profiles/propose_variants_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
syn = importlib.import_module("3dod_amd.synthetic")
modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
PN = importlib.import_module("3dod_amd.ProposalNetwork.proposals.proposals")
d2 = importlib.import_module("3dod_amd.d2lite")
NAMES = ["random", "xy", "z", "dim", "aspect", "rotation"]


def make_workload(dev, B=64, n_obj=16):
    """the model and batch of bench.py's boxnet workload"""
    cfg = syn.make_cfg(os.path.join(ROOT, "configs", "BoxNet.yaml"), ["MODEL.DEVICE", str(dev), "VIS_PERIOD", 0, "log", False])
    torch.manual_seed(0)
    model = modeling.build_model(cfg).eval()
    batch = syn.make_batch(B, 777, min_obj=n_obj, max_obj=n_obj)
    g = torch.Generator().manual_seed(2)
    yy, xx = torch.arange(512)[:, None], torch.arange(512)[None, :]
    for b in batch:
        b["image"] = b["image"].to(dev)
        b["instances"] = b["instances"].to(dev)
        b["depth_map"] = (torch.rand(512, 512, generator=g) * 3 + 1).to(dev)
        b["ground_map"] = (yy > 300).expand(512, 512).to(torch.uint8).to(dev)
        boxes = b["instances"].gt_boxes.tensor.round().long().clamp(0, 511).cpu()
        m = torch.zeros(len(boxes), 512, 512, dtype=torch.bool)
        for j, bb in enumerate(boxes):                     # an ellipse inscribed in the box: a non-trivial hull
            cx, cy, rx, ry = (bb[0] + bb[2]) / 2, (bb[1] + bb[3]) / 2, (bb[2] - bb[0]) / 2 + 0.5, (bb[3] - bb[1]) / 2 + 0.5
            m[j] = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1
        b["masks"] = m.to(dev)
    return model, batch


def per_image_route(roi_heads, counts):
    """the proposal stage as a loop over images through predict_cubes and the host samplers, with propose_variant_batched's
    signature"""
    def route(name, boxes, img_idx, depth_images, priors, K, im_shape, number_of_proposals, generator=None, defer_check=False):
        parts, o = [], 0
        for i, n in enumerate(counts):
            if n:
                c, _, _, _ = roi_heads.predict_cubes(d2.Boxes(boxes[o:o + n]), (priors[0][o:o + n], priors[1][o:o + n]),
                                                     depth_images[i], im_shape, K[i], name, None, generator=generator)
                parts.append(c.tensor.to(boxes.device))
            o += n
        cubes = torch.cat(parts).contiguous()
        return cubes, torch.zeros((1,), dtype=torch.int32, device=boxes.device)
    return route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propose_variants_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model, batch = make_workload(dev)
    counts = [len(b["instances"]) for b in batch]
    gen = torch.Generator(device=dev).manual_seed(3)
    batched = PN.propose_variant_batched
    routes = {"batched": batched, "per_image": per_image_route(model.roi_heads, counts)}

    def run(name, route):
        PN.propose_variant_batched = routes[route]
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.inference(batch, experiment_type={"use_pred_boxes": False}, generator=gen, proposal_function=name)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            PN.propose_variant_batched = batched
        assert len(out) == len(batch) and all(len(o["instances"]) == n for o, n in zip(out, counts))
        return dt * 1e3

    res = {}
    with torch.no_grad():
        for name in NAMES:
            for _ in range(args.warmup):
                for route in routes:
                    run(name, route)
            times = {route: [] for route in routes}
            for _ in range(args.reps):                     # the two routes alternate
                for route in routes:
                    times[route].append(run(name, route))
            med = {route: statistics.median(t) for route, t in times.items()}
            res[name] = {"batched_ms": round(med["batched"], 3), "per_image_ms": round(med["per_image"], 3),
                         "batched_images_per_s": round(len(batch) / med["batched"] * 1e3, 1),
                         "per_image_images_per_s": round(len(batch) / med["per_image"] * 1e3, 1),
                         "speedup": round(med["per_image"] / med["batched"], 2),
                         "batched_ms_all": [round(t, 3) for t in times["batched"]],
                         "per_image_ms_all": [round(t, 3) for t in times["per_image"]]}
            print(name, {k: v for k, v in res[name].items() if not k.endswith("_all")}, flush=True)
    doc = {"what": "BoxNet.inference(use_pred_boxes=False, proposal_function=<sampler>), synchronised wall time per batch, median "
                   f"of {args.reps} after {args.warmup} warm-up runs per route, the two routes alternating in one session",
           "workload": f"{len(batch)} images x {counts[0]} objects x {model.roi_heads.number_of_proposals} cubes, 512 x 512 depth, "
                       "ground and object masks resident on the device",
           "routes": {"batched": "propose_variant_batched -> cr_propose_sampler_batched (one launch for the batch)",
                      "per_image": "loop over images through ROIHeads_Boxer.predict_cubes and the host samplers"},
           "device": torch.cuda.get_device_name(0), "samplers": res}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
