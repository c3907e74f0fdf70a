"""Train step time with the default (disentangled) losses of the 3D head and with the non-disentangled ones
(MODEL.ROI_CUBE_HEAD.DISENTANGLED_LOSS False, which needs DIMS_PRIORS_ENABLED False: cr_cube_nondis_fwd / _bwd instead of
cr_cube_loss_fwd / _bwd) at the benchmark's train shape: solver.make_train_step (the step do_train runs, dense region replayed
from HIP graphs), DLA34-FPN, 4 x 512^2 per step, fp32.

    python scripts/nondis_step.py [--steps 30] [--warmup 5]

Prints one line per mode and a JSON summary.  Each mode runs in its own child process (fresh allocator and graph pool)."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


NONDIS = ["MODEL.ROI_CUBE_HEAD.DISENTANGLED_LOSS", False, "MODEL.ROI_CUBE_HEAD.DIMS_PRIORS_ENABLED", False]


def child(disentangled, steps, warmup):
    sys.path.insert(0, ROOT)
    import torch
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    dev = torch.device("cuda:0")
    cfg, model, opt, syn, solver = bt.build(dev, seed=0, extra=[] if disentangled else NONDIS)
    ims = bt.IMS_PER_GPU
    batches = [syn.make_batch(ims, 1234 + i) for i in range(4)]
    for b in batches:
        for d in b:
            d["image"], d["instances"] = d["image"].to(dev), d["instances"].to(dev)
    step = solver.make_train_step(cfg, model, opt)
    with d2.EventStorage(0):
        for i in range(warmup):
            step(batches[i % len(batches)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(batches[i % len(batches)])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rep = step.report()
    ms = 1e3 * dt / steps
    return {"disentangled_loss": disentangled, "ms_per_step": round(ms, 3), "images_per_s": round(ims * steps / dt, 1),
            "images_per_step": ims, "total_loss": rep["total_loss"], "iterations_explode": rep["iterations_explode"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", choices=["default", "nondis"])
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child == "default", a.steps, a.warmup)), flush=True)
        return
    res = {}
    for mode in ("default", "nondis"):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(a.steps),
                              "--warmup", str(a.warmup)], capture_output=True, text=True, cwd=ROOT, timeout=600)
        line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
        if out.returncode != 0 or not line:
            sys.stderr.write(out.stderr[-3000:])
            sys.exit(f"{mode}: child exited with {out.returncode}")
        r = res[mode] = json.loads(line[-1][7:])
        print(f"DISENTANGLED_LOSS {str(r['disentangled_loss']):5s}  {r['ms_per_step']:8.3f} ms/step  {r['images_per_s']:7.1f} images/s  "
              f"(total_loss {r['total_loss']:.3f})", flush=True)
    res["nondis_over_default"] = round(res["nondis"]["ms_per_step"] / res["default"]["ms_per_step"], 4)
    print(json.dumps({"metric": "nondis_step", "precision": os.environ.get("CR_PRECISION", "fp32"), **res}))


if __name__ == "__main__":
    main()
