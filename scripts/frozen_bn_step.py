"""Train step time with train-mode BatchNorm (MODEL.USE_BN True, the default) and with frozen BatchNorm (MODEL.USE_BN False:
solver.freeze_bn, running statistics folded into the convolutions, gamma / beta still trained) at the benchmark's train shape:
solver.make_train_step (the step do_train runs, dense region replayed from HIP graphs), DLA34-FPN, 4 x 512^2 per step, fp32.

    python scripts/frozen_bn_step.py [--steps 30] [--warmup 5]

Prints one line per mode and a JSON summary.  Each mode runs in its own child process (fresh allocator and graph pool)."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(use_bn, steps, warmup):
    sys.path.insert(0, ROOT)
    import torch
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    dev = torch.device("cuda:0")
    cfg, model, opt, syn, solver = bt.build(dev, seed=0)
    ims = bt.IMS_PER_GPU
    batches = [syn.make_batch(ims, 1234 + i) for i in range(4)]
    for b in batches:
        for d in b:
            d["image"], d["instances"] = d["image"].to(dev), d["instances"].to(dev)
    step = solver.make_train_step(cfg, model, opt)
    if not use_bn:
        # running statistics of real activations, as a pretrained trunk carries them (one train-mode pass with momentum 1;
        # the init values 0 / 1 would not normalise anything), then frozen where do_train freezes: after the step is built
        bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        for m in bns:
            m.momentum = 1.0
        with torch.no_grad():
            model.backbone(model.preprocess_image(batches[0])[1])
        for m in bns:
            m.momentum = 0.1
        solver.freeze_bn(model)
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
    return {"use_bn": use_bn, "ms_per_step": round(ms, 3), "images_per_s": round(ims * steps / dt, 1),
            "images_per_step": ims, "total_loss": rep["total_loss"], "iterations_explode": rep["iterations_explode"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", choices=["bn", "frozen"])
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child == "bn", a.steps, a.warmup)), flush=True)
        return
    res = {}
    for mode in ("bn", "frozen"):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(a.steps),
                              "--warmup", str(a.warmup)], capture_output=True, text=True, cwd=ROOT)
        line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
        if out.returncode != 0 or not line:
            sys.stderr.write(out.stderr[-3000:])
            sys.exit(f"{mode}: child exited with {out.returncode}")
        r = res[mode] = json.loads(line[-1][7:])
        print(f"MODEL.USE_BN {str(r['use_bn']):5s}  {r['ms_per_step']:8.3f} ms/step  {r['images_per_s']:7.1f} images/s  "
              f"(total_loss {r['total_loss']:.3f})", flush=True)
    res["frozen_over_bn"] = round(res["frozen"]["ms_per_step"] / res["bn"]["ms_per_step"], 4)
    print(json.dumps({"metric": "frozen_bn_step", "precision": os.environ.get("CR_PRECISION", "fp32"), **res}))


if __name__ == "__main__":
    main()
