"""Depth-Anything-V2 fine-tuning step on one MI355X: forward + backward + AdamW update (tools/train_depth.py's train_step:
SiLog loss, FlatAdam with the encoder / head groups) for vits and vitl at batch 2, 518 x 518, beside the inference forward of
the same shape (eval mode, no_grad: the path this repository had before training existed, unchanged by it).  vitl has the
reference's head; vits runs with a power-of-two head (features 64, out_channels 64 / 128 / 256 / 256) because the 3x3
convolution kernel takes power-of-two input widths only and the reference's vits head has 48 / 96 / 192 / 384.

One session, warm shapes, device events around a window of iterations after `--warmup`, ROUNDS rounds per figure; a window is
`--steps` iterations or as many more as it takes to last `--min-window-ms` (a first window of `--steps` sets the count), so
that the short vits forward is not timed over a few milliseconds.  The mean of the rounds and the spread between them are recorded, and the ratio train step / inference forward.  By FLOPs a backward
pass is twice the forward, so the ratio of a step to a forward is about 3 before the update and the unfused training
forward are counted.  The figures are recorded, not gated.

    python scripts/depth_train_step.py [--steps 10] [--min-window-ms 500] [--warmup 3] [--encoders vits vitl]
                                       [--out profiles/depth_train_step.json]
"""
import argparse
import importlib
import json
import math
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROUNDS = 3
BATCH, SIZE = 2, 518
HEADS = {"vits": {"features": 64, "out_channels": [64, 128, 256, 256]}}      # see the docstring


def window(fn, steps, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, steps, warmup, torch, min_window_ms):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    steps = max(steps, math.ceil(min_window_ms / (window(fn, steps, torch) / steps)))      # the first window only sets the count
    ms = [round(window(fn, steps, torch) / steps, 3) for _ in range(ROUNDS)]
    return {"ms": round(sum(ms) / len(ms), 3), "rounds_ms": ms, "spread_ms": round(max(ms) - min(ms), 3), "steps_per_window": steps,
            "window_ms": round(steps * sum(ms) / len(ms), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--min-window-ms", type=float, default=500.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--encoders", nargs="+", default=["vits", "vitl"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_train_step.json"))
    a = ap.parse_args()
    import torch
    tool = importlib.import_module("train_depth")
    dav2 = importlib.import_module("3dod_amd.depth_anything_v2")
    solver = importlib.import_module("3dod_amd.cubercnn.solver.build")
    ops = importlib.import_module("3dod_amd.hipops")
    dev = torch.device("cuda:0")
    res = {"metric": "depth_train_step", "device": torch.cuda.get_device_name(0), "batch": BATCH, "image_size": SIZE,
           "steps": a.steps, "min_window_ms": a.min_window_ms, "warmup": a.warmup, "rounds": ROUNDS,
           "timing": "device events around windows of back-to-back iterations, eager launches; no rocprofv3 run was made"}
    g = torch.Generator().manual_seed(0)
    img = torch.randn(BATCH, 3, SIZE, SIZE, generator=g).to(dev)
    depth = (torch.rand(BATCH, SIZE, SIZE, generator=g) * 15 + 1).to(dev)
    valid = (torch.rand(BATCH, SIZE, SIZE, generator=g) < 0.8).to(dev)
    for enc in a.encoders:
        torch.manual_seed(0)
        cfg = {**tool.MODEL_CONFIGS[enc], **HEADS.get(enc, {}), "max_depth": 20.0}
        model = dav2.DepthAnythingV2(**cfg).to(dev)
        e, h = tool.split_groups(model.named_parameters(), dav2.DepthAnythingV2.UNUSED_PARAMETERS)
        opt = solver.FlatAdam([(p, 5e-6, tool.WEIGHT_DECAY) for p in e] + [(p, 5e-5, tool.WEIGHT_DECAY) for p in h],
                              eps=tool.EPS, betas=tool.BETAS, decoupled=True)
        ops.bump_weight_epoch()
        st = types.SimpleNamespace(args=types.SimpleNamespace(min_depth=0.001, max_depth=20.0, lr=5e-6), model=model, opt=opt,
                                   ops=ops, total_iters=10 ** 6)
        model.eval()
        with torch.no_grad():
            fwd = timed(lambda: model(img), a.steps, a.warmup, torch, a.min_window_ms)
        it = [0]

        def step():
            it[0] += 1
            return tool.train_step(st, img, depth, valid, it[0])
        trn = timed(step, a.steps, a.warmup, torch, a.min_window_ms)
        loss = float(step())
        r = {"config": cfg, "inference_forward": fwd, "train_step": trn, "ratio_step_to_forward": round(trn["ms"] / fwd["ms"], 2),
             "images_per_s_training": round(BATCH / (trn["ms"] * 1e-3), 1), "loss_after": loss,
             "peak_memory_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
        res[enc] = r
        print(enc, json.dumps(r), flush=True)
        del model, opt, st
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
