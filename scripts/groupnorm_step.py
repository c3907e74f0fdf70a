"""GroupNorm (configs/cubercnn_DLA34_FPN_GN.yaml: FPN norm "GN", 4conv1fc GN box head) on one MI355X, fp32, 4 x 512^2 per step,
one session, device events, warm shapes:

  * per GroupNorm call at the four FPN shapes (4 x {128, 64, 32, 16}^2 x 256) and at the RoI tiles (2048 x 7 x 7 x 256), forward
    (with ReLU for the tiles, as the box head runs it), forward from a convolution's statistics rows, and backward:
    cr_groupnorm_fwd / cr_groupnorm_bwd.  Each form is captured as one HIP graph of GN_CALLS back-to-back calls, so a replay is
    kernel time without the host's launch rate; REPEATS rounds; per shape the mean of the rounds and the spread between them.
    torch's F.group_norm is not timed beside it (recorded as "not measured").  Beside the time:
    the bytes the algorithm needs (forward: the map read twice and written once, or read once and written once from the
    convolution's statistics rows; backward: dy and x read twice each, dx written once; with ReLU the stored output is read
    twice more) and their share of the 6.29 TB/s measured HBM copy rate.  Every call works on the same buffers and every map
    here fits the 256 MB last-level cache: warm-cache rates, not HBM rates;
  * the train step (solver.make_train_step, dense region replayed from HIP graphs), ms per step and images/s, each timing in a
    child process of its own: the default config at this tree and, with --parent-root, at a checkout of the parent commit, in
    alternation, with the spread of either side against itself; then the GN config.  The 3x3 256 -> 256 convolutions of the GN
    box head over 2048 x 7 x 7 tiles are counted from their shapes.

    python scripts/groupnorm_step.py [--steps 20] [--warmup 5] [--parent-root DIR] [--out profiles/groupnorm_step_fp32.json]

The figures are recorded, not gated."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS = 5
GN_CALLS = 10
STEP_ROUNDS = 4
HBM_COPY_TBS = 6.29
GN_SHAPES = [(4, 128, 128, 256), (4, 64, 64, 256), (4, 32, 32, 256), (4, 16, 16, 256), (2048, 7, 7, 256)]


def step_only(root, config, steps, warmup):
    """one timing of the train step in this process, the tree at `root` -> a JSON line"""
    sys.path.insert(0, root)
    import torch
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    dev = torch.device("cuda:0")
    cfg, model, opt, syn, solver = bt.build(dev, seed=0, config=config or None)
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
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(steps):
            step(batches[i % len(batches)])
        e1.record()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rep = step.report()
    print("STEP " + json.dumps({"config": config or "Base_Omni3D.yaml (DLA34)", "ms_per_step": round(e0.elapsed_time(e1) / steps, 3),
                                "wall_ms_per_step": round(1e3 * dt / steps, 3), "images_per_s": round(ims * steps / dt, 1),
                                "steps": steps, "launch_mode": os.environ.get("CR_GRAPHS", "dense"),
                                "total_loss": rep["total_loss"], "iterations_explode": rep["iterations_explode"]}))


def child_step(root, config, steps, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--step-only", "--root", root, "--config", config or "", "--steps", str(steps),
           "--warmup", str(warmup)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    lines = [l for l in out.stdout.splitlines() if l.startswith("STEP ")]
    if out.returncode != 0 or not lines:
        raise RuntimeError("step timing failed in %s: %s" % (root, out.stderr[-1500:]))
    return json.loads(lines[-1][5:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit, timed in alternation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupnorm_step_fp32.json"))
    ap.add_argument("--no-steps", action="store_true", help="the per-call figures only")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--config", default="")
    a = ap.parse_args()
    if a.step_only:
        return step_only(a.root, a.config, a.steps, a.warmup)
    sys.path.insert(0, ROOT)
    import torch
    rs = importlib.import_module("resnet50_step")             # time_gpu / capture
    ops = importlib.import_module("3dod_amd.hipops")
    dev = torch.device("cuda:0")
    assert ops.precision() == "fp32"
    res = {"metric": "groupnorm_step", "precision": "fp32", "config": "cubercnn_DLA34_FPN_GN.yaml",
           "device": torch.cuda.get_device_name(0), "images_per_step": 4, "image_size": 512, "repeats": REPEATS,
           "timing": "device events around HIP-graph replays of %d calls; no rocprofv3 run was made" % GN_CALLS,
           "hbm_copy_TBs": HBM_COPY_TBS}

    # ---- per GroupNorm call: each form captured as one HIP graph of GN_CALLS back-to-back calls, REPEATS rounds
    def rounds(fn):
        replay, err = rs.capture(lambda: [fn() for _ in range(GN_CALLS)])
        run, per = (replay, GN_CALLS) if replay is not None else (fn, 1)
        rs.time_gpu(run, 20)
        us = [round(1e3 * rs.time_gpu(run, 20) / per, 2) for _ in range(REPEATS)]
        return {"us": round(sum(us) / len(us), 2), "rounds_us": us, "spread_us": round(max(us) - min(us), 2),
                "replayed_from_graph": replay is not None, "graph_error": err}

    calls = []
    for shape in GN_SHAPES:
        N, H, W, C = shape
        relu = H == 7                                       # the box head's norm is followed by ReLU, the FPN's is not
        g = torch.Generator(device="cpu").manual_seed(C + H)
        x = (torch.randn(shape, generator=g) + 0.5).to(dev)
        dy = torch.randn(shape, generator=g).to(dev)
        gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
        rows = None
        if H * W % 128 == 0:                                # what the convolution's epilogue would have written
            xr = x.view(N * H * W // 64, 64, C)
            rows = torch.stack([xr.sum(1), (xr * xr).sum(1)], 1).contiguous()
        y, mr = ops.group_norm_fwd_raw(x, gamma, beta, 32, 1e-5, relu)
        acc = [torch.zeros(C, device=dev), torch.zeros(C, device=dev)]
        map_mb = N * H * W * C * 4 / 1e6
        moved = {"forward": 3, "forward_from_rows": 2, "backward": 5 + (2 if relu else 0)}
        r = {"shape": list(shape), "relu": relu, "map_MB": round(map_mb, 2), "maps_moved": moved,
             "small_regime_one_launch": H * W <= 64}
        with torch.no_grad():
            r["forward"] = rounds(lambda: ops.group_norm_fwd_raw(x, gamma, beta, 32, 1e-5, relu))
            if rows is not None:
                r["forward_from_rows"] = rounds(lambda: ops.group_norm_fwd_raw(x, gamma, beta, 32, 1e-5, relu, stat_rows=rows))
            r["backward"] = rounds(lambda: ops.group_norm_bwd_raw(dy, x, y, mr, gamma, 32, relu, *acc))
        for k in ("forward", "forward_from_rows", "backward"):
            if k in r:
                gbs = moved[k] * map_mb * 1e6 / (r[k]["us"] * 1e-6) / 1e9
                r[k]["needed_MB"] = round(moved[k] * map_mb, 2)
                r[k]["GBs_warm_cache"] = round(gbs, 1)
                r[k]["share_of_hbm_copy_rate"] = round(gbs / (HBM_COPY_TBS * 1e3), 3)
        calls.append(r)
        print("groupnorm call:", r, flush=True)
        del x, dy, y, rows
    res["groupnorm_calls"] = calls
    res["torch_group_norm_beside_it"] = "not measured"

    # ---- the train steps: a child process per timing, in alternation
    gn_convs = 4
    res["box_head_conv_GFLOP_per_direction_each"] = round(2 * 2048 * 49 * 9 * 256 * 256 / 1e9, 1)
    res["box_head_convs"] = gn_convs
    steps = {"this": [], "parent": []}
    for _ in range(0 if a.no_steps else STEP_ROUNDS):
        steps["this"].append(child_step(ROOT, "", a.steps, a.warmup))
        if a.parent_root:
            steps["parent"].append(child_step(os.path.abspath(a.parent_root), "", a.steps, a.warmup))
    ms = lambda rows_: [r_["ms_per_step"] for r_ in rows_]
    if steps["this"]:
        res["step_default_this_commit"] = steps["this"]
        res["step_default_this_commit_spread_ms"] = round(max(ms(steps["this"])) - min(ms(steps["this"])), 3)
    if steps["parent"]:
        res["step_default_parent_commit"] = steps["parent"]
        spread = round(max(ms(steps["parent"])) - min(ms(steps["parent"])), 3)
        res["step_default_parent_commit_spread_ms"] = spread
        diff = sum(ms(steps["this"])) / len(steps["this"]) - sum(ms(steps["parent"])) / len(steps["parent"])
        res["step_default_this_minus_parent_ms"] = round(diff, 3)
        res["step_default_not_slower_beyond_parent_spread"] = bool(diff <= spread)
    else:
        res["step_default_parent_commit"] = "not measured (no --parent-root)"
    if not a.no_steps:
        res["step_gn"] = child_step(ROOT, "cubercnn_DLA34_FPN_GN.yaml", a.steps, a.warmup)
    print("steps:", {k: v for k, v in res.items() if k.startswith("step")}, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "groupnorm_calls"}))


if __name__ == "__main__":
    main()
