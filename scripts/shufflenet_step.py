"""ShuffleNetV2 x1.0 FPN (configs/cubercnn_shufflenet_FPN.yaml) on one MI355X, fp32, 4 x 512^2 per step:

  * the train step (solver.make_train_step, dense region replayed from HIP graphs): ms per step, images/s;
  * the trunk's forward + backward alone, eager and replayed from one HIP graph, and its launch count per direction;
  * the same trunk as plain torch-ROCm ops (F.conv2d, F.batch_norm, chunk / cat / view / transpose, ... in float32, NCHW) on the same
    weights, measured the same two ways in the same session, and the relative difference of p4 between the two;
  * every kernel of csrc/shufflenet.hip at the step's shapes (M = 4 * 64^2, 4 * 32^2, 4 * 16^2 output pixels, the depthwise
    convolutions also at stride 2 from the map above): time, algorithmic bytes, GB/s, share of the 8 TB/s HBM peak.

    python scripts/shufflenet_step.py [--steps 20] [--warmup 5] [--out profiles/shufflenet_step_fp32.json]

The figures are recorded, not gated."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                      # noqa: E402
import torch.nn.functional as F   # noqa: E402

HBM_PEAK_GBS = 8000.0             # spec; a float4 copy reaches about 6 300
REPEATS = {"stage2": 4, "stage3": 8, "stage4": 4}


def torch_trunk(p, x):
    """torchvision's shufflenet_v2_x1_0 trunk in train mode from functionals over the state dict p"""
    def bn(t, k):
        return F.batch_norm(t, p[k + ".running_mean"], p[k + ".running_var"], p[k + ".weight"], p[k + ".bias"], True, 0.1, 1e-5)

    def shuffle(t):
        n, c, h, w = t.shape
        return t.view(n, 2, c // 2, h, w).transpose(1, 2).contiguous().view(n, c, h, w)

    def unit(t, pre, stride):
        dw = lambda u, k: F.conv2d(u, p[k], None, stride, 1, 1, u.shape[1])

        def branch2(u):
            u = F.relu(bn(F.conv2d(u, p[pre + "branch2.0.weight"]), pre + "branch2.1"))
            u = bn(dw(u, pre + "branch2.3.weight"), pre + "branch2.4")
            return F.relu(bn(F.conv2d(u, p[pre + "branch2.5.weight"]), pre + "branch2.6"))
        if stride == 1:
            x1, x2 = t.chunk(2, 1)
            return shuffle(torch.cat((x1, branch2(x2)), 1))
        u = bn(dw(t, pre + "branch1.0.weight"), pre + "branch1.1")
        u = F.relu(bn(F.conv2d(u, p[pre + "branch1.2.weight"]), pre + "branch1.3"))
        return shuffle(torch.cat((u, branch2(t)), 1))
    t = F.max_pool2d(F.relu(bn(F.conv2d(x, p["conv1.0.weight"], None, 2, 1), "conv1.1")), 3, 2, 1)
    outs = [t]
    for s, n in REPEATS.items():
        for i in range(n):
            t = unit(t, f"{s}.{i}.", 2 if i == 0 else 1)
        outs.append(t)
    return outs + [F.max_pool2d(t, 1, 2)]


def time_gpu(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def time_both(fn, iters):
    """ms per call: eager launches, and the same work replayed from one HIP graph (None plus the reason if capture fails)"""
    res = {"eager_ms": round(time_gpu(fn, iters), 3)}
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn(); fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        res["graph_ms"] = round(time_gpu(g.replay, iters), 3)
    except Exception as e:
        res["graph_ms"], res["graph_error"] = None, f"{type(e).__name__}: {e}"[:300]
        torch.cuda.synchronize()
    return res


def count_launches(lib, fn):
    """calls into libcr3dod.so made by fn (a call is one to three launches; torch's own kernels are not counted)"""
    n = [0]
    orig = lib.call

    def counting(name, *a, **k):
        n[0] += 1
        return orig(name, *a, **k)
    lib.call = counting
    try:
        fn()
    finally:
        lib.call = orig
    return n[0]


def kernel_table(ops, lib, dev, iters):
    rows, es = [], 4

    def add(name, M, C, ms, nbytes):
        gbs = nbytes / (ms * 1e-3) / 1e9
        rows.append({"kernel": name, "M_out": M, "C": C, "us": round(ms * 1e3, 2), "MB": round(nbytes / 1e6, 3),
                     "GBs": round(gbs, 1), "of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3)})
    # (output side, physical branch width, physical width of the stride-2 branch1 input) per stage
    for side, C, Cin in ((64, 64, 32), (32, 128, 128), (16, 256, 256)):
        N = 4
        M = N * side * side
        for stride, Cd in ((1, C), (2, C), (2, Cin)):
            Hin = side * stride
            x = torch.randn(N, Hin, Hin, Cd, device=dev)
            dy = torch.randn(N, side, side, Cd, device=dev)
            w = torch.randn(Cd, 9, device=dev)
            stats = torch.empty((M + 63) // 64, 2, Cd, device=dev)
            sink = torch.zeros(Cd, 9, device=dev)
            Min = N * Hin * Hin
            tag = f" s{stride}"
            add("cr_dwconv3x3_fwd" + tag, M, Cd, time_gpu(lambda: ops.dwconv3x3_fwd_raw(x, w, stride, stats=stats), iters),
                (Min + M) * Cd * es)
            add("cr_dwconv3x3_bwd_data" + tag, M, Cd, time_gpu(lambda: ops.dwconv3x3_bwd_data_raw(dy, w, x.shape, stride), iters),
                (Min + M) * Cd * es)
            add("cr_dwconv3x3_bwd_weight" + tag, M, Cd, time_gpu(lambda: ops.dwconv3x3_bwd_weight_raw(dy, x, stride, sink=sink), iters),
                (Min + M) * Cd * es)
        bf = {64: 58, 128: 116, 256: 232}[C]
        xin = torch.randn(N, side, side, 2 * C, device=dev)
        b = torch.randn(N, side, side, C, device=dev)
        g = torch.randn(N, side, side, 2 * C, device=dev)
        da, db = torch.empty_like(xin), torch.empty_like(b)
        y = torch.empty_like(xin)
        add("cr_shuffle_tail_fwd", M, 2 * C, time_gpu(lambda: lib.call("cr_shuffle_tail_fwd", xin, 2 * C, b, y, M, bf, C, 1), iters),
            M * (C + C + 2 * C) * es)
        add("cr_shuffle_tail_bwd", M, 2 * C, time_gpu(lambda: lib.call("cr_shuffle_tail_bwd", g, da, 2 * C, db, M, bf, C, 1), iters),
            M * (2 * C + 2 * C + C) * es)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shufflenet_step_fp32.json"))
    a = ap.parse_args()
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    ops = importlib.import_module("3dod_amd.hipops")
    lib = importlib.import_module("3dod_amd._lib")
    dev = torch.device("cuda:0")
    assert ops.precision() == "fp32"
    res = {"metric": "shufflenet_step", "precision": "fp32", "config": "cubercnn_shufflenet_FPN.yaml",
           "device": torch.cuda.get_device_name(0), "images_per_step": bt.IMS_PER_GPU, "image_size": 512}

    cfg, model, opt, syn, solver = bt.build(dev, seed=0, config="cubercnn_shufflenet_FPN.yaml")
    ims = bt.IMS_PER_GPU
    batches = [syn.make_batch(ims, 1234 + i) for i in range(4)]
    for b in batches:
        for d in b:
            d["image"], d["instances"] = d["image"].to(dev), d["instances"].to(dev)

    # ---- the trunk alone (before any optimizer step: same weights for both implementations)
    bu = model.backbone.bottom_up
    with torch.no_grad():
        _, x = model.preprocess_image(batches[0])
    params = [p for p in bu.parameters() if p.requires_grad]
    with torch.no_grad():
        phys = bu(x)
        cots_l = [torch.randn_like(o) for o in bu.logical_features(phys).values()]
    sn = importlib.import_module("3dod_amd.cubercnn.modeling.backbone.shufflenet")
    cots = [sn.to_physical(c, *bu.LAYOUTS[k]) for c, k in zip(cots_l, phys)]
    state = {}

    def ours_fwd():
        state["outs"] = list(bu(x).values())

    def ours_bwd():
        with ops.deferred_wgrad():
            torch.autograd.grad(state["outs"], params, cots, allow_unused=True)

    def ours():
        ours_fwd()
        ours_bwd()
    res["trunk_lib_calls"] = {"forward": count_launches(lib, ours_fwd), "backward": count_launches(lib, ours_bwd)}
    res["trunk_fwd_bwd_hip"] = time_both(ours, a.steps)
    print("trunk, HIP kernels:", res["trunk_fwd_bwd_hip"], res["trunk_lib_calls"], flush=True)

    p32 = {k: v.detach().clone().float().contiguous() for k, v in bu.state_dict().items() if "num_batches" not in k}
    leaves = [v.requires_grad_(True) for k, v in p32.items() if "running" not in k and not k.startswith("conv5.")]
    xt = x[..., :3].permute(0, 3, 1, 2).contiguous()
    cots_t = [c.permute(0, 3, 1, 2).contiguous() for c in cots_l]

    def plain():
        torch.autograd.grad(torch_trunk(p32, xt), leaves, cots_t, allow_unused=True)
    with torch.no_grad():
        a_, b_ = bu.logical_features(bu(x))["p4"].permute(0, 3, 1, 2), torch_trunk(p32, xt)[2]
        res["trunk_p4_rel_diff_hip_vs_torch"] = float((a_ - b_).norm() / b_.norm())
    res["trunk_fwd_bwd_torch"] = time_both(plain, a.steps)
    print("trunk, plain torch:", res["trunk_fwd_bwd_torch"], "p4 rel diff", res["trunk_p4_rel_diff_hip_vs_torch"], flush=True)
    del p32, leaves, cots_t, cots, cots_l

    # ---- the new kernels at the step's shapes
    res["kernels"] = kernel_table(ops, lib, dev, 20)
    for r in res["kernels"]:
        print(r, flush=True)

    # ---- the train step
    step = solver.make_train_step(cfg, model, opt)
    with d2.EventStorage(0):
        for i in range(a.warmup):
            step(batches[i % len(batches)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(batches[i % len(batches)])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rep = step.report()
    res["step"] = {"ms_per_step": round(1e3 * dt / a.steps, 3), "images_per_s": round(ims * a.steps / dt, 1), "steps": a.steps,
                   "launch_mode": os.environ.get("CR_GRAPHS", "dense"), "total_loss": rep["total_loss"],
                   "iterations_explode": rep["iterations_explode"]}
    print("step:", res["step"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "kernels"}))


if __name__ == "__main__":
    main()
