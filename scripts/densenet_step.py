"""DenseNet-121 FPN (configs/cubercnn_densenet_FPN.yaml) on one MI355X, fp32, 4 x 512^2 per step:

  * the train step (solver.make_train_step, dense region replayed from HIP graphs): ms per step, images/s;
  * the trunk's forward + backward alone, eager and replayed from one HIP graph;
  * the same trunk as plain torch-ROCm ops (F.conv2d, F.batch_norm, torch.cat, ... in float32, NCHW) on the same weights, measured
    the same two ways in the same session;
  * every kernel of csrc/densenet.hip at denseblock1's shape (M = 65 536 pixels, C = 64 .. 224) and denseblock3's
    (M = 4 096, C = 256 .. 992): time, bytes moved, GB/s, share of the 8 TB/s HBM peak.

    python scripts/densenet_step.py [--steps 20] [--warmup 5] [--out profiles/densenet_step_fp32.json]

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
BLOCKS = (6, 12, 24, 16)


def torch_trunk(p, x):
    """torchvision's densenet121.features in train mode from functionals over the state dict p (keys relative to `base.`)"""
    def bn(t, k):
        return F.batch_norm(t, p[k + ".running_mean"], p[k + ".running_var"], p[k + ".weight"], p[k + ".bias"], True, 0.1, 1e-5)

    def block(t, b, n):
        feats = [t]
        for l in range(1, n + 1):
            k = f"denseblock{b}.denselayer{l}."
            h = F.conv2d(F.relu(bn(torch.cat(feats, 1), k + "norm1")), p[k + "conv1.weight"])
            feats.append(F.conv2d(F.relu(bn(h, k + "norm2")), p[k + "conv2.weight"], padding=1))
        return torch.cat(feats, 1)

    def transition(t, i):
        return F.avg_pool2d(F.conv2d(F.relu(bn(t, f"transition{i}.norm")), p[f"transition{i}.conv.weight"]), 2, 2)
    t = F.max_pool2d(F.relu(bn(F.conv2d(x, p["conv0.weight"], None, 2, 3), "norm0")), 3, 2, 1)
    p2 = block(t, 1, BLOCKS[0])
    p3 = block(transition(p2, 1), 2, BLOCKS[1])
    p4 = block(transition(p3, 2), 3, BLOCKS[2])
    p5 = bn(block(transition(p4, 3), 4, BLOCKS[3]), "norm5")
    return [p2, p3, p4, p5, F.max_pool2d(p5, 1, 2)]


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


def kernel_table(ops, lib, dev, iters):
    rows = []
    es = 4

    def add(shape, name, C, ms, nbytes):
        gbs = nbytes / (ms * 1e-3) / 1e9
        rows.append({"shape": shape, "kernel": name, "C": C, "us": round(ms * 1e3, 2), "MB": round(nbytes / 1e6, 3),
                     "GBs": round(gbs, 1), "of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3)})
    for shape, (N, H, W), ld, Cs in (("denseblock1", (4, 128, 128), 256, list(range(64, 256, 32))),
                                     ("denseblock3", (4, 32, 32), 1024, list(range(256, 1024, 32)))):
        M = N * H * W
        X = torch.randn(N, H, W, ld, device=dev)
        G = torch.randn(N, H, W, ld, device=dev)
        tab = torch.zeros(3, ld, device=dev)
        ops.dense_stats(X, 0, Cs[0], tab, 0, 1e-5)
        for c in range(Cs[0], ld, 32):
            ops.dense_stats(X, c, 32, tab, c, 1e-5)
        y = torch.randn(N, H, W, 32, device=dev)
        stats = torch.rand((M + 63) // 64, 2, 32, device=dev)
        add(shape, "cr_dense_stats", Cs[0], time_gpu(lambda: ops.dense_stats(X, 0, Cs[0], tab, 0, 1e-5), iters), M * Cs[0] * es)
        add(shape, "cr_dense_stats_finalize", 32,
            time_gpu(lambda: lib.call("cr_dense_stats_finalize", stats, stats.shape[0], 32, M, tab, ld, ld - 32, 1e-5), iters),
            stats.numel() * 4)
        add(shape, "cr_dense_slice_store", 32, time_gpu(lambda: ops.dense_slice_store(y, X, ld - 32), iters), 2 * M * 32 * es)
        add(shape, "cr_dense_slice_gather", 32, time_gpu(lambda: ops.dense_slice_gather(G, ld - 32, 32, X.dtype), iters),
            M * 32 * (4 + es))
        for C in Cs:
            bn = torch.nn.BatchNorm2d(C).to(dev).train()
            da = torch.randn(N, H, W, C, device=dev)
            add(shape, "cr_dense_bn_fwd", C, time_gpu(lambda: ops.dense_bn_fwd(X, C, tab, bn, bn.weight, bn.bias, True, True), iters),
                2 * M * C * es)
            # three launches: partial sums read X and da, the finalize is negligible, the apply reads X, da, G and writes G
            add(shape, "cr_dense_bn_bwd", C,
                time_gpu(lambda: ops.dense_bn_bwd(da, X, C, tab, bn, bn.weight, bn.bias, True, True, G, True), iters),
                M * C * (4 * es + 8))
        Ct = ld
        xt = torch.randn(N, H, W, Ct, device=dev)
        yt = torch.randn(N, H // 2, W // 2, Ct, device=dev)
        add(shape, "cr_avgpool2x2_fwd", Ct, time_gpu(lambda: lib.call("cr_avgpool2x2_fwd", xt, yt, N, H, W, Ct, 1), iters),
            int(1.25 * M * Ct * es))
        add(shape, "cr_avgpool2x2_bwd", Ct, time_gpu(lambda: lib.call("cr_avgpool2x2_bwd", yt, xt, N, H, W, Ct, 1), iters),
            int(1.25 * M * Ct * es))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densenet_step_fp32.json"))
    a = ap.parse_args()
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    ops = importlib.import_module("3dod_amd.hipops")
    lib = importlib.import_module("3dod_amd._lib")
    dev = torch.device("cuda:0")
    assert ops.precision() == "fp32"
    res = {"metric": "densenet_step", "precision": "fp32", "config": "cubercnn_densenet_FPN.yaml", "device": torch.cuda.get_device_name(0),
           "images_per_step": bt.IMS_PER_GPU, "image_size": 512}

    cfg, model, opt, syn, solver = bt.build(dev, seed=0, config="cubercnn_densenet_FPN.yaml")
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
        cots = [torch.randn_like(o) for o in bu(x).values()]

    def ours():
        outs = list(bu(x).values())
        with ops.deferred_wgrad():
            torch.autograd.grad(outs, params, cots, allow_unused=True)
    res["trunk_fwd_bwd_hip"] = time_both(ours, a.steps)
    print("trunk, HIP kernels:", res["trunk_fwd_bwd_hip"], flush=True)

    p32 = {k[len("base."):]: v.detach().clone().float().contiguous() for k, v in bu.state_dict().items() if "num_batches" not in k}
    leaves = [v.requires_grad_(True) for k, v in p32.items() if "running" not in k]
    xt = x[..., :3].permute(0, 3, 1, 2).contiguous()
    cots_t = [c.permute(0, 3, 1, 2).contiguous() for c in cots]

    def plain():
        torch.autograd.grad(torch_trunk(p32, xt), leaves, cots_t, allow_unused=True)
    with torch.no_grad():
        a_, b_ = bu(x)["p4"].permute(0, 3, 1, 2), torch_trunk(p32, xt)[2]
        res["trunk_p4_rel_diff_hip_vs_torch"] = float((a_ - b_).norm() / b_.norm())
    res["trunk_fwd_bwd_torch"] = time_both(plain, a.steps)
    print("trunk, plain torch:", res["trunk_fwd_bwd_torch"], flush=True)
    del p32, leaves, cots_t, cots

    # ---- the new kernels at the step's shapes
    res["kernels"] = kernel_table(ops, lib, dev, 20)
    for r in res["kernels"]:
        if r["C"] in (32, 64, 224, 256, 992, 1024):
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
