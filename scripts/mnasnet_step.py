"""MNASNet-1.0 FPN (configs/cubercnn_mnasnet_FPN.yaml) on one MI355X, fp32, 4 x 512^2 per step, one session:

  * the trunk's forward + backward replayed from one HIP graph, timed in alternation (REPEATS rounds after warm-up) with the same
    trunk as plain torch-ROCm functionals (F.conv2d, F.batch_norm, F.relu in float32, NCHW) on the same weights, replayed from
    a graph of its own; the spread between the rounds of either, the relative difference of p4 between the two, and the
    launch count per direction;
  * every kernel of csrc/mnasnet.hip at the step's shapes: time (HIP events over back-to-back launches), algorithmic bytes, GB/s,
    share of the 8 TB/s HBM peak;
  * the train step (solver.make_train_step, dense region replayed from HIP graphs): ms per step, images/s -- and the DLA34 and
    ShuffleNetV2 steps in the same session.

    python scripts/mnasnet_step.py [--steps 20] [--warmup 5] [--out profiles/mnasnet_step_fp32.json]
    python scripts/mnasnet_step.py --bn-only      # cr_bn_bwd_anyc at the step's widest map alone, for a kernel trace

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
REPEATS = 3
BN_MOMENTUM = 1 - 0.9997
STACKS = {8: (16, 24, 3, 2, 3, 3), 9: (24, 40, 5, 2, 3, 3), 10: (40, 80, 5, 2, 6, 3), 11: (80, 96, 3, 1, 6, 2),
          12: (96, 192, 5, 2, 6, 4), 13: (192, 320, 3, 1, 6, 1)}
# the depthwise convolutions of the step: (physical C, k, stride, output side at 512^2)
DW_SHAPES = [(32, 3, 1, 256), (48, 3, 2, 128), (80, 3, 1, 128), (80, 5, 2, 64), (128, 5, 1, 64), (240, 5, 2, 32), (480, 5, 1, 32),
             (480, 3, 1, 32), (576, 3, 1, 32), (576, 5, 2, 16), (1152, 5, 1, 16), (1152, 3, 1, 16)]
# BatchNorm backward over widths that are no powers of two: (physical C, side)
BN_SHAPES = [(48, 256), (48, 128), (80, 128), (80, 64), (48, 64), (240, 64), (240, 32), (80, 32), (480, 32), (96, 32), (576, 32),
             (576, 16), (192, 16), (1152, 16), (320, 16)]


def torch_trunk(p, x):
    """torchvision's mnasnet1_0 trunk in train mode from functionals over the state dict p -> [p2, p3, p4, p5, p6]"""
    def bn(t, k):
        return F.batch_norm(t, p[k + ".running_mean"], p[k + ".running_var"], p[k + ".weight"], p[k + ".bias"], True,
                            BN_MOMENTUM, 1e-5)

    def block(t, pre, k, stride, residual):
        L = pre + "layers."
        u = F.relu(bn(F.conv2d(t, p[L + "0.weight"]), L + "1"))
        u = F.relu(bn(F.conv2d(u, p[L + "3.weight"], None, stride, k // 2, 1, u.shape[1]), L + "4"))
        u = bn(F.conv2d(u, p[L + "6.weight"]), L + "7")
        return u + t if residual else u
    t = F.relu(bn(F.conv2d(x, p["base.0.weight"], None, 2, 1), "base.1"))
    t = F.relu(bn(F.conv2d(t, p["base.3.weight"], None, 1, 1, 1, 32), "base.4"))
    t = bn(F.conv2d(t, p["base.6.weight"]), "base.7")
    outs = []
    for i, (cin, cout, k, stride, exp, repeats) in STACKS.items():
        for j in range(repeats):
            t = block(t, f"base.{i}.{j}.", k, stride if j == 0 else 1, j > 0)
        if i in (8, 9, 11, 13):
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


def capture(fn):
    """fn replayed from one HIP graph -> (replay, None), or (None, the reason) if capture fails"""
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
        return g.replay, None
    except Exception as e:
        torch.cuda.synchronize()
        return None, f"{type(e).__name__}: {e}"[:300]


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


def bn_case(ops, lib, dev, M, C):
    x, dy = torch.randn(M, C, device=dev), torch.randn(M, C, device=dev)
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
    mi = torch.stack([x.mean(0), (x.var(0, unbiased=False) + 1e-5).rsqrt()]).contiguous()
    dgamma, dbeta = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    return lambda: ops.bn_bwd_anyc_raw(dy, None, x, mi, gamma, beta, True, dgamma, dbeta)


def kernel_table(ops, lib, dev, iters):
    rows, es, N = [], 4, 4

    def add(name, M, C, ms, nbytes):
        gbs = nbytes / (ms * 1e-3) / 1e9
        rows.append({"kernel": name, "M_out": M, "C": C, "us": round(ms * 1e3, 2), "MB": round(nbytes / 1e6, 3),
                     "GBs": round(gbs, 1), "of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3)})
    for C, k, stride, side in DW_SHAPES:
        M, Hin = N * side * side, side * stride
        x = torch.randn(N, Hin, Hin, C, device=dev)
        dy = torch.randn(N, side, side, C, device=dev)
        w = torch.randn(C, k * k, device=dev)
        stats = torch.empty((M + 63) // 64, 2, C, device=dev)
        sink = torch.zeros(C, k * k, device=dev)
        nbytes = (N * Hin * Hin + M) * C * es
        tag = f" k{k} s{stride}"
        add("cr_dwconv_fwd" + tag, M, C, time_gpu(lambda: ops.dwconv_fwd_raw(x, w, k, stride, stats=stats), iters), nbytes)
        add("cr_dwconv_bwd_data" + tag, M, C, time_gpu(lambda: ops.dwconv_bwd_data_raw(dy, w, x.shape, k, stride), iters), nbytes)
        add("cr_dwconv_bwd_weight" + tag, M, C, time_gpu(lambda: ops.dwconv_bwd_weight_raw(dy, x, k, stride, sink=sink), iters),
            nbytes)
        del x, dy
    for C, side in BN_SHAPES:
        M = N * side * side
        # the algorithm's bytes: dy and x read once, dx written (the kernel reads dy and x twice: reduce, then apply)
        add("cr_bn_bwd_anyc relu, mask from x", M, C, time_gpu(bn_case(ops, lib, dev, M, C), iters), 3 * M * C * es)
    return rows


def step_time(bt, d2, dev, config, steps, warmup):
    cfg, model, opt, syn, solver = bt.build(dev, seed=0, config=config)
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
    return {"config": config or "Base_Omni3D.yaml (DLA34)", "ms_per_step": round(1e3 * dt / steps, 3),
            "images_per_s": round(ims * steps / dt, 1), "steps": steps, "launch_mode": os.environ.get("CR_GRAPHS", "dense"),
            "total_loss": rep["total_loss"], "iterations_explode": rep["iterations_explode"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bn-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mnasnet_step_fp32.json"))
    a = ap.parse_args()
    ops = importlib.import_module("3dod_amd.hipops")
    lib = importlib.import_module("3dod_amd._lib")
    dev = torch.device("cuda:0")
    assert ops.precision() == "fp32"
    if a.bn_only:                   # the step's widest non-power-of-two map: 576 channels at stride 16 of 4 x 512^2
        fn = bn_case(ops, lib, dev, 4 * 32 * 32, 576)
        print("cr_bn_bwd_anyc M=4096 C=576 f32: %.2f us per call (events)" % (1e3 * time_gpu(fn, 200, warmup=20)))
        return
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    mn = importlib.import_module("3dod_amd.cubercnn.modeling.backbone.mnasnet")
    res = {"metric": "mnasnet_step", "precision": "fp32", "config": "cubercnn_mnasnet_FPN.yaml",
           "device": torch.cuda.get_device_name(0), "images_per_step": bt.IMS_PER_GPU, "image_size": 512}

    cfg, model, opt, syn, solver = bt.build(dev, seed=0, config="cubercnn_mnasnet_FPN.yaml")
    batch = syn.make_batch(bt.IMS_PER_GPU, 1234)
    for d in batch:
        d["image"], d["instances"] = d["image"].to(dev), d["instances"].to(dev)

    # ---- the trunk alone (before any optimizer step: same weights for both implementations)
    bu = model.backbone.bottom_up
    with torch.no_grad():
        _, x = model.preprocess_image(batch)
    params = [p for p in bu.parameters() if p.requires_grad]
    with torch.no_grad():
        phys = bu(x)
        cots_l = [torch.randn_like(o) for o in bu.logical_features(phys).values()]
    cots = [mn.to_physical(c, bu.WIDTHS[k]) for c, k in zip(cots_l, phys)]
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

    p32 = {k: v.detach().clone().float().contiguous() for k, v in bu.state_dict().items() if "num_batches" not in k}
    head = ("base.14.", "base.15.", "base.16.")
    leaves = [v.requires_grad_(True) for k, v in p32.items() if "running" not in k and not k.startswith(head)]
    xt = x[..., :3].permute(0, 3, 1, 2).contiguous()
    cots_t = [c.permute(0, 3, 1, 2).contiguous() for c in cots_l]

    def plain():
        torch.autograd.grad(torch_trunk(p32, xt), leaves, cots_t, allow_unused=True)
    with torch.no_grad():
        a_, b_ = bu.logical_features(bu(x))["p4"].permute(0, 3, 1, 2), torch_trunk(p32, xt)[2]
        res["trunk_p4_rel_diff_hip_vs_torch"] = float((a_ - b_).norm() / b_.norm())
    eager = {"hip_eager_ms": round(time_gpu(ours, a.steps), 3), "torch_eager_ms": round(time_gpu(plain, a.steps), 3)}
    g_ours, err_ours = capture(ours)
    g_plain, err_plain = capture(plain)
    run_ours, run_plain = g_ours or ours, g_plain or plain
    rounds = {"hip": [], "torch": []}
    for _ in range(REPEATS):                                # in alternation, after the warm-up above
        rounds["hip"].append(round(time_gpu(run_ours, a.steps), 3))
        rounds["torch"].append(round(time_gpu(run_plain, a.steps), 3))
    res["trunk_fwd_bwd"] = dict(eager, hip_replayed_from_graph=g_ours is not None, torch_replayed_from_graph=g_plain is not None,
                                hip_graph_error=err_ours, torch_graph_error=err_plain, hip_ms=rounds["hip"], torch_ms=rounds["torch"],
                                hip_spread_ms=round(max(rounds["hip"]) - min(rounds["hip"]), 3),
                                torch_spread_ms=round(max(rounds["torch"]) - min(rounds["torch"]), 3))
    print("trunk forward + backward:", res["trunk_fwd_bwd"], res["trunk_lib_calls"], "p4 rel diff",
          res["trunk_p4_rel_diff_hip_vs_torch"], flush=True)
    del p32, leaves, cots_t, cots, cots_l, g_ours, g_plain, run_ours, run_plain

    # ---- the new kernels at the step's shapes
    res["kernels"] = kernel_table(ops, lib, dev, 20)
    for r in res["kernels"]:
        print(r, flush=True)

    # ---- the train steps of the three trunks, same session
    del cfg, model, opt
    res["step"] = step_time(bt, d2, dev, "cubercnn_mnasnet_FPN.yaml", a.steps, a.warmup)
    print("step:", res["step"], flush=True)
    res["step_shufflenet"] = step_time(bt, d2, dev, "cubercnn_shufflenet_FPN.yaml", a.steps, a.warmup)
    print("step, ShuffleNetV2:", res["step_shufflenet"], flush=True)
    res["step_dla34"] = step_time(bt, d2, dev, None, a.steps, a.warmup)
    print("step, DLA34:", res["step_dla34"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "kernels"}))


if __name__ == "__main__":
    main()
