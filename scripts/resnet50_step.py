"""ResNet-50 FPN (configs/cubercnn_ResNet50_FPN.yaml) on one MI355X, fp32, 4 x 512^2 per step, one session:

  * the projection-shortcut tail out = relu(bn3(ya) + bn_d(yb)) at the four real shapes (256 @ 128^2, 512 @ 64^2, 1024 @ 32^2,
    2048 @ 16^2, 4 images): the fused kernels (cr_bn_pair_fwd / cr_bn_pair_bwd) against the two-call composition
    (cr_bn_fwd x 2 / cr_bn_bwd x 2, what Bottleneck.fused_tail = False runs), forward and backward separately.  Each form is
    captured as one HIP graph of TAIL_CALLS back-to-back calls, so a replay is kernel time without the host's launch rate; HIP
    events around replays, REPEATS rounds in alternation after warm-up; per shape the mean of the rounds, the spread between
    them (max - min of either side, whichever is larger) and whether the fused form is faster by more than that spread; the
    maps both forms move.  Every call works on the same buffers, and the largest shape's maps fit the 256 MB last-level cache:
    the GB/s figures are warm-cache rates, not HBM rates.  The two convolutions in front are the same kernels in both forms
    and are not part of these figures;
  * the first block of every stage (the one with the tail), forward + backward, fused against composition, same method;
  * the trunk's forward + backward replayed from one HIP graph, timed in alternation with the same trunk as plain torch-ROCm
    functionals (F.conv2d, F.batch_norm, F.relu, F.max_pool2d in float32, NCHW) on the same weights, replayed from a graph of
    its own; the spread between the rounds of either and the relative difference of p4 between the two;
  * the train step (solver.make_train_step, dense region replayed from HIP graphs): ms per step, images/s -- and the DLA34 step
    in the same session.

    python scripts/resnet50_step.py [--steps 20] [--warmup 5] [--out profiles/resnet50_step_fp32.json] [--no-torch]

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

REPEATS = 5
TAIL_CALLS = 10                   # calls per captured graph of the tail comparison
LAYERS = [3, 4, 6, 3]
TAIL_SHAPES = [(256, 128), (512, 64), (1024, 32), (2048, 16)]          # (C, side) at 4 x 512^2
BLOCKS = [(64, 64, 1, 128), (256, 128, 2, 128), (512, 256, 2, 64), (1024, 512, 2, 32)]     # inplanes, planes, stride, input side
N_IMG = 4


def torch_trunk(p, x):
    """torchvision's resnet50 trunk in train mode from functionals over the state dict p -> [p2, p3, p4, p5, p6]"""
    def bn(t, k):
        return F.batch_norm(t, p[k + ".running_mean"], p[k + ".running_var"], p[k + ".weight"], p[k + ".bias"], True, 0.1, 1e-5)

    def block(t, pre, stride):
        u = F.relu(bn(F.conv2d(t, p[pre + "conv1.weight"]), pre + "bn1"))
        u = F.relu(bn(F.conv2d(u, p[pre + "conv2.weight"], None, stride, 1), pre + "bn2"))
        u = bn(F.conv2d(u, p[pre + "conv3.weight"]), pre + "bn3")
        if pre + "downsample.0.weight" in p:
            t = bn(F.conv2d(t, p[pre + "downsample.0.weight"], None, stride), pre + "downsample.1")
        return F.relu(u + t)
    t = F.max_pool2d(F.relu(bn(F.conv2d(x, p["conv1.weight"], None, 2, 3), "bn1")), 3, 2, 1)
    outs = []
    for li, blocks in enumerate(LAYERS, 1):
        for b in range(blocks):
            t = block(t, f"layer{li}.{b}.", 2 if (b == 0 and li > 1) else 1)
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


def alternate(fused, comp, iters, graph_calls=0):
    """REPEATS rounds of each in alternation -> the figures of one comparison (microseconds per call).  graph_calls > 0: each
    side is replayed from a HIP graph of that many back-to-back calls (eager launches if the capture fails; recorded)"""
    per, graphs = [1, 1], None
    if graph_calls:
        def many(fn):
            def run():
                for _ in range(graph_calls):
                    fn()
            return run
        (gf, ef), (gc, ec) = capture(many(fused)), capture(many(comp))
        graphs = {"calls_per_graph": graph_calls, "fused_replayed_from_graph": gf is not None,
                  "composition_replayed_from_graph": gc is not None, "fused_graph_error": ef, "composition_graph_error": ec}
        if gf is not None:
            fused, per[0] = gf, graph_calls
        if gc is not None:
            comp, per[1] = gc, graph_calls
    time_gpu(fused, iters), time_gpu(comp, iters)            # warm-up of both
    f, c = [], []
    for _ in range(REPEATS):
        f.append(1e3 * time_gpu(fused, iters) / per[0])
        c.append(1e3 * time_gpu(comp, iters) / per[1])
    spread = max(max(f) - min(f), max(c) - min(c))
    mf, mc = sum(f) / len(f), sum(c) / len(c)
    res = {"fused_us": round(mf, 2), "composition_us": round(mc, 2), "fused_rounds_us": [round(v, 2) for v in f],
           "composition_rounds_us": [round(v, 2) for v in c], "spread_us": round(spread, 2), "saved_us": round(mc - mf, 2),
           "fused_faster_by_more_than_spread": bool(mc - mf > spread)}
    if graphs:
        res.update(graphs)
    return res


def tail_case(ops, lib, dev, C, side):
    M = N_IMG * side * side
    nparts = (M + 63) // 64
    g = torch.Generator(device="cpu").manual_seed(C)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev)
    ya, yb, dout = mk(M, C), mk(M, C), mk(M, C)

    def rows(y):
        yp = torch.zeros(nparts * 64, C, device=dev)
        yp[:M] = y
        yp = yp.view(nparts, 64, C)
        return torch.stack([yp.sum(1), (yp * yp).sum(1)], 1).contiguous()
    sa, sb = rows(ya), rows(yb)
    ga, gb = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) + 0.5
    ba, bb = torch.randn(C, device=dev) * 0.1, torch.randn(C, device=dev) * 0.1
    run = [torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev), torch.ones(C, device=dev)]
    acc = [torch.zeros(C, device=dev) for _ in range(4)]
    out, mia, mib = ops.bn_pair_fwd_raw(ya, yb, sa, sb, (ga, ba, run[0], run[1], 1e-5, 0.1), (gb, bb, run[2], run[3], 1e-5, 0.1))
    idn, out_c, dxa, dxb, dres = (torch.empty_like(ya) for _ in range(5))
    mia_c, mib_c = torch.empty_like(mia), torch.empty_like(mib)
    sums = torch.empty(1025, 2, C, device=dev)

    def fwd_fused():
        ops.bn_pair_fwd_raw(ya, yb, sa, sb, (ga, ba, run[0], run[1], 1e-5, 0.1), (gb, bb, run[2], run[3], 1e-5, 0.1))

    def fwd_comp():
        lib.call("cr_bn_fwd", yb, sb, nparts, gb, bb, None, idn, M, C, 0, 1e-5, 0.1, mib_c, run[2], run[3], 1)
        lib.call("cr_bn_fwd", ya, sa, nparts, ga, ba, idn, out_c, M, C, 1, 1e-5, 0.1, mia_c, run[0], run[1], 1)

    def bwd_fused():
        ops.bn_pair_bwd_raw(dout, out, ya, yb, mia, mib, ga, gb, *acc)

    def bwd_comp():
        lib.call("cr_bn_bwd", dout, out, ya, mia, ga, sums, dxa, dres, acc[0], acc[1], M, C, 1, 1)
        lib.call("cr_bn_bwd", dres, None, yb, mib, gb, sums, dxb, None, acc[2], acc[3], M, C, 0, 1)
    es = 4
    map_mb = M * C * es / 1e6
    res = {"C": C, "side": side, "M": M, "map_MB": round(map_mb, 2),
           # forward: ya, yb read, out written | yb read, shortcut written; ya and shortcut read, out written
           "forward_maps_moved": {"fused": 3, "composition": 5},
           # backward: dout, out, ya, yb read twice, two gradients written | dout, out, ya read twice, dx and the masked gradient
           # written; the masked gradient and yb read twice, dx written
           "backward_maps_moved": {"fused": 10, "composition": 13},
           "forward": alternate(fwd_fused, fwd_comp, 20, TAIL_CALLS), "backward": alternate(bwd_fused, bwd_comp, 20, TAIL_CALLS)}
    for k, n in (("forward", res["forward_maps_moved"]["fused"]), ("backward", res["backward_maps_moved"]["fused"])):
        # the same buffers in every call: served in part by the last-level cache, not an HBM rate
        res[k]["fused_GBs_warm_cache"] = round(n * map_mb * 1e6 / (res[k]["fused_us"] * 1e-6) / 1e9, 1)
    return res


def block_case(rn, ops, dev, inplanes, planes, stride, side):
    torch.manual_seed(inplanes)
    down = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(planes * 4))
    blk = rn.to_channels_last(rn.Bottleneck(inplanes, planes, stride, down)).to(dev).train()
    x0 = torch.randn(N_IMG, side, side, inplanes, device=dev)
    so = (side - 1) // stride + 1
    cot = torch.randn(N_IMG, so, so, planes * 4, device=dev)
    params = list(blk.parameters())

    def run(fused):
        def fn():
            blk.fused_tail = fused
            x = x0.detach().requires_grad_(True)            # a fresh leaf per call: a gradient slot lives on the tensor it serves
            torch.autograd.grad(blk(x), [x] + params, cot)
        return fn
    res = alternate(run(True), run(False), 10)
    res.update({"inplanes": inplanes, "planes": planes, "stride": stride, "input_side": side})
    return res


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
    ap.add_argument("--no-torch", action="store_true", help="without the plain torch trunk")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet50_step_fp32.json"))
    a = ap.parse_args()
    ops = importlib.import_module("3dod_amd.hipops")
    lib = importlib.import_module("3dod_amd._lib")
    rn = importlib.import_module("3dod_amd.cubercnn.modeling.backbone.resnet")
    dev = torch.device("cuda:0")
    assert ops.precision() == "fp32"
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    res = {"metric": "resnet50_step", "precision": "fp32", "config": "cubercnn_ResNet50_FPN.yaml",
           "device": torch.cuda.get_device_name(0), "images_per_step": bt.IMS_PER_GPU, "image_size": 512, "repeats": REPEATS}

    # ---- the tail kernels at the four real shapes, then the blocks that hold them
    res["tail"] = [tail_case(ops, lib, dev, C, side) for C, side in TAIL_SHAPES]
    for r in res["tail"]:
        print("tail:", r, flush=True)
    res["tail_fused_faster_everywhere"] = all(r[k]["fused_faster_by_more_than_spread"] for r in res["tail"]
                                              for k in ("forward", "backward"))
    res["first_blocks_fwd_bwd"] = [block_case(rn, ops, dev, *b) for b in BLOCKS]
    for r in res["first_blocks_fwd_bwd"]:
        print("block:", r, flush=True)

    # ---- the trunk alone (before any optimizer step: same weights for both implementations)
    cfg, model, opt, syn, solver = bt.build(dev, seed=0, config="cubercnn_ResNet50_FPN.yaml")
    batch = syn.make_batch(bt.IMS_PER_GPU, 1234)
    for d in batch:
        d["image"], d["instances"] = d["image"].to(dev), d["instances"].to(dev)
    bu = model.backbone.bottom_up
    with torch.no_grad():
        _, x = model.preprocess_image(batch)
        cots = [torch.randn_like(o) for o in bu(x).values()]
    params = [p for p in bu.parameters() if p.requires_grad]

    def ours():
        outs = list(bu(x).values())
        with ops.deferred_wgrad():
            torch.autograd.grad(outs, params, cots, allow_unused=True)
    trunk = {"hip_eager_ms": round(time_gpu(ours, a.steps), 3)}
    g_ours, err_ours = capture(ours)
    run_ours = g_ours or ours
    rounds = {"hip": [], "torch": []}
    run_plain = None
    if not a.no_torch:
        p32 = {k: v.detach().clone().float().contiguous() for k, v in bu.state_dict().items() if "num_batches" not in k}
        leaves = [v.requires_grad_(True) for k, v in p32.items() if "running" not in k]
        xt = x[..., :3].permute(0, 3, 1, 2).contiguous()
        cots_t = [c.permute(0, 3, 1, 2).contiguous() for c in cots]

        def plain():
            torch.autograd.grad(torch_trunk(p32, xt), leaves, cots_t, allow_unused=True)
        with torch.no_grad():
            a_, b_ = bu(x)["p4"].permute(0, 3, 1, 2), torch_trunk(p32, xt)[2]
            res["trunk_p4_rel_diff_hip_vs_torch"] = float((a_ - b_).norm() / b_.norm())
        trunk["torch_eager_ms"] = round(time_gpu(plain, a.steps), 3)
        g_plain, err_plain = capture(plain)
        run_plain = g_plain or plain
        trunk.update(torch_replayed_from_graph=g_plain is not None, torch_graph_error=err_plain)
    for _ in range(REPEATS):                                # in alternation, after the warm-up above
        rounds["hip"].append(round(time_gpu(run_ours, a.steps), 3))
        if run_plain is not None:
            rounds["torch"].append(round(time_gpu(run_plain, a.steps), 3))
    trunk.update(hip_replayed_from_graph=g_ours is not None, hip_graph_error=err_ours, hip_ms=rounds["hip"],
                 hip_spread_ms=round(max(rounds["hip"]) - min(rounds["hip"]), 3))
    if rounds["torch"]:
        trunk.update(torch_ms=rounds["torch"], torch_spread_ms=round(max(rounds["torch"]) - min(rounds["torch"]), 3))
    res["trunk_fwd_bwd"] = trunk
    print("trunk forward + backward:", trunk, flush=True)
    del g_ours, run_ours, run_plain, cots, cfg, model, opt

    # ---- the train steps, same session
    res["step"] = step_time(bt, d2, dev, "cubercnn_ResNet50_FPN.yaml", a.steps, a.warmup)
    print("step:", res["step"], flush=True)
    res["step_dla34"] = step_time(bt, d2, dev, None, a.steps, a.warmup)
    print("step, DLA34:", res["step_dla34"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("tail", "first_blocks_fwd_bwd")}))


if __name__ == "__main__":
    main()
