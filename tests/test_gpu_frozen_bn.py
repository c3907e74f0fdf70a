"""GPU: training with frozen BatchNorm (MODEL.USE_BN False -> solver.freeze_bn, solver/build.py:71-76 of the reference): the
layers run on their running statistics, which never change, while gamma / beta (and everything else) still learn.

  layer        conv_bn_act(training=False) with gradients at the trunk's own configurations, every precision, against float64
               autograd of F.conv2d + F.batch_norm(training=False) (+ residual, ReLU) on the device with MIOpen off; the ReLU
               mask of the float64 backward is the GPU's (tests/test_gpu_step_shapes_f64.py).  Some channels carry
               |mean| * invstd ~ 8, where the dgamma identity of the backward subtracts two large terms;
  Root         root_conv_bn_act(training=False) with 2 and 3 children on the per-child route;
  dense region trunk + FPN + RPN head gradients after freeze_bn vs the CPU oracle (DLA34 and ResNet34);
  graphs       a frozen GraphedDense replay equals the eager frozen region, follows parameter updates (the fold is captured),
               and a region captured in train mode is never replayed after freeze_bn;
  do_train     MODEL.USE_BN False end to end with an evaluation in between: running statistics bitwise unchanged;
  determinism  CR_DETERMINISTIC=1: two frozen runs give bitwise-identical parameters."""
import importlib
import itertools
import os
import subprocess
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
ops = importlib.import_module("3dod_amd.hipops")
syn = importlib.import_module("3dod_amd.synthetic")
modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
solver = importlib.import_module("3dod_amd.cubercnn.solver")
TOL = {"fp32": (2e-5, 1e-4), "fp32x3": (2e-5, 1e-4), "bf16": (2e-2, 3e-2)}      # (y, every gradient), max-norm relative


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def relerr(got, ref):
    got = got.to(ref.device, f64)
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


@pytest.fixture(scope="module", autouse=True)
def no_miopen():
    prev = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    yield
    torch.backends.cudnn.enabled = prev


def _inputs(seed, N, H, W, Cin, Cout, k, stride, pad, has_res, dt, cin_real=None):
    """x >= 0 (post-ReLU activations; the stem's padded channels zero), a He-scaled weight with a constant added to every
    8th output channel (their conv outputs then sit at |mean| / std ~ 8), running statistics drawn near the batch's own"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    cr = cin_real or Cin
    x = torch.randn((N, H, W, Cin), generator=g, device=DEV).abs()
    if cr < Cin:
        x[..., cr:] = 0
    x = x.to(dt).float()                       # the values the kernels see
    sd = (2.0 / (k * k * cr)) ** 0.5
    w = torch.randn((Cout, cr, k, k), generator=g, device=DEV) * sd
    w[::8] += 13 * sd / (k * k * cr) ** 0.5
    with torch.no_grad():
        y = F.conv2d(nchw(x[..., :cr]).to(f64), w.to(f64), None, stride, pad)
    bm, bv = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    rm = (bm + 0.1 * bv.sqrt() * torch.randn(Cout, generator=g, device=DEV, dtype=f64)).float()
    rv = (bv * (0.8 + 0.4 * torch.rand(Cout, generator=g, device=DEV, dtype=f64))).float()
    gamma = 0.5 + torch.rand(Cout, generator=g, device=DEV)
    beta = 0.3 * torch.randn(Cout, generator=g, device=DEV)
    Ho, Wo = y.shape[2], y.shape[3]
    res = torch.randn((N, Ho, Wo, Cout), generator=g, device=DEV).to(dt).float() if has_res else None
    dy = torch.randn((N, Ho, Wo, Cout), generator=g, device=DEV).to(dt).float()
    ratio = float((rm.abs() * torch.rsqrt(rv + 1e-5)).max())
    return dict(x=x, w=w.contiguous(memory_format=torch.channels_last), rm=rm, rv=rv, gamma=gamma, beta=beta, res=res,
                dy=dy, ratio=ratio)


def _f64_ref(xs, w, gamma, beta, rm, rv, stride, pad, res, relu, y_gpu, dy, x_grad):
    x64 = [nchw(x.detach()).to(f64).requires_grad_(x_grad) for x in xs]
    w64, g64, b64 = [t.detach().to(f64).requires_grad_(True) for t in (w, gamma, beta)]
    r64 = nchw(res.detach()).to(f64).requires_grad_(True) if res is not None else None
    xc = torch.cat(x64, 1) if len(x64) > 1 else x64[0]
    z = F.batch_norm(F.conv2d(xc[:, :w64.shape[1]], w64, None, stride, pad), rm.to(f64), rv.to(f64), g64, b64, False, 0.1, 1e-5)
    if r64 is not None:
        z = z + r64
    y64 = z * (nchw(y_gpu.detach().float()) > 0).to(f64) if relu else z
    y64.backward(nchw(dy).to(f64))
    return y64.detach(), x64, w64, g64, b64, r64


# (name, N, H, W, Cin, Cout, k, stride, pad, relu, residual)
LAYERS = [
    ("stem 7x7 s1", 2, 64, 64, None, 16, 7, 1, 3, True, False),
    ("3x3 s1", 2, 32, 32, 64, 64, 3, 1, 1, True, False),
    ("3x3 s2", 2, 32, 32, 64, 128, 3, 2, 1, True, False),
    ("block conv2 + residual", 2, 16, 16, 128, 128, 3, 1, 1, True, True),
    ("1x1 project, no ReLU", 2, 16, 16, 64, 128, 1, 1, 0, False, False),
    ("512ch 3x3, 8x8 map", 2, 8, 8, 512, 512, 3, 1, 1, True, False),
]


@pytest.mark.parametrize("layer", LAYERS, ids=[l[0] for l in LAYERS])
def test_frozen_conv_bn_layer_vs_float64(layer, precision):
    name, N, H, W, Cin, Cout, k, stride, pad, relu, has_res = layer
    dt = bf16 if precision == "bf16" else f32
    stem = Cin is None
    if stem:
        Cin = 8 if dt == bf16 else 4                  # the stem's activations: 3 real channels + zeros
    e = _inputs(zlib.crc32(name.encode()), N, H, W, Cin, Cout, k, stride, pad, has_res, dt, cin_real=3 if stem else None)
    if not stem:
        assert e["ratio"] > 4.5, e["ratio"]         # the dgamma cancellation is exercised (~8; ~5 on the 8x8 map)
    x = e["x"].to(dt, copy=True).requires_grad_(not stem)
    w = e["w"].clone(memory_format=torch.channels_last).requires_grad_(True)
    gamma, beta = e["gamma"].clone().requires_grad_(True), e["beta"].clone().requires_grad_(True)
    res = e["res"].to(dt, copy=True).requires_grad_(True) if has_res else None
    rm, rv = e["rm"].clone(), e["rv"].clone()
    wk = ops.pad_input_channels(w, Cin) if stem else w
    y = ops.conv_bn_act(x, wk, gamma, beta, rm, rv, stride, pad, relu, res, training=False)
    y.backward(e["dy"].to(dt))
    torch.cuda.synchronize()
    assert torch.equal(rm, e["rm"]) and torch.equal(rv, e["rv"]), "running statistics changed"
    y64, x64, w64, g64, b64, r64 = _f64_ref([e["x"]], e["w"], e["gamma"], e["beta"], e["rm"], e["rv"], stride, pad, e["res"],
                                            relu, y, e["dy"], not stem)
    err = {"y": relerr(nchw(y.detach()), y64), "dw": relerr(w.grad, w64.grad), "dgamma": relerr(gamma.grad, g64.grad),
           "dbeta": relerr(beta.grad, b64.grad)}
    if not stem:
        err["dx"] = relerr(nchw(x.grad), x64[0].grad)
    else:
        assert x.grad is None
    if has_res:
        err["dres"] = relerr(nchw(res.grad), r64.grad)
    ty, tg = TOL[precision]
    print(f"\n[{precision}] {name}: |mean|*invstd max {e['ratio']:.1f}  " + " ".join(f"{k}={v:.1e}" for k, v in err.items()))
    bad = {k: v for k, v in err.items() if v > (ty if k == "y" else tg)}
    assert not bad, bad


def _graph_nodes(fn):
    seen, todo = set(), [fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        todo.extend(n for n, _ in f.next_functions)
    return [type(f).__name__ for f in seen]


@pytest.mark.parametrize("nchild", [2, 3])
def test_frozen_root_per_child_route(nchild, precision):
    dt = bf16 if precision == "bf16" else f32
    N, H, W, ci, Cout = 2, 16, 16, 64, 128
    e = _inputs(100 + nchild, N, H, W, ci * nchild, Cout, 1, 1, 0, False, dt)
    xs = [e["x"][..., i * ci:(i + 1) * ci].contiguous() for i in range(nchild)]
    kids = [c.to(dt, copy=True).requires_grad_(True) for c in xs]
    w = e["w"].clone(memory_format=torch.channels_last).requires_grad_(True)
    gamma, beta = e["gamma"].clone().requires_grad_(True), e["beta"].clone().requires_grad_(True)
    rm, rv = e["rm"].clone(), e["rv"].clone()
    y = ops.root_conv_bn_act(kids, w, gamma, beta, rm, rv, relu=True, training=False)
    names = _graph_nodes(y.grad_fn)
    assert type(y.grad_fn).__name__.startswith("_RootConvBN"), type(y.grad_fn).__name__
    assert not any(n.startswith("Cat") for n in names), names
    y.backward(e["dy"].to(dt))
    torch.cuda.synchronize()
    assert torch.equal(rm, e["rm"]) and torch.equal(rv, e["rv"])
    y64, x64, w64, g64, b64, _ = _f64_ref(xs, e["w"], e["gamma"], e["beta"], e["rm"], e["rv"], 1, 0, None, True, y, e["dy"], True)
    err = {"y": relerr(nchw(y.detach()), y64), "dw": relerr(w.grad, w64.grad), "dgamma": relerr(gamma.grad, g64.grad),
           "dbeta": relerr(beta.grad, b64.grad)}
    for i, (a, b) in enumerate(zip(kids, x64)):
        err[f"dx{i}"] = relerr(nchw(a.grad), b.grad)
    ty, tg = TOL[precision]
    print(f"\n[{precision}] Root x{nchild}: " + " ".join(f"{k}={v:.1e}" for k, v in err.items()))
    bad = {k: v for k, v in err.items() if v > (ty if k == "y" else tg)}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# the dense region (trunk + FPN + RPN head) vs the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------
def _build(config=None, dev=DEV, seed=0):
    args = [os.path.join(ROOT, "configs", config)] if config else []
    cfg = syn.make_cfg(*args, overrides=["MODEL.DEVICE", str(dev), "VIS_PERIOD", 0, "log", False, "SOLVER.BASE_LR", 0.002])
    torch.manual_seed(seed)
    model = modeling.build_model(cfg).to(dev).train()
    return cfg, model


def _randomize_bn(model, seed, batch=None):
    """pretrained-like BatchNorm state: running statistics of real activations (one train-mode pass over `batch` with
    momentum 1, as a trained trunk would carry; without a batch: drawn at random) and affine parameters away from 1 / 0"""
    g = torch.Generator().manual_seed(seed)
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    if batch is not None:
        mom = [m.momentum for m in bns]
        for m in bns:
            m.momentum = 1.0
        model.train()
        with torch.no_grad():
            model.backbone(model.preprocess_image(batch)[1])
        for m, mo in zip(bns, mom):
            m.momentum = mo
    with torch.no_grad():
        for m in bns:
            C = m.num_features
            if batch is None:
                m.running_mean.copy_(0.2 * torch.randn(C, generator=g))
                m.running_var.copy_(0.5 + torch.rand(C, generator=g))
            m.weight.copy_(0.7 + 0.6 * torch.rand(C, generator=g))
            m.bias.copy_(0.1 * torch.randn(C, generator=g))
    ops.bump_weight_epoch()


def _dense(model, x, ups):
    feats = model.backbone(x)
    pg = model.proposal_generator
    logits, deltas = pg.rpn_head([feats[f] for f in pg.in_features])
    outs = list(logits) + list(deltas)
    if ups is None:
        g = torch.Generator().manual_seed(5)
        ups = [torch.randn(tuple(o.shape), generator=g) for o in outs]
    loss = sum((o.float() * u.to(o.device)).sum() for o, u in zip(outs, ups))
    return loss, ups


# bf16 is held at the layer level above: over the whole region the bf16 gradients of the unchanged train-mode path already
# differ from the bf16-emulating oracle by ~0.7 relative L2 (rounding of the stored activation gradients through the tree)
DENSE = [("Base_Omni3D.yaml", "fp32"), ("Base_Omni3D.yaml", "fp32x3"), ("cubercnn_ResNet34_FPN.yaml", "fp32")]


@pytest.mark.parametrize("config,prec", DENSE, ids=[f"{c.split('.')[0]}-{p}" for c, p in DENSE])
def test_frozen_dense_region_gradients_vs_cpu_oracle(config, prec):
    """Run with the gradient-slot fan-in off (autograd adds the contributions of several consumers): with slots AND the
    fused Root on, DLA34's gradients differ from the oracle's by ~0.19 relative L2 in TRAIN mode as well (measured on the
    unchanged train-mode path; 1.1e-2 with slots off, as frozen), so that route is not what this test can pin; the frozen
    layers are the same either way."""
    from oracle import cpu_backend
    prev = ops.set_precision(prec)
    slots, ops._SLOTS_ON[0] = ops._SLOTS_ON[0], False
    try:
        cfg, model = _build(None if config == "Base_Omni3D.yaml" else config)
        opt = solver.build_optimizer(cfg, model)
        batch = syn.make_batch(2, 61, with_gt=False, size=256)
        _randomize_bn(model, 3, syn.make_batch(2, 62, with_gt=False, size=256))
        solver.freeze_bn(model)
        stats0 = {k: v.clone() for k, v in model.state_dict().items() if "running" in k}
        opt.zero_grad()
        images, x = model.preprocess_image(batch)
        loss, ups = _dense(model, x, None)
        loss.backward()
        opt.collect_grads()
        torch.cuda.synchronize()
        for k, v in model.state_dict().items():
            if "running" in k:
                assert torch.equal(v, stats0[k]), k
        names = [n for n, p in model.named_parameters() if n.startswith(("backbone.", "proposal_generator.rpn_head."))
                 and p.requires_grad]
        params = dict(model.named_parameters())
        got = {n: params[n]._cr_grad.detach().float().cpu().clone() for n in names}
        xin = x.detach().float().cpu()
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    finally:
        ops.set_precision(prev)
        ops._SLOTS_ON[0] = slots
    del model, opt
    torch.cuda.empty_cache()
    saved = {n: importlib.import_module(n).ops for n in cpu_backend.PATCHED}
    try:
        cpu_backend.install()
        args = [os.path.join(ROOT, "configs", config)] if config != "Base_Omni3D.yaml" else []
        ref = modeling.build_model(syn.make_cfg(*args, overrides=["MODEL.DEVICE", "cpu", "VIS_PERIOD", 0, "log", False]))
        ref.load_state_dict(sd)
        ref.train()
        solver.freeze_bn(ref)
        loss_r, _ = _dense(ref, xin, ups)
        loss_r.backward()
        rp = dict(ref.named_parameters())
    finally:
        for n, o in saved.items():
            importlib.import_module(n).ops = o
    # relative L2 per tensor, and over all of them.  A pre-activation within rounding of zero flips a ReLU mask between the
    # two runs; on the small maps of the upper levels (a few hundred pixels) one flip moves a weight gradient by ~1/sqrt(P)
    # (measured, fp32: 1.1e-2 over all for DLA34, 3.7e-3 for ResNet34), so the bounds catch O(1) errors -- a wrong BatchNorm
    # gradient -- and not rounding.
    tol, tol_all = 0.1, 3e-2
    worst, fails, nbn, num, den = 0.0, [], 0, 0.0, 0.0
    for n in names:
        r = rp[n].grad
        if r is None:              # computed but unused by the trunk (the project of a Tree with levels > 1)
            r = torch.zeros_like(got[n])
        num += float((got[n] - r).norm()) ** 2
        den += float(r.norm()) ** 2
        e = float((got[n] - r).norm() / (r.norm() + 1e-12))
        if float(r.norm()) == 0.0:
            e = float(got[n].abs().max())
        worst = max(worst, e)
        nbn += ".bn" in n or "bn1" in n or "bn2" in n or "downsample.1" in n or ".project.1" in n
        if e > tol:
            fails.append((n, e))
    rel_all = (num / den) ** 0.5
    print(f"\n[{prec}] {config}: {len(names)} parameter gradients ({nbn} BatchNorm), relative L2 over all {rel_all:.1e}, "
          f"worst tensor {worst:.1e}")
    assert nbn >= 20, nbn
    assert rel_all < tol_all and not fails, (rel_all, sorted(fails, key=lambda t: -t[1])[:20])


# ---------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------
def test_frozen_graphed_dense_region():
    bt = importlib.import_module("bench_train")
    graphed = importlib.import_module("3dod_amd.cubercnn.modeling.graphed")
    cfg, model, opt, syn_, _ = bt.build(DEV, seed=0)
    _randomize_bn(model, 4)
    batch = syn.make_batch(2, 33, with_gt=False)
    pg = model.proposal_generator
    images, u8 = model._stack_images(batch)
    stats0 = {k: v.clone() for k, v in model.state_dict().items() if "running" in k}

    # a region captured with train-mode BatchNorm is never replayed after freeze_bn (and comes back after model.train())
    model.enable_graphs(None, max_shapes=4)
    g_train = model._train_graph_for(u8)
    solver.freeze_bn(model)
    assert not g_train.matches(u8)
    g_frozen = model._train_graph_for(u8)
    assert g_frozen is not g_train and g_frozen.bn_mode != g_train.bn_mode and not any(g_frozen.bn_mode)
    model.train()
    assert model._train_graph_for(u8) is g_train
    solver.freeze_bn(model)
    assert model._train_graph_for(u8) is g_frozen
    for k, v in model.state_dict().items():
        if "running" in k:
            assert torch.equal(v, stats0[k]), k

    def loss_of(feats, logits, deltas):
        return sum((f.float() ** 2).mean() for f in feats.values()) + sum(l.mean() for l in logits) + \
            sum((d ** 2).mean() for d in deltas)

    def eager():
        opt.zero_grad()
        _, x = model.preprocess_image(batch)
        feats = model.backbone(x)
        logits, deltas = pg.rpn_head([feats[f] for f in pg.in_features])
        return feats, logits, deltas

    def replay():
        opt.zero_grad()
        feats, ys = g_frozen(u8)
        A = pg.rpn_head.num_anchors
        ys = pg.rpn_head.level_views(ys, [feats[f] for f in pg.in_features])
        return feats, [y[..., :A].reshape(y.shape[0], -1) for y in ys], [y[..., A:5 * A].reshape(y.shape[0], -1, 4) for y in ys]

    try:
        feats, logits, deltas = eager()
        loss_of(feats, logits, deltas).backward()
        opt.collect_grads()
        g_eager = opt.flat_g.clone()
        f_eager = {k: v.detach().clone() for k, v in feats.items()}
        feats2, logits2, deltas2 = replay()
        loss_of(feats2, logits2, deltas2).backward()
        opt.collect_grads()
        for k in f_eager:
            assert torch.equal(f_eager[k], feats2[k]), k
        rel = float((opt.flat_g - g_eager).norm() / g_eager.norm())
        assert rel < 1e-3, rel
        # an update of the weights, gamma and beta (all views of the flat buffer): the replay follows (the fold is captured)
        bn_w = [m.weight for m in graphed.dense_bn_modules(model)]
        w0 = bn_w[0].detach().clone()
        opt.flat_p.mul_(1.01)
        opt.flat_p.add_(1e-3)
        ops.bump_weight_epoch()
        assert not torch.equal(w0, bn_w[0].detach())
        feats3, _, _ = replay()
        assert not torch.equal(feats3["p2"], f_eager["p2"])
        f4, _, _ = eager()
        for k in f4:
            assert torch.equal(f4[k], feats3[k]), k
        for k, v in model.state_dict().items():
            if "running" in k:
                assert torch.equal(v, stats0[k]), k
    finally:
        model._graphed = None
        opt.zero_grad()


# ---------------------------------------------------------------------------------------------------------------------
# do_train with MODEL.USE_BN False
# ---------------------------------------------------------------------------------------------------------------------
def test_do_train_use_bn_false(tmp_path):
    data = []
    for i in range(4):
        b = syn.make_batch(2, 70 + i, size=256)
        for d in b:
            d["image"], d["instances"] = d["image"].to(DEV), d["instances"].to(DEV)
        data.append(b)
    cfg = syn.make_cfg(overrides=["MODEL.DEVICE", str(DEV), "VIS_PERIOD", 0, "log", False, "SOLVER.BASE_LR", 0.002,
                                  "SOLVER.MAX_ITER", 6, "SOLVER.CHECKPOINT_PERIOD", 100, "TEST.EVAL_PERIOD", 3,
                                  "MODEL.USE_BN", False, "OUTPUT_DIR", str(tmp_path)])
    torch.manual_seed(0)
    model = modeling.build_model(cfg)
    _randomize_bn(model, 5, data[3])
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) >= 30
    stats0 = [(m.running_mean.clone(), m.running_var.clone()) for m in bns]
    affine0 = [(m.weight.detach().clone(), m.bias.detach().clone()) for m in bns]
    tests = []

    def do_test(cfg_, model_, iteration=None, storage=None):
        model_.eval()
        with torch.no_grad():
            out = model_([{k: v for k, v in d.items() if k != "instances"} for d in data[0]])
        assert len(out) == len(data[0])
        tests.append(iteration)

    ok = solver.do_train(cfg, model, itertools.cycle(data), resume=False, world_size=1, rank=0, do_test=do_test,
                         check_period=1)
    assert ok and tests == [3], tests
    assert all(not m.training for m in bns), "freeze_bn is re-applied after the evaluation"
    import json
    lines = [json.loads(l) for l in open(tmp_path / "metrics.json")]
    assert len(lines) == 6 and all(l["total_loss"] == l["total_loss"] and abs(l["total_loss"]) < 1e4 for l in lines), lines
    for m, (a, b) in zip(bns, stats0):
        assert torch.equal(m.running_mean, a) and torch.equal(m.running_var, b)
    moved = sum(int(not torch.equal(m.weight.detach(), g0) and not torch.equal(m.bias.detach(), b0))
                for m, (g0, b0) in zip(bns, affine0))
    assert moved >= len(bns) // 2, (moved, len(bns))


# ---------------------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------------------
PROG = r'''
import hashlib, importlib, sys, torch
sys.path.insert(0, %r)
bt = importlib.import_module("bench_train")
d2 = importlib.import_module("3dod_amd.d2lite")
dev = torch.device("cuda:0")
cfg, model, opt, syn, solver = bt.build(dev, seed=3)
bn = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
for m in bn:
    m.momentum = 1.0                      # running statistics of real activations (a trained trunk's), then frozen
with torch.no_grad():
    model.backbone(model.preprocess_image(syn.make_batch(2, 39, with_gt=False))[1])
for m in bn:
    m.momentum = 0.1
stats = [(m.running_mean.clone(), m.running_var.clone()) for m in bn]
solver.freeze_bn(model)
step = solver.TrainStep(cfg, model, opt, world_size=1)
with d2.EventStorage(0):
    for i in range(3):
        torch.manual_seed(100 + i)
        step(syn.make_batch(2, 40 + i))
    rep = step.report()
torch.cuda.synchronize()
assert all(torch.equal(m.running_mean, a) and torch.equal(m.running_var, b) for m, (a, b) in zip(bn, stats))
print("HASH", hashlib.sha256(opt.flat_p.cpu().numpy().tobytes()).hexdigest(), rep["total_loss"], rep["iterations_explode"])
''' % ROOT


def _run_det():
    env = dict(os.environ, CR_DETERMINISTIC="1", CR_GRAPHS="none")
    out = subprocess.run([sys.executable, "-c", PROG], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    line = [l for l in out.stdout.splitlines() if l.startswith("HASH")]
    assert line, out.stderr[-2000:]
    _, h, loss, bad = line[-1].split()
    return h, float(loss), float(bad)


def test_frozen_deterministic_mode_is_bit_reproducible():
    a = _run_det()
    b = _run_det()
    assert a[2] == 0 and b[2] == 0 and a[1] == a[1]
    assert a[0] == b[0], "frozen-BatchNorm parameters after three steps differ between two deterministic runs"
