"""GPU: FPN(norm="GN") and the whole model of configs/cubercnn_DLA34_FPN_GN.yaml on the GroupNorm kernels.

detectron2 is absent, so the module's structure is restated from its public definition ("parity unpinned" w.r.t. detectron2)
and pinned by the ratio method of tests/test_gpu_mnasnet.py: a float64 restatement from plain functionals over the module's own
state dict is the reference; the same restatement in float32 on the CPU gives `ref32_err`; the product must stay within
K_FWD * ref32_err (outputs) and K_GRAD * ref32_err (gradients of the inputs and of every parameter under a random cotangent),
the constants of tests/test_gpu_dla_types.py.  bf16: the yardstick is the float32 restatement with the roundings of the bf16 mode
written in (conv weights, every stored map forward, their gradients on the way back: a straight-through rounding), as
tests/test_gpu_resnet_bottleneck.py builds it.  Every ratio is printed.

norm="" must keep the bits of the composition of conv_bias_act / upsample2x_add / conv_bias_act_group it has always been.

Measured on MI355X (ratio = error / ref32_err): GN outputs 1.62 .. 1.81, input gradients at most 1.99, parameter gradients at most
1.96 in f32, the same with gradient sinks; bf16 0.99 .. 1.01; norm "" outputs 1.53 .. 1.79."""
import importlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
K_FWD = 2.966          # tests/test_gpu_dla_types.py
K_GRAD = 2.31
MAPS = {"c2": (2, 16, 16, 64), "c3": (2, 8, 8, 128), "c4": (2, 4, 4, 256), "c5": (2, 2, 2, 512)}   # the stub trunk's maps
OUTS = ("p2", "p3", "p4", "p5", "p6")


def _mods():
    return (importlib.import_module("3dod_amd.cubercnn.modeling.backbone.fpn"), importlib.import_module("3dod_amd.hipops"))


def _stub(fpn_mod):
    class Stub(fpn_mod.Backbone):
        def __init__(self):
            super().__init__()
            self._out_features = list(MAPS)
            self._out_feature_channels = {k: s[3] for k, s in MAPS.items()}
            self._out_feature_strides = {k: 2 ** (i + 2) for i, k in enumerate(MAPS)}
            self.maps = None

        def forward(self, x):
            return self.maps
    return Stub()


def _make_fpn(norm, fuse, seed=0):
    fpn_mod, ops = _mods()
    torch.manual_seed(seed)
    fpn = fpn_mod.FPN(_stub(fpn_mod), list(MAPS), 256, norm=norm, top_block=fpn_mod.LastLevelMaxPool(), fuse_type=fuse)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in fpn.named_parameters():
            if ".norm.weight" in n:                      # away from (1, 0)
                p.copy_(1.0 + 0.4 * torch.randn(p.shape, generator=gen))
            elif ".norm.bias" in n or n.endswith(".bias"):
                p.copy_(0.3 * torch.randn(p.shape, generator=gen))
    return fpn.to(DEV)


def _data(dtype, seed=7):
    gen = torch.Generator().manual_seed(seed)
    exact = (lambda t: t.to(bf16).to(f32)) if dtype == bf16 else (lambda t: t)
    maps = {k: exact(torch.randn(s, generator=gen)) for k, s in MAPS.items()}                  # NHWC
    cots = {"p2": (2, 16, 16), "p3": (2, 8, 8), "p4": (2, 4, 4), "p5": (2, 2, 2), "p6": (2, 1, 1)}
    cots = {k: exact(torch.randn(s + (256,), generator=gen)) for k, s in cots.items()}
    return maps, cots


class _Rt(torch.autograd.Function):
    """straight-through bf16 rounding of a tensor and of its gradient: what storing it in bf16 does in both directions"""

    @staticmethod
    def forward(ctx, t):
        return t.to(bf16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(bf16).to(g.dtype)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _restate(sd, maps, cots, norm, fuse, dt, emulate):
    """the FPN from plain functionals on the CPU -> (outputs, input gradients, parameter gradients), NHWC / state-dict keys"""
    rt = _Rt.apply if emulate else (lambda t: t)
    P = {k: v.detach().cpu().to(dt).contiguous().requires_grad_() for k, v in sd.items()}
    xs = {k: _nchw(v).to(dt).requires_grad_() for k, v in maps.items()}

    def conv_norm(name, x, pad):
        t = rt(F.conv2d(x, rt(P[name + ".weight"]), P.get(name + ".bias"), padding=pad))
        if norm == "GN":
            t = rt(F.group_norm(t, 32, P[name + ".norm.weight"], P[name + ".norm.bias"], 1e-5))
        return t

    prev = conv_norm("fpn_lateral5", xs["c5"], 0)
    inner = [prev]
    for s in (4, 3, 2):
        lat = conv_norm("fpn_lateral%d" % s, xs["c%d" % s], 0)
        prev = rt(lat + F.interpolate(prev, scale_factor=2, mode="nearest"))
        if fuse == "avg":
            prev = prev / 2
        inner.append(prev)
    outs = [conv_norm("fpn_output%d" % s, t, 1) for s, t in zip((5, 4, 3, 2), inner)][::-1]
    outs.append(F.max_pool2d(outs[-1], kernel_size=1, stride=2, padding=0))
    loss = sum((o * _nchw(cots[k]).to(dt)).sum() for k, o in zip(OUTS, outs))
    names = list(P)
    grads = torch.autograd.grad(loss, [xs[k] for k in MAPS] + [P[k] for k in names])
    gx = {k: _nhwc(g) for k, g in zip(MAPS, grads[:4])}
    gp = dict(zip(names, grads[4:]))
    return {k: _nhwc(o.detach()) for k, o in zip(OUTS, outs)}, gx, gp


def _product(fpn, maps, cots, dtype, sinks=False):
    fpn_mod, ops = _mods()
    leaves = {k: v.to(DEV, dtype).requires_grad_() for k, v in maps.items()}
    fpn.bottom_up.maps = leaves
    params = dict(fpn.named_parameters())
    bufs = {}
    if sinks:
        for n, p in params.items():
            bufs[n] = torch.full(p.shape, 0.5, device=DEV).contiguous(memory_format=torch.channels_last) if p.dim() == 4 \
                else torch.full(p.shape, 0.5, device=DEV)
            p._cr_grad = bufs[n]
    try:
        def run():
            outs = fpn(None)
            assert list(outs) == list(OUTS)
            loss = sum((outs[k].float() * cots[k].to(DEV)).sum() for k in OUTS)
            return outs, torch.autograd.grad(loss, list(leaves.values()) + list(params.values()), allow_unused=True)
        if sinks:
            with ops.deferred_wgrad():
                outs, grads = run()
            assert ops.wgrad_pending() == 0
            assert all(g is None for g in grads[4:]), "a parameter with a sink still got an autograd gradient"
            gp = {n: bufs[n] - 0.5 for n in params}
        else:
            outs, grads = run()
            gp = dict(zip(params, grads[4:]))
    finally:
        for p in params.values():
            if hasattr(p, "_cr_grad"):
                del p._cr_grad
    torch.cuda.synchronize()
    return {k: v.detach() for k, v in outs.items()}, dict(zip(MAPS, grads[:4])), gp


def _rel(got, ref):
    got, ref = got.detach().to("cpu", f64), ref.detach().to("cpu", f64)
    return float((got - ref).norm() / (ref.norm() + 1e-300))


_REFS = {}


def _refs(norm, fuse, dtype):
    """float64 reference and float32 yardstick, computed once per case and shared"""
    key = (norm, fuse, dtype)
    if key not in _REFS:
        fpn = _make_fpn(norm, fuse)
        maps, cots = _data(dtype)
        sd = fpn.state_dict()
        _REFS[key] = (fpn, maps, cots, _restate(sd, maps, cots, norm, fuse, f64, False),
                      _restate(sd, maps, cots, norm, fuse, f32, dtype == bf16))
    return _REFS[key]


def _check(tag, got, ref64, yard, sinks=False, parts=(0, 1, 2)):
    worst = 0.0
    for part, K in ((0, K_FWD), (1, K_GRAD), (2, K_GRAD)):
        if part not in parts:
            continue
        for k, ref in ref64[part].items():
            err, r32 = _rel(got[part][k], ref), _rel(yard[part][k], ref)
            # a sink holds 0.5 + g: subtracting costs up to 2^-24 * 0.5 per element on top of the gradient's own error
            floor = 2.0 ** -24 * 0.5 * (ref.numel() ** 0.5) / float(ref.norm()) if sinks and part == 2 else 0.0
            print("%s %s %s: error %.3g, ref32_err %.3g, ratio %.3f" % (tag, ("out", "dx", "grad")[part], k, err, r32,
                                                                        err / max(r32, 1e-300)))
            assert err <= K * r32 + floor, (tag, part, k, err, r32)
            worst = max(worst, err / max(r32, 1e-300))
    return worst


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fuse", ["sum", "avg"])
def test_fpn_gn_against_float64(fuse, dtype):
    fpn, maps, cots, ref64, yard = _refs("GN", fuse, dtype)
    got = _product(fpn, maps, cots, dtype)
    assert all(v.dtype == dtype for v in got[0].values())
    _check("fpn GN %s %s" % (fuse, dtype), got, ref64, yard)


def test_fpn_gn_with_gradient_sinks_and_deferred_weight_gradients():
    """the route the train step takes: every parameter has a gradient sink (the kernels accumulate, autograd sees None), inside
    deferred_wgrad() -- against the run without sinks and the same float64 reference"""
    fpn, maps, cots, ref64, yard = _refs("GN", "sum", f32)
    plain = _product(fpn, maps, cots, f32)
    got = _product(fpn, maps, cots, f32, sinks=True)
    _check("fpn GN sinks", got, ref64, yard, sinks=True)
    for k in MAPS:
        assert torch.equal(got[1][k], plain[1][k]), k
    for k, g in plain[2].items():
        if ".norm." in k:            # GroupNorm's parameter gradients: the same launches, 0.5 + g rounded once
            assert float((got[2][k] - g).abs().max()) <= 2.0 ** -23 * (0.5 + float(g.abs().max())), k


@pytest.mark.parametrize("fuse", ["sum", "avg"])
def test_fpn_without_norm_keeps_its_bits(fuse):
    """norm="": the forward is still conv_bias_act -> upsample2x_add -> one conv_bias_act_group, bit for bit"""
    fpn_mod, ops = _mods()
    fpn, maps, cots, ref64, yard = _refs("", fuse, f32)
    got = _product(fpn, maps, cots, f32)
    _check("fpn plain %s" % fuse, got, ref64, yard, parts=(0,))
    with torch.no_grad():
        x = {k: v.to(DEV) for k, v in maps.items()}
        lat = {s: getattr(fpn, "fpn_lateral%d" % s) for s in (2, 3, 4, 5)}
        out = {s: getattr(fpn, "fpn_output%d" % s) for s in (2, 3, 4, 5)}
        prev = ops.conv_bias_act(x["c5"], lat[5].weight, lat[5].bias, 1, 0)
        inner = [prev]
        for s in (4, 3, 2):
            prev = ops.upsample2x_add(ops.conv_bias_act(x["c%d" % s], lat[s].weight, lat[s].bias, 1, 0), prev)
            if fuse == "avg":
                prev = prev / 2
            inner.append(prev)
        ys = ops.conv_bias_act_group(inner, [out[s].weight for s in (5, 4, 3, 2)], [out[s].bias for s in (5, 4, 3, 2)], pad=1)[::-1]
        ys.append(ops.subsample2x(ys[-1]))
    for k, y in zip(OUTS, ys):
        assert torch.equal(got[0][k], y), k


# ---------------------------------------------------------------------------------------------------------------------
# the whole model: configs/cubercnn_DLA34_FPN_GN.yaml on 2 x 256^2 synthetic images
# ---------------------------------------------------------------------------------------------------------------------
def _build_model(seed=0):
    syn = importlib.import_module("3dod_amd.synthetic")
    modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
    solver = importlib.import_module("3dod_amd.cubercnn.solver")
    cfg = syn.make_cfg(os.path.join(ROOT, "configs", "cubercnn_DLA34_FPN_GN.yaml"),
                       overrides=["MODEL.DEVICE", "cuda:0", "VIS_PERIOD", 0, "log", False, "SOLVER.BASE_LR", 0.0025])
    torch.manual_seed(seed)
    model = modeling.build_model(cfg).to(DEV).train()
    opt = solver.build_optimizer(cfg, model)
    return cfg, model, opt, syn, solver


def _to_dev(batch):
    for d in batch:
        d["image"] = d["image"].to(DEV)
        d["instances"] = d["instances"].to(DEV)
    return batch


def test_gn_model_learns_and_infers():
    fpn_mod, ops = _mods()
    cfg, model, opt, syn, solver = _build_model()
    d2 = importlib.import_module("3dod_amd.d2lite")
    step = solver.TrainStep(cfg, model, opt, world_size=1)
    batch = syn.make_batch(2, 7, size=256)
    norm_params = [(n, p) for n, p in model.named_parameters() if ".norm." in n]
    assert len(norm_params) == 2 * (2 * len(model.backbone.lateral_convs) + 4)
    totals = []
    with d2.EventStorage(0):
        for i in range(8):
            step(batch)
            rep = step.report()
            totals.append(rep["total_loss"])
            if i == 0:                                      # the step leaves this iteration's gradient in the sinks
                for name, p in norm_params:
                    gbuf = ops.grad_sink(p)
                    assert gbuf is not None, name
                    assert bool(torch.isfinite(gbuf).all()), name
                    assert float(gbuf.abs().sum()) > 0.0, f"{name} received no gradient"
    print("GN totals", totals)
    assert all(t == t and abs(t) < 1e4 for t in totals), totals
    assert rep["iterations_explode"] == 0, rep
    assert min(totals[-3:]) < totals[0], totals
    # inference on the trained model, eager and through the forward-only graph
    model.eval()
    thr = model.roi_heads.box_predictor.test_score_thresh
    model.roi_heads.box_predictor.test_score_thresh = -1.0
    try:
        test_batch = syn.make_batch(2, 23, size=256, with_gt=False)
        with torch.no_grad():
            eager = model(test_batch)
            model.enable_graphs_eval(test_batch)
            graphed = model(test_batch)
        assert model._graphed_eval is not None
        for a, b in zip(eager, graphed):
            ia, ib = a["instances"], b["instances"]
            assert len(ia) == len(ib) > 0
            assert torch.allclose(ia.pred_boxes.tensor, ib.pred_boxes.tensor, atol=1e-3)
            assert torch.allclose(ia.scores, ib.scores, atol=1e-4) and torch.equal(ia.pred_classes, ib.pred_classes)
    finally:
        model._graphed_eval = None
        model.roi_heads.box_predictor.test_score_thresh = thr


def test_graphed_step_equals_eager_step(monkeypatch):
    """one step through solver.make_train_step (dense region replayed from HIP graphs) returns the losses of the eager step
    from the same state"""
    d2 = importlib.import_module("3dod_amd.d2lite")
    reports = {}
    for mode in ("none", "dense"):
        monkeypatch.setenv("CR_GRAPHS", mode)
        cfg, model, opt, syn, solver = _build_model(seed=0)
        step = solver.make_train_step(cfg, model, opt, world_size=1)
        batch = _to_dev(syn.make_batch(2, 11, size=256))
        torch.manual_seed(5)
        with d2.EventStorage(0):
            step(batch)
            reports[mode] = step.report()
        assert (model._graphed is not None) == (mode == "dense")
    eager, graph = reports["none"], reports["dense"]
    print("eager", eager, "\ngraphed", graph)
    assert eager["iterations_explode"] == 0 and graph["iterations_explode"] == 0
    keys = [k for k in eager if not k.startswith("iterations")]
    assert keys and set(keys) == set(k for k in graph if not k.startswith("iterations"))
    for k in keys:
        assert abs(graph[k] - eager[k]) <= 1e-6 * max(abs(eager[k]), 1e-30), (k, eager[k], graph[k])


def test_bf16_step_is_finite():
    fpn_mod, ops = _mods()
    d2 = importlib.import_module("3dod_amd.d2lite")
    prev = ops.set_precision("bf16")
    try:
        cfg, model, opt, syn, solver = _build_model()
        step = solver.TrainStep(cfg, model, opt, world_size=1)
        with d2.EventStorage(0):
            step(syn.make_batch(2, 7, size=256))
            rep = step.report()
        losses = {k: v for k, v in rep.items() if not k.startswith("iterations")}
        assert all(v == v and abs(v) < 1e4 for v in losses.values()), losses
    finally:
        ops.set_precision(prev)


# CR_DETERMINISTIC=1 is read once by the library, hence a child process: one train step from the same state twice
DET_PROG = r'''
import hashlib, importlib, sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
t = importlib.import_module("test_gpu_fpn_gn")
ops = importlib.import_module("3dod_amd.hipops")
d2 = importlib.import_module("3dod_amd.d2lite")
for run in range(2):
    cfg, model, opt, syn, solver = t._build_model(seed=0)
    step = solver.TrainStep(cfg, model, opt, world_size=1)
    with d2.EventStorage(0):
        step(syn.make_batch(2, 7, size=256))
        rep = step.report()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    n = 0
    for name, p in model.named_parameters():
        g = ops.grad_sink(p)
        if g is not None:
            h.update(g.contiguous().cpu().numpy().tobytes())
            n += ".norm." in name
        h.update(p.detach().contiguous().cpu().numpy().tobytes())
    print("HASH", h.hexdigest(), n, repr(rep["total_loss"]))
''' % (ROOT, os.path.join(ROOT, "tests"))


def test_deterministic_step_is_bit_reproducible():
    env = dict(os.environ, CR_DETERMINISTIC="1", CR_PRECISION="fp32")
    out = subprocess.run([sys.executable, "-c", DET_PROG], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    got = [l.split() for l in out.stdout.splitlines() if l.startswith("HASH")]
    assert len(got) == 2, out.stderr[-2000:]
    print(got)
    assert int(got[0][2]) == 28                               # every GroupNorm parameter has a gradient sink
    assert got[0][1:] == got[1][1:], "one train step differs between two runs in deterministic mode"
