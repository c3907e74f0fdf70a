"""Every dense-region convolution of the benchmarked train step (DLA34 trunk, FPN, RPN head at 4 x 512^2, float32) at the
step's own shapes, against float64, in both float32-accurate modes ("fp32" and "fp32x3").

The shapes are not typed in: `census` wraps the public entry points of hipops for one forward of the default model on the
device and records every distinct call, so that the host code picks the same kernel, tile shape and split count here as in
the step.  Floors on the census keep a broken wrapper from making the file vacuous.

Checks, per census configuration:
  raw directions   conv_fwd_raw / conv_bwd_data_raw / conv_bwd_weight_raw (+ the fused bias gradient), accumulating into a
                   gradient sink as the step does, each held element-wise to tests/f64_bound.py's bound;
  module level     conv_bn_act and root_conv_bn_act with autograd against float64 autograd of oracle/torch_ref.conv_bn_act,
                   the ReLU mask of the float64 backward taken from the GPU's own output (so mask flips at a pre-activation
                   of ~0 are not compared, and dx needs no L2 escape hatch).  Tolerances, max-norm relative to the
                   reference: y 2e-5, every gradient, running_mean and running_var 1e-4 (those of test_gpu_convops_f32.py);
  groups           both five-level 3x3 groups through conv_bias_act_group, forward, input gradients and weight / bias
                   gradients into the sinks, once with the default plan (Winograd on the big levels, the direct grouped
                   kernel on the small ones) and once with CR_WINOGRAD=0 (the direct grouped route); the Winograd levels
                   are held to the Winograd form of the bound (f64_bound.wino_fwd);
  glue             max-pool, 1x1 subsample and upsample-add with their backwards: bit-exact against float32 ATen where one
                   rounding (or none) is involved, the 4-term sum of upsample-add's backward within 2 ulp of float64.

The float64 references run on the device as plain ATen convolutions (never this project's kernels; MIOpen is switched off
so that ATen's own implementation runs): on 16 CPU threads they would take several minutes for the 4 x 512^2 shapes.  Each
is computed once and shared by both precisions (module-scoped cache); only the module-level backward depends on the mask of
the precision under test and is recomputed."""
import importlib
import inspect
import math
import time
import zlib

import pytest
import torch
import torch.nn.functional as F

import f64_bound as B
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dod_amd.hipops")
DEV = torch.device("cuda:0")
f32, f64 = torch.float32, torch.float64
CENSUS_OPS = ("conv_bn_act", "root_conv_bn_act", "conv_bias_act", "conv_bias_act_group", "maxpool2x2", "subsample2x",
              "upsample2x_add")
TOL_Y, TOL_GRAD = 2e-5, 1e-4


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def relerr(got, ref):
    got = got.to(ref.device, f64)
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def _key(name, args):
    """the distinct-configuration key of one call (shapes and flags only)"""
    a = args
    if name == "conv_bn_act":
        return (tuple(a["x"].shape), tuple(a["weight"].shape), int(a["stride"]), int(a["pad"]), bool(a["relu"]),
                a["residual"] is not None, bool(a["x"].requires_grad))
    if name == "root_conv_bn_act":
        ch = list(a["children"])
        return (tuple(ch[0].shape[:3]), tuple(c.shape[3] for c in ch), tuple(a["weight"].shape), bool(a["relu"]))
    if name == "conv_bias_act":
        return (tuple(a["x"].shape), tuple(a["weight"].shape), int(a["stride"]), int(a["pad"]), bool(a["relu"]),
                a["bias"] is not None, bool(a["x"].requires_grad))
    if name == "conv_bias_act_group":
        ws = list(a["weights"])
        return (tuple(tuple(x.shape) for x in a["xs"]), tuple(ws[0].shape), int(a["pad"]), bool(a["relu"]),
                all(w is ws[0] for w in ws), bool(a.get("stacked", False)), all(b is not None for b in a["biases"]))
    if name == "upsample2x_add":
        return tuple(a["lat"].shape)
    return tuple(a["x"].shape)


def take_census(mod, run):
    """call run() with the CENSUS_OPS of `mod` wrapped; -> name -> list of distinct keys in first-call order.  Calls made
    from inside a wrapped entry point (a fallback of one onto another) are not counted; every wrapper is restored."""
    rec = {n: [] for n in CENSUS_OPS}
    orig = {n: getattr(mod, n) for n in CENSUS_OPS}
    depth = [0]

    def wrap(name):
        f, sig = orig[name], inspect.signature(orig[name])

        def w(*a, **k):
            if depth[0] == 0:
                ba = sig.bind(*a, **k)
                ba.apply_defaults()
                key = _key(name, ba.arguments)
                if key not in rec[name]:
                    rec[name].append(key)
            depth[0] += 1
            try:
                return f(*a, **k)
            finally:
                depth[0] -= 1
        return w
    try:
        for n in CENSUS_OPS:
            setattr(mod, n, wrap(n))
        run()
    finally:
        for n, f in orig.items():
            setattr(mod, n, f)
    return rec


@pytest.fixture(scope="module")
def census():
    bt = importlib.import_module("bench_train")
    prev = ops.set_precision("fp32")
    try:
        cfg, model, opt, syn, solver = bt.build(DEV, seed=0)
        batch = syn.make_batch(4, 3, with_gt=False)
        pg = model.proposal_generator

        def run():
            images, x = model.preprocess_image(batch)
            assert tuple(x.shape[:3]) == (4, 512, 512)
            feats = model.backbone(x)
            pg.rpn_head([feats[f] for f in pg.in_features])
        model.train()
        rec = take_census(ops, run)
        torch.cuda.synchronize()
    finally:
        ops.set_precision(prev)
    del model, opt
    torch.cuda.empty_cache()
    for n in CENSUS_OPS:
        assert getattr(ops, n).__module__ == ops.__name__ and not hasattr(getattr(ops, n), "__wrapped__"), n
    return rec


@pytest.fixture(scope="module")
def refs():
    """the module-scoped cache of inputs and float64 references, shared by both precisions"""
    prev = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    yield {}
    torch.backends.cudnn.enabled = prev


@pytest.fixture(params=["fp32", "fp32x3"])
def mode(request):
    prev = ops.set_precision(request.param)
    yield request.param
    ops.set_precision(prev)


def _gen(key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, generator=g, device=DEV) * scale


def _weight(co, ci, k, g):
    return _randn((co, ci, k, k), g, (2.0 / (k * k * ci)) ** 0.5).contiguous(memory_format=torch.channels_last)


def _print_table(title, rows):
    print(f"\n{title}: {len(rows)} checks")
    for r in rows:
        print("  " + "  ".join(str(v) for v in r))


def test_census_floors(census):
    n = {k: len(v) for k, v in census.items()}
    print("\ncensus (distinct configurations):", n)
    for k, v in census.items():
        for key in v:
            print(f"  {k}: {key}")
    # distinct (shape, stride, pad, ReLU, residual) configurations of one forward of the default model: 19 conv+BN
    # (stem, blocks with and without residual, stride-2 transitions, 1x1 projects) + 6 Root concatenations
    assert n["conv_bn_act"] >= 19 and n["conv_bn_act"] + n["root_conv_bn_act"] >= 25, n
    assert n["root_conv_bn_act"] == 6, n
    groups = census["conv_bias_act_group"]
    assert len(groups) == 2 and all(len(g[0]) == 5 for g in groups), groups
    assert all(sorted(s[1] for s in g[0]) == [8, 16, 32, 64, 128] for g in groups), "levels 128^2 .. 8^2"
    assert any(g[4] for g in groups) and any(not g[4] for g in groups), "one shared-weight group (RPN), one per-level (FPN)"
    # FPN laterals 1x1 64/128/256/512 -> 256 at five maps and the RPN predictors (one stacked map, or one per level)
    assert n["conv_bias_act"] >= 6 and n["upsample2x_add"] == 4 and n["maxpool2x2"] == 4 and n["subsample2x"] >= 1, n
    assert any(k[0][0] == 4 and k[0][1] == 512 for k in census["conv_bn_act"]), "the 4 x 512^2 stem is in the census"


# ---------------------------------------------------------------------------------------------------------------------
# raw directions
# ---------------------------------------------------------------------------------------------------------------------
def _raw_cases(census):
    """(x shape NHWC, w shape, stride, pad, relu, bias, needs dx, BN statistics) of every census convolution; a Root is the
    1x1 convolution of its concatenation"""
    out = []
    for (xs, ws, st, pd, relu, res, rg) in census["conv_bn_act"]:
        out.append(("conv_bn", xs, ws, st, pd, False, False, rg, True))
    for (nhw, ch, ws, relu) in census["root_conv_bn_act"]:
        out.append(("root", nhw + (sum(ch),), ws, 1, 0, False, False, True, True))
    for (xs, ws, st, pd, relu, has_b, rg) in census["conv_bias_act"]:
        out.append(("conv_bias", xs, ws, st, pd, relu, has_b, rg, False))
    seen, uniq = set(), []
    for c in out:
        if c[1:] not in seen:
            seen.add(c[1:])
            uniq.append(c)
    return uniq


def _raw_ref(refs, case):
    key = ("raw",) + case[1:]
    if key in refs:
        return refs[key]
    _, xs, ws, st, pd, relu, has_b, rg, _ = case
    g = _gen(key)
    N, H, W, Ci = xs
    Co, _, k, _ = ws
    Ho, Wo = (H + 2 * pd - k) // st + 1, (W + 2 * pd - k) // st + 1
    e = {"x": _randn(xs, g), "w": _weight(Co, Ci, k, g), "b": _randn((Co,), g, 0.1) if has_b else None,
         "dy": _randn((N, Ho, Wo, Co), g), "dw0": _randn(ws, g).contiguous(memory_format=torch.channels_last),
         "db0": _randn((Co,), g) if has_b else None}
    x64, dy64 = nchw(e["x"]).to(f64), nchw(e["dy"]).to(f64)
    y, ay, K = B.conv_fwd(x64, e["w"], e["b"], st, pd)
    e["fwd"] = ((y.relu() if relu else y), ay, K)
    if rg:
        e["dx"] = B.conv_bwd_data(dy64, e["w"], x64.shape, st, pd)
    d, ad, K = B.conv_bwd_weight(dy64, x64, ws, st, pd)
    e["dw"] = (d + e["dw0"].to(f64), ad + e["dw0"].to(f64).abs(), K)
    if has_b:
        d, ad, K = B.bias_grad(dy64)
        e["db"] = (d + e["db0"].to(f64), ad + e["db0"].to(f64).abs(), K)
    refs[key] = e
    return e


def test_raw_directions(census, refs, mode):
    """forward, backward-data and weight (+ bias) gradient of every census convolution on the raw entry points, as the
    autograd ops call them (BN-statistics epilogue for conv+BN layers, accumulation into a gradient sink)"""
    t0 = time.time()
    rows, fails, n_dir = [], [], 0
    for case in _raw_cases(census):
        kind, xs, ws, st, pd, relu, has_b, rg, stats = case
        e = _raw_ref(refs, case)
        Co, Ci, k, _ = ws
        wb, wt = ops.prepared_weights(e["w"], rg, f32)
        st_buf = None
        if stats:
            M = xs[0] * ((xs[1] + 2 * pd - k) // st + 1) * ((xs[2] + 2 * pd - k) // st + 1)
            st_buf = torch.empty(((M + 63) // 64, 2, Co), dtype=f32, device=DEV)
        got = {"fwd": nchw(ops.conv_fwd_raw(e["x"], wb, Co, k, st, pd, bias=e["b"], relu=relu, stats=st_buf))}
        if rg:
            got["dx"] = nchw(ops.conv_bwd_data_raw(e["dy"], wt, xs, k, st, pd))
        sink = e["dw0"].clone()
        bacc = e["db0"].clone() if has_b else None
        ops.conv_bwd_weight_raw(e["dy"], e["x"], k, st, pd, sink=sink, bias_acc=bacc)
        got["dw"] = sink
        if has_b:
            got["db"] = bacc
        torch.cuda.synchronize()
        for d, v in got.items():
            r = B.report(v, *e[d])
            n_dir += 1
            rows.append((kind, xs, ws, f"s{st}", d, f"K={r['K']}", f"ratio={r['ratio']:.3f}", f"norm={r['norm']:.2e}"))
            if r["bad"]:
                fails.append((kind, xs, ws, st, d, r))
    _print_table(f"[{mode}] raw directions, {len(_raw_cases(census))} configurations, {n_dir} directions, "
                 f"{time.time() - t0:.1f} s", rows)
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------
# conv + BN (+ residual) (+ ReLU) and Root with autograd
# ---------------------------------------------------------------------------------------------------------------------
def _bn_inputs(refs, key, xs, Cin_list, ws, Ho, Wo, has_res):
    if key in refs:
        return refs[key]
    g = _gen(key)
    Co, Ci, k, _ = ws
    e = {"xs": [_randn(xs[:3] + (c,), g) for c in Cin_list], "w": _weight(Co, Ci, k, g), "gamma": _randn((Co,), g).abs() + 0.5,
         "beta": _randn((Co,), g, 0.1), "res": _randn((xs[0], Ho, Wo, Co), g) if has_res else None,
         "dy": _randn((xs[0], Ho, Wo, Co), g)}
    refs[key] = e
    return e


def _bn_module_check(e, st, pd, relu, rg, run_gpu):
    """run the GPU op, then float64 autograd of torch_ref.conv_bn_act on the same inputs with the GPU's ReLU mask; -> the
    max-norm relative errors per tensor"""
    Co = e["w"].shape[0]
    xd = [x.clone().requires_grad_(rg) for x in e["xs"]]
    wd = e["w"].clone(memory_format=torch.channels_last).requires_grad_(True)
    gd, bd = e["gamma"].clone().requires_grad_(True), e["beta"].clone().requires_grad_(True)
    rd = e["res"].clone().requires_grad_(True) if e["res"] is not None else None
    rm, rv = torch.zeros(Co, device=DEV), torch.ones(Co, device=DEV)
    y = run_gpu(xd, wd, gd, bd, rd, rm, rv)
    y.backward(e["dy"])
    torch.cuda.synchronize()
    # float64
    x64 = [nchw(x).to(f64).requires_grad_(rg) for x in e["xs"]]
    w64, g64, b64 = [t.detach().to(f64).requires_grad_(True) for t in (e["w"], e["gamma"], e["beta"])]
    r64 = nchw(e["res"]).to(f64).requires_grad_(True) if e["res"] is not None else None
    rm64, rv64 = torch.zeros(Co, device=DEV, dtype=f64), torch.ones(Co, device=DEV, dtype=f64)
    xc = torch.cat(x64, 1) if len(x64) > 1 else x64[0]
    z = F.batch_norm(F.conv2d(xc, w64, None, st, pd), rm64, rv64, g64, b64, True, 0.1, 1e-5)
    if r64 is not None:
        z = z + r64
    # R.conv_bn_act is this without the ReLU; the mask is the GPU's (see the module docstring)
    y64 = z * (nchw(y.detach()) > 0).to(f64) if relu else z
    y64.backward(nchw(e["dy"]).to(f64))
    err = {"y": relerr(nchw(y.detach()), y64.detach()), "dw": relerr(wd.grad, w64.grad), "dgamma": relerr(gd.grad, g64.grad),
           "dbeta": relerr(bd.grad, b64.grad), "running_mean": relerr(rm, rm64), "running_var": relerr(rv, rv64)}
    if rg:
        for i, (a, b) in enumerate(zip(xd, x64)):
            err[f"dx{i}" if len(xd) > 1 else "dx"] = relerr(nchw(a.grad), b.grad)
    if rd is not None:
        err["dres"] = relerr(nchw(rd.grad), r64.grad)
    return err


def _bn_assert(err):
    return {k: v for k, v in err.items() if v > (TOL_Y if k == "y" else TOL_GRAD)}


def test_reference_conv_bn_is_torch_ref():
    """the float64 expression of _bn_module_check (without the ReLU) is oracle/torch_ref.conv_bn_act"""
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(2, 8, 6, 6, generator=g, dtype=f64), torch.randn(4, 8, 3, 3, generator=g, dtype=f64)
    ga, be, r = torch.rand(4, generator=g, dtype=f64) + 0.5, torch.randn(4, generator=g, dtype=f64), torch.randn(2, 4, 6, 6, generator=g, dtype=f64)
    z = F.batch_norm(F.conv2d(x, w, None, 1, 1), None, None, ga, be, True, 0.1, 1e-5) + r
    assert torch.equal(F.relu(z), R.conv_bn_act(x, w, ga, be, 1, 1, True, r))


def test_conv_bn_act_module(census, refs, mode):
    t0 = time.time()
    rows, fails = [], []
    for key in census["conv_bn_act"]:
        xs, ws, st, pd, relu, has_res, rg = key
        Co, Ci, k, _ = ws
        Ho, Wo = (xs[1] + 2 * pd - k) // st + 1, (xs[2] + 2 * pd - k) // st + 1
        e = _bn_inputs(refs, ("bn",) + key, xs, [Ci], ws, Ho, Wo, has_res)
        run = lambda xd, wd, gd, bd, rd, rm, rv: ops.conv_bn_act(xd[0], wd, gd, bd, rm, rv, st, pd, relu, rd)
        err = _bn_module_check(e, st, pd, relu, rg, run)
        rows.append((xs, ws, f"s{st}", "relu" if relu else "", "res" if has_res else "",
                     " ".join(f"{k}={v:.1e}" for k, v in err.items())))
        if _bn_assert(err):
            fails.append((key, _bn_assert(err)))
    _print_table(f"[{mode}] conv_bn_act module, {len(rows)} configurations, {time.time() - t0:.1f} s "
                 f"(tolerances y {TOL_Y}, gradients / running statistics {TOL_GRAD})", rows)
    assert not fails, fails


def test_root_conv_bn_act_module(census, refs, mode):
    rows, fails = [], []
    for key in census["root_conv_bn_act"]:
        nhw, ch, ws, relu = key
        e = _bn_inputs(refs, ("root",) + key, nhw + (sum(ch),), list(ch), ws, nhw[1], nhw[2], False)
        run = lambda xd, wd, gd, bd, rd, rm, rv: ops.root_conv_bn_act(xd, wd, gd, bd, rm, rv, relu=relu)
        err = _bn_module_check(e, 1, 0, relu, True, run)
        assert sum(1 for k in err if k.startswith("dx")) == len(ch), "a gradient for every child"
        rows.append((nhw, ch, ws, " ".join(f"{k}={v:.1e}" for k, v in err.items())))
        if _bn_assert(err):
            fails.append((key, _bn_assert(err)))
    _print_table(f"[{mode}] root_conv_bn_act module, {len(rows)} concatenations", rows)
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------
# the two five-level 3x3 groups
# ---------------------------------------------------------------------------------------------------------------------
def _group_ref(refs, key):
    if ("group",) + key in refs:
        return refs[("group",) + key]
    shapes, ws, pad, relu, shared, stacked, has_b = key
    g = _gen(key)
    O, Ci, k, _ = ws
    n = len(shapes)
    nw = 1 if shared else n
    e = {"xs": [_randn(s, g) for s in shapes], "w": [_weight(O, Ci, k, g) for _ in range(nw)],
         "b": [_randn((O,), g, 0.1) for _ in range(nw)] if has_b else [None] * nw,
         "dw0": [_randn(ws, g).contiguous(memory_format=torch.channels_last) for _ in range(nw)],
         "db0": [_randn((O,), g) for _ in range(nw)]}
    wi = (lambda i: 0) if shared else (lambda i: i)
    e["wi"] = [wi(i) for i in range(n)]
    lv = []
    for i, x in enumerate(e["xs"]):
        x64 = nchw(x).to(f64)
        w, b = e["w"][wi(i)], e["b"][wi(i)]
        y, ay, K = B.conv_fwd(x64, w, b, 1, pad)
        ayw = B.wino_fwd(x64, w, b, absval=True)
        dy = _randn(x.shape[:3] + (O,), g)
        if relu:
            # the upstream gradient is zeroed where the sign of the pre-activation is within the (Winograd) forward bound:
            # there a float32 route may put the ReLU either way, anywhere else it must agree with float64 -- so the
            # masked gradient below is the same for every route and precision, and can be shared
            amb = y.abs() <= B.C * B.U * math.sqrt(Ci * 9 + B.WINO_DEPTH) * ayw
            dy = dy * ~nhwc(amb)
            y = y.relu()
        g64 = nchw(dy).to(f64) * ((y > 0).to(f64) if relu else 1.0)
        dx = B.conv_bwd_data(g64, w, x64.shape, 1, pad)
        d = {"x64": x64, "dy": dy, "g64": g64, "y": (y, ay, K), "y_w": (y, ayw, Ci + B.WINO_DEPTH), "dx": dx,
             "dx_w": (dx[0], B.wino_bwd_data(g64, w, absval=True), O + B.WINO_DEPTH)}
        lv.append(d)
    e["lv"] = lv
    # weight / bias gradients per parameter: direct form summed over the levels it serves, and the Winograd magnitudes
    e["dw"], e["db"] = [], []
    for j in range(nw):
        mine = [d for i, d in enumerate(lv) if wi(i) == j]
        parts = [B.conv_bwd_weight(d["g64"], d["x64"], ws, 1, pad) for d in mine]
        ref = sum(p[0] for p in parts) + e["dw0"][j].to(f64)
        absd = sum(p[1] for p in parts) + e["dw0"][j].to(f64).abs()
        absw = sum(B.wino_wgrad(d["g64"], d["x64"], absval=True) for d in mine) + e["dw0"][j].to(f64).abs()
        Kd = sum(p[2] for p in parts)
        Kw = sum(B.wino_tiles(d["g64"]) for d in mine) + B.WINO_DEPTH
        e["dw"].append({"direct": (ref, absd, Kd), "wino": (ref, absw, Kw)})
        bp = [B.bias_grad(d["g64"]) for d in mine]
        e["db"].append((sum(p[0] for p in bp) + e["db0"][j].to(f64), sum(p[1] for p in bp) + e["db0"][j].to(f64).abs(),
                        sum(p[2] for p in bp)))
    refs[("group",) + key] = e
    return e


@pytest.mark.parametrize("route", ["default", "direct"])
def test_conv_bias_act_group(census, refs, mode, route, monkeypatch):
    """default: the step's own plan (fp32: Winograd on the levels with >= WINO_MIN_TILES tiles, or on all levels at once
    when they share the weight; the direct grouped kernel on the rest).  direct: CR_WINOGRAD=0, the direct grouped kernels
    in all three directions.  (fp32x3 has no grouped or Winograd route: both runs take its per-level convolutions.)"""
    if route == "direct":
        monkeypatch.setenv("CR_WINOGRAD", "0")
    t0 = time.time()
    rows, fails, plans = [], [], []
    for key in census["conv_bias_act_group"]:
        shapes, ws, pad, relu, shared, stacked, has_b = key
        e = _group_ref(refs, key)
        n, O = len(shapes), ws[0]
        wts = [w.clone(memory_format=torch.channels_last).requires_grad_(True) for w in e["w"]]
        bts = [None if b is None else b.clone().requires_grad_(True) for b in e["b"]]
        for j, w in enumerate(wts):
            w._cr_grad = e["dw0"][j].clone()
            if bts[j] is not None:
                bts[j]._cr_grad = e["db0"][j].clone()
        xd = [x.clone().requires_grad_(True) for x in e["xs"]]
        wl, bl = [wts[j] for j in e["wi"]], [bts[j] for j in e["wi"]]
        plan = ops._wino_plan(xd, wl, bl, 3, pad)
        plans.append(plan)
        wino = [plan == "shared" or plan[i] for i in range(n)]
        stk = stacked and ops.group_supported(xd, wl)
        out = ops.conv_bias_act_group(xd, wl, bl, pad=pad, relu=relu, stacked=stk)
        if stk:
            ys, off, flat = [], 0, out.view(-1, O)
            for s in shapes:
                m = s[0] * s[1] * s[2]
                ys.append(flat[off:off + m].view(s[:3] + (O,)))
                off += m
            out.backward(torch.cat([d["dy"].reshape(-1, O) for d in e["lv"]]).view(out.shape))
        else:
            ys = out
            torch.autograd.backward(ys, [d["dy"] for d in e["lv"]])
        torch.cuda.synchronize()
        tag = ("shared" if shared else "per-level") + (" relu" if relu else "") + (" stacked" if stk else "")
        for i, d in enumerate(e["lv"]):
            for name, got, ref in (("y", nchw(ys[i]), d["y_w" if wino[i] else "y"]), ("dx", nchw(xd[i].grad), d["dx_w" if wino[i] else "dx"])):
                r = B.report(got, *ref)
                rows.append((tag, shapes[i], "wino" if wino[i] else "direct", name, f"K={r['K']}", f"ratio={r['ratio']:.3f}",
                             f"norm={r['norm']:.2e}"))
                if r["bad"]:
                    fails.append((tag, shapes[i], name, r))
        for j, w in enumerate(wts):
            assert w.grad is None, "weight gradient goes to the sink"
            lvls = [i for i in range(n) if e["wi"][i] == j]
            form = "wino" if all(wino[i] for i in lvls) and ops.wino_wgrad_on() else "direct"
            assert form == "direct" or all(wino[i] for i in lvls)
            checks = [("dW", w._cr_grad, e["dw"][j][form])]
            if bts[j] is not None:
                checks.append(("db", bts[j]._cr_grad, e["db"][j]))
            for name, got, ref in checks:
                r = B.report(got, *ref)
                rows.append((tag, f"param {j} ({len(lvls)} levels)", form, name, f"K={r['K']}", f"ratio={r['ratio']:.3f}",
                             f"norm={r['norm']:.2e}"))
                if r["bad"]:
                    fails.append((tag, j, name, r))
    _print_table(f"[{mode}/{route}] conv_bias_act_group, plans {plans}, {time.time() - t0:.1f} s", rows)
    if mode == "fp32":
        per_level = [p for p in plans if p != "shared"]
        if route == "default":
            assert "shared" in plans and any(any(p) and not all(p) for p in per_level), ("the mixed plan of the step", plans)
        else:
            assert all(p != "shared" and not any(p) for p in plans), plans
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------
# pooling / upsample glue
# ---------------------------------------------------------------------------------------------------------------------
def _ulp(x):
    """spacing of float32 at |x| (float64 tensor)"""
    a = x.abs().to(f32).clamp_min(torch.finfo(f32).tiny)
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).to(f64)


def test_glue(census, mode):
    n = 0
    for name, window in (("maxpool2x2", 2), ("subsample2x", 1)):
        for xs in census[name]:
            g = _gen((name, xs))
            # distinct values (integers, exact in float32): no ties, so the arg-max of every window is unique
            n_el = math.prod(xs)
            assert n_el <= 2 ** 24
            x = (torch.randperm(n_el, generator=g, device=DEV).to(f32) - n_el // 2).view(xs).requires_grad_(True)
            y = getattr(ops, name)(x)
            dy = _randn(y.shape, g)
            y.backward(dy)
            xr = nchw(x.detach()).clone().requires_grad_(True)
            yr = F.max_pool2d(xr, window, 2)
            yr.backward(nchw(dy))
            assert torch.equal(nchw(y.detach()), yr.detach()), (name, xs)
            assert torch.equal(nchw(x.grad), xr.grad), (name, xs, "backward")
            n += 1
    for ls in census["upsample2x_add"]:
        g = _gen(("upsample2x_add", ls))
        lat = _randn(ls, g).requires_grad_(True)
        top = _randn((ls[0], ls[1] // 2, ls[2] // 2, ls[3]), g).requires_grad_(True)
        y = ops.upsample2x_add(lat, top)
        dy = _randn(ls, g)
        y.backward(dy)
        assert torch.equal(nchw(y.detach()), R.upsample2x_add(nchw(lat.detach()), nchw(top.detach()))), ls
        assert torch.equal(lat.grad, dy), (ls, "lateral gradient")
        d64 = nchw(dy).to(f64)
        # three float32 additions, each off by at most half an ulp of a partial sum, and no partial sum exceeds the sum of
        # the magnitudes: within 2 ulp of that
        ref, mag = F.avg_pool2d(d64, 2) * 4, F.avg_pool2d(d64.abs(), 2) * 4
        err = (nchw(top.grad).to(f64) - ref).abs()
        assert bool((err <= 2 * _ulp(mag)).all()), (ls, "4-term sum off by more than 2 ulp", float((err / _ulp(mag)).max()))
        n += 1
    print(f"\n[{mode}] glue: {n} census shapes, forward and backward")
    assert n >= 7
