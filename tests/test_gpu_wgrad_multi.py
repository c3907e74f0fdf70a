"""GPU: cr_conv2d_bwd_weight_multi (a queue of float32 weight gradients of mixed shapes, the eligible ones sharing grids of up to
8 problems) and the deferral queue in front of it (hipops.deferred_wgrad).

* default (atomic) mode: dW / dbias of one mixed queue against a float64 conv2d weight gradient on the CPU, with the tolerance of
  the solo f32 weight gradient (tests/test_gpu_convops_f32.py: 1e-4 of the tensor's scale, summation order only);
* CR_DETERMINISTIC=1 (read once by the library, hence a fresh child process): the grouped results are bitwise those of the same
  problems run one by one through cr_conv2d_bwd_weight[_bias], also when the slab workspace fills up and the group is cut, and
  bitwise equal between two processes;
* one DLA34 dense-region backward at 2 x 64 x 64 with the deferral on and off: bit-equal flat gradients in deterministic mode,
  nothing left in the queue, and an exception inside the context still launches what was queued."""
import contextlib
import hashlib
import importlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

# N, H, W, Cin, Cout, k, stride, pad, bias, shares dW (and dbias) with problem
MIXED = [
    (2, 12, 20, 64, 64, 3, 1, 1, False, None),      # 64-row tiles, 3x3
    (3, 10, 14, 64, 128, 1, 2, 0, False, None),     # 1x1 stride 2 (project), 105 output pixels: not a multiple of 16
    (1, 24, 40, 32, 64, 3, 2, 1, False, None),      # 3x3 stride 2, non-square
    (2, 16, 16, 64, 256, 3, 1, 1, True, None),      # 256 channels, with a bias gradient
    (2, 16, 16, 8, 16, 7, 1, 3, False, None),       # not groupable (7x7): the single-problem route, in the middle of the queue
    (1, 8, 8, 128, 256, 3, 2, 1, False, None),      # 16 output pixels: one sub-step, far from 8 per block
    (2, 11, 13, 64, 256, 3, 1, 1, True, 3),         # shares dW and dbias with problem 3; 286 pixels
]
# seven 256 -> 256 3x3 layers of 1280 pixels: 10 splits x 2.36 MB of slabs each, the 128 MB workspace holds five
FULL_WS = [(2, 32, 20, 256, 256, 3, 1, 1, False, None)] * 7


def make_problems(cases, seed, dev):
    g = torch.Generator().manual_seed(seed)
    out = []
    for N, H, W, Ci, Co, k, st, pd, bias, share in cases:
        Ho, Wo = (H + 2 * pd - k) // st + 1, (W + 2 * pd - k) // st + 1
        x = torch.randn(N, H, W, Ci, generator=g)
        dy = torch.randn(N, Ho, Wo, Co, generator=g)
        out.append({"x": x.to(dev), "dy": dy.to(dev), "geo": (k, st, pd), "bias": bias, "share": share, "shape": (Co, Ci, k)})
    return out


def fresh_sinks(probs, dev):
    """(dw, dbias) per problem, zeroed; sharing problems get the same tensors"""
    sinks = []
    for p in probs:
        if p["share"] is not None:
            sinks.append(sinks[p["share"]])
            continue
        Co, Ci, k = p["shape"]
        dw = torch.zeros(Co, Ci, k, k, device=dev).contiguous(memory_format=torch.channels_last)
        sinks.append((dw, torch.zeros(Co, device=dev) if p["bias"] else None))
    return sinks


def run_multi(ops, probs, dev):
    sinks = fresh_sinks(probs, dev)
    ops.conv_bwd_weight_multi_raw([(p["dy"], p["x"], s[0], s[1]) + p["geo"] for p, s in zip(probs, sinks)])
    return sinks


def run_solo(probs, dev):
    lib = importlib.import_module("3dod_amd._lib")
    sinks = fresh_sinks(probs, dev)
    for p, (dw, db) in zip(probs, sinks):
        N, H, W, Ci = p["x"].shape
        k, st, pd = p["geo"]
        if db is not None:
            lib.call("cr_conv2d_bwd_weight_bias", p["dy"], p["x"], dw, db, N, H, W, Ci, p["shape"][0], k, st, pd, 1, 1)
        else:
            lib.call("cr_conv2d_bwd_weight", p["dy"], p["x"], dw, N, H, W, Ci, p["shape"][0], k, st, pd, 1, 1)
    return sinks


def relerr(a, b):
    a = a.double().cpu(); b = b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def test_mixed_queue_matches_float64():
    ops = importlib.import_module("3dod_amd.hipops")
    assert ops.precision() == "fp32"
    probs = make_problems(MIXED, 11, DEV)
    sinks = run_multi(ops, probs, DEV)
    torch.cuda.synchronize()
    # float64 reference; problems that share a sink add up
    ref = {}
    for i, p in enumerate(probs):
        k, st, pd = p["geo"]
        x = p["x"].cpu().double().permute(0, 3, 1, 2)
        dy = p["dy"].cpu().double().permute(0, 3, 1, 2)
        w = torch.zeros(p["shape"][0], p["shape"][1], k, k, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w, None, st, pd).backward(dy)
        j = i if p["share"] is None else p["share"]
        dw, db = ref.get(j, (0, 0))
        ref[j] = (dw + w.grad, db + dy.sum((0, 2, 3)))
    for j, (dw, db) in ref.items():
        e = relerr(sinks[j][0], dw)
        print("problem", j, MIXED[j][:8], "dW err", e)
        assert e < 1e-4, (j, e)
        if sinks[j][1] is not None:
            e = relerr(sinks[j][1], db)
            print("problem", j, "dbias err", e)
            assert e < 1e-4, (j, e)


# ---- deterministic mode: in a child process --------------------------------------------------------------------------------
def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def child_kernels():
    ops = importlib.import_module("3dod_amd.hipops")
    dev = torch.device(DEV)
    digests = []
    for name, cases in (("MIXED", MIXED), ("FULL_WS", FULL_WS)):
        probs = make_problems(cases, 5, dev)
        a, b = run_multi(ops, probs, dev), run_solo(probs, dev)
        torch.cuda.synchronize()
        same = all(torch.equal(s[0], t[0]) and (s[1] is None or torch.equal(s[1], t[1])) for s, t in zip(a, b))
        nonzero = all(float(s[0].abs().max()) > 0 for s in a)
        print(name, "EQUAL" if same and nonzero else "DIFFERENT")
        digests.append(_digest([t for s in a for t in s]))
    print("HASH", *digests)


def dense_backward(ops, model, opt, img, defer):
    """the dense region's backward as GraphedDense runs it (gradient slots of the pyramid maps included) -> flat gradient"""
    opt.zero_grad()
    pg = model.proposal_generator
    x = ops.preprocess(img, model.pixel_mean_list, model.pixel_std_list)
    feats = model.backbone(x)
    ys = pg.rpn_head.forward_raw([feats[f] for f in pg.in_features])
    outs = list(feats.values()) + list(ys)
    ps = [p for m in (model.backbone, pg.rpn_head) for p in m.parameters() if p.requires_grad]
    g = torch.Generator().manual_seed(1)
    keep_o, keep_g = [], []
    for o in outs:
        go = torch.randn(o.shape, generator=g).to(o.device)
        slot = getattr(o, "_cr_slot", None)
        if slot is not None and ops._SLOTS_ON[0]:
            ops._slot_put(slot, go)
        else:
            keep_o.append(o); keep_g.append(go)
    queued = 0
    with (ops.deferred_wgrad() if defer else contextlib.nullcontext()):
        res = torch.autograd.grad(keep_o, ps, keep_g, allow_unused=True)
        queued = ops.wgrad_pending()
    assert ops.wgrad_pending() == 0
    for p, gr in zip(ps, res):
        if gr is not None:
            ops.grad_sink(p).add_(gr)
    torch.cuda.synchronize()
    return opt.flat_g.clone(), queued


def child_model():
    sys.path.insert(0, ROOT)
    ops = importlib.import_module("3dod_amd.hipops")
    bt = importlib.import_module("bench_train")
    dev = torch.device(DEV)
    cfg, model, opt, syn, solver = bt.build(dev, seed=3)
    img = torch.randint(0, 256, (2, 3, 64, 64), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(dev)
    g_off, _ = dense_backward(ops, model, opt, img, False)
    g_on, queued = dense_backward(ops, model, opt, img, True)
    print("MODEL", "EQUAL" if torch.equal(g_on, g_off) and float(g_on.abs().max()) > 0 else "DIFFERENT", "queued-at-exit", queued)
    # an exception inside the context: what was queued is launched all the same
    p = make_problems(MIXED[:1], 9, dev)[0]
    want = run_solo([p], dev)[0][0]
    sink = fresh_sinks([p], dev)[0][0]
    try:
        with ops.deferred_wgrad():
            ops.conv_bwd_weight_raw(p["dy"], p["x"], *p["geo"], sink=sink)
            assert ops.wgrad_pending() == 1 and float(sink.abs().max()) == 0
            raise KeyError("inside")
    except KeyError:
        pass
    torch.cuda.synchronize()
    print("RAISE", "KEPT" if ops.wgrad_pending() == 0 and torch.equal(sink, want) else "DROPPED")


def _child(mode):
    env = dict(os.environ, CR_DETERMINISTIC="1", CR_PRECISION="fp32")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True, timeout=300, env=env,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


def test_deterministic_grouped_equals_one_by_one_bitwise():
    a = _child("kernels")
    assert "MIXED EQUAL" in a, a
    assert "FULL_WS EQUAL" in a, a            # the workspace fills after five problems: the group is cut, results unchanged
    b = _child("kernels")
    ha, hb = ([l for l in s.splitlines() if l.startswith("HASH")] for s in (a, b))
    assert ha and ha == hb, (ha, hb)


def test_deferred_dense_backward_is_bit_equal_and_never_drops():
    out = _child("model")
    assert "MODEL EQUAL" in out, out
    assert "RAISE KEPT" in out, out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    {"kernels": child_kernels, "model": child_model}[sys.argv[1]]()
