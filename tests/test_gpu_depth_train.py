"""Depth-Anything-V2 training step on the HIP kernels against the REFERENCE's float32 CPU run with the same seeded weights
(tests/golden/make_golden_depth_train.py -> golden/depth_anything_vits_train.npz): loss, prediction, every parameter's
gradient, five AdamW steps, the fine-tuning tool's loop, and that inference is left exactly as it was.

The yardstick for the gradients is the reference's own error under torch.autocast("cpu", bfloat16), recorded per parameter
in the fixture; this implementation rounds every branch activation to bf16 (autocast keeps LayerNorm and softmax in
float32), hence the margin of 3."""
import importlib
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dav2 = importlib.import_module("3dod_amd.depth_anything_v2")
syn = importlib.import_module("3dod_amd.synthetic")
ops = importlib.import_module("3dod_amd.hipops")
solver = importlib.import_module("3dod_amd.cubercnn.solver.build")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
tool = importlib.import_module("train_depth")
GOLD = os.path.join(os.path.dirname(__file__), "golden", "depth_anything_vits_train.npz")
CFG = dict(encoder="vits", features=64, out_channels=[64, 128, 256, 256], max_depth=20.0)
DEV = torch.device("cuda:0")
MARGIN = 3.0


def inputs(seed, shape):
    """make_golden_depth_train.inputs"""
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(shape, generator=g)
    target = torch.rand((shape[0],) + tuple(shape[2:]), generator=g) * 15 + 1
    mask = torch.rand((shape[0],) + tuple(shape[2:]), generator=g) < 0.8
    return x.to(DEV), target.to(DEV), mask.to(DEV)


def grad_slice(g):
    return g.reshape(-1) if g.numel() <= 4096 else g.reshape(g.shape[0], -1)[:16, :64].reshape(-1)


def build(seed):
    m = dav2.DepthAnythingV2(**CFG)
    m.load_state_dict(syn.seeded_state_dict(m, seed))
    return m.to(DEV)


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def step(gold):
    """one forward + backward in train mode, shared by the tests below"""
    seed, shape = int(gold["seed"]), tuple(int(v) for v in gold["shape"])
    x, target, mask = inputs(seed, shape)
    model = build(seed).train()
    pred = model(x)
    loss = ops.silog_loss(pred, target, mask)
    loss.backward()
    torch.cuda.synchronize()
    return types.SimpleNamespace(model=model, pred=pred.detach(), loss=float(loss.detach()), x=x, target=target, mask=mask,
                                 grads={n: p.grad for n, p in model.named_parameters()})


def loss_bound(gold):
    ref = float(gold["loss"])
    return max(MARGIN * abs(float(gold["loss_autocast"]) - ref), 2.0 ** -8 * ref)


def test_loss_and_prediction(gold, step):
    ref = float(gold["loss"])
    print(f"loss {step.loss:.6f} reference {ref:.6f} autocast {float(gold['loss_autocast']):.6f} bound {loss_bound(gold):.2e}")
    assert abs(step.loss - ref) <= loss_bound(gold)
    want = gold["pred"]
    err = np.abs(step.pred.cpu().numpy() - want)
    rng = float(want.max() - want.min())
    print(f"prediction: mean err {err.mean() / rng:.4%} max err {err.max() / rng:.4%} of the range {rng:.3f}")
    assert step.pred.shape == want.shape and err.mean() < 0.005 * rng and err.max() < 0.03 * rng


def test_gradients_match_reference(gold, step):
    """every parameter's gradient slice within 3 x the reference's own autocast error (normwise and 1 - cos).

    Measured on an MI355X: over the 234 parameters with a gradient the ratio error / autocast error has median 1.04 and
    maximum 1.87 (1 - cos: 2.85), on depth_head.scratch.refinenet3.resConfUnit2.conv1.bias.  With the residual stream
    rounded to bf16 like the inference path's, one parameter missed the bound (refinenet3.resConfUnit1.conv1.weight:
    4.17 % against an autocast error of 1.34 %, ratio 3.11): the 0.92 % error of that unit's input flips ReLU masks
    inside it, and a weight gradient summed over 70 pixels feels every flip.  The training route therefore keeps the
    stream in float32."""
    names, bad, worst, ratios = [str(n) for n in gold["names"]], [], (0.0, 0.0, ""), []
    assert names == [n for n, _ in step.model.named_parameters()]
    for i, n in enumerate(names):
        if not gold["has_grad"][i]:
            continue
        assert step.grads[n] is not None, f"{n}: no gradient"
        a = torch.from_numpy(gold[f"g{i}"]).double()
        b = grad_slice(step.grads[n]).double().cpu()
        rel = float((b - a).norm() / a.norm())
        omc = float(1 - (a @ b) / (a.norm() * b.norm()))
        # (1e-15: the float64 rounding of the cosine itself; a one-element gradient has 1 - cos = 0 on both sides)
        r1, r2 = rel / float(gold["ac_rel"][i]), max(omc - 1e-15, 0.0) / max(float(gold["ac_one_minus_cos"][i]), 1e-300)
        worst = max(worst, (r1, r2, n))
        ratios.append((round(r1, 2), n))
        nr = abs(float(step.grads[n].double().norm()) / float(gold["grad_norm"][i]) - 1)
        if r1 > MARGIN or r2 > MARGIN or nr > MARGIN * float(gold["ac_rel"][i]):
            bad.append((n, round(rel, 5), round(float(gold["ac_rel"][i]), 5), round(r1, 2), round(r2, 2), round(nr, 4)))
    print(f"worst ratio to the autocast error: rel {worst[0]:.2f}, 1-cos {worst[1]:.2f} ({worst[2]})")
    rs = sorted(ratios)
    print(f"ratio rel / autocast rel over {len(rs)} parameters: median {rs[len(rs) // 2][0]}, largest {rs[-6:]}")
    assert not bad, f"{len(bad)} parameters over {MARGIN} x their autocast error (name, rel, autocast rel, ratios): {bad[:8]}"


def test_unused_parameters_get_no_gradient(gold, step):
    unused = [str(n) for n, h in zip(gold["names"], gold["has_grad"]) if not h]
    assert len(unused) == 5 and "pretrained.mask_token" in unused
    for n in unused:
        g = step.grads[n]
        assert g is None or not bool(g.any()), n


def test_five_adamw_steps_follow_the_reference(gold, step):
    seed = int(gold["seed"])
    model = build(seed).train()
    enc, head = tool.split_groups(model.named_parameters(), dav2.DepthAnythingV2.UNUSED_PARAMETERS)
    lr = float(gold["traj_lr"])
    opt = solver.FlatAdam([(p, lr, 0.01) for p in enc] + [(p, lr * 10.0, 0.01) for p in head], eps=1e-8, betas=(0.9, 0.999),
                          decoupled=True)
    ops.bump_weight_epoch()
    losses = []
    for _ in range(len(gold["traj_losses"])):
        opt.zero_grad()
        loss = ops.silog_loss(model(step.x), step.target, step.mask)
        loss.backward()
        opt.collect_grads()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", [round(v, 5) for v in losses], "reference", [round(float(v), 5) for v in gold["traj_losses"]])
    for k, (a, b) in enumerate(zip(losses, gold["traj_losses"]), 1):
        assert abs(a - float(b)) <= k * loss_bound(gold), (k, a, float(b))
    assert losses[-1] < 0.95 * losses[0]
    for n, p in model.named_parameters():           # the unused parameters are outside the optimizer and untouched
        if any(n.startswith(u) for u in dav2.DepthAnythingV2.UNUSED_PARAMETERS):
            assert p.grad is None and not hasattr(p, "_cr_grad")


def _write_pairs(root, n, name, seed):
    """the project's synthetic images (3dod_amd.synthetic.make_omni3d_dataset: <name>/images/<id>.png, 70 x 98) with their
    .npz depth maps (depth_maps/<id>.npz, half resolution, 1 .. 8 m) -> a split file of `image depth` lines"""
    import json
    jf = syn.make_omni3d_dataset(str(root), name=name, n_images=n, seed=seed, sizes=((70, 98),), first_image_id=1000 * (seed + 1))
    ids = [im["id"] for im in json.load(open(jf))["images"]]
    assert len(ids) == n
    split = root / f"{name}.txt"
    split.write_text("".join(f"{name}/images/{i}.png depth_maps/{i}.npz\n" for i in ids))
    return str(split)


def test_tool_trains_validates_and_resumes(tmp_path):
    m0 = dav2.DepthAnythingV2(**CFG)
    args = types.SimpleNamespace(encoder="vits", features=None, out_channels=None,
                                 train_split=_write_pairs(tmp_path, 4, "train", 0), val_split=_write_pairs(tmp_path, 2, "val", 1),
                                 img_size=70, min_depth=0.001, max_depth=20.0, epochs=3, bs=2, lr=1e-5, pretrained_from=None,
                                 save_path=str(tmp_path / "out"), seed=0)
    st = tool.build(args, model_config=CFG, init_state_dict=syn.seeded_state_dict(m0, 7))
    assert st.iters_per_epoch == 2 and st.total_iters == 6
    losses = tool.train_one_epoch(st, 0)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    assert st.lrs == [tool.poly_lr(1e-5, 0, 6), tool.poly_lr(1e-5, 1, 6)]
    assert [g["lr"] for g in st.opt.param_groups] == [st.lrs[-1], st.lrs[-1] * 10.0]
    assert [s[2] for s in st.opt.segments] == [st.lrs[-1], st.lrs[-1] * 10.0]
    results = tool.validate(st)
    assert list(results) == list(ops.DEPTH_METRICS) and all(math.isfinite(v) for v in results.values())
    assert st.previous_best["abs_rel"] == results["abs_rel"] and st.previous_best["d1"] == results["d1"]
    path = tool.save_checkpoint(st, 0)
    ck = torch.load(path, map_location="cpu")
    assert sorted(ck) == ["epoch", "model", "optimizer", "previous_best"] and ck["epoch"] == 0
    assert list(ck["model"]) == list(m0.state_dict())
    # the next step from the live state and from the reloaded checkpoint: the same loss, bit for bit
    g = torch.Generator().manual_seed(3)
    img = torch.randn(2, 3, 70, 70, generator=g).to(DEV)
    depth = (torch.rand(2, 70, 70, generator=g) * 15 + 1).to(DEV)
    valid = (torch.rand(2, 70, 70, generator=g) < 0.8).to(DEV)
    live = tool.train_step(st, img, depth, valid, 2)
    st2 = tool.build(args, model_config=CFG)
    assert tool.load_checkpoint(st2, path) == 1 and st2.opt.param_groups[0]["lr"] == tool.poly_lr(1e-5, 1, 6)
    again = tool.train_step(st2, img, depth, valid, 2)
    assert torch.equal(live, again), (float(live), float(again))


def test_inference_untouched_by_training(gold, step):
    seed = int(gold["seed"])
    with torch.no_grad():
        y = step.model.eval()(step.x)
    step.model.train()
    fresh = build(seed).eval()
    assert torch.equal(y, fresh(step.x))
    assert not y.requires_grad and not fresh(step.x).requires_grad
