"""Golden vector for the Depth-Anything-V2 training step: runs the REFERENCE's DepthAnythingV2 in train() mode
(depth/metric_depth/depth_anything_v2/dpt.py) with its SiLogLoss (util/loss.py) on CPU in float32, weights from
`3dod_amd.synthetic.seeded_state_dict`, and records

  * the loss and the prediction of one forward pass,
  * for every parameter: its gradient norm, a slice of its gradient (the whole tensor if <= 4096 elements, otherwise the
    leading 16 x 64 block of its 2-D view) and the error of the reference's OWN run under torch.autocast("cpu", bfloat16) on
    that slice (normwise relative error and 1 - cosine): the yardstick for a bf16 implementation,
  * the reference's loss over 5 torch.optim.AdamW steps on that one batch (two groups as in train.py: encoder lr, head
    10 lr), with a learning rate at which the loss falls by at least 10 % (asserted here).

Only data is written (tests/golden/depth_anything_vits_train.npz); inputs are regenerated from the seed by the test.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_depth_train.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _refimport  # noqa: E402

_refimport.install()
sys.path.insert(0, os.path.join(_refimport.REFERENCE, "depth", "metric_depth"))
from depth_anything_v2.dpt import DepthAnythingV2  # noqa: E402  (reference)
from util.loss import SiLogLoss  # noqa: E402  (reference)

syn = importlib.import_module("3dod_amd.synthetic")

CFG = dict(encoder="vits", features=64, out_channels=[64, 128, 256, 256], max_depth=20.0)
SEED, SHAPE, STEPS = 5, (2, 3, 70, 98), 5
LR_CANDIDATES = (1e-6, 2e-6, 3e-6, 5e-6, 1e-5)      # the smallest that makes the loss fall by 10 % in 5 steps


def inputs(seed=SEED, shape=SHAPE):
    """image, target depth U(1,16) and a mask with about 80 % true, all from one generator (the test calls this too)"""
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(shape, generator=g)
    target = torch.rand((shape[0],) + tuple(shape[2:]), generator=g) * 15 + 1
    mask = torch.rand((shape[0],) + tuple(shape[2:]), generator=g) < 0.8
    return x, target, mask


def grad_slice(g):
    return g.reshape(-1) if g.numel() <= 4096 else g.reshape(g.shape[0], -1)[:16, :64].reshape(-1)


def build():
    m = DepthAnythingV2(**CFG).train()
    m.load_state_dict(syn.seeded_state_dict(m, SEED))
    return m


def run(model, x, target, mask, autocast=False):
    model.zero_grad(set_to_none=True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        pred = model(x)
    loss = SiLogLoss()(pred.float(), target, mask)
    loss.backward()
    return float(loss.detach()), pred.detach().float(), {n: (None if p.grad is None else p.grad.detach().float().clone())
                                                for n, p in model.named_parameters()}


def trajectory(lr, x, target, mask):
    model = build()
    named = list(model.named_parameters())
    opt = torch.optim.AdamW([{"params": [p for n, p in named if "pretrained" in n], "lr": lr},
                             {"params": [p for n, p in named if "pretrained" not in n], "lr": lr * 10.0}],
                            lr=lr, betas=(0.9, 0.999), weight_decay=0.01)
    losses = []
    for _ in range(STEPS):
        opt.zero_grad()
        loss = SiLogLoss()(model(x), target, mask)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


if __name__ == "__main__":
    torch.set_num_threads(4)
    x, target, mask = inputs()
    model = build()
    loss, pred, grads = run(model, x, target, mask)
    loss_ac, _, grads_ac = run(model, x, target, mask, autocast=True)
    names = [n for n, _ in model.named_parameters()]
    has = np.array([grads[n] is not None for n in names])
    rec = {"seed": np.array(SEED), "shape": np.array(SHAPE), "loss": np.array(loss), "loss_autocast": np.array(loss_ac),
           "pred": pred.numpy(), "names": np.array(names), "has_grad": has}
    norms, ac_rel, ac_cos = [], [], []
    for i, n in enumerate(names):
        if grads[n] is None:
            norms.append(0.0); ac_rel.append(0.0); ac_cos.append(0.0)
            continue
        a, b = grad_slice(grads[n]).double(), grad_slice(grads_ac[n]).double()
        norms.append(float(grads[n].double().norm()))
        ac_rel.append(float((b - a).norm() / a.norm()))
        ac_cos.append(float(1 - (a @ b) / (a.norm() * b.norm())))
        rec[f"g{i}"] = a.float().numpy()
    rec.update(grad_norm=np.array(norms), ac_rel=np.array(ac_rel), ac_one_minus_cos=np.array(ac_cos))
    for lr in LR_CANDIDATES:
        losses = trajectory(lr, x, target, mask)
        print("lr", lr, "losses", losses)
        if losses[-1] <= 0.9 * losses[0]:
            break
    assert losses[-1] <= 0.9 * losses[0], "no candidate learning rate makes the reference's loss fall by 10 % in 5 steps"
    rec.update(traj_lr=np.array(lr), traj_losses=np.array(losses))
    rec["notes"] = np.array("reference DepthAnythingV2(vits, features=64, out_channels=[64,128,256,256]).train() + SiLogLoss, float32 "
                            "on CPU, weights = seeded_state_dict(model, 5), inputs = make_golden_depth_train.inputs()")
    out = os.path.join(HERE, "depth_anything_vits_train.npz")
    np.savez_compressed(out, **rec)
    r = np.array(ac_rel)[has]
    print("loss", loss, "autocast", loss_ac, "no grad:", [n for n, h in zip(names, has) if not h])
    print("autocast rel: min %.4f median %.4f max %.4f; min cos %.6f" % (r.min(), np.median(r), r.max(),
                                                                          1 - np.array(ac_cos)[has].max()))
    print("bytes", os.path.getsize(out))
