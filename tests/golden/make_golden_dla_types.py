"""Golden vectors for the ten DLA trunk types: the REFERENCE's own DLA classes (cubercnn/modeling/backbone/dla.py:71-153,
233-450, pure torch.nn) built on the CPU with seeded random-init weights.  The product builds the same module trees in the
same creation order, so the same seed gives the same weights.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dla_types.py

Writes, next to this script:

  dla_types_weights.npz       every type: state-dict keys, per-tensor sum / abs-sum, p2..p6 channel counts of DLABackbone
  dla_trunk_<type>.npz        dla34, dla46_c, dla46x_c, dla60x, dla102x2: train-mode forward computed in FLOAT64, stored in
                              float32 (x, level1, p2..p5), plus per stage `ref32_err_<stage>`: the relative L2 distance between
                              the reference's own float32 forward of that stage, fed the float64 input of the stage, and the
                              float64 result -- how far float32 arithmetic alone drifts on that stage
  dla46x_c_level3_grads.npz   level3 of dla46x_c alone: input = the fixture's p2, loss = sum(out * R); float64 gradients of the
                              stage input, of tree1.tree1.conv2.weight (grouped, stride 2), tree2.tree1.conv2.weight (grouped,
                              stride 1), tree1.root.conv.weight and tree2.root.conv.weight, and `ref32_err_<name>` of a float32
                              CPU autograd run of the same thing
  dla34_level3_grads.npz      the same for dla34 (stage input, tree1.tree1.conv1.weight and the two Root convolutions): what the
                              dense kernels reach against such a fixture.  Its float64 gradients are stored in float32 (the
                              3x3 weights are 64 times larger than the grouped ones)

The reference's constructors leave BottleneckX.cardinality / expansion behind as class attributes (dla.py:400-401): both are
reset before every type here."""
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refimport  # noqa: E402

_refimport.install()
spec = importlib.util.spec_from_file_location("_ref_dla", os.path.join(_refimport.REFERENCE, "cubercnn/modeling/backbone/dla.py"))
ref_dla = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_dla)
torch.set_num_threads(8)

SEED = 1234
TYPES = ["dla34", "dla46_c", "dla46x_c", "dla60x_c", "dla60", "dla60x", "dla102", "dla102x", "dla102x2", "dla169"]
TRUNKS = ["dla34", "dla46_c", "dla46x_c", "dla60x", "dla102x2"]
STAGES = [("level1", "x"), ("p2", "level1"), ("p3", "p2"), ("p4", "p3"), ("p5", "p4")]       # (output, its input)
GRAD_WEIGHTS = {"dla46x_c": ["tree1.tree1.conv2.weight", "tree2.tree1.conv2.weight", "tree1.root.conv.weight",
                             "tree2.root.conv.weight"],
                "dla34": ["tree1.tree1.conv1.weight", "tree1.root.conv.weight", "tree2.root.conv.weight"]}


def reset_class_state():
    ref_dla.BottleneckX.cardinality = 32
    ref_dla.BottleneckX.expansion = 2
    ref_dla.Bottleneck.expansion = 2


def build(kind):
    reset_class_state()
    torch.manual_seed(SEED)
    return getattr(ref_dla, kind)(pretrained=False)


def out_channels(kind):
    reset_class_state()
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(DLA=types.SimpleNamespace(TYPE=kind, TRICKS=False)))
    torch.manual_seed(SEED)
    bb = ref_dla.DLABackbone(cfg, None, pretrained=False)
    return [int(bb._out_feature_channels[k]) for k in ("p2", "p3", "p4", "p5", "p6")]


def stage_fn(net, out):
    if out == "level1":
        return lambda x: net.level1(net.level0(net.base_layer(x)))
    return getattr(net, "level" + out[1])


def rel_l2(a, b):
    return float((a.double() - b).norm() / b.norm())


def weights_file():
    rec = {"seed": np.int64(SEED), "types": np.array(TYPES)}
    for kind in TYPES:
        sd = build(kind).state_dict()
        names = [k for k in sd if not k.startswith("fc") and "num_batches" not in k and "running" not in k]
        rec[kind + "_names"] = np.array(names)
        rec[kind + "_sums"] = np.array([float(sd[k].double().sum()) for k in names])
        rec[kind + "_abs"] = np.array([float(sd[k].double().abs().sum()) for k in names])
        rec[kind + "_channels"] = np.array(out_channels(kind), dtype=np.int64)
        print(kind, len(names), rec[kind + "_channels"].tolist())
    np.savez_compressed(os.path.join(HERE, "dla_types_weights.npz"), **rec)


def trunk_file(kind):
    net32 = build(kind).train()
    net64 = copy.deepcopy(net32).double().train()
    g = torch.Generator().manual_seed(99)
    x = torch.randn(2, 3, 64, 96, generator=g)
    vals = {"x": x.double()}
    rec = {"seed": np.int64(SEED)}
    with torch.no_grad():
        for out, inp in STAGES:
            vals[out] = stage_fn(net64, out)(vals[inp])
            got32 = stage_fn(net32, out)(vals[inp].float())
            rec["ref32_err_" + out] = np.float64(rel_l2(got32, vals[out]))
    for k, v in vals.items():
        rec[k] = v.float().numpy()
    rec["notes"] = "reference DLA forward in train mode in float64, torch.manual_seed(1234) init; pinned by reference"
    path = os.path.join(HERE, "dla_trunk_{}.npz".format(kind))
    np.savez_compressed(path, **rec)
    print(kind, {k: float(rec["ref32_err_" + k]) for k, _ in STAGES}, os.path.getsize(path))
    return net32, vals


def grads_file(kind, net32, vals, store):
    g = torch.Generator().manual_seed(7)
    R = torch.randn(vals["p3"].shape, generator=g)
    x32 = vals["p2"].float()                     # what the fixture stores = what the product is fed
    res = {}
    for dt in (torch.float64, torch.float32):
        stage = copy.deepcopy(net32.level3).to(dt).train()
        x = x32.to(dt).requires_grad_(True)
        ws = [dict(stage.named_parameters())[n] for n in GRAD_WEIGHTS[kind]]
        loss = (stage(x) * R.to(dt)).sum()
        res[dt] = torch.autograd.grad(loss, [x] + ws)
    rec = {"seed": np.int64(SEED), "R": R.numpy(), "weight_names": np.array(GRAD_WEIGHTS[kind])}
    for name, g64, g32 in zip(["input"] + GRAD_WEIGHTS[kind], res[torch.float64], res[torch.float32]):
        rec["grad_" + name] = g64.to(store).numpy()
        rec["ref32_err_" + name] = np.float64(rel_l2(g32, g64))
        print("grad", name, tuple(g64.shape), float(rec["ref32_err_" + name]))
    path = os.path.join(HERE, "{}_level3_grads.npz".format(kind))
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    weights_file()
    for kind in TRUNKS:
        net32, vals = trunk_file(kind)
        if kind in GRAD_WEIGHTS:
            grads_file(kind, net32, vals, torch.float64 if kind == "dla46x_c" else torch.float32)
    reset_class_state()
