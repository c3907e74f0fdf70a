"""CPU: bench.py --dump-outputs helpers -- flattening of a step's result (dicts, Instances, Boxes, per-image lists), the dtype
mapping of the written arrays, the seeded sample of large outputs and the size cap."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import bench

st = importlib.import_module("3dod_amd.d2lite.structures")


def test_output_tensors_flattens_instances_lists_and_dicts():
    inst = [st.Instances((8, 8), pred_boxes=st.Boxes(torch.arange(4 * n, dtype=torch.float32).reshape(n, 4)),
                         scores=torch.rand(n), pred_classes=torch.arange(n)) for n in (3, 5)]
    out = bench.output_tensors({"dets": [{"instances": i} for i in inst], "loss": torch.tensor(1.5)})
    assert set(out) == {"dets.instances.pred_boxes", "dets.instances.scores", "dets.instances.pred_classes", "loss"}
    assert out["dets.instances.pred_boxes"].shape == (32,)
    assert torch.equal(out["dets.instances.pred_classes"], torch.tensor([0, 1, 2, 0, 1, 2, 3, 4]))
    assert torch.equal(out["dets.instances.scores"], torch.cat([inst[0].scores, inst[1].scores]))
    assert bench.output_tensors(None) == {}


def test_dump_outputs_dtypes_names_and_seeded_sample(tmp_path):
    big = torch.rand(bench.DUMP_MAX_ELEMS + 1000)
    outs = {"BoxHead/loss_cls": torch.tensor(0.25), "argmax": torch.arange(7), "flag": torch.tensor([True, False]),
            "f64": torch.rand(5, dtype=torch.float64), "bf16": torch.rand(6).bfloat16(), "big": big}
    for d in ("a", "b"):
        bench.dump_outputs(types.SimpleNamespace(dump_outputs=str(tmp_path / d)), outs)
    load = lambda d, n: np.load(os.path.join(tmp_path, d, n + ".npy"))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(["BoxHead.loss_cls.npy", "argmax.npy", "flag.npy", "f64.npy",
                                                         "bf16.npy", "big.npy"])
    assert load("a", "BoxHead.loss_cls").dtype == np.float32 and float(load("a", "BoxHead.loss_cls")) == 0.25
    assert load("a", "argmax").dtype == np.float64 and (load("a", "argmax") == np.arange(7)).all()
    assert load("a", "flag").dtype == np.float64 and load("a", "flag").tolist() == [1.0, 0.0]
    assert load("a", "f64").dtype == np.float64 and (load("a", "f64") == outs["f64"].numpy()).all()
    assert load("a", "bf16").dtype == np.float32 and (load("a", "bf16") == outs["bf16"].float().numpy()).all()
    s = load("a", "big")
    assert s.shape == (bench.DUMP_MAX_ELEMS,) and np.isin(s, big.numpy()).all()
    assert (s == load("b", "big")).all()                            # the same positions in every run


def test_dump_outputs_over_the_cap_writes_nothing(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    d = tmp_path / "out"
    with pytest.raises(RuntimeError, match="more than"):
        bench.dump_outputs(types.SimpleNamespace(dump_outputs=str(d)), {"a": torch.zeros(200), "b": torch.zeros(200)})
    assert not d.exists()
