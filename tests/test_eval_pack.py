"""CPU: the host side of the evaluator's device backend (3dod_amd/evalops.py pack / unpack, the backend= plumbing, the config
key).  The kernels' outputs are stood in for by the host's own _ious / _evaluate_img, written into the packed output layout:
unpack must then reproduce the host's evalImgs exactly."""
import importlib

import numpy as np
import pytest

from oracle import iou3d as O
from tests import eval_device_helpers as H

ev_mod = H.ev_mod
evalops = H.evalops


def oracle_iou3d(d, g):
    return O.box3d_overlap(np.asarray(d), np.asarray(g))[1]


def fixture(seed=0):
    """image 1: category 0 with tied scores and 5 detections (cut to 3 by maxDets), category 1 with detections only, category 2
    with ground truth only; image 2: category 0 again; image 9 is left out of params.imgIds."""
    rng = np.random.default_rng(seed)
    gts, dts = [], []

    def add(img, cat, n_gt, scores, ignore=()):
        cs = [H.cuboid(rng, spread=0.5) for _ in range(max(n_gt, 1))]
        for k in range(n_gt):
            x, y = rng.uniform(0, 40, 2)
            gts.append(H.gt_rec(img, cat, len(gts) + 1, cs[k], [x, y, 30, 30], rng.choice([5.0, 10.0, 20.0, 35.0, 50.0]),
                                rng.choice([500.0, 1024.0, 5000.0, 9216.0, 20000.0]), ignore=k in ignore))
        for k, s in enumerate(scores):
            x, y = rng.uniform(0, 40, 2)
            dts.append(H.dt_rec(img, cat, cs[k % len(cs)] + rng.normal(size=3) * 0.1, [x, y, 30, 30],
                                rng.choice([5.0, 10.0, 40.0, 2e5]), rng.choice([500.0, 1024.0, 9216.0, -1.0]), s))
    add(1, 0, 3, [0.5, 0.9, 0.5, 0.5, 0.9], ignore=(1,))
    add(1, 1, 0, [0.3, 0.3])
    add(1, 2, 2, [])
    add(2, 0, 2, [0.7, 0.2, 0.7])
    add(9, 0, 1, [0.6])
    return gts, dts


@pytest.mark.parametrize("mode,prox", [("2D", False), ("3D", False), ("3D", True)])
def test_unpack_reproduces_the_host_eval_imgs(mode, prox):
    gts, dts = fixture()
    ev = ev_mod.Omni3Deval(gts, dts, mode, eval_prox=prox, iou3d_fn=oracle_iou3d)
    ev.params.imgIds = [1, 2, 3]                       # 9 is outside; 3 has no record at all
    ev.params.maxDets = [1, 2, 3]
    want = dict(ev.evaluate().evalImgs)
    assert want[0, 0, 3] is None and want[1, 0, 2] is None and (0, 0, 9) not in want
    assert want[0, 0, 1]["dtMatches"].shape == (10, 3)                                    # 5 detections cut to 3

    packed = evalops.pack(ev)
    assert packed["n_groups"] == 4 and packed["grp_cat"] == [0, 0, 1, 2] and packed["grp_img"] == [1, 2, 1, 1]
    assert packed["dt_off"].tolist() == [0, 3, 6, 8, 8] and packed["gt_off"].tolist() == [0, 3, 5, 5, 7]
    assert packed["iou_off"].tolist() == [0, 9, 15, 15, 15] and packed["iou_off"].dtype == np.int64
    # stable order under tied scores: 0.9 (second record), 0.9 (fifth), then the first of the three 0.5s
    assert packed["dt_score"][:3].tolist() == [0.9, 0.9, 0.5]
    first = [d for d in dts if d["image_id"] == 1 and d["category_id"] == 0]
    key = "bbox3D" if mode == "3D" else "bbox"
    for k, src in enumerate((1, 4, 0)):
        got = packed["dt_box3d"][k] if mode == "3D" else packed["dt_bbox"][k]
        assert np.array_equal(got, np.asarray(first[src][key], dtype=got.dtype))
    assert (packed["dt_bbox"] is None) == (mode == "3D" and not prox) and (packed["dt_box3d"] is None) == (mode == "2D")

    out = H.kernel_outputs_from_host(ev, packed, H.host_eval_imgs(ev, packed))
    got = ev_mod.Omni3Deval(gts, dts, mode, eval_prox=prox, iou3d_fn=oracle_iou3d)
    got.params.imgIds, got.params.maxDets = [1, 2, 3], [1, 2, 3]
    evalops.unpack(got, packed, out)
    H.assert_same_eval_imgs(got.evalImgs, want)
    # and the tables that follow from them (summarize() needs maxDets to hold 100)
    a, b = got.accumulate().eval, ev.accumulate().eval
    assert np.array_equal(a["precision"], b["precision"]) and np.array_equal(a["recall"], b["recall"])


def test_unpack_sends_flagged_groups_to_the_host_route():
    gts, dts = fixture()
    ev = ev_mod.Omni3Deval(gts, dts, "3D", iou3d_fn=oracle_iou3d)
    want = dict(ev.evaluate().evalImgs)
    packed = evalops.pack(ev)
    out = H.kernel_outputs_from_host(ev, packed, H.host_eval_imgs(ev, packed))
    g = packed["grp_img"].index(2)
    d0, d1 = 40 * packed["dt_off"][g], 40 * packed["dt_off"][g + 1]
    out["match"][d0:d1] = -7                          # garbage where the flag sends the group to the host
    out["nonfinite"][g] = 1
    calls = []
    got = ev_mod.Omni3Deval(gts, dts, "3D", iou3d_fn=oracle_iou3d)
    inner = got._evaluate_img
    got._evaluate_img = lambda img, cat, *a: calls.append((img, cat)) or inner(img, cat, *a)
    evalops.unpack(got, packed, out)
    H.assert_same_eval_imgs(got.evalImgs, want)
    assert set(calls) == {(2, 0)} and len(calls) == 4


def test_backend_argument_and_config_key():
    gts, dts = fixture()
    with pytest.raises(ValueError, match="backend"):
        ev_mod.Omni3Deval(gts, dts, "3D", backend="gpu")
    with pytest.raises(ValueError, match="iou3d_fn"):
        ev_mod.Omni3Deval(gts, dts, "3D", backend="device", iou3d_fn=oracle_iou3d)
    assert ev_mod.Omni3Deval(gts, dts, "3D").backend == "host" and ev_mod.Omni3Deval(gts, dts, "2D", backend="device").backend == "device"
    with pytest.raises(ValueError):
        ev_mod.check_backend("Host")
    import inspect
    for cls in (ev_mod.Omni3DEvaluator, ev_mod.Omni3DEvaluationHelper):
        assert inspect.signature(cls.__init__).parameters["backend"].default == "host"
    syn = importlib.import_module("3dod_amd.synthetic")
    cfg = syn.make_cfg()
    assert cfg.TEST.EVAL_BACKEND == "host"
    assert syn.make_cfg(overrides=["TEST.EVAL_BACKEND", "device"]).TEST.EVAL_BACKEND == "device"


def test_evaluator_and_helper_refuse_a_bad_backend_at_construction(monkeypatch):
    """the check runs before any dataset is touched"""
    with pytest.raises(ValueError, match="backend"):
        ev_mod.Omni3DEvaluator("no_such_dataset", backend="cuda")
    with pytest.raises(ValueError, match="backend"):
        ev_mod.Omni3DEvaluationHelper([], {}, "/nonexistent", backend="cuda")
    with pytest.raises(ValueError, match="iou3d_fn"):
        ev_mod.Omni3DEvaluationHelper([], {}, "/nonexistent", backend="device", iou3d_fn=oracle_iou3d)


def test_entry_points_are_declared_with_the_headers_arity():
    import os
    import re
    _lib = importlib.import_module("3dod_amd._lib")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cr3dod.h")).read()
    for name in ("cr_eval_iou_groups", "cr_eval_match_groups"):
        decl = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
