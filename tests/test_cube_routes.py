"""CPU: which entry points the 3D head's Python layer launches, and in which order, for every route of ops.cube_head_loss,
for ops.weak_cube_loss and for both forms of ops.cube_decode_infer.  _lib.call is replaced by a recorder that launches nothing
(the outputs stay uninitialised: only the names, their order and the argument counts are looked at)."""
import importlib

import pytest
import torch

ops = importlib.import_module("3dod_amd.hipops")
_lib = importlib.import_module("3dod_amd._lib")

B, S, KF, K, G = 2, 4, 3, 3, 2
N = B * KF


@pytest.fixture
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(ops, "_need_cuda", lambda t, name: None)
    monkeypatch.setattr(_lib, "call", lambda name, *args, device=None: rec.append((name, len(args))))
    return rec


def head_inputs(pose_width=6, conf=True):
    g = torch.Generator().manual_seed(0)
    layout = (0, 2 * K, 5 * K, (5 + pose_width) * K, (6 + pose_width) * K if conf else -1)
    raw = torch.randn(N, (6 + pose_width + (1 if conf else 0)) * K, generator=g).requires_grad_(True)
    cls = torch.randint(0, K, (B, S), generator=g)
    valid = torch.ones(B, S, dtype=torch.bool)
    gt_idx = torch.randint(0, G, (B, S), generator=g)
    gt3d, gtpose = torch.rand(B, G, 9, generator=g) + 0.5, torch.eye(3).repeat(B, G, 1, 1)
    meta = torch.tensor([[500.0, 500.0, 256.0, 256.0, 1.0]] * B)
    boxes = torch.tensor([[10.0, 20.0, 110.0, 140.0]] * N)
    return raw, layout, cls, valid, gt_idx, gt3d, gtpose, meta, boxes


def run_loss(calls, pose_width=6, conf=True, priors=None, **kw):
    raw, layout, cls, valid, gt_idx, gt3d, gtpose, meta, boxes = head_inputs(pose_width, conf)
    losses, u_sel, dec, buf, validf = ops.cube_head_loss(raw, layout, K, cls, valid, gt_idx, KF, gt3d, gtpose, priors, meta, boxes,
                                                         use_conf=conf, **kw)
    assert losses.shape == (N, 5) and u_sel.shape == (N,) and dec.shape == (N, 17) and buf.shape == (39 * N,) and validf.shape == (N,)
    (losses.sum() + u_sel.sum()).backward()
    assert raw.grad is not None and raw.grad.shape == raw.shape
    check_arity(calls)
    return [name for name, _ in calls]


def check_arity(calls):
    for name, nargs in calls:
        assert nargs == len(_lib.SIGNATURES[name]) - 1, (name, nargs)


def test_default_disentangled_route(calls):
    assert run_loss(calls, priors=torch.ones(K, 3)) == ["cr_cube_select", "cr_cube_loss_fwd", "cr_cube_loss_bwd", "cr_cube_select_bwd"]


def test_default_non_disentangled_route(calls):
    assert run_loss(calls, disentangled=False) == ["cr_cube_select", "cr_cube_select_norm", "cr_cube_nondis_fwd", "cr_cube_nondis_bwd",
                                                   "cr_cube_select_bwd"]


def test_default_non_disentangled_route_adds_the_raw_depth_gradient_off_direct(calls):
    assert run_loss(calls, disentangled=False, z_type="log") == ["cr_cube_select", "cr_cube_select_norm", "cr_cube_nondis_fwd",
                                                                 "cr_cube_nondis_bwd", "cr_cube_select_bwd", "cr_cube_select_bwd_zraw"]


def test_param_disentangled_route(calls):
    assert run_loss(calls, pose_width=4, pose_type="quaternion", priors=torch.ones(K, 3)) == [
        "cr_cube_select_param", "cr_cube_loss_fwd", "cr_cube_loss_bwd", "cr_cube_select_param_bwd"]


def test_param_non_disentangled_route(calls):
    want = ["cr_cube_select_param", "cr_cube_nondis_fwd", "cr_cube_nondis_bwd", "cr_cube_select_param_bwd"]
    assert run_loss(calls, conf=False, disentangled=False) == want
    del calls[:]
    assert run_loss(calls, pose_width=3, pose_type="euler", disentangled=False, z_type="sigmoid") == want


def test_weak_head_route(calls):
    raw, layout, cls, valid, gt_idx, gt3d, gtpose, meta, boxes = head_inputs()
    gt_boxes = torch.tensor([[10.0, 20.0, 110.0, 140.0]] * (B * G)).reshape(B, G, 4)
    red, stats, dec, pbox, validf = ops.weak_cube_loss(raw, layout, K, cls, valid, gt_idx, KF, gt_boxes, gt3d, gtpose, None, None, meta,
                                                       torch.zeros(B, 20), None, boxes, None, 0xFF, 0, (1.0,) * 9)
    assert red.shape == (9,) and dec.shape == (N, 17) and pbox.shape == (N, 4)
    red.sum().backward()
    assert raw.grad is not None and raw.grad.shape == raw.shape
    check_arity(calls)
    assert [name for name, _ in calls] == ["cr_cube_select", "cr_weak_loss_fwd", "cr_weak_loss_reduce", "cr_weak_loss_bwd",
                                           "cr_cube_select_bwd"]


def test_inference_decode_forms(calls):
    raw, layout, cls, _, _, _, _, _, boxes = head_inputs()
    args = (K, cls[:, :KF].reshape(-1), torch.zeros(N, dtype=torch.int64), boxes, torch.ones(B, 6), None)
    assert ops.cube_decode_infer(raw.detach(), layout, *args).shape == (N, 42)
    raw4, layout4 = head_inputs(4, False)[:2]
    assert ops.cube_decode_infer(raw4.detach(), layout4, *args, pose_type="quaternion", use_conf=False).shape == (N, 42)
    check_arity(calls)
    assert [name for name, _ in calls] == ["cr_cube_decode_infer", "cr_cube_decode_infer_param"]
