"""HIP path of the weakly supervised 3D head: cr_box_median bit-exact against the oracle's torch.median loop, and the
whole ROIHeads3DScore._forward_cube (RANSAC kernel with the triples the reference drew + median kernel) against the
reference's recorded outputs."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

geo = importlib.import_module("3dod_amd.geometry")
from oracle import weak as ow                      # noqa: E402
from test_weakhead import check_case               # noqa: E402


def test_box_median_bit_exact():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    depth = torch.randn(3, 97, 131, generator=g) * 3
    depth[1] = torch.randint(0, 4, (97, 131), generator=g).float()          # many duplicates
    depth[2, :40] = -depth[2, :40].abs()                                   # negative block
    depth[2, 50, 60] = 0.0
    depth[2, 50, 61] = -0.0
    n = 300
    x1 = torch.randint(-5, 131, (n,), generator=g)
    y1 = torch.randint(-5, 97, (n,), generator=g)
    x2 = x1 + torch.randint(0, 140, (n,), generator=g)
    y2 = y1 + torch.randint(0, 100, (n,), generator=g)
    boxes = torch.stack((x1, y1, x2, y2), 1).to(torch.int32)
    boxes[0] = torch.tensor([0, 0, 131, 97])                               # the whole map
    boxes[1] = torch.tensor([5, 5, 5, 20])                                 # empty
    boxes[2] = torch.tensor([7, 9, 8, 10])                                 # one pixel
    boxes[3] = torch.tensor([60, 50, 62, 51])                              # {0.0, -0.0}
    img = torch.randint(0, 3, (n,), generator=g).to(torch.int32)
    img[3] = 2
    want = ow.box_median(depth, boxes.clamp(min=0), img)
    got = geo.box_median(depth.to(dev), boxes.to(dev), img.to(dev)).cpu()
    nan = torch.isnan(want)
    assert nan[1] and torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan], want[~nan])                               # selection: bit-exact values
    assert (~nan).sum() > 200


def test_box_median_full_size_maps():
    """4 x 512 x 512 maps, 512 windows up to the whole image (the size of the train step's depth maps)"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    depth = torch.rand(4, 512, 512, generator=g) * 8 + 0.5
    n = 512
    c = torch.rand(n, 2, generator=g) * 512
    wh = torch.rand(n, 2, generator=g) * 500 + 2
    boxes = torch.cat((c - wh / 2, c + wh / 2), 1).clamp(0, 512).long().to(torch.int32)
    boxes[0] = torch.tensor([0, 0, 512, 512])
    img = torch.randint(0, 4, (n,), generator=g).to(torch.int32)
    got = geo.box_median(depth.to(dev), boxes.to(dev), img.to(dev)).cpu()
    want = ow.box_median(depth, boxes, img)
    assert torch.equal(got, want)


def test_hull8_matches_the_reference_march():
    """random corner sets, sets with duplicated points (the reference bumps them apart), clamped (collinear) sets"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    pts = torch.rand(200, 8, 2, generator=g) * 300
    pts[20:60] = pts[20:60].round()                                   # integer coordinates: collinear triples and ties
    pts[60:90, 3] = pts[60:90, 0]                                     # one duplicate
    pts[90:110, 5] = pts[90:110, 0]
    pts[90:110, 6] = pts[90:110, 1]                                   # two different duplicates
    pts[110:130, 2] = pts[110:130, 0]
    pts[110:130, 4] = pts[110:130, 0]                                 # a triple
    pts[130:160, :, 0] = pts[130:160, :, 0].clamp(50, 120).round()    # many points on the clamp lines
    pts[160:180] = pts[160:180].clamp(0, 40).round()
    o, c, b = geo.hull8(pts.to(dev))
    oo, oc, ob = ow.hull8(pts)
    assert torch.equal(c.cpu(), oc) and torch.equal(b.cpu(), ob)
    for r in range(pts.shape[0]):
        k = int(oc[r])
        assert o[r, :k].cpu().tolist() == oo[r, :k].tolist(), r
    assert int(oc.min()) >= 2 and int(oc.max()) <= 8 and float(ob.max()) >= 2


def test_polygon_focal_forward_and_gradient():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    H, W, n = 96, 128, 12
    ctr = torch.rand(n, 1, 2, generator=g) * torch.tensor([W * 0.6, H * 0.6]) + torch.tensor([W * 0.2, H * 0.2])
    pts = ctr + (torch.rand(n, 8, 2, generator=g) - 0.5) * 60
    pts[:3] = pts[:3].round()                                         # integer vertices: clamp arguments hit 0 / 1 exactly
    masks = torch.zeros(5, H, W, dtype=torch.uint8)
    for i in range(5):
        masks[i, 10 + 9 * i:60 + 5 * i, 20 + 11 * i:90 + 6 * i] = 1
    midx = torch.randint(0, 5, (n,), generator=g)
    order, count, bump = ow.hull8(pts)
    base = (pts + bump[..., None])

    def run(fn, device):
        p = base.clone().to(device).requires_grad_()
        hull = torch.gather(p, 1, order.to(device)[..., None].expand(-1, -1, 2))
        loss = fn(hull, count.to(device), masks.to(device), midx.to(device))
        (loss * torch.arange(1, n + 1, device=device)).sum().backward()
        return loss.detach().cpu(), p.grad.cpu()
    l_ref, g_ref = run(ow.polygon_focal, torch.device("cpu"))
    l_hip, g_hip = run(geo.polygon_focal, dev)
    assert torch.allclose(l_hip, l_ref, rtol=2e-4, atol=1e-6), (l_hip - l_ref).abs().max()
    assert float((g_hip - g_ref).abs().max()) <= 2e-3 * float(g_ref.abs().max()) + 1e-7, ((g_hip - g_ref).abs().max(), g_ref.abs().max())
    assert float(g_ref.abs().max()) > 0


@pytest.mark.parametrize("name", ["weakhead_a.npz", "weakhead_b.npz", "weakhead_c.npz", "weakhead_d.npz"])
def test_forward_cube_matches_reference_hip(name):
    check_case(name, torch.device("cuda:0"), (None, None))


@pytest.mark.parametrize("dense", [True, False])
def test_weak_model_trains_from_the_data_path(tmp_path, monkeypatch, dense):
    """configs/Omni_combined.yaml (RCNN3D_combined_features + ROIHeads3DScore) fed by the Omni3D loader with depth and
    ground maps: a few SGD steps with finite losses of every configured kind, then inference through the same model."""
    import os
    syn = importlib.import_module("3dod_amd.synthetic")
    data = importlib.import_module("3dod_amd.cubercnn.data")
    D = importlib.import_module("3dod_amd.d2lite.data")
    d2 = importlib.import_module("3dod_amd.d2lite")
    util = importlib.import_module("3dod_amd.cubercnn.util")
    modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
    solver = importlib.import_module("3dod_amd.cubercnn.solver")
    dev = torch.device("cuda:0")
    root = tmp_path / "datasets"
    root.mkdir()
    syn.make_omni3d_dataset(str(root), name="Synth_train", n_images=12, seed=5)
    monkeypatch.chdir(tmp_path)
    for n in list(D.DatasetCatalog):
        D.DatasetCatalog.remove(n)
    for n in ("omni3d_model", "Synth_train"):
        D.MetadataCatalog.pop(n, None)
    cats = ["bed", "car", "chair", "sofa", "table", "truck"]
    here = os.path.dirname(os.path.abspath(__file__))
    cfg = syn.make_cfg(os.path.join(here, "..", "configs", "Omni_combined.yaml"), overrides=[
        "MODEL.DEVICE", str(dev), "DATASETS.TRAIN", ("Synth_train",), "DATASETS.TEST", ("Synth_train",),
        "DATASETS.CATEGORY_NAMES", cats, "MODEL.ROI_HEADS.NUM_CLASSES", len(cats), "SOLVER.IMS_PER_BATCH", 2,
        "DATALOADER.NUM_WORKERS", 0, "INPUT.MIN_SIZE_TRAIN", (256,), "INPUT.MAX_SIZE_TRAIN", 512, "INPUT.MIN_SIZE_TEST", 256,
        "INPUT.MAX_SIZE_TEST", 512, "SOLVER.BASE_LR", 0.001, "VIS_PERIOD", 0, "log", False, "SEED", 2])
    fs = data.get_filter_settings_from_cfg(cfg)
    omni = data.Omni3D([os.path.join("datasets", "Omni3D", "Synth_train.json")], filter_settings=fs)
    data.register_and_store_model_metadata(omni, str(tmp_path), fs)
    data.simple_register("Synth_train", fs, filter_empty=True)
    meta = D.MetadataCatalog.get("omni3d_model")
    unknown, id_to_src = data.build.dataset_id_maps(omni, len(cats), meta.thing_dataset_id_to_contiguous_id)
    mapper = data.DatasetMapper3D(cfg, is_train=True)
    mapper.dataset_id_to_unknown_cats = unknown
    np.random.seed(0)
    torch.manual_seed(0)
    model = modeling.build_model(cfg, priors=util.compute_priors(cfg, omni)).train()
    assert type(model).__name__ == "RCNN3D_combined_features" and type(model.roi_heads).__name__ == "ROIHeads3DScore"
    model.dense_train = dense          # fused static-shape RPN / sampling / box head, or the instance-list path
    if not dense:
        from oracle import list_path
        list_path.install(model)       # the per-image list formulation is test infrastructure (oracle/list_path.py)
    opt = solver.build_optimizer(cfg, model)
    step = solver.TrainStep(cfg, model, opt, world_size=1)
    feed = data.DevicePrefetcher(data.build_detection_train_loader(cfg, mapper=mapper, dataset_id_to_src=id_to_src,
                                                                   rank=0, world_size=1), dev)
    with d2.EventStorage(1):
        for _ in range(3):
            step(next(feed))
        rep = step.report()
    want = {"Cube/loss_iou", "Cube/loss_pose", "Cube/loss_normal_vec", "Cube/loss_z", "Cube/loss_pseudo_gt_z",
            "Cube/loss_dims_w", "Cube/uncert", "BoxHead/loss_cls", "rpn/cls"}
    assert want <= set(rep), sorted(rep)
    assert all(v == v and abs(v) < 1e5 for v in rep.values()), rep

    model.eval()
    with torch.no_grad():
        outs = model(next(iter(data.build_detection_test_loader(cfg, "Synth_train", batch_size=2, rank=0, world_size=1,
                                                                num_workers=0))))
    assert len(outs) == 2 and all("instances" in o for o in outs)


@pytest.mark.parametrize("dense", [True, False])
def test_mask_losses_through_a_pluggable_segmentor(dense):
    """'segmentation' and 'depth' need one mask per GT object; the model takes them from `roi_heads.segmentor` (SAM-HQ in
    the reference).  Here: the GT box as mask."""
    import os
    syn = importlib.import_module("3dod_amd.synthetic")
    d2 = importlib.import_module("3dod_amd.d2lite")
    modeling = importlib.import_module("3dod_amd.cubercnn.modeling")
    solver = importlib.import_module("3dod_amd.cubercnn.solver")
    dev = torch.device("cuda:0")
    here = os.path.dirname(os.path.abspath(__file__))
    cfg = syn.make_cfg(os.path.join(here, "..", "configs", "Omni_combined.yaml"), overrides=[
        "MODEL.DEVICE", str(dev), "SOLVER.BASE_LR", 0.001, "VIS_PERIOD", 0, "log", False,
        "loss_functions", ["dims", "iou", "segmentation", "depth", "z_pseudo_gt_center"]])
    torch.manual_seed(0)
    model = modeling.build_model(cfg).train()
    model.dense_train = dense
    if not dense:
        from oracle import list_path
        list_path.install(model)
    opt = solver.build_optimizer(cfg, model)
    step = solver.TrainStep(cfg, model, opt, world_size=1)
    batch = syn.add_scene_maps(syn.make_batch(2, 31, size=256), 5)
    for d in batch:
        d["image"], d["instances"], d["depth_map"], d["ground_map"] = d["image"].to(dev), d["instances"].to(dev), d["depth_map"].to(dev), d["ground_map"].to(dev)
    with d2.EventStorage(1):
        with pytest.raises(RuntimeError, match="segmentor"):
            step(batch)
        seen = {}

        def box_segmentor(images_raw, targets):
            seen["shape"], seen["dtype"] = tuple(images_raw.shape), images_raw.dtype
            out = []
            for t in targets:
                m = torch.zeros((len(t), 1) + tuple(images_raw.shape[-2:]), dtype=torch.bool, device=images_raw.device)
                for j, b in enumerate(t.gt_boxes.tensor.long().tolist()):
                    m[j, 0, b[1]:b[3], b[0]:b[2]] = True
                out.append(m)
            return out
        model.roi_heads.segmentor = box_segmentor
        opt.zero_grad()
        for _ in range(2):
            step(batch)
        rep = step.report()
    assert seen["shape"] == (2, 3, 256, 256) and seen["dtype"] == torch.uint8
    assert {"Cube/loss_seg", "Cube/loss_depth", "Cube/loss_iou"} <= set(rep), sorted(rep)
    assert all(v == v and abs(v) < 1e5 for v in rep.values()), rep
