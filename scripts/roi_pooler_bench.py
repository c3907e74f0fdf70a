"""Measurements of the RoI pooler's other types / fixed sampling ratio -> profiles/roi_pooler_bench.json (merged per part).

    python scripts/roi_pooler_bench.py default --parent DIR     # DIR: a built checkout of the parent commit
    python scripts/roi_pooler_bench.py kernels

default  The default configuration computes and costs what it did: `bench.py --dump-outputs` of the train, weak and inference
         workloads compared byte by byte between the two trees, and `bench.py --gpus 1 --steps 20 --warmup 5`, parent and change
         alternated, three runs each, one process per run.  Guard: the change's median ms_per_step is no worse than the parent's
         median plus the parent's own spread (max - min).
kernels  The pooling kernels on the supervised train step's own RoIs (taken as scripts/roi_tile_load.py takes them: 4 x 512^2,
         512 sampled RoIs per image, C = 256, P = 7, f32): forward and backward us per call (device events around 20 calls after
         3 warm-up calls) of every type x ratio {0, 2} through cr_roi_pool_*, beside the default kernels through cr_roi_align_* in
         the same process, each with its HBM floor = algorithmic bytes / 6.29 TB/s (the measured copy rate of
         MI355X_MICROARCH.md): forward = output (+ argmax) written + every map read once; tile-owner backward = dY read + every
         map written once; atomic backward = dY (+ argmax) read + every map zero-filled, read and written once."""
import argparse
import ctypes
import filecmp
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "roi_pooler_bench.json")
HBM = 6.29e12


def merge(part):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    d = json.load(open(OUT)) if os.path.exists(OUT) else {}
    d.update(part)
    with open(OUT, "w") as f:
        json.dump(d, f, indent=1)


def bench(tree, extra, limit=300):
    """one bench.py process in `tree`; -> its JSON result line.  A failing or hanging run ends the script."""
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + extra, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("bench.py %s in %s: exit status %d" % (" ".join(extra), tree, p.returncode))
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def part_default(parent, dump_root):
    res = {"default_note": "default bench.py --gpus 1 runs (20 steps after 5 warm-up), parent and change alternated on one MI355X, one "
                           "process per run. Guard: the change's median ms_per_step is no worse than the parent's median plus the "
                           "parent's own spread (max - min). --dump-outputs (its own runs, deterministic weight-gradient reduce) of "
                           "train, weak and inference compared byte by byte between parent and change."}
    same = {}
    for w in ("train", "weak", "inference"):
        dirs = {}
        for name, tree in (("parent", parent), ("change", ROOT)):
            dirs[name] = os.path.join(dump_root, name, w)
            bench(tree, ["--workload", w, "--dump-outputs", dirs[name]])
        files = sorted(os.listdir(dirs["parent"]))
        differ = [f for f in files if not filecmp.cmp(os.path.join(dirs["parent"], f), os.path.join(dirs["change"], f), shallow=False)]
        same[w] = {"identical": files == sorted(os.listdir(dirs["change"])) and not differ, "files": len(files), "differ": differ}
        print("[dump]", w, same[w], flush=True)
    res["dump_outputs_byte_identical"] = same
    merge(res)
    runs = {"parent": [], "change": []}
    for i in range(3):
        for name, tree in (("parent", parent), ("change", ROOT)):
            r = bench(tree, ["--steps", "20", "--warmup", "5"])
            runs[name].append({k: r[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "dtype") if k in r})
            print("[step]", name, i, r["ms_per_step"], flush=True)
    summ = {}
    for name in runs:
        ms = [r["ms_per_step"] for r in runs[name]]
        summ[name] = {"summary": {"ms_per_step": ms, "median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms)}, "runs": runs[name]}
    bound = summ["parent"]["summary"]["median_ms"] + summ["parent"]["summary"]["spread_ms"]
    summ["guard"] = {"bound_ms": bound, "change_median_ms": summ["change"]["summary"]["median_ms"],
                     "met": summ["change"]["summary"]["median_ms"] <= bound}
    print("[guard]", summ["guard"], flush=True)
    merge({"train": summ})


def step_rois():
    """the RoIs the pooler sees in a supervised train step of the bench setup, and the shapes of its maps"""
    os.environ.setdefault("CR_GRAPHS", "none")
    import torch
    sys.path.insert(0, ROOT)
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    ops = importlib.import_module("3dod_amd.hipops")
    dev = torch.device("cuda:0")
    cfg, model, opt, syn, solver = bt.build(dev)
    batches = [syn.make_batch(4, 777 + i) for i in range(4)]
    for b in batches:
        for d in b:
            for k in ("image", "instances"):
                d[k] = d[k].to(dev)
    step = solver.TrainStep(cfg, model, opt, world_size=1)
    seen = []
    orig = ops.roi_align_pyramid

    def spy(feats, rois, scales, out_size, **kw):
        seen.append((rois.detach().clone(), [tuple(f.shape) for f in feats], tuple(scales), feats[0].dtype))
        return orig(feats, rois, scales, out_size, **kw)
    ops.roi_align_pyramid = spy
    with d2.EventStorage(1):
        for i in range(6):
            del seen[:]
            step(batches[i % 4])
    torch.cuda.synchronize()
    ops.roi_align_pyramid = orig
    return seen[0]


def part_kernels():
    import torch
    rois, shapes, scales, dt = step_rois()
    _lib = importlib.import_module("3dod_amd._lib")
    dev = rois.device
    g = torch.Generator().manual_seed(0)
    R, P, N, C = rois.shape[0], 7, shapes[0][0], shapes[0][3]
    feats = [torch.randn(s, generator=g).to(dev).to(dt) for s in shapes]
    dout = torch.randn(R, P, P, C, generator=g).to(dev).to(dt)
    grads = [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes]
    out = torch.empty(R, P, P, C, dtype=dt, device=dev)
    arg = torch.empty(R, P, P, C, dtype=torch.int32, device=dev)
    af = 1 if dt == torch.float32 else 0
    es = out.element_size()
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)

    def pyr(ts):
        n = len(ts)
        keep = ((ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]), (ctypes.c_int * n)(*[t.shape[1] for t in ts]),
                (ctypes.c_int * n)(*[t.shape[2] for t in ts]), (ctypes.c_float * n)(*[float(s) for s in scales]))
        return keep, [cast(k) for k in keep]
    kf, (fp, fH, fW, fs) = pyr(feats)
    kg, (gp, gH, gW, gs) = pyr(grads)
    nl = len(shapes)
    map_elems = sum(s[0] * s[1] * s[2] * s[3] for s in shapes)
    y_bytes = R * P * P * C * es

    def timed(fn, zero=False):
        for _ in range(3):                                   # (the zero fill is warmed up too: its first launch loads its code)
            if zero:
                torch._foreach_zero_(grads)
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            if zero:
                torch._foreach_zero_(grads)                  # the zero fill the atomic kernels need (what the step pays)
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 20 * 1e3

    rows = []
    modes = [("cr_roi_align_* (default kernels)", None, 0, 0)] + [("cr_roi_pool_* %s ratio %d" % (nm, ra), nm, pt, ra)
                                                                  for pt, nm in enumerate(("ROIAlignV2", "ROIAlign", "ROIPool"))
                                                                  for ra in ((0, 2) if pt < 2 else (0,))]
    for label, nm, pt, ra in modes:
        am = arg if pt == 2 else None
        if nm is None:
            fwd = lambda: _lib.call("cr_roi_align_fwd", fp, fH, fW, fs, nl, C, rois, R, P, P, out, af)
            tiles = lambda: _lib.call("cr_roi_align_bwd_set", gp, gH, gW, gs, nl, C, N, rois, R, P, P, dout, af)
            atomic = lambda: _lib.call("cr_roi_align_bwd", gp, gH, gW, gs, nl, C, rois, R, P, P, dout, af)
        else:
            fwd = lambda: _lib.call("cr_roi_pool_fwd", fp, fH, fW, fs, nl, C, N, rois, R, P, P, pt, ra, out, am, af)
            tiles = lambda: _lib.call("cr_roi_pool_bwd_set", gp, gH, gW, gs, nl, C, N, rois, R, P, P, pt, ra, dout, af)
            atomic = lambda: _lib.call("cr_roi_pool_bwd", gp, gH, gW, gs, nl, C, N, rois, R, P, P, pt, ra, dout, am, af)
        row = {"mode": label, "forward_us": timed(fwd),
               "forward_hbm_floor_us": (y_bytes + (R * P * P * C * 4 if pt == 2 else 0) + map_elems * es) / HBM * 1e6}
        if pt != 2:
            row["backward_tile_owner_us"] = timed(tiles)
            row["backward_tile_owner_hbm_floor_us"] = (y_bytes + map_elems * 4) / HBM * 1e6
        row["backward_atomic_with_zero_fill_us"] = timed(atomic, zero=True)
        row["backward_atomic_hbm_floor_us"] = (y_bytes + (R * P * P * C * 4 if pt == 2 else 0) + 3 * map_elems * 4) / HBM * 1e6
        row["backward_route_of_the_step"] = "atomic" if pt == 2 else "tile-owner"
        rows.append(row)
        print(json.dumps(row), flush=True)
    merge({"new_modes": {"note": "pooling kernels on the supervised train step's own RoIs; us per call, device events around 20 calls "
                                 "after 3 warm-up calls, one process; HBM floor = algorithmic bytes / 6.29 TB/s (see the script's "
                                 "docstring for the bytes counted)",
                         "rois": R, "maps": [list(s) for s in shapes], "pooled": [P, P], "dtype": str(dt).replace("torch.", ""),
                         "rows": rows}})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["default", "kernels"])
    ap.add_argument("--parent", default=None, help="default: a built checkout of the parent commit")
    ap.add_argument("--out", default=OUT, help="the JSON to merge into")
    ap.add_argument("--dumps", default=None, help="default: where the dumps go (a temporary directory if not given)")
    a = ap.parse_args()
    OUT = os.path.abspath(a.out)
    if a.part == "default":
        if not a.parent:
            ap.error("default needs --parent DIR")
        import tempfile
        part_default(os.path.abspath(a.parent), a.dumps or tempfile.mkdtemp(prefix="roi_pooler_dumps_"))
    else:
        part_kernels()
