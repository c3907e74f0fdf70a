"""Measurements of the RPN's / box head's other 2D loss options -> profiles/loss_options_bench.json (merged per part).

    python scripts/loss_options_bench.py default --parent DIR     # DIR: a built checkout of the parent commit
    python scripts/loss_options_bench.py kernels
    rocprofv3 --kernel-trace --stats -d DIR -o lossopt -- python scripts/loss_options_bench.py kernels --out /dev/null
    python scripts/loss_options_bench.py durations --db DIR/lossopt_results.db

default  as scripts/roi_pooler_bench.py's part of that name (its code): `bench.py --dump-outputs` of the train, weak and inference
         workloads byte by byte between the two trees, and `bench.py --gpus 1 --steps 20 --warmup 5`, parent and change alternated,
         three runs each, one process per run.
kernels  every variant of the two loss passes on the supervised train step's own tensors (4 x 512^2: the RPN's anchors of all five
         levels, the 512 sampled RoIs per image), us per call = device events around 50 calls after 5 warm-up calls, one process.  A
         call is the loss kernel plus the one-block reduction of its partial sums (two launches), as the step pays it.
durations  the kernels' own durations in a rocprofv3 kernel trace of the `kernels` part (a run of its own, as above): median / min /
         max us per template instantiation, read from the trace database (needs no GPU)."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "loss_options_bench.json")


def merge(part):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    d = json.load(open(OUT)) if os.path.exists(OUT) else {}
    d.update(part)
    with open(OUT, "w") as f:
        json.dump(d, f, indent=1)


def step_tensors():
    """the arguments ops.rpn_loss / ops.box_loss get in a supervised train step of the bench setup"""
    os.environ.setdefault("CR_GRAPHS", "none")
    import torch
    bt = importlib.import_module("bench_train")
    d2 = importlib.import_module("3dod_amd.d2lite")
    dense = importlib.import_module("3dod_amd.cubercnn.modeling.dense_train")
    dev = torch.device("cuda:0")
    cfg, model, opt, syn, solver = bt.build(dev)
    batches = [syn.make_batch(4, 777 + i) for i in range(4)]
    for b in batches:
        for d in b:
            for k in ("image", "instances"):
                d[k] = d[k].to(dev)
    step = solver.TrainStep(cfg, model, opt, world_size=1)
    seen = {}
    ops = dense.ops

    class Spy:
        def __getattr__(self, name):
            fn = getattr(ops, name)
            if name not in ("rpn_loss", "box_loss"):
                return fn

            def wrapped(*a, **kw):
                seen[name] = [x.detach().clone() if torch.is_tensor(x) else x for x in a]
                return fn(*a, **kw)
            return wrapped
    dense.ops = Spy()
    with d2.EventStorage(1):
        for i in range(4):
            step(batches[i % 4])
    torch.cuda.synchronize()
    dense.ops = ops
    return seen["rpn_loss"], seen["box_loss"]


def part_kernels():
    import torch
    ops = importlib.import_module("3dod_amd.hipops")
    rpn_args, box_args = step_tensors()

    def timed(fn):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(50):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 50 * 1e3

    rows = []
    with torch.no_grad():
        rpn_modes = [("cr_rpn_loss (default: IoU-weighted, L1)", ops.rpn_loss, {})]
        for none in (False, True):
            for beta in (0.0, 0.11):
                rpn_modes.append(("cr_rpn_loss_opt %s smooth_l1 beta %g" % ("none" if none else "IoU-weighted", beta), ops.rpn_loss_opt,
                                  dict(objectness_none=none, beta=beta)))
        for kind in ("giou", "diou", "ciou"):
            rpn_modes.append(("cr_rpn_loss_opt none " + kind, ops.rpn_loss_opt, dict(objectness_none=True, box_reg_loss_type=kind)))
        for label, fn, kw in rpn_modes:
            rows.append({"pass": "rpn", "mode": label, "us_per_call": timed(lambda: fn(*rpn_args, **kw))})
            print(json.dumps(rows[-1]), flush=True)
        agn_args = list(box_args)
        agn_args[1] = box_args[1][:, :4].contiguous()
        box_modes = [("cr_box_loss (default: L1, class-specific)", ops.box_loss, box_args, {})]
        for agn in (False, True):
            for beta in (0.0, 0.5):
                box_modes.append(("cr_box_loss_opt beta %g %s" % (beta, "class-agnostic" if agn else "class-specific"), ops.box_loss_opt,
                                  agn_args if agn else box_args, dict(beta=beta, cls_agnostic=agn)))
        for label, fn, args, kw in box_modes:
            rows.append({"pass": "box", "mode": label, "us_per_call": timed(lambda: fn(*args, **kw))})
            print(json.dumps(rows[-1]), flush=True)
    merge({"kernels": {"note": "loss kernel + reduction of its partial sums (two launches) through the Python binding, on the supervised "
                               "train step's own tensors; us per call, device events around 50 calls after 5 warm-up calls, one process. "
                               "At this size a call is launch-bound: the figures are the cost of two launches and their allocations.",
                       "rpn_logits": list(rpn_args[0].shape), "box_scores": list(box_args[0].shape), "rows": rows}})


def part_durations(db):
    import collections
    import sqlite3
    import statistics
    con = sqlite3.connect(db)
    rows = con.execute("select name, start, end from kernels where name like '%k_rpn_loss%' or name like '%k_box_loss%' "
                       "or name like '%k_sum_partials%' order by start").fetchall()
    per = collections.defaultdict(list)
    for name, start, end in rows:
        per[name.split("(")[0].replace("void ", "")].append((end - start) / 1e3)
    out = {n: {"calls": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
           for n, v in sorted(per.items())}
    for n, v in out.items():
        print(n, v)
    merge({"kernel_durations": {"note": "rocprofv3 --kernel-trace of the `kernels` part (one process, a run of its own): duration of "
                                        "every launch of each instantiation; <0, 0> and <false, false> are the default kernels (their "
                                        "count includes the four train steps the tensors are taken from); k_sum_partials follows every "
                                        "loss kernel", "kernels": out}})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["default", "kernels", "durations"])
    ap.add_argument("--parent", default=None, help="default: a built checkout of the parent commit")
    ap.add_argument("--out", default=OUT, help="the JSON to merge into")
    ap.add_argument("--db", default=None, help="durations: the rocprofv3 database of a traced `kernels` run")
    ap.add_argument("--dumps", default=None, help="default: where the dumps go (a temporary directory if not given)")
    a = ap.parse_args()
    OUT = os.path.abspath(a.out)
    if a.part == "default":
        if not a.parent:
            ap.error("default needs --parent DIR")
        import tempfile
        rp = importlib.import_module("roi_pooler_bench")
        rp.OUT = OUT
        rp.part_default(os.path.abspath(a.parent), a.dumps or tempfile.mkdtemp(prefix="loss_options_dumps_"))
    elif a.part == "durations":
        if not a.db:
            ap.error("durations needs --db FILE")
        part_durations(a.db)
    else:
        part_kernels()
