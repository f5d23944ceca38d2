"""Row f-11: time of the pillar scatter on the GPU -- the stage (bev_ops.pillar_scatter: three launches forward, one
backward) next to a torch-only comparator written for this tool: per sample a zero canvas, a boolean mask, an index
assignment of the transposed rows, and a stack (what a user without the stage would run; it reads the device where
boolean indexing does).  Both alternate in one process on the same inputs; HIP events around the call (warm-up,
median, p10 / p90 of the runs).  The config's shape: B = 4, C = 64, ny = 512, nx = 256, at P = 14 036 (the pillar count
of the encoder's benchmark) and P = 4 x 30 000.  Forward, and forward plus backward.  Also the stage's bytes per second
against its algorithmic bytes: the canvas written once, 4 P C read, the cell map cleared, marked and read.

With --model: one CenterPoint training step and one evaluation step at the full config with B = 4, split by module with
HIP events (no bar: there is nothing to compare it with).

    python tools/bench_pillar_scatter.py [--reps 50] [--warmup 10] [--pillars 14036,120000] [--model]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dfu3d_amd import bev_ops  # noqa: E402
from tools.bench_center_loss import launches, timed  # noqa: E402

B, C, NY, NX = 4, 64, 512, 256


def make(P, rng, dev):
    """P pillars on distinct cells, in the grouping's key order (b, x, y)."""
    cells = np.sort(rng.choice(B * NX * NY, size=P, replace=False))          # key = (b * NX + x) * NY + y
    b, x, y = cells // (NX * NY), cells % (NX * NY) // NY, cells % NY
    coords = np.stack([b, np.zeros_like(b), y, x], 1).astype(np.int32)
    return (torch.from_numpy(rng.standard_normal((P, C)).astype(np.float32)).to(dev), torch.from_numpy(coords).to(dev))


def comparator(features, coords):
    """Not the code under test."""
    out = []
    for b in range(B):
        canvas = torch.zeros(C, NX * NY, dtype=features.dtype, device=features.device)
        mask = coords[:, 0] == b
        this = coords[mask, :]
        idx = (this[:, 1] + this[:, 2] * NX + this[:, 3]).long()
        canvas[:, idx] = features[mask, :].t()
        out.append(canvas)
    return torch.stack(out, 0).view(B, C, NY, NX)


def scatter_rows(args, dev):
    for P in (int(v) for v in args.pillars.split(",")):
        f, coords = make(P, np.random.default_rng(P), dev)
        f.requires_grad_(True)
        grad = torch.randn(B, C, NY, NX, device=dev)
        out = torch.empty(B, C, NY, NX, device=dev)

        def both(fn):
            f.grad = None
            fn().backward(grad)
        paths = {"stage": lambda: bev_ops.pillar_scatter(f.detach(), coords, B, (NX, NY, 1), out=out),
                 "torch_comparator": lambda: comparator(f.detach(), coords)}
        paths_fb = {"stage": lambda: both(lambda: bev_ops.pillar_scatter(f, coords, B, (NX, NY, 1))),
                    "torch_comparator": lambda: both(lambda: comparator(f, coords))}
        same = bool(torch.equal(paths["stage"]().view(torch.int32), paths["torch_comparator"]().view(torch.int32)))
        paths_fb["stage"]()
        g_stage = f.grad.clone()
        paths_fb["torch_comparator"]()
        same_grad = bool(torch.equal(g_stage.view(torch.int32), f.grad.view(torch.int32)))
        cells = B * NY * NX
        nbytes = {"forward": 4 * C * cells + 4 * P * C + 2 * 4 * cells + 16 * P}
        nbytes["forward_backward"] = nbytes["forward"] + 2 * 4 * P * C + 4 * cells + 16 * P
        for what, fns in (("forward", paths), ("forward_backward", paths_fb)):
            t = timed(fns, args.reps, warmup=args.warmup)
            for name in fns:
                e, p10, p90, w = t[name]
                row = {"what": "pillar_scatter", "pass": what, "path": name, "B": B, "C": C, "ny": NY, "nx": NX, "P": P,
                       "gpu_event_ms": round(e, 4), "p10": round(p10, 4), "p90": round(p90, 4), "call_ms": round(w, 4),
                       "kernels": launches(fns[name]), "same_canvas_bits": same, "same_gradient_bits": same_grad}
                if name == "stage":
                    row["algorithmic_MB"] = round(nbytes[what] / 1e6, 1)
                    row["algorithmic_GB_per_s"] = round(nbytes[what] / (e * 1e-3) / 1e9, 1)
                    row["median_below_comparator_p10"] = bool(e < t["torch_comparator"][1])
                print(json.dumps(row), flush=True)


def model_rows(args, dev):
    """One training and one evaluation step of the full config, B = 4, split by module."""
    from dfu3d_amd.pcdet_kitti.centerpoint import CenterPoint
    from tests import centerpoint_cases as K
    rng = np.random.default_rng(0)
    r = K.FULL_DATASET['point_cloud_range']
    n = 30000
    pts = np.concatenate([np.stack([np.full(n, b), rng.uniform(r[0], r[3], n), rng.uniform(r[1], r[4], n),
                                    rng.uniform(-3, 1, n), rng.random(n)], 1) for b in range(B)]).astype(np.float32)
    gt = np.zeros((B, 20, 8), np.float32)
    gt[:, :, 0:3] = rng.uniform([r[0] + 2, r[1] + 2, -2], [r[3] - 2, r[4] - 2, 0], (B, 20, 3))
    gt[:, :, 3:6] = rng.uniform([1.5, 0.6, 1.2], [5, 2.2, 2], (B, 20, 3))
    gt[:, :, 6] = rng.uniform(-3, 3, (B, 20))
    gt[:, :, 7] = rng.integers(1, 11, (B, 20))
    torch.manual_seed(0)
    model = CenterPoint(K.cfg(K.FULL_MODEL), len(K.FULL_CLASSES), **K.FULL_DATASET).to(dev)

    def batch():
        return {'batch_size': B, 'points': torch.from_numpy(pts).to(dev), 'gt_boxes': torch.from_numpy(gt).to(dev)}
    marks = []

    def mark(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))
    for m_name in ('vfe', 'map_to_bev_module', 'backbone_2d', 'dense_head'):
        getattr(model, m_name).register_forward_hook(lambda mod, a, o, m_name=m_name: mark(m_name))
    opt = torch.optim.SGD(model.parameters(), lr=1e-4)
    for mode in ("train", "eval"):
        model.train(mode == "train")
        runs = []
        for rep in range(args.warmup // 2 + max(args.reps // 5, 3)):
            d = batch()
            torch.cuda.synchronize()
            del marks[:]
            mark("start")
            if mode == "train":
                ret, _, _ = model(d)
                mark("loss")
                opt.zero_grad()
                ret['loss'].backward()
                mark("backward")
                opt.step()
                mark("optimizer")
            else:
                with torch.no_grad():
                    model(d)
                mark("post_processing")
            torch.cuda.synchronize()
            if rep >= args.warmup // 2:
                runs.append({marks[i][0]: marks[i - 1][1].elapsed_time(marks[i][1]) for i in range(1, len(marks))})
        row = {"what": "centerpoint_step", "mode": mode, "B": B, "points": len(pts), "runs": len(runs)}
        row.update({k + "_ms": round(statistics.median(x[k] for x in runs), 3) for k in runs[0]})
        row["total_ms"] = round(statistics.median(sum(x.values()) for x in runs), 3)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pillars", default="14036,120000")
    ap.add_argument("--model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    scatter_rows(args, dev)
    if args.model:
        model_rows(args, dev)


if __name__ == "__main__":
    main()
