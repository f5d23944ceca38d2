"""Row f-10: time of the world augmentation + range masks + collate on the GPU -- the stage (stages.world_aug_collate, four
launches) next to a torch-only composition of the same steps on the same GPU (per-scene slices, matmul, boolean masks,
cat; it synchronises where boolean indexing does).  Both alternate in one process on the same inputs; HIP events around
the call (warm-up, median, p10 / p90 of the runs).  B scenes of 34 720 points plus 4 000 pasted object points each (the
f-5 bench's sizes), 4 point columns, 40 float32 boxes per scene, every world entry on, the KITTI range.  Also the
stage's bytes per second against its algorithmic bytes: 4 C read per input point, 4 (C + 1) written per kept point.

    python tools/bench_world_aug.py [--reps 50] [--warmup 10] [--batches 4,64]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dfu3d_amd import stages as st  # noqa: E402
from dfu3d_amd.pcdet_kitti.data_augmentor import params_record  # noqa: E402
from tools.bench_center_loss import launches, timed  # noqa: E402

RANGE = [0.0, -39.68, -3.0, 69.12, 39.68, 1.0]
N_SCENE, N_OBJ, N_BOX, C = 34720, 4000, 40, 4


def make(B, rng, dev):
    n = N_SCENE + N_OBJ
    pts = np.zeros((B * n, C), np.float32)
    pts[:, 0] = rng.uniform(-10, 80, B * n)
    pts[:, 1] = rng.uniform(-50, 50, B * n)
    pts[:, 2] = rng.uniform(-3, 1, B * n)
    pts[:, 3] = rng.random(B * n)
    boxes = np.zeros((B * N_BOX, 7), np.float32)
    boxes[:, 0:3] = rng.uniform([-5, -45, -3.5], [75, 45, 1.5], (B * N_BOX, 3))
    boxes[:, 3:6] = rng.uniform(0.5, 5, (B * N_BOX, 3))
    boxes[:, 6] = rng.uniform(-7, 7, B * N_BOX)
    drawn = [{'flips': [('x', bool(rng.integers(2)))], 'noise_rot': float(rng.uniform(-0.785, 0.785)),
              'noise_scale': float(rng.uniform(0.95, 1.05)),
              'noise_translate': rng.normal(0, 0.5, (1, 3)).astype(np.float32)} for _ in range(B)]
    recs = [params_record(d) for d in drawn]
    h = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return {'points': h(pts), 'point_off': h(np.arange(B + 1, dtype=np.int64) * n), 'boxes': h(boxes),
            'box_off': h(np.arange(B + 1, dtype=np.int32) * N_BOX), 'box_cnt': h(np.full(B, N_BOX, np.int32)),
            'box_cls': h(rng.integers(0, 4, B * N_BOX).astype(np.int32)), 'params': h(st.aug_params(recs)),
            'range': h(np.array(RANGE, np.float32)), 'recs': recs, 'n': n, 'B': B}


def stage(u, status):
    return st.world_aug_collate(u['points'], u['point_off'], u['boxes'], u['box_off'], u['box_cnt'], u['box_cls'],
                                u['params'], u['range'], st.AUG_MASK_POINTS | st.AUG_MASK_BOXES | st.AUG_FILTER_CLASS,
                                N_BOX, status)


def torch_composition(u):
    """The comparator: the same steps with torch ops only.  Not the code under test."""
    r = u['range']
    pts_out, box_out = [], []
    two_pi = torch.tensor(2 * np.pi, dtype=torch.float32, device=r.device)
    for b, rec in enumerate(u['recs']):
        p = u['points'][b * u['n']:(b + 1) * u['n']].clone()
        g = u['boxes'][b * N_BOX:(b + 1) * N_BOX].clone()
        cls = u['box_cls'][b * N_BOX:(b + 1) * N_BOX]
        if rec['flags'] & st.AUG_FLIP_X:
            p[:, 1] = -p[:, 1]
            g[:, 1] = -g[:, 1]
            g[:, 6] = -g[:, 6]
        c, s = rec['cos_a'], rec['sin_a']
        rot = torch.tensor([[c, s, 0], [-s, c, 0], [0, 0, 1]], dtype=torch.float32, device=r.device)
        p[:, 0:3] = p[:, 0:3] @ rot
        g[:, 0:3] = g[:, 0:3] @ rot
        g[:, 6] += rec['noise_rot_f']
        p[:, 0:3] *= rec['scale_f']
        g[:, 0:6] *= rec['scale_f']
        t = torch.tensor([rec['tx'], rec['ty'], rec['tz']], dtype=torch.float32, device=r.device)
        p[:, 0:3] += t
        g[:, 0:3] += t
        g[:, 6] = g[:, 6] - torch.floor(g[:, 6] / two_pi + 0.5) * two_pi
        keep = (p[:, 0] >= r[0]) & (p[:, 0] <= r[3]) & (p[:, 1] >= r[1]) & (p[:, 1] <= r[4])
        p = p[keep]
        pts_out.append(torch.cat([torch.full((len(p), 1), float(b), device=r.device), p], 1))
        kb = (cls > 0) & ((g[:, 0:3] >= r[0:3]) & (g[:, 0:3] <= r[3:6])).all(-1)
        box_out.append(torch.cat([g[kb], cls[kb].float()[:, None]], 1))
    gt = torch.zeros((u['B'], max(len(x) for x in box_out), 8), device=r.device)
    for b, x in enumerate(box_out):
        gt[b, :len(x)] = x
    return torch.cat(pts_out, 0), gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", default="4,64")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for B in (int(v) for v in args.batches.split(",")):
        u = make(B, np.random.default_rng(B), dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        fns = {"stage": lambda: stage(u, status), "torch_composition": lambda: torch_composition(u)}
        t = timed(fns, args.reps, warmup=args.warmup)
        out, n_kept, _, gt, gt_cnt, _, _ = fns["stage"]()
        tp, tg = fns["torch_composition"]()
        kept = int(n_kept.item())
        same_rows = kept == len(tp) and int(gt_cnt.sum()) == int((tg[:, :, 7] > 0).sum())
        close = same_rows and bool(torch.allclose(out[:kept], tp, rtol=0, atol=1e-4))
        nbytes = 4 * C * B * u['n'] + 4 * (C + 1) * kept
        for name in fns:
            e, p10, p90, w = t[name]
            row = {"what": "world_aug", "path": name, "B": B, "points": B * u['n'], "kept": kept,
                   "gpu_event_ms": round(e, 4), "p10": round(p10, 4), "p90": round(p90, 4), "call_ms": round(w, 4),
                   "kernels": launches(fns[name]), "same_decisions_as_comparator": same_rows, "values_close": close}
            if name == "stage":
                row["algorithmic_GB_per_s"] = round(nbytes / (e * 1e-3) / 1e9, 1)
                row["median_below_comparator_p10"] = bool(e < t["torch_composition"][1])
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
