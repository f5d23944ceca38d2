"""Row f-6: time of CenterHead.assign_targets and decode_bbox_from_heatmap on the GPU (kernel time by HIP events: warm-up,
many repetitions, median; whole-call time by the host clock around call + synchronise) next to the CPU restatement
(tests/center_head_ref.py) on the same host, with a parity flag.  Configuration A of the CenterPoint config, about 30
boxes per sample, B = 4 (the config's batch) and B = 64.

    python tools/bench_center_head.py [--reps 200]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import center_head_ref as ref  # noqa: E402
from dfu3d_amd.pcdet_kitti import centernet_utils  # noqa: E402
from dfu3d_amd.pcdet_kitti.center_head import CenterHead  # noqa: E402


def gpu_times(fn, reps, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return statistics.median(ev), statistics.median(wall)


def scene(rng, cfg, B, n):
    r = cfg['point_cloud_range']
    gt = np.zeros((B, 64, 8), np.float32)
    gt[:, :n, 0] = rng.uniform(r[0], r[3], (B, n))
    gt[:, :n, 1] = rng.uniform(r[1], r[4], (B, n))
    gt[:, :n, 2] = rng.uniform(-3, 1, (B, n))
    gt[:, :n, 3:6] = rng.uniform([0.5, 0.4, 0.8], [10, 3, 3.5], (B, n, 3))
    gt[:, :n, 6] = rng.uniform(-3.14, 3.14, (B, n))
    gt[:, :n, 7] = rng.integers(1, len(cfg['class_names']) + 1, (B, n))
    return gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    cfg = ref.CFG_A
    H, W = cfg['map_hw']
    model_cfg = dict(CLASS_NAMES_EACH_HEAD=cfg['heads'],
                     TARGET_ASSIGNER_CONFIG=dict(FEATURE_MAP_STRIDE=cfg['stride'], NUM_MAX_OBJS=cfg['num_max_objs'],
                                                 GAUSSIAN_OVERLAP=cfg['gaussian_overlap'], MIN_RADIUS=cfg['min_radius']))
    head = CenterHead(model_cfg, cfg['class_names'], np.array(cfg['point_cloud_range'], np.float32), cfg['voxel_size'])
    rng = np.random.default_rng(0)
    lim = [0, -61.2, -10.0, 61.2, 61.2, 10.0]
    for B in (4, 64):
        gt = scene(rng, cfg, B, 30)
        gt_t = torch.from_numpy(gt).cuda()
        k_ms, call_ms = gpu_times(lambda: head.assign_targets(gt_t, feature_map_size=[H, W]), args.reps)
        t0 = time.perf_counter()
        want = ref.assign_targets(gt, cfg)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        got = head.assign_targets(gt_t, feature_map_size=[H, W], check=True)
        parity = all(np.array_equal(got[k][h].cpu().numpy()[..., :3], want[k][h][..., :3]) for h in range(6)
                     for k in ('inds', 'masks', 'target_boxes', 'target_boxes_src')) and \
            all(ref.ulp_diff(got['heatmaps'][h].cpu().numpy(), want['heatmaps'][h]).max() <= 1 for h in range(6))
        print(json.dumps({"what": "assign_targets", "B": B, "boxes_per_sample": 30, "gpu_event_ms": round(k_ms, 4),
                          "gpu_call_ms": round(call_ms, 4), "cpu_restatement_ms": round(cpu_ms, 2), "parity": bool(parity)}))
        d = ref.decode_inputs(3, B, 2, H, W, False, False)
        t = {k: (None if v is None else torch.from_numpy(v).cuda()) for k, v in d.items()}
        kw = dict(point_cloud_range=cfg['point_cloud_range'], voxel_size=cfg['voxel_size'], feature_map_stride=cfg['stride'],
                  K=500, score_thresh=0.1, post_center_limit_range=torch.tensor(lim).cuda())
        raw = lambda: centernet_utils.decode_raw(t['heatmap'], t['rot_cos'], t['rot_sin'], t['center'], t['center_z'],  # noqa: E731
                                                 t['dim'], **kw)
        k_ms, _ = gpu_times(raw, args.reps)
        full = lambda: centernet_utils.decode_bbox_from_heatmap(t['heatmap'], t['rot_cos'], t['rot_sin'], t['center'],  # noqa: E731
                                                                t['center_z'], t['dim'], **kw)
        _, call_ms = gpu_times(full, args.reps)
        t0 = time.perf_counter()
        want = ref.decode_bbox_from_heatmap(d['heatmap'], d['rot_cos'], d['rot_sin'], d['center'], d['center_z'], d['dim'],
                                            cfg['point_cloud_range'], cfg['voxel_size'], cfg['stride'], K=500,
                                            score_thresh=0.1, post_center_limit_range=lim)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        got = full()
        parity = all(np.array_equal(g['pred_labels'].cpu().numpy(), w['pred_labels'])
                     and g['pred_scores'].cpu().numpy().tobytes() == w['pred_scores'].tobytes()
                     and g['pred_boxes'].cpu().numpy()[:, :6].tobytes() == w['pred_boxes'][:, :6].tobytes()
                     for g, w in zip(got, want))
        print(json.dumps({"what": "decode_bbox_from_heatmap", "B": B, "K": 500, "scores_per_sample": 2 * H * W,
                          "gpu_event_ms": round(k_ms, 4), "gpu_call_ms": round(call_ms, 4),
                          "cpu_restatement_ms": round(cpu_ms, 2), "parity": bool(parity)}))


if __name__ == "__main__":
    main()
