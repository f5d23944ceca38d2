#!/usr/bin/env python
"""Time PointRCNN's target assignment of csrc/rcnntarget_stage.hip at the shapes of the configuration (B = 8, N = 16384
points, 8 classes, 512 proposals, ROI_PER_IMAGE = 128, some 30 ground-truth boxes per sample padded to 48 rows) against
the plain per-sample / per-class formulation in the reference's shape (tests/rcnn_target_ref.py: masks, two point-in-box
searches, boolean-indexed scatters and the encode per sample; the trim with a host read per row, an IoU call per class
between host reads, nonzero and indexing per sample) on the same GPU in the same process.

Timing: wall time around each call with a synchronisation before and after (the plain formulation reads from the device
all along, so HIP events alone would not see its host side), after warm-up, the median and the spread over the steps; the
HIP op and the plain formulation alternate.  `launches` is what one call of the HIP op costs.

    python tools/bench_rcnn_target.py [--batch 8] [--points 16384] [--steps 20] [--warmup 5] [--table]
prints one JSON line (and, with --table, the markdown table of DESIGN.md).  No time is asserted anywhere.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfu3d_amd import rcnn_target_ops as ops  # noqa: E402
from dfu3d_amd.pcdet_kitti import box_coder_utils  # noqa: E402
from tests import rcnn_target_ref as T  # noqa: E402
from tests import roipoint_ref as R  # noqa: E402


def timed_pair(fns, steps, warmup):
    """The functions alternate, call by call; -> per function the median, p10 and p90 in ms."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0))
    return [dict(median_ms=float(np.median(m)), p10_ms=float(np.percentile(m, 10)), p90_ms=float(np.percentile(m, 90)))
            for m in ms]


def scene(B, N, G, rows, classes, M, seed, dev):
    """Clouds of N points around G boxes per sample (padded to `rows` rows), M proposals jittered from them."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((B, rows, 8), np.float32)
    gt[:, :G] = T.random_boxes(rng, B, G, classes=classes, spread=35.0)
    pts = rng.uniform(-40.0, 40.0, (B, N, 3)).astype(np.float32)
    pts[..., 2] *= np.float32(0.05)
    for b in range(B):                                        # a fifth of the points inside or just around a box
        g = rng.integers(0, G, N // 5)
        local = rng.uniform(-0.56, 0.56, (N // 5, 3)) * gt[b, g, 3:6]
        c, s = np.cos(gt[b, g, 6]), np.sin(gt[b, g, 6])
        pts[b, :N // 5, 0] = gt[b, g, 0] + local[:, 0] * c - local[:, 1] * s
        pts[b, :N // 5, 1] = gt[b, g, 1] + local[:, 0] * s + local[:, 1] * c
        pts[b, :N // 5, 2] = gt[b, g, 2] + local[:, 2]
    rois, labels = T.jittered_rois(rng, gt[:, :G], M)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    coords = torch.cat([torch.arange(B, device=dev).repeat_interleave(N)[:, None].float(), to(pts).view(-1, 3)], dim=1)
    return coords.contiguous(), to(gt), to(rois), to(labels), to(rng.uniform(0, 1, (B, M)).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--points', type=int, default=16384)
    ap.add_argument('--boxes', type=int, default=30)
    ap.add_argument('--rois', type=int, default=512)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--table', action='store_true')
    a = ap.parse_args()
    dev = 'cuda:0'
    B, N, G, M = a.batch, a.points, a.boxes, a.rois
    full = R.full_model_cfg()
    mean_size = full['POINT_HEAD']['TARGET_CONFIG']['BOX_CODER_CONFIG']['mean_size']
    extra = full['POINT_HEAD']['TARGET_CONFIG']['GT_EXTRA_WIDTH']
    cfg = full['ROI_HEAD']['TARGET_CONFIG']
    classes = len(mean_size)
    coords, gt, rois, labels, scores = scene(B, N, G, 48, classes, M, 2016, dev)
    mean = torch.tensor(mean_size, dtype=torch.float32, device=dev)
    coder = box_coder_utils.PointResidualCoder(use_mean_size=True, mean_size=mean_size)
    gen = torch.Generator(device=dev).manual_seed(1)
    inds = ops.proposal_targets(rois, scores, labels, gt, cfg, generator=gen)['sampled_inds']
    res = dict(batch=B, points=N, boxes=G, rois=M, classes=classes, sampled=cfg['ROI_PER_IMAGE'], steps=a.steps,
               device=torch.cuda.get_device_name(0), rows=[])
    pairs = [
        ('point_targets', ops.POINT_LAUNCHES,
         lambda: ops.point_targets(coords, gt, extra, classes, mean),
         lambda: T.plain_point_targets(coords, gt, extra, classes, coder)),
        ('roi_max_iou', ops.IOU_LAUNCHES,
         lambda: ops.roi_max_iou(rois, labels, gt, True),
         lambda: T.plain_max_iou(rois, labels, gt, True, T.gpu_iou3d)),
        ('proposal_targets', ops.IOU_LAUNCHES + ops.SAMPLE_LAUNCHES,
         lambda: ops.proposal_targets(rois, scores, labels, gt, cfg, generator=gen),
         lambda: T.plain_proposal_targets(rois, scores, labels, gt, cfg, inds, T.gpu_iou3d)),
    ]
    for name, launches, hip_fn, plain_fn in pairs:
        hip, plain = timed_pair([hip_fn, plain_fn], a.steps, a.warmup)
        res['rows'].append(dict(op=name, launches=launches, hip=hip, plain=plain))
    print(json.dumps(res))
    if a.table:
        print("| op | HIP launches | HIP median (p10 .. p90) ms | plain median (p10 .. p90) ms |")
        print("|---|---|---|---|")
        for r in res['rows']:
            print("| %s | %d | %.3f (%.3f .. %.3f) | %.2f (%.2f .. %.2f) |" % (
                r['op'], r['launches'], r['hip']['median_ms'], r['hip']['p10_ms'], r['hip']['p90_ms'],
                r['plain']['median_ms'], r['plain']['p10_ms'], r['plain']['p90_ms']))


if __name__ == '__main__':
    main()
