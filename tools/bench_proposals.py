#!/usr/bin/env python
"""Time PointRCNN's proposal stage for a whole batch (csrc/proposal_stage.hip through PointRCNNHead.proposal_layer_batched)
against the per-sample loop it stands in for (PointRCNNHead.proposal_layer, unchanged: topk, argsort, gather, the whole
suppression mask, the walk, a host read and four index assignments per sample) at the shapes of the configuration:
N = 16384 points per sample, NMS_PRE_MAXSIZE = 9000, (NMS_POST_MAXSIZE, NMS_THRESH) = (512, 0.8) in training and
(100, 0.85) in evaluation, for B = 8 and B = 1, on the same GPU in the same process.

The input is a synthetic first-stage output: some 30 objects per sample, a few hundred near-duplicate boxes around each
(what a trained first stage emits for the points of an object), the other points' boxes scattered over the field; the
score falls with the distance from the object.  Both functions give the same RoIs on it (checked before timing).

Timing: wall time around each call with a synchronisation before and after (the loop reads from the device all along, so
HIP events alone would not see its host side), after warm-up, the median and the spread over the steps; the two alternate.

    python tools/bench_proposals.py [--points 16384] [--steps 20] [--warmup 5] [--table]
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

from dfu3d_amd import proposal_ops as ops  # noqa: E402
from dfu3d_amd.pcdet_kitti.pointrcnn_head import PointRCNNHead  # noqa: E402
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


def distinct_f32(v):
    """v as float32 with every repeated value moved up to the next float that is free."""
    v = np.asarray(v, np.float32)
    by_value = np.argsort(v, kind="stable")
    s = v[by_value]
    for k in range(1, len(s)):
        if s[k] <= s[k - 1]:
            s[k] = np.nextafter(s[k - 1], np.float32(np.inf))
    out = np.empty_like(v)
    out[by_value] = s
    return out


def first_stage(B, N, objects, per_object, classes, seed, dev):
    """-> batch_cls_preds (B * N, classes), batch_box_preds (B * N, 7), stacked in sample order."""
    rng = np.random.default_rng(seed)
    cls = np.zeros((B, N, classes), np.float32)
    box = np.zeros((B, N, 7), np.float32)
    near = min(objects * per_object, N)
    for b in range(B):
        centre = rng.uniform(-40.0, 40.0, (objects, 2))
        size = np.array([4.6, 1.9, 1.7]) * rng.uniform(0.8, 1.2, (objects, 3))
        heading = rng.uniform(-np.pi, np.pi, objects)
        kind = rng.integers(0, classes, objects)
        which = rng.integers(0, objects, near)
        off = rng.normal(0, 0.25, (near, 2))
        box[b, :near, 0:2] = centre[which] + off
        box[b, :near, 2] = rng.normal(-1.0, 0.1, near)
        box[b, :near, 3:6] = size[which] * (1 + rng.normal(0, 0.05, (near, 3)))
        box[b, :near, 6] = heading[which] + rng.normal(0, 0.08, near)
        rest = N - near
        box[b, near:, 0:2] = rng.uniform(-45.0, 45.0, (rest, 2))
        box[b, near:, 2] = rng.normal(-1.0, 0.3, rest)
        box[b, near:, 3:6] = np.array([4.6, 1.9, 1.7]) * rng.uniform(0.5, 1.5, (rest, 3))
        box[b, near:, 6] = rng.uniform(-np.pi, np.pi, rest)
        logit = np.concatenate([4.0 - 6.0 * np.linalg.norm(off, axis=1), rng.normal(-4.0, 1.0, rest)])
        logit = distinct_f32(logit)                                        # no two scores equal: torch.topk has no tie
        best = np.concatenate([kind[which], rng.integers(0, classes, rest)])
        cls[b] = logit[:, None] - 2.0 - rng.uniform(0, 1, (N, classes))
        cls[b, np.arange(N), best] = logit
        mix = rng.permutation(N)                                           # the objects' points anywhere in the cloud
        cls[b], box[b] = cls[b][mix], box[b][mix]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    return to(cls.reshape(B * N, classes)), to(box.reshape(B * N, 7))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=16384)
    ap.add_argument('--objects', type=int, default=30)
    ap.add_argument('--per-object', type=int, default=300)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--table', action='store_true')
    a = ap.parse_args()
    dev = 'cuda:0'
    N = a.points
    nms_cfg = R.full_model_cfg()['ROI_HEAD']['NMS_CONFIG']
    head = PointRCNNHead(16, R.g20_model_cfg()['ROI_HEAD'], num_class=1)
    res = dict(points=N, objects=a.objects, per_object=a.per_object, steps=a.steps, launches=ops.LAUNCHES,
               device=torch.cuda.get_device_name(0), rows=[])
    for B in (8, 1):
        cls, box = first_stage(B, N, a.objects, a.per_object, 8, 2017 + B, dev)
        for mode in ('TRAIN', 'TEST'):
            nms = nms_cfg[mode]
            src = lambda: {'batch_size': B, 'batch_cls_preds': cls, 'batch_box_preds': box}       # noqa: E731
            one, two = head.proposal_layer(src(), nms), head.proposal_layer_batched(src(), nms)
            same = all(torch.equal(one[k], two[k]) for k in ('rois', 'roi_scores', 'roi_labels', 'roi_point_idx'))
            batched, loop = timed_pair([lambda: head.proposal_layer_batched(src(), nms),
                                        lambda: head.proposal_layer(src(), nms)], a.steps, a.warmup)
            res['rows'].append(dict(batch=B, mode=mode, pre_max=nms['NMS_PRE_MAXSIZE'], post_max=nms['NMS_POST_MAXSIZE'],
                                    thresh=nms['NMS_THRESH'], same_result=bool(same), num_rois=two['num_rois'].tolist(),
                                    batched=batched, loop=loop))
    print(json.dumps(res))
    if a.table:
        print("| B | post_max, thresh | RoIs kept per sample | batched median (p10 .. p90) ms | per-sample loop median (p10 .. p90) ms |")
        print("|---|---|---|---|---|")
        for r in res['rows']:
            print("| %d | %d, %.2f | %d .. %d | %.3f (%.3f .. %.3f) | %.2f (%.2f .. %.2f) |" % (
                r['batch'], r['post_max'], r['thresh'], min(r['num_rois']), max(r['num_rois']),
                r['batched']['median_ms'], r['batched']['p10_ms'], r['batched']['p90_ms'],
                r['loop']['median_ms'], r['loop']['p10_ms'], r['loop']['p90_ms']))


if __name__ == '__main__':
    main()
