#!/usr/bin/env python
"""Time the anchor target stage for a whole batch (csrc/anchor_stage.hip through dfu3d_amd.anchor_target_ops) against a
torch restatement of the reference's AxisAlignedTargetAssigner on the same GPU in the same process: the loop over samples
and, inside it, over anchor classes, with the class mask through a host copy, the dense (anchors x boxes) IoU matrix, the
two arg maxima, the nonzero calls and the scatter of labels and encoded targets, as
pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py does them.

The shape is second_ps.yaml's on the KITTI grid: 200 x 176 locations x 3 classes x 2 rotations = 211 200 anchors, B = 4,
about 15 boxes per sample.  Both give the same labels and weights on it (checked before timing).

Timing: wall time around each call with a synchronisation before and after (the loop reads from the device all along, so
HIP events alone would not see its host side), after warm-up, the median and the spread over the steps; the two
alternate.  For the stage alone also the time between two HIP events around --burst calls in a row, per call.  Bytes per
second: the B * A * 9 words written plus the A * 7 words of anchors read once, over the stage's median.

    python tools/bench_anchor_target.py [--batch 4] [--boxes 15] [--steps 30] [--warmup 5] [--table]
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

from dfu3d_amd import anchor_target_ops as ops  # noqa: E402
from dfu3d_amd.pcdet_kitti import box_utils  # noqa: E402
from dfu3d_amd.pcdet_kitti.box_coder_utils import ResidualCoder  # noqa: E402
from tests import anchor_target_ref as R  # noqa: E402

RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
FMAP = [(176, 200)] * 3


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


def torch_single(anchors, gt_boxes, gt_classes, matched, unmatched, coder):
    """assign_targets_single for POS_FRACTION < 0, statement by statement."""
    n, dev = anchors.shape[0], anchors.device
    labels = torch.ones((n,), dtype=torch.int32, device=dev) * -1
    if len(gt_boxes) > 0 and n > 0:
        iou = box_utils.boxes3d_nearest_bev_iou(anchors[:, 0:7], gt_boxes[:, 0:7])
        arg = iou.argmax(dim=1)
        best = iou[torch.arange(n, device=dev), arg]
        gt_arg = iou.argmax(dim=0)
        top = iou[gt_arg, torch.arange(gt_boxes.shape[0], device=dev)]
        top[top == 0] = -1
        forced = (iou == top).nonzero()[:, 0]
        force_cls = gt_classes[arg[forced]]
        labels[forced] = force_cls
        pos = best >= matched
        labels[pos] = gt_classes[arg[pos]]
        bg = (best < unmatched).nonzero()[:, 0]
        labels[bg] = 0
        labels[forced] = force_cls
    else:
        labels[:] = 0
    fg = (labels > 0).nonzero()[:, 0]
    targets = anchors.new_zeros((n, 7))
    if len(gt_boxes) > 0 and n > 0:
        targets[fg, :] = coder.encode_torch(gt_boxes[arg[fg], :], anchors[fg, :])
    weights = anchors.new_zeros((n,))
    weights[labels > 0] = 1.0
    return labels, targets, weights


def torch_loop(all_anchors, gt, names, coder):
    """assign_targets: per sample the trailing zero rows cut, per anchor class the mask through the host."""
    class_names = np.array(R.CLASS_NAMES)
    out = ([], [], [])
    for k in range(gt.shape[0]):
        cur = gt[k, :, :-1]
        cnt = len(cur) - 1
        while cnt > 0 and cur[cnt].sum() == 0:
            cnt -= 1
        cur = cur[:cnt + 1]
        classes = gt[k, :cnt + 1, -1].int()
        per = []
        for name, anchors, c in zip(names, all_anchors, R.ANCHOR_CFG):
            mask = torch.from_numpy(class_names[classes.cpu().numpy() - 1] == name).to(gt.device)
            fmap = anchors.shape[:3]
            lab, tgt, wgt = torch_single(anchors.view(-1, 7), cur[mask], classes[mask], c['matched_threshold'],
                                         c['unmatched_threshold'], coder)
            per.append((lab.view(*fmap, -1), tgt.view(*fmap, -1, 7), wgt.view(*fmap, -1)))
        out[0].append(torch.cat([p[0] for p in per], dim=-1).view(-1))
        out[1].append(torch.cat([p[1] for p in per], dim=-2).view(-1, 7))
        out[2].append(torch.cat([p[2] for p in per], dim=-1).view(-1))
    return torch.stack(out[0]), torch.stack(out[1]), torch.stack(out[2])


def make_boxes(B, n, M, seed):
    rng = np.random.default_rng(seed)
    gt = np.zeros((B, M, 8), np.float32)
    for b in range(B):
        for k in range(n):
            box = np.array([R.car, R.ped, R.bike][k % 3](rng.uniform(2.0, 68.0), rng.uniform(-38.0, 38.0),
                                                       rng.uniform(-np.pi, np.pi)), np.float32)
            box[3:6] *= rng.uniform(0.85, 1.15, 3).astype(np.float32)
            gt[b, k] = box
    return gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--boxes', type=int, default=15)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--burst', type=int, default=50)
    ap.add_argument('--table', action='store_true')
    a = ap.parse_args()
    dev = 'cuda:0'
    anchors_np, _ = R.generate_anchors(RANGE, FMAP)
    all_anchors = [torch.from_numpy(x).to(dev) for x in anchors_np]
    flat = torch.cat(all_anchors, dim=-3).view(-1, 7).contiguous()
    sets = R.class_sets(anchors_np)
    names = [c['class_name'] for c in R.ANCHOR_CFG]
    gt = torch.from_numpy(make_boxes(a.batch, a.boxes, a.boxes + 5, 2025)).to(dev)
    coder = ResidualCoder()
    B, A = a.batch, int(flat.shape[0])
    one, two = ops.assign_targets(flat, sets, gt), torch_loop(all_anchors, gt, names, coder)
    same = bool(torch.equal(one[0], two[0]) and torch.equal(one[2], two[2]))
    worst = float((one[1] - two[1]).abs().max())
    stage, loop = timed_pair([lambda: ops.assign_targets(flat, sets, gt), lambda: torch_loop(all_anchors, gt, names, coder)],
                             a.steps, a.warmup)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    bursts = []
    for _ in range(5):
        torch.cuda.synchronize()
        start.record()
        for _ in range(a.burst):
            ops.assign_targets(flat, sets, gt)
        stop.record()
        torch.cuda.synchronize()
        bursts.append(start.elapsed_time(stop) / a.burst)
    nbytes = 4 * (B * A * 9 + A * 7)
    res = dict(batch=B, anchors=A, boxes=a.boxes, classes=len(sets), steps=a.steps, launches=ops.LAUNCHES,
               device=torch.cuda.get_device_name(0), same_labels_and_weights=same, largest_target_difference=worst,
               foreground=[int(v) for v in (one[0] > 0).sum(1).tolist()], stage=stage, torch_loop=loop,
               stage_in_a_burst_ms=float(np.median(bursts)), bytes=nbytes,
               gbytes_per_s=nbytes / (stage['median_ms'] * 1e-3) / 1e9,
               gbytes_per_s_in_a_burst=nbytes / (float(np.median(bursts)) * 1e-3) / 1e9)
    print(json.dumps(res))
    if a.table:
        print("| B | anchors | boxes | launches | stage median (p10) ms | in a burst ms | GB/s (burst) | torch loop median (p10) ms |")
        print("|---|---|---|---|---|---|---|---|")
        print("| %d | %d | %d | %d | %.3f (%.3f) | %.3f | %.0f (%.0f) | %.2f (%.2f) |" % (
            B, A, a.boxes, ops.LAUNCHES, stage['median_ms'], stage['p10_ms'], res['stage_in_a_burst_ms'],
            res['gbytes_per_s'], res['gbytes_per_s_in_a_burst'], loop['median_ms'], loop['p10_ms']))


if __name__ == '__main__':
    main()
