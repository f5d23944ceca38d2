#!/usr/bin/env python
"""Time the RoI-point pooling of csrc/roipoint_stage.hip, both forms, at the shapes of the PointRCNN configuration
(B = 8, N = 16384, S = 512, C = 128; M = 128 RoIs in training, 100 in test) against a plain-torch formulation on the same
GPU in the same process: a broadcast in-box mask (B, M, N), cumsum for the ranks, a scatter of the first S indices, the
k % cnt wrap, a gather -- and, for the fused form, what PointRCNNHead.roipool3d_gpu puts around the op: the
concatenation of [score, depth, features], the subtraction of the RoI centre, the rotation by -heading, the zeroing of the
empty RoIs.

Timing: HIP events around each call after warm-up, the median and the spread over the steps; the HIP op and its torch
formulation alternate.  `bytes` is what the op must move given its shapes -- the points, scores and features once, the
boxes, the three outputs -- and `hbm_share` that over the time over the HBM peak (8.0 TB/s).

    python tools/bench_roipoint.py [--batch 8] [--points 16384] [--steps 20] [--warmup 5] [--table]
prints one JSON line (and, with --table, the markdown table of DESIGN.md).  No time is asserted anywhere.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfu3d_amd import roipoint_ops as ops  # noqa: E402
from tools.bench_pointnet2 import make_cloud  # noqa: E402

HBM_PEAK = 8.0e12
MARGIN = 1e-5


def timed_pair(fns, steps, warmup):
    """The functions alternate, call by call; -> per function the median, p10 and p90 in ms."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [dict(median_ms=float(np.median(m)), p10_ms=float(np.percentile(m, 10)), p90_ms=float(np.percentile(m, 90)))
            for m in ms]


def make_rois(xyz, M, seed):
    """M boxes per sample around points of the cloud: vehicle-sized, every heading."""
    B, N, _ = xyz.shape
    g = torch.Generator(device=xyz.device).manual_seed(seed)
    pick = torch.randint(N, (B, M), generator=g, device=xyz.device)
    ctr = torch.gather(xyz, 1, pick[..., None].expand(-1, -1, 3))
    dims = torch.tensor([4.6, 2.0, 1.8], device=xyz.device) * (0.6 + 0.8 * torch.rand(B, M, 3, generator=g, device=xyz.device))
    rz = (2 * torch.rand(B, M, 1, generator=g, device=xyz.device) - 1) * np.pi
    return torch.cat([ctr, dims, rz], dim=2).contiguous()


def pool_torch(points, rows, boxes, S):
    """points (B, N, 3), rows (B, N, W), boxes (B, M, 7) -> gathered rows (B, M, S, W), empty flags (B, M)."""
    B, N, _ = points.shape
    M = boxes.shape[1]
    d = points[:, None, :, :] - boxes[:, :, None, 0:3]
    cosa, sina = torch.cos(-boxes[:, :, 6:7]), torch.sin(-boxes[:, :, 6:7])
    lx = d[..., 0] * cosa - d[..., 1] * sina
    ly = d[..., 0] * sina + d[..., 1] * cosa
    mask = (d[..., 2].abs() <= boxes[:, :, 5:6] / 2) & (lx.abs() < boxes[:, :, 3:4] / 2 + MARGIN) \
        & (ly.abs() < boxes[:, :, 4:5] / 2 + MARGIN)
    rank = torch.cumsum(mask, dim=2) - 1
    cnt = mask.sum(dim=2).clamp(max=S)
    slot = torch.where(mask & (rank < S), rank, S)
    idx = torch.zeros((B, M, S + 1), dtype=torch.long, device=points.device)
    idx.scatter_(2, slot, torch.arange(N, device=points.device).expand(B, M, N))
    wrap = torch.arange(S, device=points.device).expand(B, M, S) % cnt.clamp(min=1)[..., None]
    idx = torch.gather(idx[..., :S], 2, wrap)
    out = torch.gather(rows, 1, idx.view(B, M * S, 1).expand(-1, -1, rows.shape[2])).view(B, M, S, -1)
    return out, (cnt == 0).int()


def plain_torch(points, feats, boxes, S):
    out, flag = pool_torch(points, torch.cat([points, feats], dim=2), boxes, S)
    return out * (flag == 0)[..., None, None], flag


def fused_torch(points, scores, feats, boxes, S, normalizer):
    B, N, _ = points.shape
    depth = points.norm(dim=2) / normalizer - 0.5
    rows = torch.cat([points, scores.view(B, N, 1), depth[..., None], feats.view(B, N, -1)], dim=2)     # the concatenation
    pooled, flag = pool_torch(points, rows, boxes, S)
    pooled[..., 0:3] -= boxes[:, :, None, 0:3]
    pooled = pooled.view(-1, S, pooled.shape[-1])
    ang = boxes.view(-1, 7)[:, 6]
    cosa, sina = torch.cos(-ang), torch.sin(-ang)
    zeros, ones = torch.zeros_like(ang), torch.ones_like(ang)
    rot = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3)
    pooled[..., 0:3] = torch.matmul(pooled[..., 0:3], rot)
    pooled[flag.view(-1) > 0] = 0
    return pooled


def needed_bytes(B, N, M, S, C, fused):
    W = (ops.PREFIX_FUSED if fused else ops.PREFIX_PLAIN) + C
    reads = B * N * (3 + C + (1 if fused else 0)) + B * M * 7
    writes = B * M * S * W + B * M * S + B * M
    return 4 * (reads + writes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--points', type=int, default=16384)
    ap.add_argument('--sampled', type=int, default=512)
    ap.add_argument('--channels', type=int, default=128)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--table', action='store_true')
    a = ap.parse_args()
    dev = 'cuda:0'
    B, N, S, C = a.batch, a.points, a.sampled, a.channels
    xyz = make_cloud(B, N, dev)
    g = torch.Generator(device=dev).manual_seed(15)
    feats = torch.randn(B, N, C, generator=g, device=dev)
    scores = torch.rand(B * N, generator=g, device=dev)
    coords = torch.cat([torch.arange(B, device=dev).repeat_interleave(N)[:, None].float(), xyz.view(-1, 3)], dim=1)
    res = dict(batch=B, points=N, sampled=S, channels=C, steps=a.steps, device=torch.cuda.get_device_name(0), rows=[])
    for M in (128, 100):
        boxes = make_rois(xyz, M, 1500 + M)
        flag = ops.pool(xyz, feats, boxes, 0.0, S)[1]
        occupancy = dict(empty_rois=int(flag.sum()), total_rois=B * M)
        for form in ('plain', 'fused'):
            if form == 'plain':
                fns = [lambda: ops.pool(xyz, feats, boxes, 0.0, S), lambda: plain_torch(xyz, feats, boxes, S)]
            else:
                fns = [lambda: ops.pool_fused(coords, scores, feats.view(B * N, C), boxes, 0.0, S, 70.0),
                       lambda: fused_torch(xyz, scores, feats, boxes, S, 70.0)]
            hip, plain = timed_pair(fns, a.steps, a.warmup)
            nbytes = needed_bytes(B, N, M, S, C, form == 'fused')
            res['rows'].append(dict(form=form, rois=M, hip=hip, torch=plain, bytes=nbytes,
                                    hbm_share=nbytes / (hip['median_ms'] * 1e-3) / HBM_PEAK, **occupancy))
    print(json.dumps(res))
    if a.table:
        print("| form | M | HIP median (p10 .. p90) ms | torch median (p10 .. p90) ms | bytes needed | share of 8.0 TB/s |")
        print("|---|---|---|---|---|---|")
        for r in res['rows']:
            print("| %s | %d | %.3f (%.3f .. %.3f) | %.2f (%.2f .. %.2f) | %.1f MB | %.1f %% |" % (
                r['form'], r['rois'], r['hip']['median_ms'], r['hip']['p10_ms'], r['hip']['p90_ms'], r['torch']['median_ms'],
                r['torch']['p10_ms'], r['torch']['p90_ms'], r['bytes'] / 1e6, 100 * r['hbm_share']))


if __name__ == '__main__':
    main()
