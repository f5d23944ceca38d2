#!/usr/bin/env python
"""Time StackSAModuleMSG on csrc/pointstack_stage.hip at two shapes of cfgs/kitti_models/pv_rcnn_ps.yaml, B = 2:

  roi_grid   the RoI-grid pooling: 100 RoIs x 216 grid points as centres over 2 048 keypoints per sample, C = 128,
             radii 0.8 / 1.6, 16 samples, MLPs [64, 64];
  x_conv1    the PFE's first sparse level: 2 048 keypoints as centres over --voxels occupied voxels per sample, C = 16,
             radii 0.4 / 0.8, 16 samples, MLPs [16, 16];

against the plain torch a user without the stage would run, in the same process and with the same layers: per sample a
cdist, a masked sort for the first nsample indices in ascending order, fancy-index gathers, the subtraction, the masked
fill, the permute.  The module and the comparator alternate; their outputs are compared once before timing (the ball
indices are equal away from exact ties of cdist's rounding against the kernel's, the number of differing balls is
reported).  The ball query and the grouping of the stage are also timed alone.

Timing: HIP events around each call after warm-up, the median and the spread over the steps.

    python tools/bench_point_stack.py [--steps 20] [--warmup 5] [--voxels 16000] [--table]
prints one JSON line (and, with --table, the markdown table of DESIGN.md).  No time is asserted anywhere.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfu3d_amd import point_stack_ops as ops  # noqa: E402
from dfu3d_amd.pcdet_kitti.pointnet2_stack_modules import StackSAModuleMSG  # noqa: E402

B = 2
RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.asarray(ms)
    return dict(median_ms=float(np.median(ms)), p10_ms=float(np.percentile(ms, 10)), p90_ms=float(np.percentile(ms, 90)))


def scene(n, g, dev):
    """LiDAR-like rows in the configuration's range: most near the ground, denser near the sensor."""
    r = 2.0 + 60.0 * torch.rand(n, generator=g, device=dev) ** 1.5
    a = (torch.rand(n, generator=g, device=dev) - 0.5) * (np.pi * 0.95)
    z = -1.6 + 0.1 * torch.randn(n, generator=g, device=dev) + (torch.rand(n, generator=g, device=dev) < 0.3) * \
        1.8 * torch.rand(n, generator=g, device=dev)
    xyz = torch.stack([r * torch.cos(a), r * torch.sin(a), z], dim=1)
    lo, hi = torch.tensor(RANGE[:3], device=dev), torch.tensor(RANGE[3:], device=dev)
    return torch.minimum(torch.maximum(xyz, lo + 0.01), hi - 0.01).contiguous()


def plain_module(layer, xyz, cnt, ctr, ccnt, feats):
    """The forward of StackSAModuleMSG in plain torch; cnt, ccnt: Python lists.  -> (features (M, C_out), [idx per scale])."""
    pooled, all_idx = [], [[] for _ in layer.groupers]
    per_scale = [[] for _ in layer.groupers]
    p0 = c0 = 0
    for n, m in zip(cnt, ccnt):
        x, c, f = xyz[p0:p0 + n], ctr[c0:c0 + m], feats[p0:p0 + n]
        d = torch.cdist(c, x)
        ar = torch.arange(n, device=xyz.device).view(1, n)
        for s, grouper in enumerate(layer.groupers):
            key = torch.where(d < grouper.radius, ar, n).sort(dim=1)[0][:, :grouper.nsample]
            empty = key[:, 0] == n
            idx = torch.where(key == n, key[:, :1], key).remainder(n)
            grouped = torch.cat([x[idx] - c[:, None, :], f[idx]], dim=-1)             # (m, ns, 3 + C)
            grouped[empty] = 0
            per_scale[s].append(grouped)
            all_idx[s].append(idx)
        p0, c0 = p0 + n, c0 + m
    for s, mlp in enumerate(layer.mlps):
        g = torch.cat(per_scale[s], dim=0).permute(2, 0, 1).unsqueeze(0)              # (1, 3 + C, M, ns), strided
        y = mlp(g)
        pooled.append(torch.nn.functional.max_pool2d(y, kernel_size=[1, y.size(3)]).squeeze(-1).squeeze(0).permute(1, 0))
    return torch.cat(pooled, dim=1), [torch.cat(i, dim=0) for i in all_idx]


def case(name, xyz, cnt, ctr, ccnt, C, radii, nsamples, widths, a, g, rows):
    dev = xyz.device
    layer = StackSAModuleMSG(radii=radii, nsamples=nsamples, mlps=[[C] + widths, [C] + widths]).to(dev).eval()
    feats = torch.randn(xyz.shape[0], C, generator=g, device=dev)
    cnt_t = torch.tensor(cnt, dtype=torch.int32, device=dev)
    ccnt_t = torch.tensor(ccnt, dtype=torch.int32, device=dev)
    with torch.no_grad():
        mine = layer(xyz, cnt_t, ctr, ccnt_t, feats)[1]
        ref, ref_idx = plain_module(layer, xyz, cnt, ctr, ccnt, feats)
        balls = layer.ball_indices(xyz, cnt_t, ctr, ccnt_t)
        differ = [int((b[0].long() != r).any(dim=1).sum()) for b, r in zip(balls, ref_idx)]
        same_rows = torch.ones(ctr.shape[0], dtype=torch.bool, device=dev)
        for b, r in zip(balls, ref_idx):
            same_rows &= ~(b[0].long() != r).any(dim=1)
        err = float((mine - ref)[same_rows].abs().max())
        start, cstart = ops.starts_of(cnt_t), ops.starts_of(ccnt_t)
        module = timed(lambda: layer(xyz, cnt_t, ctr, ccnt_t, feats), a.steps, a.warmup)
        plain = timed(lambda: plain_module(layer, xyz, cnt, ctr, ccnt, feats), a.steps, a.warmup)
        ball = timed(lambda: ops.ball_query(xyz, start, ctr, cstart, radii, nsamples), a.steps, a.warmup)
        group = timed(lambda: [ops.group(xyz, start, ctr, cstart, feats, i, e) for i, e in balls], a.steps, a.warmup)
    rows.append(dict(case=name, points=cnt, centres=ccnt, C=C, module=module, torch=plain, ball_query=ball, group_both_scales=group,
                     ratio_torch_over_hip=plain["median_ms"] / module["median_ms"], balls_with_other_indices=differ,
                     max_abs_diff_on_equal_balls=err, empty_balls=[int(e.sum()) for _, e in balls]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--voxels", type=int, default=16000)
    ap.add_argument("--keypoints", type=int, default=2048)
    ap.add_argument("--rois", type=int, default=100)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(26)
    rows = []
    # keypoints: the stage's own FPS of a raw cloud
    raw = torch.cat([scene(a.voxels, g, dev) for _ in range(B)])
    raw_cnt = torch.full((B,), a.voxels, dtype=torch.int32, device=dev)
    kp = ops.fps(raw, ops.starts_of(raw_cnt), a.keypoints)[1]
    kxyz = kp[:, 1:4].contiguous()
    fps_t = timed(lambda: ops.fps(raw, ops.starts_of(raw_cnt), a.keypoints), max(a.steps // 4, 2), 1)
    # RoI grid: boxes of car size around keypoints, 6 x 6 x 6 cell centres each
    grid = []
    for b in range(B):
        own = kxyz[b * a.keypoints:(b + 1) * a.keypoints]
        centre = own[torch.randint(a.keypoints, (a.rois,), generator=g, device=dev)]
        size = torch.tensor([3.9, 1.6, 1.56], device=dev) * (0.8 + 0.4 * torch.rand(a.rois, 3, generator=g, device=dev))
        ang = (torch.rand(a.rois, generator=g, device=dev) - 0.5) * 2 * np.pi
        i = torch.arange(6, device=dev, dtype=torch.float32)
        cell = torch.stack(torch.meshgrid(i, i, i, indexing='ij'), dim=-1).view(1, -1, 3)
        local = (cell + 0.5) / 6 * size[:, None] - size[:, None] / 2
        c, s = torch.cos(ang)[:, None], torch.sin(ang)[:, None]
        glob = torch.stack([local[..., 0] * c - local[..., 1] * s, local[..., 0] * s + local[..., 1] * c, local[..., 2]], dim=-1)
        grid.append((glob + centre[:, None]).view(-1, 3))
    grid = torch.cat(grid).contiguous()
    case("roi_grid", kxyz, [a.keypoints] * B, grid, [a.rois * 216] * B, 128, [0.8, 1.6], [16, 16], [64, 64], a, g, rows)
    # x_conv1: voxel centres of the raw cloud on the 0.05 x 0.05 x 0.1 grid
    vox = torch.tensor([0.05, 0.05, 0.1], device=dev)
    lo = torch.tensor(RANGE[:3], device=dev)
    centres = (torch.floor((raw - lo) / vox) + 0.5) * vox + lo
    case("x_conv1", centres.contiguous(), [a.voxels] * B, kxyz, [a.keypoints] * B, 16, [0.4, 0.8], [16, 16], [16, 16], a, g, rows)
    print(json.dumps(dict(batch=B, steps=a.steps, warmup=a.warmup, fps=dict(points=a.voxels, keypoints=a.keypoints, **fps_t),
                          rows=rows)))
    if a.table:
        print("| case | module median ms (p10 - p90) | plain torch median ms (p10 - p90) | torch / HIP | ball query ms | grouping ms |")
        print("|---|---|---|---|---|---|")
        for r in rows:
            print("| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.1f | %.3f | %.3f |"
                  % (r["case"], r["module"]["median_ms"], r["module"]["p10_ms"], r["module"]["p90_ms"], r["torch"]["median_ms"],
                     r["torch"]["p10_ms"], r["torch"]["p90_ms"], r["ratio_torch_over_hip"], r["ball_query"]["median_ms"],
                     r["group_both_scales"]["median_ms"]))


if __name__ == "__main__":
    main()
