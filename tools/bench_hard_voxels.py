#!/usr/bin/env python
"""Time the hard-voxel stage for a whole batch (csrc/hardvoxel_stage.hip through hard_voxel_ops.hard_voxels), in its
voxels form and in its mean-only form, against a plain-torch formulation of the same result on the same device: the cell
of every row in float32, one int64 key per row, torch.unique with the inverse, the first row of every cell by a
scatter-min, an argsort of the first rows for the first-seen order, the per-scene cap by a cumulative count, a stable
argsort of the rows by voxel for the slots, and one scatter into the (V, T, C) block; its mean is a sum over the block.
The torch side reads the number of voxels from the device (torch.unique and the block's shape need it); the stage reads
nothing.  Voxels, coordinates and counts of the two are compared bit for bit before timing.

Shape: B = 4 sweeps of dfu3d_amd.synth.lidar_sweep (64 rings x 1300 azimuth steps) cut to the range
[-54, -54, -5, 54, 54, 3], about 60 000 rows per scene, voxel 0.075 / 0.075 / 0.2, T = 10, max_voxels 120 000, C = 4.

Timing: HIP events around each call on the current stream, every shape warmed up, the median and the spread over the
steps; the three alternate inside one process.

    python tools/bench_hard_voxels.py [--batch 4] [--steps 50] [--warmup 10] [--table]
prints one JSON line (and, with --table, the markdown table of DESIGN.md).  No time is asserted anywhere.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfu3d_amd import hard_voxel_ops as ops  # noqa: E402
from dfu3d_amd import synth  # noqa: E402

RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
VOXEL = [0.075, 0.075, 0.2]


def timed(fns, steps, warmup):
    """The functions alternate, call by call; -> per function the median, p10 and p90 in ms (HIP events)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for k, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms[k].append(t0.elapsed_time(t1))
    return [dict(median_ms=float(np.median(m)), p10_ms=float(np.percentile(m, 10)), p90_ms=float(np.percentile(m, 90)))
            for m in ms]


def scenes(B, rings, az, seed, dev):
    """-> points (R, 5) on the device with the scene index in column 0, point_cnt int32 (B), the sizes on the host."""
    lo, hi = torch.tensor(RANGE[:3], device=dev), torch.tensor(RANGE[3:], device=dev)
    rows, sizes = [], []
    for b in range(B):
        rng = np.random.default_rng(seed + b)
        gen = torch.Generator(device=dev).manual_seed(seed + b)
        p = synth.lidar_sweep(synth._boxes(rng), gen, dev, rings=rings, az=az)
        p = p[((p[:, :3] >= lo) & (p[:, :3] < hi)).all(1)]
        rows.append(torch.cat([torch.full((len(p), 1), float(b), device=dev), p], 1))
        sizes.append(len(p))
    return torch.cat(rows, 0).contiguous(), torch.tensor(sizes, dtype=torch.int32, device=dev), sizes


def torch_formulation(points, sizes, rmin, vs, grid, T, max_voxels, want_mean):
    """-> (voxels (V, T, C) or their mean (V, C), voxel_coords (V, 4), voxel_num_points (V))."""
    dev = points.device
    R, C = points.shape[0], points.shape[1] - 1
    b = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.tensor(sizes, device=dev))
    c = torch.floor((points[:, 1:4] - rmin) / vs)
    inside = ((c >= 0) & (c < grid.float())).all(1)
    ci = c.long()
    key = ((b * grid[2] + ci[:, 2]) * grid[1] + ci[:, 1]) * grid[0] + ci[:, 0]
    rows = torch.nonzero(inside).flatten()
    uniq, inv = torch.unique(key[rows], return_inverse=True)
    first = torch.full((len(uniq),), R, dtype=torch.int64, device=dev).scatter_reduce(0, inv, rows, 'amin')
    order = torch.argsort(first)                                # cells in first-seen order (scene by scene: rows are)
    scene = b[first[order]]
    before = torch.cumsum(torch.bincount(scene, minlength=len(sizes)), 0) - torch.bincount(scene, minlength=len(sizes))
    made = (torch.arange(len(order), device=dev) - before[scene]) < max_voxels
    out_row = torch.cumsum(made, 0) - 1
    vox_of_cell = torch.full((len(uniq),), -1, dtype=torch.int64, device=dev)
    vox_of_cell[order] = torch.where(made, out_row, torch.full_like(out_row, -1))
    V = int(made.sum())                                         # the host read
    v = vox_of_cell[inv]
    rows, v = rows[v >= 0], v[v >= 0]
    by_vox = torch.argsort(v, stable=True)
    rows, v = rows[by_vox], v[by_vox]
    cnt = torch.bincount(v, minlength=V)
    slot = torch.arange(len(v), device=dev) - (torch.cumsum(cnt, 0) - cnt)[v]
    keep = slot < T
    voxels = torch.zeros((V, T, C), dtype=torch.float32, device=dev)
    voxels[v[keep], slot[keep]] = points[rows[keep], 1:]
    num = torch.clamp(cnt, max=T).int()
    cells = first[order][made]
    coords = torch.stack([b[cells], ci[cells, 2], ci[cells, 1], ci[cells, 0]], 1).int()
    if want_mean:
        return voxels.sum(1) / num.clamp(min=1).float().unsqueeze(1), coords, num
    return voxels, coords, num


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--rings', type=int, default=64)
    ap.add_argument('--az', type=int, default=1300)
    ap.add_argument('--max-points', type=int, default=10)
    ap.add_argument('--max-voxels', type=int, default=120000)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--table', action='store_true')
    a = ap.parse_args()
    dev = 'cuda:0'
    B, T, mv = a.batch, a.max_points, a.max_voxels
    points, cnt, sizes = scenes(B, a.rings, a.az, 2019, dev)
    R, C = int(points.shape[0]), 4
    grid = np.round((np.array(RANGE[3:]) - np.array(RANGE[:3])) / np.array(VOXEL)).astype(np.int64)
    rmin_t = torch.tensor(RANGE[:3], dtype=torch.float32, device=dev)
    vs_t = torch.tensor(VOXEL, dtype=torch.float32, device=dev)
    grid_t = torch.from_numpy(grid).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def stage(mean):
        return ops.hard_voxels(points, cnt, RANGE, VOXEL, grid, T, mv, want_voxels=not mean, want_mean=mean, status=status)
    full, tv = stage(False), torch_formulation(points, sizes, rmin_t, vs_t, grid_t, T, mv, False)
    nv = int(full.n_voxels.item())
    same = (nv == len(tv[0]) and int(status.item()) == 0
            and bool(torch.equal(full.voxels[:nv].view(torch.int32), tv[0].view(torch.int32)))
            and bool(torch.equal(full.voxel_coords[:nv], tv[1])) and bool(torch.equal(full.voxel_num_points[:nv], tv[2])))
    fns = [lambda: stage(False), lambda: stage(True),
           lambda: torch_formulation(points, sizes, rmin_t, vs_t, grid_t, T, mv, False),
           lambda: torch_formulation(points, sizes, rmin_t, vs_t, grid_t, T, mv, True)]
    t_vox, t_mean, t_torch, t_torch_mean = timed(fns, a.steps, a.warmup)
    cap = ops.voxel_cap(B, R, mv)
    # the mean-only form's compulsory traffic: every input row read once, every output element written once
    moved = R * (1 + C) * 4 + B * 4 + cap * (4 * 4 + 4 + C * 4) + R * 4 + 8
    res = dict(batch=B, rows=sizes, voxel=VOXEL, grid=grid.tolist(), max_points=T, max_voxels=mv, n_voxels=nv, v_cap=cap,
               steps=a.steps, launches=ops.LAUNCHES, device=torch.cuda.get_device_name(0), same_result=same,
               stage_voxels=t_vox, stage_mean=t_mean, torch_voxels=t_torch, torch_mean=t_torch_mean,
               mean_form_bytes=moved, mean_form_gb_per_s=moved / (t_mean['median_ms'] * 1e-3) / 1e9,
               mean_form_share_of_8_tb_per_s=moved / (t_mean['median_ms'] * 1e-3) / 8e12)
    print(json.dumps(res))
    if a.table:
        print("| B | rows per scene | voxels | form | stage median (p10 .. p90) ms | torch formulation median (p10 .. p90) ms |")
        print("|---|---|---|---|---|---|")
        for name, s, t in (("voxels", t_vox, t_torch), ("mean only", t_mean, t_torch_mean)):
            print("| %d | %d .. %d | %d | %s | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) |" % (
                B, min(sizes), max(sizes), nv, name, s['median_ms'], s['p10_ms'], s['p90_ms'], t['median_ms'], t['p10_ms'],
                t['p90_ms']))


if __name__ == '__main__':
    main()
