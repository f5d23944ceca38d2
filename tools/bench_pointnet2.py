#!/usr/bin/env python
"""Time the PointNet++ ops of csrc/pointnet2_stage.hip, op by op, at the shapes of the PointRCNN configuration's
backbone (B = 8, N = 16384; SA levels 16384 -> 4096 -> 1024 -> 256 -> 64 with their radii, sample counts and channel
widths; the four FP levels), against a plain-torch formulation of each op in the same process: a Python loop for
farthest point sampling, cdist + sort for the ball query, gather for grouping and interpolation, cdist + topk for the
three nearest neighbours, index_add_ for the two backwards.

Timing: HIP events around each call after warm-up, the median and the spread over the steps; the HIP op and its torch
formulation alternate.  The torch sampling loop is thousands of launches per call: it gets --torch-fps-steps calls.

    python tools/bench_pointnet2.py [--batch 8] [--points 16384] [--steps 20] [--warmup 5] [--table]
prints one JSON line (and, with --table, the markdown table of DESIGN.md).  No time is asserted anywhere.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfu3d_amd import pointnet2_ops as ops  # noqa: E402

NPOINTS = [4096, 1024, 256, 64]
RADIUS = [[0.1, 0.5], [0.5, 1.0], [1.0, 2.0], [2.0, 4.0]]
NSAMPLE = [[16, 32], [16, 32], [16, 32], [16, 32]]
C_IN = [1, 96, 256, 512]                 # feature channels entering SA level k
C_KNOWN = [256, 512, 512, 1024]          # channels interpolated by FP level k (from level k + 1)


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


def make_cloud(B, N, dev):
    """LiDAR-like: a ground disc of 50 m with clusters on it, in the configuration's range."""
    g = torch.Generator(device=dev).manual_seed(1900)
    r = 50.0 * torch.rand(B, N, generator=g, device=dev).sqrt()
    a = 2 * np.pi * torch.rand(B, N, generator=g, device=dev)
    z = -1.7 + 0.05 * torch.randn(B, N, generator=g, device=dev) + (torch.rand(B, N, generator=g, device=dev) < 0.3) * \
        2.0 * torch.rand(B, N, generator=g, device=dev)
    return torch.stack([r * torch.cos(a), r * torch.sin(a), z], dim=2).contiguous()


def fps_torch(xyz, npoint):
    B, N, _ = xyz.shape
    idx = torch.zeros(B, npoint, dtype=torch.long, device=xyz.device)
    run = torch.full((B, N), 1e10, device=xyz.device)
    old = torch.zeros(B, dtype=torch.long, device=xyz.device)
    ar = torch.arange(B, device=xyz.device)
    for s in range(1, npoint):
        d = ((xyz - xyz[ar, old].unsqueeze(1)) ** 2).sum(-1)
        run = torch.minimum(run, d)
        old = run.argmax(dim=1)
        idx[:, s] = old
    return idx


def ball_torch(xyz, ctr, radii, nsamples):
    N = xyz.shape[1]
    d = torch.cdist(ctr, xyz)
    ar = torch.arange(N, device=xyz.device).view(1, 1, N)
    out = []
    for r, ns in zip(radii, nsamples):
        key = torch.where(d < r, ar, N).sort(dim=2)[0][:, :, :ns]
        first = key[:, :, :1]
        out.append(torch.where(key == N, first, key).remainder(N))
    return out


def group_torch(xyz_t, ctr, feat, idx):
    B, M, ns = idx.shape
    flat = idx.reshape(B, 1, M * ns)
    gx = torch.gather(xyz_t, 2, flat.expand(B, 3, M * ns)).view(B, 3, M, ns) - ctr.transpose(1, 2).unsqueeze(-1)
    gf = torch.gather(feat, 2, flat.expand(B, feat.shape[1], M * ns)).view(B, feat.shape[1], M, ns)
    return torch.cat([gx, gf], dim=1)


def scatter_torch(grad, idx, N):
    """grad (B, C, E), idx (B, E) long -> (B, C, N) by index_add_."""
    out = torch.zeros(grad.shape[0], grad.shape[1], N, device=grad.device)
    for b in range(grad.shape[0]):
        out[b].index_add_(1, idx[b], grad[b])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-fps-steps", type=int, default=2)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    B = a.batch
    g = torch.Generator(device=dev).manual_seed(7)
    l_xyz = [make_cloud(B, a.points, dev)]
    rows = []

    def row(name, hip, ref, hip_steps=None, ref_steps=None):
        h = timed(hip, hip_steps or a.steps, a.warmup if hip_steps is None else 1)
        t = timed(ref, ref_steps or a.steps, a.warmup if ref_steps is None else 1)
        rows.append(dict(op=name, hip=h, torch=t, ratio_torch_over_hip=t["median_ms"] / h["median_ms"]))

    for k, npoint in enumerate(NPOINTS):
        xyz = l_xyz[k]
        N = xyz.shape[1]
        if npoint >= N:
            break
        idx_fps, new_xyz = ops.fps(xyz, npoint)
        l_xyz.append(new_xyz)
        row("SA%d fps %d -> %d" % (k, N, npoint), lambda: ops.fps(xyz, npoint), lambda: fps_torch(xyz, npoint),
            ref_steps=a.torch_fps_steps)
        balls = ops.ball_query(xyz, new_xyz, RADIUS[k], NSAMPLE[k])
        row("SA%d ball query r %s ns %s" % (k, RADIUS[k], NSAMPLE[k]),
            lambda: ops.ball_query(xyz, new_xyz, RADIUS[k], NSAMPLE[k]),
            lambda: ball_torch(xyz, new_xyz, RADIUS[k], NSAMPLE[k]))
        feat = torch.randn(B, C_IN[k], N, generator=g, device=dev)
        xyz_t = xyz.transpose(1, 2).contiguous()
        longs = [i.long() for i in balls]
        row("SA%d group C %d (both scales)" % (k, C_IN[k]),
            lambda: [ops.group(xyz, new_xyz, feat, i) for i in balls],
            lambda: [group_torch(xyz_t, new_xyz, feat, i) for i in longs])
        grads = [torch.randn(B, C_IN[k], npoint * i.shape[2], generator=g, device=dev) for i in balls]
        row("SA%d group backward (inverse + ordered sum, both scales)" % k,
            lambda: [ops.gather_backward(gr, ops.invert(i, N)) for gr, i in zip(grads, balls)],
            lambda: [scatter_torch(gr, i.view(B, -1), N) for gr, i in zip(grads, longs)])
    for k in range(len(l_xyz) - 2, -1, -1):
        unknown, known = l_xyz[k], l_xyz[k + 1]
        n, m, C = unknown.shape[1], known.shape[1], C_KNOWN[k]
        dist, idx = ops.three_nn(unknown, known)
        row("FP%d three_nn %d in %d" % (k, n, m), lambda: ops.three_nn(unknown, known),
            lambda: torch.cdist(unknown, known).topk(3, dim=2, largest=False))
        recip = 1.0 / (dist + 1e-8)
        w = (recip / recip.sum(dim=2, keepdim=True)).contiguous()
        feat = torch.randn(B, C, m, generator=g, device=dev)
        long = idx.long()

        def interp_torch():
            f = [torch.gather(feat, 2, long[:, :, r].unsqueeze(1).expand(B, C, n)) for r in range(3)]
            return (w[:, :, 0].unsqueeze(1) * f[0] + w[:, :, 1].unsqueeze(1) * f[1]) + w[:, :, 2].unsqueeze(1) * f[2]
        row("FP%d interpolate C %d" % (k, C), lambda: ops.three_interpolate(feat, idx, w), interp_torch)
        grad = torch.randn(B, C, n, generator=g, device=dev)

        def interp_bwd_torch():
            out = torch.zeros(B, C, m, device=dev)
            for r in range(3):
                gw = grad * w[:, :, r].unsqueeze(1)
                for b in range(B):
                    out[b].index_add_(1, long[b, :, r], gw[b])
            return out
        row("FP%d interpolate backward (inverse + ordered sum)" % k,
            lambda: ops.gather_backward(grad, ops.invert(idx, m), w.view(B, -1), 3), interp_bwd_torch)
    print(json.dumps(dict(batch=B, points=a.points, steps=a.steps, warmup=a.warmup, rows=rows)))
    if a.table:
        print("| op | HIP median ms (p10 - p90) | torch median ms (p10 - p90) | torch / HIP |")
        print("|---|---|---|---|")
        for r in rows:
            print("| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.1f |"
                  % (r["op"], r["hip"]["median_ms"], r["hip"]["p10_ms"], r["hip"]["p90_ms"], r["torch"]["median_ms"],
                     r["torch"]["p10_ms"], r["torch"]["p90_ms"], r["ratio_torch_over_hip"]))


if __name__ == "__main__":
    main()
