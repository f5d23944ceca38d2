#!/usr/bin/env python
"""Time the dynamic pillar feature encoder: the HIP path (dfu3d_amd.pcdet_kitti.dynamic_pillar_vfe.DynamicPillarVFE)
against a torch-only composition of the same layers (torch.unique + index_add_ + scatter_reduce), in one process.

Shape: the CenterPoint config of the labels (range [0,-51.2,-5,51.2,51.2,3], voxel [0.2,0.2,8], filters [64,64], 4 point
features) at batch size 4; the points are dfu3d_amd.synth LiDAR sweeps cut to the range.  Timing: HIP events around
each call after warm-up, the median and the spread over the steps; both paths alternate so that neither runs only on
a warm or only on a cold clock.  Launches per forward are counted by torch's profiler (kernels of one forward).

    python tools/bench_pillar_vfe.py [--batch 4] [--sweeps 10] [--steps 50] [--warmup 10]
prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfu3d_amd import synth  # noqa: E402
from dfu3d_amd.pcdet_kitti.dynamic_pillar_vfe import DynamicPillarVFE  # noqa: E402

RANGE = [0, -51.2, -5, 51.2, 51.2, 3]
VOXEL = [0.2, 0.2, 8]
GRID = [256, 512, 1]
MODEL_CFG = dict(USE_NORM=True, WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, NUM_FILTERS=[64, 64])


def make_points(batch, sweeps, device):
    out = []
    for b in range(batch):
        rng = np.random.default_rng(900 + b)
        boxes = torch.from_numpy(synth._boxes(rng)).to(device)
        gen = torch.Generator(device=device).manual_seed(900 + b)
        pts = torch.cat([synth.lidar_sweep(boxes, gen, device) for _ in range(sweeps)])
        pts[:, 3] /= 255.0
        keep = (pts[:, 0] >= RANGE[0]) & (pts[:, 0] < RANGE[3]) & (pts[:, 1] >= RANGE[1]) & (pts[:, 1] < RANGE[4]) \
            & (pts[:, 2] >= RANGE[2]) & (pts[:, 2] < RANGE[5])
        pts = pts[keep]
        out.append(torch.cat([torch.full((len(pts), 1), float(b), device=device), pts], 1))
    return torch.cat(out).contiguous()


class TorchVFE(torch.nn.Module):
    """The same layers on torch alone (the reference's forward with torch_scatter replaced by torch's own scatter)."""

    def __init__(self, hip):
        super().__init__()
        self.pfn_layers = hip.pfn_layers
        self.h = hip

    def forward(self, points):
        h = self.h
        rng = points.new_tensor(h.point_cloud_range[:2])
        vox = points.new_tensor(h.voxel_size[:2])
        grid = torch.tensor(h.grid_size[:2], device=points.device)
        c = torch.floor((points[:, [1, 2]] - rng) / vox).int()
        mask = ((c >= 0) & (c < grid)).all(dim=1)
        points, c = points[mask], c[mask]
        xyz = points[:, 1:4].contiguous()
        key = points[:, 0].int() * h.scale_xy + c[:, 0] * h.scale_y + c[:, 1]
        unq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
        mean = torch.zeros((unq.shape[0], 3), device=points.device).index_add_(0, inv, xyz) / cnt[:, None].float()
        f_center = torch.stack([xyz[:, 0] - (c[:, 0].float() * h.voxel_x + h.x_offset),
                                xyz[:, 1] - (c[:, 1].float() * h.voxel_y + h.y_offset), xyz[:, 2] - h.z_offset], 1)
        x = torch.cat([points[:, 1:], xyz - mean[inv], f_center], 1)
        idx = None
        for layer in self.pfn_layers:
            x = torch.relu(layer.norm(layer.linear(x)))
            if idx is None or idx.shape != x.shape:
                idx = inv.view(-1, 1).expand_as(x)
            x_max = torch.zeros((unq.shape[0], x.shape[1]), device=x.device).scatter_reduce(0, idx, x, 'amax', include_self=False)
            x = x_max if layer.last_vfe else torch.cat([x, x_max[inv]], 1)
        return x


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


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name)
    except Exception as e:                                        # noqa: BLE001 -- the count is a side figure
        return "profiler unavailable: %r" % (e,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda")
    points = make_points(a.batch, a.sweeps, dev)
    torch.manual_seed(0)
    hip = DynamicPillarVFE(MODEL_CFG, 4, VOXEL, GRID, RANGE).to(dev).train()
    ref = TorchVFE(hip).train()

    def hip_fwd():
        return hip({'points': points, 'batch_size': a.batch})['pillar_features']

    def ref_fwd():
        return ref(points)

    def fwd_bwd(f):
        def run():
            hip.zero_grad(set_to_none=True)
            f().sum().backward()
        return run

    with torch.no_grad():
        same = torch.allclose(hip_fwd(), ref_fwd(), atol=1e-4)
    res = {"points": int(points.shape[0]), "pillars": int(hip_fwd().shape[0]), "batch": a.batch, "outputs_close": bool(same)}
    # alternate the two paths, forward then forward + backward
    with torch.no_grad():
        res["hip_forward"] = timed(hip_fwd, a.steps, a.warmup)
        res["torch_forward"] = timed(ref_fwd, a.steps, a.warmup)
    res["hip_forward_backward"] = timed(fwd_bwd(hip_fwd), a.steps, a.warmup)
    res["torch_forward_backward"] = timed(fwd_bwd(ref_fwd), a.steps, a.warmup)
    with torch.no_grad():
        res["hip_launches_per_forward"] = launches(hip_fwd)
        res["torch_launches_per_forward"] = launches(ref_fwd)
    res["forward_ratio_torch_over_hip"] = res["torch_forward"]["median_ms"] / res["hip_forward"]["median_ms"]
    res["forward_backward_ratio_torch_over_hip"] = (res["torch_forward_backward"]["median_ms"]
                                                    / res["hip_forward_backward"]["median_ms"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
