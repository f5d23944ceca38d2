#!/usr/bin/env python
"""Time the sparse-convolution stage (csrc/sparseconv_stage.hip through sparse_conv_ops) on the five layer shapes of
VoxelResBackBone8x and on a whole forward plus backward of that backbone, against a plain-torch formulation of the same
result on the same device: per kernel offset a gather of the input rows of the offset's (input, output) pairs, a matmul
with the offset's weight slice and an index_add_ into the output rows.  The pair lists of the torch side are made from
the stage's own neighbour table before the timing (its index plan is not what is compared); the stage's plan is timed
on its own line.  y of the two is compared within the float32 bound before timing.

Input: B = 4 sweeps of dfu3d_amd.synth.lidar_sweep cut to KITTI's range [0, -40, -3, 70.4, 40, 1], voxels of
0.05 / 0.05 / 0.1 m (grid 1408 x 1600 x 40) by hard_voxel_ops.hard_voxels, the voxel means as features.

Timing: HIP events around each call on the current stream, every shape warmed up, the median and the spread over the
steps; stage and baseline alternate inside one process.  The achieved rate is 2 * pairs * Cin * Cout over the forward
kernel's time, against the 157 TFLOP/s f32 matrix peak; the gather traffic is pairs * Cin * 4 bytes against 8 TB/s.

    python tools/bench_sparse_conv.py [--batch 4] [--steps 30] [--warmup 5] [--table]
prints one JSON line (and, with --table, the markdown table of DESIGN.md).  No time is asserted anywhere.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfu3d_amd import hard_voxel_ops, sparse_conv_ops as ops, synth  # noqa: E402
from dfu3d_amd.pcdet_kitti import spconv_utils  # noqa: E402
from dfu3d_amd.pcdet_kitti.spconv_backbone import VoxelResBackBone8x  # noqa: E402
from tools.bench_hard_voxels import timed  # noqa: E402

RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
VOXEL = [0.05, 0.05, 0.1]
GRID = [1408, 1600, 40]
# name, channels in and out, and which convolution of the backbone has the shape
SHAPES = [("conv_input subm 3^3", 4, 16, lambda bb: bb.conv_input[0]), ("spconv2 3^3 s2 p1", 16, 32, lambda bb: bb.conv2[0][0]),
          ("res3 subm 3^3", 64, 64, lambda bb: bb.conv3[1].conv1), ("spconv4 3^3 s2 p(0,1,1)", 64, 128, lambda bb: bb.conv4[0][0]),
          ("conv_out (3,1,1) s(2,1,1)", 128, 128, lambda bb: bb.conv_out[0])]


def voxels(B, rings, az, seed, dev):
    lo, hi = torch.tensor(RANGE[:3], device=dev), torch.tensor(RANGE[3:], device=dev)
    rows, sizes = [], []
    for b in range(B):
        rng = np.random.default_rng(seed + b)
        gen = torch.Generator(device=dev).manual_seed(seed + b)
        p = synth.lidar_sweep(synth._boxes(rng), gen, dev, rings=rings, az=az)
        p = p[((p[:, :3] >= lo) & (p[:, :3] < hi)).all(1)]
        rows.append(torch.cat([torch.full((len(p), 1), float(b), device=dev), p], 1))
        sizes.append(len(p))
    pts = torch.cat(rows, 0).contiguous()
    hv = hard_voxel_ops.hard_voxels(pts, torch.tensor(sizes, dtype=torch.int32, device=dev), RANGE, VOXEL, GRID, 5, 40000,
                                    want_voxels=False, want_mean=True)
    n = int(hv.n_voxels.item())
    return hv.voxel_mean[:n].contiguous(), hv.voxel_coords[:n].contiguous(), sizes


def pair_lists(t):
    """Per offset the (input rows, output rows) of the table's pairs."""
    out = []
    for K in range(t.kv):
        col = t.nbr[:, K]
        o = torch.nonzero(col >= 0).flatten()
        out.append((col[o].long(), o))
    return out


def torch_conv(x, w, pairs, n_out):
    """y of the header's sum, in torch's order: per offset gather, matmul, index_add_."""
    cout = w.shape[0]
    wf = w.reshape(cout, -1, w.shape[-1])
    y = torch.zeros((n_out, cout), dtype=x.dtype, device=x.device)
    for K, (i, o) in enumerate(pairs):
        if len(i):
            y.index_add_(0, o, x[i] @ wf[:, K, :].t())
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--rings', type=int, default=64)
    ap.add_argument('--az', type=int, default=1300)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--table', action='store_true')
    a = ap.parse_args()
    dev = 'cuda:0'
    torch.manual_seed(0)
    feats, coords, sizes = voxels(a.batch, a.rings, a.az, 2019, dev)
    bb = VoxelResBackBone8x({}, 4, GRID).to(dev).train()
    specs = spconv_utils.chain_specs(bb)
    plan = spconv_utils.plan_for(coords, a.batch, bb.sparse_shape, specs)
    level_of = {}
    for m, sp in zip([m for m in bb.modules() if isinstance(m, spconv_utils.SparseConvolution)], specs):
        level_of[m] = plan.lookup[tuple(sp)]
    rows = []
    for name, cin, cout, pick in SHAPES:
        conv = pick(bb)
        t = level_of[conv]
        x = torch.randn((t.n_in, cin), device=dev)
        w = conv.weight.detach()
        dy = torch.randn((t.n_out, cout), device=dev)
        pairs = pair_lists(t)
        n_pairs = int(sum(len(i) for i, _ in pairs))
        y, yt = ops.conv_forward(x, w, t), torch_conv(x, w, pairs, t.n_out)
        # both are float32 sums of the same n = KV * Cin terms in some order: within 2 gamma_n sum |x w| of each other
        mag = torch_conv(x.abs(), w.abs(), pairs, t.n_out)
        n = t.kv * cin
        close = bool(((y - yt).abs() <= 2 * n * 2.0 ** -24 / (1 - n * 2.0 ** -24) * mag + 1e-30).all())

        def torch_fb():
            xx, ww = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
            torch_conv(xx, ww, pairs, t.n_out).backward(dy)
        fns = [lambda: ops.conv_forward(x, w, t), lambda: torch_conv(x, w, pairs, t.n_out),
               lambda: ops.conv_dgrad(dy, w, t), lambda: ops.conv_wgrad(x, dy, t, w.shape), torch_fb]
        f, tf, dg, wg, tfb = timed(fns, a.steps, a.warmup)
        sec = f['median_ms'] * 1e-3
        rows.append(dict(layer=name, cin=cin, cout=cout, n_in=t.n_in, n_out=t.n_out, pairs=n_pairs, same_result=close,
                         forward=f, torch_forward=tf, dgrad=dg, wgrad=wg, torch_forward_backward=tfb,
                         tflops=2.0 * n_pairs * cin * cout / sec / 1e12, share_of_157_tflops=2.0 * n_pairs * cin * cout / sec / 157e12,
                         gather_gb_per_s=n_pairs * cin * 4 / sec / 1e9, gather_share_of_8_tb_per_s=n_pairs * cin * 4 / sec / 8e12))
    # the whole backbone, forward plus backward, the plan included; then the same modules on the torch formulation
    batch = {'batch_size': a.batch, 'voxel_features': feats, 'voxel_coords': coords}

    def whole():
        bb.zero_grad(set_to_none=True)
        out = bb(dict(batch))['encoded_spconv_tensor'].features
        out.sum().backward()
    cache = {}

    def by_torch(features, weight, t):
        key = (t.in_level, t.out_level, t.kv, t.n_in, t.n_out)         # (the same coordinates every call: the same tables)
        if key not in cache:
            cache[key] = pair_lists(t)
        return torch_conv(features, weight, cache[key], t.n_out)
    own = ops.sparse_conv

    def whole_torch():
        ops.sparse_conv = by_torch
        try:
            whole()
        finally:
            ops.sparse_conv = own
    whole_torch()                                                # (fills the cache of pair lists, outside the timing)
    t_plan, t_whole, t_whole_torch = timed([lambda: spconv_utils.plan_for(coords, a.batch, bb.sparse_shape, specs), whole,
                                            whole_torch], max(a.steps // 3, 3), 2)
    res = dict(batch=a.batch, rows=sizes, voxels=int(feats.shape[0]), levels=[lv.rows for lv in plan.levels], grid=GRID,
               steps=a.steps, device=torch.cuda.get_device_name(0), layers=rows, plan=t_plan,
               backbone_forward_backward=t_whole, backbone_forward_backward_torch_products=t_whole_torch)
    print(json.dumps(res))
    if a.table:
        print("| layer | Cin -> Cout | rows in -> out | pairs | forward ms (p10 .. p90) | torch forward ms | dgrad ms | wgrad ms |"
              " torch fwd + bwd ms | TFLOP/s (of 157) | gather GB/s (of 8000) |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print("| %s | %d -> %d | %d -> %d | %d | %.3f (%.3f .. %.3f) | %.3f | %.3f | %.3f | %.3f | %.2f (%.1f %%) | %.0f (%.1f %%) |" % (
                r['layer'], r['cin'], r['cout'], r['n_in'], r['n_out'], r['pairs'], r['forward']['median_ms'],
                r['forward']['p10_ms'], r['forward']['p90_ms'], r['torch_forward']['median_ms'], r['dgrad']['median_ms'],
                r['wgrad']['median_ms'], r['torch_forward_backward']['median_ms'], r['tflops'],
                100 * r['share_of_157_tflops'], r['gather_gb_per_s'], 100 * r['gather_share_of_8_tb_per_s']))
        print("| index plan (one read) | | | | %.3f (%.3f .. %.3f) | | | | | | |" % (t_plan['median_ms'], t_plan['p10_ms'], t_plan['p90_ms']))
        print("| VoxelResBackBone8x forward + backward | | | | %.3f (%.3f .. %.3f) | | | | %.3f | | |" % (
            t_whole['median_ms'], t_whole['p10_ms'], t_whole['p90_ms'], t_whole_torch['median_ms']))


if __name__ == '__main__':
    main()
