"""Row f-8: time of CenterHead.get_loss + backward on the GPU next to a torch-only composition of the same contract with
the cost profile of an unfused implementation (per head: clamped sigmoid, the focal terms and their sums, cat of the
regression maps, permute + gather, the masked L1, and two .item() reads per head plus one for the total).  Both paths
alternate in one process; kernel time by HIP events (warm-up, median, p10 / p90), whole-call time by the host clock
around call + synchronise, launches per call from the profiler's kernel count.  Configuration A of the CenterPoint
config, 30 boxes per sample, B = 4 (the config's batch) and B = 64.

    python tools/bench_center_loss.py [--reps 200]"""
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
from tools.bench_center_head import scene  # noqa: E402
from dfu3d_amd.pcdet_kitti.center_head import CenterHead  # noqa: E402

ORDER = ['center', 'center_z', 'dim', 'rot']
CHANNELS = {'center': 2, 'center_z': 1, 'dim': 3, 'rot': 2}
WEIGHTS = dict(cls_weight=1.0, loc_weight=0.25, code_weights=[1.0] * 8)


def torch_get_loss(pred_dicts, tg):
    """The loss contract of DESIGN.md row f-8 as one torch operation after the other, float32, head by head, with the
    cost profile of an unfused implementation: the regression maps are concatenated and permuted to channels-last before
    the gather at `inds`, and every head reads its two losses back to the host, as does the total."""
    total, report = None, {}
    code_w = None
    for h, d in enumerate(pred_dicts):
        heat = tg['heatmaps'][h]
        p = d['hm'].sigmoid().clamp(1e-4, 1 - 1e-4)
        is_pos = heat == 1
        focal = torch.where(is_pos, p.log() * (1 - p).square(), (1 - p).log() * p.square() * (1 - heat).square().square())
        focal = torch.where(heat <= 1, focal, torch.zeros_like(focal))
        n_pos = is_pos.sum()
        hm_loss = WEIGHTS['cls_weight'] * (-focal.sum() / n_pos.clamp(min=1))
        maps = torch.cat([d[k] for k in ORDER], 1)
        B, D = maps.shape[:2]
        cells = maps.permute(0, 2, 3, 1).contiguous().reshape(B, -1, D)
        at = torch.gather(cells, 1, tg['inds'][h][:, :, None].expand(-1, -1, D))
        target = tg['target_boxes'][h]
        use = (tg['masks'][h] != 0)[:, :, None] & ~target.isnan()
        l1 = torch.where(use, (at - target).abs(), torch.zeros_like(target)).sum((0, 1))
        per_channel = l1 / (tg['masks'][h] != 0).sum().clamp(min=1)
        if code_w is None:
            code_w = per_channel.new_tensor(WEIGHTS['code_weights'])
        loc_loss = WEIGHTS['loc_weight'] * (per_channel * code_w).sum()
        total = hm_loss + loc_loss if total is None else total + (hm_loss + loc_loss)
        report['hm_loss_head_%d' % h] = hm_loss.item()
        report['loc_loss_head_%d' % h] = loc_loss.item()
    report['rpn_loss'] = total.item()
    return total, report


def timed(fns, reps, warmup=20):
    """fns: {name: callable}; the callables alternate.  -> {name: (event median, p10, p90, wall median)} in ms."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            ev[name].append(a.elapsed_time(b))
    q = lambda v, p: sorted(v)[int(p * (len(v) - 1))]  # noqa: E731
    return {k: (statistics.median(ev[k]), q(ev[k], 0.1), q(ev[k], 0.9), statistics.median(wall[k])) for k in fns}


def launches(fn):
    """Kernels per call, counted by torch's profiler (every kernel of the process, the library's included)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA and 'Memcpy' not in e.key
               and 'Memset' not in e.key)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    cfg = ref.CFG_A
    H, W = cfg['map_hw']
    model_cfg = dict(CLASS_NAMES_EACH_HEAD=cfg['heads'], LOSS_CONFIG=dict(LOSS_WEIGHTS=WEIGHTS),
                     TARGET_ASSIGNER_CONFIG=dict(FEATURE_MAP_STRIDE=cfg['stride'], NUM_MAX_OBJS=cfg['num_max_objs'],
                                                 GAUSSIAN_OVERLAP=cfg['gaussian_overlap'], MIN_RADIUS=cfg['min_radius']))
    head = CenterHead(model_cfg, cfg['class_names'], np.array(cfg['point_cloud_range'], np.float32), cfg['voxel_size'])
    rng = np.random.default_rng(0)
    for B in (4, 64):
        tg = head.assign_targets(torch.from_numpy(scene(rng, cfg, B, 30)).cuda(), feature_map_size=[H, W], check=True)
        gen = torch.Generator(device='cuda').manual_seed(B)
        preds = []
        for names in cfg['heads']:
            d = {'hm': (torch.randn(B, len(names), H, W, device='cuda', generator=gen) * 2 - 2.19).requires_grad_()}
            for k in ORDER:
                d[k] = torch.randn(B, CHANNELS[k], H, W, device='cuda', generator=gen).requires_grad_()
            preds.append(d)

        def hip():
            head.get_loss(preds, tg)[0].backward()

        def hip_nosync():
            head.get_loss(preds, tg, as_tensors=True)[0].backward()

        def composition():
            torch_get_loss(preds, tg)[0].backward()
        fns = {"hip": hip, "hip_as_tensors": hip_nosync, "torch": composition}
        t = timed(fns, args.reps)
        l_hip, l_torch = head.get_loss(preds, tg)[1]['rpn_loss'], torch_get_loss(preds, tg)[1]['rpn_loss']
        for name, fn in fns.items():
            e, p10, p90, w = t[name]
            print(json.dumps({"what": "get_loss+backward", "path": name, "B": B, "boxes_per_sample": 30,
                              "gpu_event_ms": round(e, 4), "p10": round(p10, 4), "p90": round(p90, 4),
                              "call_ms": round(w, 4), "launches": launches(fn), "rpn_loss": l_hip if name != "torch" else l_torch}))


if __name__ == "__main__":
    main()
