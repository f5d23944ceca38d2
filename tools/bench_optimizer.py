"""Row f-12: time of the optimiser step on the GPU -- the fused stage (train_utils OptimWrapper.step: gradient clipping,
true weight decay and Adam in DFU3D_OPT_LAUNCHES launches) next to the reference's recipe written in torch for this tool:
clip_grad_norm_, the per-parameter decay loop, torch.optim.Adam over the same two groups.  Both run on the parameter
tensors of the full centerpoint_nuscenes2kitti.yaml model (247 tensors, 5 759 738 floats) with random gradients, each on
its own copy of the parameters; they alternate in one process; HIP events around the call (warm-up, median, p10 / p90 of
the runs).  Also the stage's bytes per second against its algorithmic bytes: 7 words per element (p, g, m, v read and p,
m, v written) plus the norm pass over g, 184 MB.

    python tools/bench_optimizer.py [--reps 50] [--warmup 10]"""
import argparse
import json
import os
import sys

import torch
from torch.nn.utils import clip_grad_norm_

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dfu3d_amd.train_utils.optimization import build_optimizer  # noqa: E402
from tools.bench_center_loss import launches, timed  # noqa: E402

LR, MOM, WD, MAX_NORM = 1e-3, 0.9, 0.01, 10.0


def full_model(dev):
    from dfu3d_amd.pcdet_kitti.centerpoint import CenterPoint
    from tests import centerpoint_cases as K
    torch.manual_seed(0)
    return CenterPoint(K.cfg(K.FULL_MODEL), len(K.FULL_CLASSES), **K.FULL_DATASET).to(dev)


class Cfg(dict):
    __getattr__ = dict.__getitem__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = Cfg(OPTIMIZER='adam_onecycle', LR=LR, WEIGHT_DECAY=WD, GRAD_NORM_CLIP=MAX_NORM)
    a, b = full_model(dev), full_model(dev)
    fused = build_optimizer(a, cfg)
    fused.lr, fused.mom = LR, MOM
    names = {id(p): n for n, p in a.named_parameters()}
    b_named = dict(b.named_parameters())
    groups = [[b_named[names[id(p)]] for p in g['params']] for g in fused.param_groups]
    adam = torch.optim.Adam([{'params': g, 'lr': LR, 'betas': (MOM, 0.99)} for g in groups])
    b_params = [p for g in groups for p in g]
    gen = torch.Generator(device=dev).manual_seed(12)
    for pa, pb in zip(fused.params, b_params):
        pa.grad = torch.randn(pa.shape, device=dev, generator=gen) * 0.05
        pb.grad = pa.grad.clone()
    elements = sum(p.numel() for p in fused.params)

    def comparator():
        """Not the code under test: train_one_epoch's clipping, OptimWrapper.step's decay loop, Adam."""
        clip_grad_norm_(b_params, MAX_NORM)
        with torch.no_grad():
            for p in b_params:
                p.mul_(1 - WD * LR)
        adam.step()

    fns = {"stage": fused.step, "torch_comparator": comparator}
    t = timed(fns, args.reps, warmup=args.warmup)
    nbytes = 4 * elements * 8
    for name in fns:
        e, p10, p90, w = t[name]
        row = {"what": "optimizer_step", "path": name, "tensors": len(fused.params), "elements": elements,
               "gpu_event_ms": round(e, 4), "p10": round(p10, 4), "p90": round(p90, 4), "call_ms": round(w, 4),
               "kernels": launches(fns[name])}
        if name == "stage":
            row["algorithmic_MB"] = round(nbytes / 1e6, 1)
            row["algorithmic_GB_per_s"] = round(nbytes / (e * 1e-3) / 1e9, 1)
            row["median_below_comparator_p10"] = bool(e < t["torch_comparator"][1])
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
