"""Row f-9: time of the CenterHead post-processing on the GPU -- the existing per-(head, sample) path
`generate_predicted_boxes` next to `generate_predicted_boxes_batched` in its list form (one host read) and its padded
form (none).  The three paths alternate in one process on the same inputs; kernel time by HIP events around the call
(warm-up, median, p10 / p90), whole-call time by the host clock around call + synchronise, kernels per call from torch's
profiler.  Configuration A of the CenterPoint config (6 heads, 128 x 64 map), K = 500, the config's POST_PROCESSING, maps
scaled as in tests/test_gpu_center_postprocess.py (30 .. 700 cells above the score threshold per head and sample, boxes
that overlap their neighbours), B = 4 (the config's batch) and B = 64.

    python tools/bench_center_postprocess.py [--reps 100] [--batches 4,64]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_gpu_center_postprocess import _post, e2e_maps, make_head  # noqa: E402
from tools.bench_center_loss import launches, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--batches", default="4,64")
    args = ap.parse_args()
    head = make_head(_post(83))
    for B in (int(v) for v in args.batches.split(",")):
        rng = np.random.default_rng(B)
        above = rng.integers(30, 701, (6, B)).tolist()
        preds = [{k: torch.from_numpy(v).cuda() for k, v in d.items()} for d in e2e_maps(seed=B, B=B, above=above)]
        fns = {"per_sample": lambda: head.generate_predicted_boxes(B, preds),
               "batched_list": lambda: head.generate_predicted_boxes_batched(B, preds),
               "batched_padded": lambda: head.generate_predicted_boxes_batched(B, preds, as_padded=True)}
        t = timed(fns, args.reps, warmup=20)
        kept = sum(int(d['pred_scores'].shape[0]) for d in fns["batched_list"]())
        same = all(torch.equal(a[k], b[k]) for a, b in zip(fns["per_sample"](), fns["batched_list"]())
                   for k in ('pred_boxes', 'pred_scores', 'pred_labels'))
        for name, fn in fns.items():
            e, p10, p90, w = t[name]
            print(json.dumps({"what": "center_postprocess", "path": name, "B": B, "heads": 6, "K": 500,
                              "gpu_event_ms": round(e, 4), "p10": round(p10, 4), "p90": round(p90, 4),
                              "call_ms": round(w, 4), "kernels": launches(fn), "boxes_kept": kept,
                              "equal_to_per_sample": same}), flush=True)


if __name__ == "__main__":
    main()
