"""Row f-13: time of the FOV ingest end to end -- B frames of raw points in host memory to the kept points in device
memory -- on two paths that alternate in one process on the same inputs:
  gpu_ingest      one upload of the raw points (pinned, asynchronous) and one ingest_ops.fov_ingest (DFU3D_ING_EMIT);
  numpy_recipe    the reference's recipe per frame on the host -- lidar_to_rect and rect_to_img as float32 np.dot, the five
                  comparisons, the boolean index (kitti_dataset.py:140-156, 480-486) -- then one upload of the kept points.
A host clock around each call, which ends in a device synchronise (warm-up, median, p10 / p90 of the runs): the host
path's time is host time, which device events would not see.  B = 4 frames of 34 720 points, 4 columns, one calibration
and one of two image shapes per frame.  `--gpu-only` runs the first path alone, for a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_ingest.py --gpu-only

    python tools/bench_ingest.py [--reps 50] [--warmup 10] [--B 4] [--gpu-only]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dfu3d_amd import ingest_ops  # noqa: E402
from dfu3d_amd.calibration import Calibration  # noqa: E402
from dfu3d_amd.pcdet_kitti.data_augmentor import _h2d  # noqa: E402

N_SCENE, C = 34720, 4
SHAPES = [(900, 1600), (375, 1242)]


def calib(b):
    h, w = SHAPES[b % 2]
    yaw = 0.02 * b
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], np.float64) @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], np.float64)
    f = 1260.0 if b % 2 == 0 else 720.0
    return Calibration({'P2': np.array([[f, 0, w / 2 - 0.5, -44.0], [0, f, h / 2 - 0.5, 0.2], [0, 0, 1, 0.003]], np.float32),
                        'R0': np.eye(3, dtype=np.float32),
                        'Tr_velo2cam': np.concatenate([R, [[0.0], [-0.08], [-0.27]]], 1).astype(np.float32)})


def make(B, rng):
    frames = []
    for b in range(B):
        p = np.stack([rng.uniform(-50, 50, N_SCENE), rng.uniform(-50, 50, N_SCENE), rng.uniform(-3, 1, N_SCENE),
                      rng.random(N_SCENE)], 1).astype(np.float32)
        frames.append((np.ascontiguousarray(p), calib(b), np.array(SHAPES[b % 2], np.int32)))
    return frames


def gpu_ingest(frames, dev):
    raw = [f[0] for f in frames]
    r = ingest_ops.fov_ingest(
        _h2d(np.concatenate(raw, 0), dev), _h2d(np.concatenate([[0], np.cumsum([len(p) for p in raw])]).astype(np.int64), dev),
        _h2d(np.stack([f[1].record() for f in frames]), dev), _h2d(np.stack([f[2] for f in frames]), dev))
    return r.points, r.out_off


def numpy_recipe(frames, dev):
    """The comparator: the reference's host recipe with float32 np.dot.  Not the code under test."""
    kept = []
    for p, c, shape in frames:
        one = np.ones((p.shape[0], 1), np.float32)
        rect = np.dot(np.hstack((p[:, 0:3], one)), c.M43)
        hom = np.hstack((rect, one))
        h = np.dot(hom, c.P2.T)
        with np.errstate(all="ignore"):
            img = (h[:, 0:2].T / hom[:, 2]).T
        depth = h[:, 2] - c.P2.T[3, 2]
        flag = np.logical_and(np.logical_and(img[:, 0] >= 0, img[:, 0] < shape[1]), np.logical_and(img[:, 1] >= 0, img[:, 1] < shape[0]))
        kept.append(p[np.logical_and(flag, depth >= 0)])
    off = np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.int64)
    return _h2d(np.concatenate(kept, 0), dev), off


def timed(fns, reps, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    wall = {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    q = lambda v, p: sorted(v)[int(p * (len(v) - 1))]  # noqa: E731
    return {k: (statistics.median(v), q(v, 0.1), q(v, 0.9)) for k, v in wall.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--gpu-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ingest.py needs cuda:0")
    dev = torch.device("cuda:0")
    frames = make(args.B, np.random.default_rng(args.B))
    fns = {"gpu_ingest": lambda: gpu_ingest(frames, dev)}
    if not args.gpu_only:
        fns["numpy_recipe"] = lambda: numpy_recipe(frames, dev)
    t = timed(fns, args.reps, args.warmup)
    out, off = fns["gpu_ingest"]()
    off = off.cpu().numpy()
    row = {"what": "fov_ingest", "B": args.B, "points": args.B * N_SCENE, "kept": int(off[-1])}
    if not args.gpu_only:
        want, want_off = fns["numpy_recipe"]()
        # np.dot's float32 sums are the BLAS's; the stage's are the defined chain: a point on an image border may differ
        row["kept_numpy_recipe"] = int(want_off[-1])
        row["same_rows"] = bool(off.tolist() == want_off.tolist() and torch.equal(out[:int(off[-1])], want))
    for name in fns:
        m, p10, p90 = t[name]
        print(json.dumps(dict(row, path=name, wall_ms=round(m, 4), p10=round(p10, 4), p90=round(p90, 4),
                              upload_bytes=int(args.B * N_SCENE * C * 4) if name == "gpu_ingest" else int(row["kept"] * C * 4))),
              flush=True)


if __name__ == "__main__":
    main()
