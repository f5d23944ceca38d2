"""Measurement of SURVEY.md §8 row f-5 on the GPU box: ground-truth sampling (DataBaseSampler.sample_batch) over 64
synthetic scenes of 34 720 points, with the database built from the same frames by create_groundtruth_database and the
CenterPoint config's SAMPLE_GROUPS (LIMIT_WHOLE_SCENE, filter_by_min_points 5).
Prints one JSON line: scenes/s of the whole call (host draw + packing + copies + kernels) and of the kernels alone
(HIP events, after warm-up), the kernels' achieved GB/s against their algorithmic bytes (scene points read once,
pasted object rows read once, every output row written once), the NumPy restatement's scenes/s on one core, and
`parity`: the GPU's 64 scenes equal the restatement's bit for bit.  Numbers are reported, not gated on."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dfu3d_amd import kitti_io, synth  # noqa: E402
from dfu3d_amd.calibration import Calibration  # noqa: E402
from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler  # noqa: E402
from dfu3d_amd.pcdet_kitti.gt_database import create_groundtruth_database  # noqa: E402
from tests.gt_sampling_ref import RefSampler  # noqa: E402

GROUPS = ['Car:2', 'Truck:3', 'Construction_vehicle:7', 'Bus:4', 'Trailer:6', 'Barrier:2', 'Motorcycle:6',
          'Bicycle:6', 'Pedestrian:2', 'Traffic_cone:2']
FRAMES = 64
DEV = "cuda:0"


def write_kitti(root):
    for d in ("velodyne", "calib", "label_2"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    scenes = []
    for f in range(FRAMES):
        sc = synth.make_scene(f, H=90, W=160, M=1, cams=1, dense=False, k_min=30, k_max=40)
        sid = "%06d" % f
        pts = sc.points.numpy()
        pts.tofile(os.path.join(root, "velodyne", sid + ".bin"))
        cal = sc.calibs[0]
        kitti_io.write_calib(os.path.join(root, "calib", sid + ".txt"), cal.P2, cal.R0, cal.V2C)
        b = np.asarray(sc.boxes3d, np.float64)
        bottom = b[:, :3].copy()
        bottom[:, 2] -= b[:, 5] / 2
        loc = Calibration(os.path.join(root, "calib", sid + ".txt")).lidar_to_rect(bottom)
        with open(os.path.join(root, "label_2", sid + ".txt"), "w") as fh:
            for k in range(b.shape[0]):
                fh.write("%s 0.00 0 0.00 10.00 10.00 120.00 120.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n" % (
                    synth.BOX_TYPES[int(b[k, 7])][0], b[k, 5], b[k, 4], b[k, 3], loc[k, 0], loc[k, 1], loc[k, 2],
                    -b[k, 6] - np.pi / 2))
        names = np.array([synth.BOX_TYPES[int(t)][0] for t in b[:, 7]])
        scenes.append({'points': pts, 'gt_boxes': b[:, :7].astype(np.float32), 'gt_names': names,
                       'gt_boxes_mask': np.ones(len(names), bool)})
    return scenes


def main():
    with tempfile.TemporaryDirectory() as root:
        scenes = write_kitti(root)
        infos = create_groundtruth_database(root, ["%06d" % f for f in range(FRAMES)], batch_frames=32)
        classes = [c for c in infos if any(i['num_points_in_gt'] >= 5 for i in infos[c])]
        cfg = {'DB_INFO_PATH': ['kitti_dbinfos_train.pkl'], 'USE_SHARED_MEMORY': False,
               'PREPARE': {'filter_by_min_points': [g.split(':')[0] + ':5' for g in GROUPS]},
               'SAMPLE_GROUPS': GROUPS, 'NUM_POINT_FEATURES': 4, 'DATABASE_WITH_FAKELIDAR': False,
               'REMOVE_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'LIMIT_WHOLE_SCENE': True}
        copy = lambda: [{k: v.copy() for k, v in d.items()} for d in scenes]   # noqa: E731
        smp = DataBaseSampler(root, cfg, classes, device=DEV)
        # parity first, on fresh RNG state
        np.random.seed(0)
        got = smp.sample_batch(copy()).split()
        ref = RefSampler(root, cfg, classes)
        np.random.seed(0)
        t0 = time.perf_counter()
        exp = [ref(d)[0] for d in copy()]
        cpu_s = time.perf_counter() - t0
        parity = all(np.array_equal(g['points'].view(np.uint32), e['points'].view(np.uint32)) and
                     np.array_equal(g['gt_boxes'], e['gt_boxes']) and np.array_equal(g['gt_names'], e['gt_names'])
                     for g, e in zip(got, exp))
        pasted = sum(len(g['gt_names']) - len(d['gt_names']) for g, d in zip(got, scenes))
        # whole call: draw + pack + copies + kernels + the copy-back of split()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            smp.sample_batch(copy()).split()
        torch.cuda.synchronize()
        K = 10
        dd = [copy() for _ in range(K)]
        e0.record()
        for k in range(K):
            smp.sample_batch(dd[k]).split()
        e1.record()
        torch.cuda.synchronize()
        call_ms = e0.elapsed_time(e1) / K
        # kernels alone on one uploaded batch
        u = smp.upload_batch(copy())
        for _ in range(3):
            b = smp.launch_batch(u)
        torch.cuda.synchronize()
        K2 = 50
        e0.record()
        for _ in range(K2):
            b = smp.launch_batch(u)
        e1.record()
        torch.cuda.synchronize()
        kern_ms = e0.elapsed_time(e1) / K2
        n_in = sum(len(d['points']) for d in scenes)
        n_out = int(b.point_off[-1].item())
        acc = b.accept.cpu().numpy().astype(bool)
        obj_rows = int(u['obj_cnt'].cpu().numpy()[acc].sum())
        alg = 16.0 * (n_in + obj_rows + n_out)
        print(json.dumps({
            "metric": "gt_sampling", "scenes": FRAMES, "points_per_scene": 34720, "db_objects": sum(map(len, infos.values())),
            "classes": classes, "pasted_objects": pasted, "scenes_per_s_call": round(FRAMES / (call_ms * 1e-3), 1),
            "call_ms": round(call_ms, 3), "kernels_ms": round(kern_ms, 4),
            "scenes_per_s_kernels": round(FRAMES / (kern_ms * 1e-3), 1),
            "kernels_GBps": round(alg / (kern_ms * 1e-3) / 1e9, 1), "algorithmic_MB": round(alg / 1e6, 2),
            "cpu_restatement_scenes_per_s": round(FRAMES / cpu_s, 2), "parity": bool(parity)}))


if __name__ == "__main__":
    main()
