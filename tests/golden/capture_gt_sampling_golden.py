"""Golden G11: the reference's own ground-truth sampling augmentor (`DataBaseSampler`, row f-5 of SURVEY.md section 8)
over a small synthetic database and ten scenes, under two configurations.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_gt_sampling_golden.py REFERENCE_ROOT      ->  tests/golden/g11_gt_sampling.npz

pcdet/datasets/augmentor/database_sampler.py, pcdet/utils/box_utils.py and pcdet/utils/common_utils.py are imported
UNMODIFIED as members of a package skeleton (pcdet/__init__ and the compiled ops are not touched).  Import-time stand-ins:
`skimage`, `SharedArray` and `kitti_common` are empty modules (unused on this path); the two compiled leaves are
replaced -- `iou3d_nms_utils.boxes_bev_iou_cpu` by oracle.iou3d_oracle.boxes_bev and
`roiaware_pool3d_utils.points_in_boxes_cpu` by oracle.gtdb_oracle.points_in_boxes_cpu.  G11 therefore pins the
reference's orchestration (group order, LIMIT_WHOLE_SCENE, the pointer / permutation walk on NumPy's global RNG, the
acceptance rule, mask handling, enlargement dtype, output order), not those two leaves.

Configuration 0: the CenterPoint config's shape (LIMIT_WHOLE_SCENE, filter_by_min_points, zero REMOVE_EXTRA_WIDTH,
float32 scene boxes, a group whose class is not sampled).  Configuration 1: fixed sample numbers, filter_by_difficulty,
REMOVE_EXTRA_WIDTH [0.3, 0.2, 0.1] and float64 scene boxes.  Scenes: one with no boxes, one whose single huge box makes
every candidate collide, one with no points; the Car group (7 objects, 3 per draw) wraps with a short slice.
Per scene the file stores the inputs, the reference's outputs and the candidate ids `sample_with_fixed_number` returned
(recorded by wrapping the bound method), per configuration the final state of NumPy's global RNG.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('PCDET_REFERENCE', '')

from oracle.gtdb_oracle import points_in_boxes_cpu  # noqa: E402
from oracle.iou3d_oracle import boxes_bev  # noqa: E402
from tests.gt_sampling_ref import write_database  # noqa: E402

CLASSES = ['Car', 'Pedestrian', 'Cyclist']
SEEDS = [11, 12]


class Cfg(dict):
    __getattr__ = dict.__getitem__


def load_reference():
    import torch
    for name in ('pcdet', 'pcdet.ops', 'pcdet.ops.iou3d_nms', 'pcdet.ops.roiaware_pool3d', 'pcdet.utils',
                 'pcdet.datasets', 'pcdet.datasets.augmentor', 'pcdet.datasets.kitti',
                 'pcdet.datasets.kitti.kitti_object_eval_python', 'skimage'):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    for name in ('SharedArray', 'pcdet.utils.calibration_kitti', 'pcdet.datasets.kitti.kitti_object_eval_python.kitti_common'):
        sys.modules[name] = types.ModuleType(name)
    sys.modules['skimage'].io = types.ModuleType('skimage.io')
    iou = types.ModuleType('pcdet.ops.iou3d_nms.iou3d_nms_utils')
    iou.boxes_bev_iou_cpu = lambda a, b: boxes_bev(np.asarray(a), np.asarray(b)).astype(np.float32)
    sys.modules[iou.__name__] = iou
    sys.modules['pcdet.ops.iou3d_nms'].iou3d_nms_utils = iou
    ra = types.ModuleType('pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils')
    ra.points_in_boxes_cpu = lambda p, b: torch.from_numpy(points_in_boxes_cpu(p.numpy(), b.numpy()))
    sys.modules[ra.__name__] = ra
    sys.modules['pcdet.ops.roiaware_pool3d'].roiaware_pool3d_utils = ra
    sys.modules['pcdet.datasets.kitti.kitti_object_eval_python'].kitti_common = \
        sys.modules['pcdet.datasets.kitti.kitti_object_eval_python.kitti_common']

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], mod)
        return mod
    load('pcdet.utils.common_utils', os.path.join(REF, 'pcdet/utils/common_utils.py'))
    load('pcdet.utils.box_utils', os.path.join(REF, 'pcdet/utils/box_utils.py'))
    return load('pcdet.datasets.augmentor.database_sampler', os.path.join(REF, 'pcdet/datasets/augmentor/database_sampler.py'))


def apart(rng, n, lo, hi, taken, sizes):
    """n boxes in [lo, hi)^2 whose footprints stay >= 0.3 m clear of each other and of `taken` (no near touches)."""
    out = []
    while len(out) < n:
        l, w, h = sizes[int(rng.integers(len(sizes)))]
        x, y = rng.uniform(lo, hi, 2)
        r = 0.5 * np.hypot(l, w)
        if all(np.hypot(x - o[0], y - o[1]) > r + 0.5 * np.hypot(o[3], o[4]) + 0.3 for o in taken + out):
            out.append([x, y, rng.uniform(-1.5, -0.5), l, w, h, rng.uniform(-np.pi, np.pi)])
    return out


def make_database(rng):
    sizes = {'Car': [(4.2, 1.8, 1.6), (3.9, 1.7, 1.5)], 'Pedestrian': [(0.8, 0.7, 1.8)], 'Cyclist': [(1.8, 0.7, 1.7)]}
    n_per = {'Car': 7, 'Pedestrian': 9, 'Cyclist': 5}
    classes, boxes = [], []
    for c in CLASSES:
        # database boxes come from different frames, so they may overlap: within a class apart() keeps them clear,
        # and one shifted copy per class makes a pair that clearly overlaps (the within-group rule)
        bs = apart(rng, n_per[c] - 1, -30.0, 30.0, [], sizes[c])
        bs.append([bs[0][0] + 0.4, bs[0][1] - 0.3] + list(bs[0][2:]))
        for b in bs:
            classes.append(c)
            boxes.append(b)
    boxes = np.array(boxes)
    counts = rng.integers(3, 40, len(classes))
    counts[3] = 2                                              # one Car under filter_by_min_points' 'Car:3'
    pts = []
    for k in range(len(classes)):
        p = np.zeros((counts[k], 4), np.float32)
        p[:, :3] = (rng.uniform(-0.5, 0.5, (counts[k], 3)) * boxes[k, 3:6]).astype(np.float32)
        p[:, 3] = rng.random(counts[k]).astype(np.float32)
        pts.append(p)
    return classes, boxes, counts, pts, rng.integers(0, 3, len(classes))


def make_scenes(rng, db_boxes):
    scenes = []
    for s in range(10):
        n_pts = 0 if s == 9 else int(rng.integers(300, 600))
        p = np.zeros((n_pts, 4), np.float32)
        p[:, :2] = rng.uniform(-32, 32, (n_pts, 2))
        p[:, 2] = rng.uniform(-2.0, 0.5, n_pts)
        p[:, 3] = rng.random(n_pts)
        near = db_boxes[rng.choice(len(db_boxes), 8, replace=False)]
        extra = []
        for b in near:                                         # points in, on and just outside database boxes
            q = np.zeros((12, 4), np.float32)
            q[:, 0:3] = b[:3] + rng.uniform(-0.7, 0.7, (12, 3)) * np.r_[b[3:5], b[5]]
            q[:, 3] = rng.random(12)
            extra.append(q)
        if n_pts:
            p = np.concatenate([p] + extra, 0)
        if s == 7:
            names, gt = np.array([], dtype='<U10'), np.zeros((0, 7))
        elif s == 8:
            names, gt = np.array(['Truck']), np.array([[0.0, 0.0, -1.0, 200.0, 200.0, 3.0, 0.0]])
        else:
            k = int(rng.integers(1, 6))
            gt = np.array(apart(rng, k, -40.0, 40.0, [], [(4.0, 1.8, 1.5), (0.8, 0.8, 1.7)]))
            names = np.array([['Car', 'Pedestrian', 'Cyclist', 'Van'][int(rng.integers(4))] for _ in range(k)])
        mask = rng.random(len(names)) < 0.8
        scenes.append({'points': p, 'gt_boxes': gt, 'gt_names': names, 'gt_boxes_mask': mask})
    return scenes


def no_near_touch(boxes):
    """Every pair either overlaps by more than 1e-3 m^2 or stays clear when both grow by 2 cm: the float32 overlap of
    the product and the exact one decide alike."""
    b = np.asarray(boxes, np.float64)
    g = b.copy()
    g[:, 3:5] += 0.02
    ov, ovg = boxes_bev(b, b, iou=False), boxes_bev(g, g, iou=False)
    np.fill_diagonal(ov, 1.0)
    np.fill_diagonal(ovg, 1.0)
    assert not np.any((ov <= 1e-3) & ((ov > 0) | (ovg > 0))), "near-touching boxes in G11's inputs"


def configs():
    return [
        {'DB_INFO_PATH': ['kitti_dbinfos_train.pkl'], 'USE_SHARED_MEMORY': False,
         'PREPARE': {'filter_by_min_points': ['Car:3', 'Pedestrian:3', 'Cyclist:0']},
         'SAMPLE_GROUPS': ['Car:3', 'Truck:2', 'Pedestrian:4', 'Cyclist:2'], 'NUM_POINT_FEATURES': 4,
         'DATABASE_WITH_FAKELIDAR': False, 'REMOVE_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'LIMIT_WHOLE_SCENE': True},
        {'DB_INFO_PATH': ['kitti_dbinfos_train.pkl'], 'USE_SHARED_MEMORY': False,
         'PREPARE': {'filter_by_difficulty': [2], 'filter_by_min_points': ['Pedestrian:5']},
         'SAMPLE_GROUPS': ['Cyclist:2', 'Car:3', 'Pedestrian:3'], 'NUM_POINT_FEATURES': 4,
         'DATABASE_WITH_FAKELIDAR': False, 'REMOVE_EXTRA_WIDTH': [0.3, 0.2, 0.1], 'LIMIT_WHOLE_SCENE': False},
    ]


def main():
    ref = load_reference()
    rng = np.random.default_rng(2011)
    classes, boxes, counts, pts, diff = make_database(rng)
    scenes = make_scenes(rng, boxes)
    for d in scenes:
        no_near_touch(np.concatenate([boxes, d['gt_boxes']], 0))
    out = {'db_classes': np.array(classes), 'db_boxes': boxes, 'db_off': np.r_[0, np.cumsum(counts)].astype(np.int64),
           'db_points': np.concatenate(pts, 0), 'db_difficulty': diff, 'class_names': np.array(CLASSES),
           'n_scenes': np.array(len(scenes)), 'numpy_version': np.array(np.__version__)}
    for s, d in enumerate(scenes):
        for k, v in d.items():
            out['scene/%d/%s' % (s, k if k != 'gt_boxes_mask' else 'mask')] = v
    with tempfile.TemporaryDirectory() as root:
        write_database(root, classes, boxes, counts, pts, diff)
        from pathlib import Path
        for ci, cfg in enumerate(configs()):
            out['cfg/%d' % ci] = np.array(json.dumps(cfg))
            sampler = ref.DataBaseSampler(Path(root), Cfg(cfg), CLASSES)
            inv = {c: {id(i): k for k, i in enumerate(sampler.db_infos[c])} for c in CLASSES}
            drawn = []
            orig = sampler.sample_with_fixed_number

            def rec(class_name, sample_group):
                got = orig(class_name, sample_group)
                drawn.append((class_name, [inv[class_name][id(i)] for i in got]))
                return got
            sampler.sample_with_fixed_number = rec
            np.random.seed(SEEDS[ci])
            for s, d in enumerate(scenes):
                dd = {k: v.copy() for k, v in d.items()}
                if ci == 1:
                    dd['gt_boxes'] = dd['gt_boxes'].astype(np.float64)
                else:
                    dd['gt_boxes'] = dd['gt_boxes'].astype(np.float32)
                del drawn[:]
                res = sampler(dd)
                pre = 'out/%d/%d/' % (ci, s)
                out[pre + 'points'] = res['points']
                out[pre + 'gt_boxes'] = res['gt_boxes']
                out[pre + 'gt_names'] = res['gt_names']
                out[pre + 'drawn_classes'] = np.array([c for c, _ in drawn], dtype='<U16')
                out[pre + 'drawn_ids'] = np.array([i for _, ids in drawn for i in ids], np.int64)
                out[pre + 'drawn_len'] = np.array([len(ids) for _, ids in drawn], np.int64)
            st = np.random.get_state()
            out['rng/%d/keys' % ci] = st[1]
            out['rng/%d/pos' % ci] = np.array(st[2])
    path = os.path.join(HERE, 'g11_gt_sampling.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %.1f KB' % (path, os.path.getsize(path) / 1e3))
    for ci in range(2):
        print('config %d: points in / out per scene' % ci,
              [(len(scenes[s]['points']), len(out['out/%d/%d/points' % (ci, s)])) for s in range(len(scenes))])


if __name__ == '__main__':
    main()
