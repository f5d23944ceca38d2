"""NumPy restatement of OpenPCDet's ground-truth sampling augmentor -- TEST INFRASTRUCTURE ONLY (tests/ and the
cpu_baseline leg of tools/bench_gt_sampling.py import it; the product path never does).

Follows pcdet/datasets/augmentor/database_sampler.py (DataBaseSampler: __init__ :16-61, filter_by_min_points /
filter_by_difficulty :100-127, sample_with_fixed_number :129-146, add_sampled_boxes_to_scene :364-442, __call__
:444-501) and pcdet/utils/box_utils.py (enlarge_box3d: the boxes go to float32 through check_numpy_to_torch first;
remove_points_in_boxes3d), one scene at a time, one .bin file read per sampled object.  The BEV overlap is
oracle.iou3d_oracle.boxes_bev (exact float64 polygon), the point test oracle.gtdb_oracle.points_in_boxes_cpu.
Parity with the reference's orchestration and RNG order: tests/golden/g11_gt_sampling.npz."""
import os
import pickle

import numpy as np

from oracle.gtdb_oracle import points_in_boxes_cpu
from oracle.iou3d_oracle import boxes_bev


class RefSampler:
    def __init__(self, root_path, cfg, class_names):
        self.root_path = str(root_path)
        self.cfg = cfg
        self.class_names = class_names
        self.db_infos = {c: [] for c in class_names}
        for p in cfg['DB_INFO_PATH']:
            with open(os.path.join(self.root_path, p), 'rb') as f:
                infos = pickle.load(f)
            for c in class_names:
                self.db_infos[c].extend(infos[c])
        for name, val in cfg['PREPARE'].items():
            if name == 'filter_by_min_points':
                for name_num in val:
                    c, k = name_num.split(':')
                    if int(k) > 0 and c in self.db_infos:
                        self.db_infos[c] = [i for i in self.db_infos[c] if i['num_points_in_gt'] >= int(k)]
            elif name == 'filter_by_difficulty':
                self.db_infos = {c: [i for i in v if i['difficulty'] not in val] for c, v in self.db_infos.items()}
            else:
                raise ValueError(name)
        self.groups = []                                   # [class, configured number, pointer, indices]
        for x in cfg['SAMPLE_GROUPS']:
            c, n = x.split(':')
            if c in class_names:
                self.groups.append([c, int(n), len(self.db_infos[c]), np.arange(len(self.db_infos[c]))])
        self.limit_whole_scene = cfg.get('LIMIT_WHOLE_SCENE', False)
        self.C = int(cfg['NUM_POINT_FEATURES'])

    def draw(self, g, num):
        c, _, pointer, indices = g
        if pointer >= len(self.db_infos[c]):
            indices = np.random.permutation(len(self.db_infos[c]))
            pointer = 0
        ids = np.asarray(indices[pointer:pointer + num], np.int64)
        g[2], g[3] = pointer + num, indices
        return ids

    def __call__(self, d):
        """-> (output dict, [(class, candidate ids)] of the scene)."""
        gt_boxes, names = d['gt_boxes'], d['gt_names']
        existed = gt_boxes
        drawn, acc_infos = [], []
        for g in self.groups:
            c, num = g[0], g[1]
            if self.limit_whole_scene:
                num = g[1] - int(np.sum(names.astype(str) == c))
            if num <= 0:
                continue
            ids = self.draw(g, num)
            drawn.append((c, ids))
            cand = np.stack([self.db_infos[c][i]['box3d_lidar'] for i in ids]).astype(np.float32)
            hit = np.zeros(len(ids), bool)
            if existed.shape[0]:
                hit |= (boxes_bev(cand, existed, iou=False) > 0).any(1)
            pair = boxes_bev(cand, cand, iou=False) > 0
            np.fill_diagonal(pair, False)
            hit |= pair.any(1)
            ok = np.nonzero(~hit)[0]
            existed = np.concatenate([existed, cand[ok]], 0)
            acc_infos += [self.db_infos[c][ids[k]] for k in ok]
        out = dict(d)
        mask = out.pop('gt_boxes_mask')
        if not acc_infos:
            return out, drawn
        sampled = existed[gt_boxes.shape[0]:]
        objs = []
        for info in acc_infos:
            o = np.fromfile(os.path.join(self.root_path, info['path']), np.float32).reshape(-1, self.C)
            o[:, :3] += info['box3d_lidar'][:3].astype(np.float32)
            objs.append(o)
        large = sampled[:, :7].astype(np.float32)
        large[:, 3:6] += np.asarray(self.cfg['REMOVE_EXTRA_WIDTH'], np.float64).astype(np.float32)[None, :]
        pts = d['points']
        keep = points_in_boxes_cpu(pts[:, :3], large).sum(0) == 0
        out['points'] = np.concatenate([np.concatenate(objs, 0)[:, :pts.shape[1]], pts[keep]], 0)
        out['gt_names'] = np.concatenate([names[mask], np.array([i['name'] for i in acc_infos])], 0)
        out['gt_boxes'] = np.concatenate([gt_boxes[mask], sampled], 0)
        return out, drawn


def write_database(root, classes, boxes, counts, points, difficulty=None):
    """A GT database as gt_database.py writes it: root/gt_database/<k>_<class>.bin + root/kitti_dbinfos_train.pkl.
    classes: name per object, boxes (n,7) float64, counts (n,), points: list of (count_k, C) float32."""
    os.makedirs(os.path.join(str(root), 'gt_database'), exist_ok=True)
    infos = {}
    for k, c in enumerate(classes):
        c = str(c)
        rel = os.path.join('gt_database', '%06d_%s_0.bin' % (k, c))
        with open(os.path.join(str(root), rel), 'w') as f:
            np.asarray(points[k], np.float32).tofile(f)
        infos.setdefault(c, []).append({'name': c, 'path': rel, 'image_idx': '%06d' % k, 'gt_idx': 0,
                                        'box3d_lidar': np.asarray(boxes[k], np.float64),
                                        'num_points_in_gt': int(counts[k]),
                                        'difficulty': int(0 if difficulty is None else difficulty[k]),
                                        'bbox': np.zeros(4, np.float32), 'score': -1.0})
    with open(os.path.join(str(root), 'kitti_dbinfos_train.pkl'), 'wb') as f:
        pickle.dump(infos, f)
    return infos


def database_from_golden(z, root):
    """Re-create G11's database under `root` from the stored arrays."""
    off = z['db_off']
    pts = [z['db_points'][off[k]:off[k + 1]] for k in range(len(off) - 1)]
    return write_database(root, z['db_classes'], z['db_boxes'], np.diff(off), pts, z['db_difficulty'])


def golden_cfg(z, i):
    import json
    return json.loads(str(z['cfg/%d' % i]))


def golden_scene(z, s):
    return {'points': z['scene/%d/points' % s].copy(), 'gt_boxes': z['scene/%d/gt_boxes' % s].copy(),
            'gt_names': z['scene/%d/gt_names' % s].copy(), 'gt_boxes_mask': z['scene/%d/mask' % s].copy()}
