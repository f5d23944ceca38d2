"""Row f-5: OpenPCDet's ground-truth sampling augmentor (`gt_sampling`, copy-paste of database objects
into a scene) over the database that gt_database.py writes, with its collision test and point surgery on the GPU.

Reference: pcdet/datasets/augmentor/database_sampler.py, class DataBaseSampler (`__init__` :16-61,
`filter_by_difficulty` / `filter_by_min_points` :100-127, `sample_with_fixed_number` :129-146,
`add_sampled_boxes_to_scene` :364-442, `__call__` :444-501) and pcdet/utils/box_utils.py (`enlarge_box3d`,
`remove_points_in_boxes3d`).

The candidate draw stays on the host and follows the reference call for call on NumPy's global RNG (it does not depend
on the collision results, so a batch of B scenes draws exactly what B calls of the reference draw, in the same order).
Collision, box assembly, point removal and the paste are dfu3d_gt_sample_collide + dfu3d_gt_sample_paste, one launch
chain for the whole batch; every kept object's points live in one device pool, read once at construction.

Use it in the main process after collation (`sample_batch` over the collated scenes, or `__call__` per scene), never
inside DataLoader worker processes: it owns device memory and launches kernels.

Divergences from the reference: the BEV overlap is the exact area (dfu3d_boxes_bev), not the reference's
margin-inflated one; USE_ROAD_PLANE, IMG_AUG_TYPE, FILTER_OBJ_POINTS_BY_TIMESTAMP, DATABASE_WITH_FAKELIDAR, a
NUM_POINT_FEATURES other than the scene's, a database file of the wrong size, an empty database for a sampled class,
boxes with other than 7 columns and scene points that are not float32 raise; USE_SHARED_MEMORY is accepted and
ignored (the database always lives in device memory).
"""
import os
import pickle
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from pathlib import Path
from typing import List

import numpy as np
import torch

from .. import stages as st
from .._lib import Dfu3dError

UNSUPPORTED = ('USE_ROAD_PLANE', 'IMG_AUG_TYPE', 'FILTER_OBJ_POINTS_BY_TIMESTAMP', 'DATABASE_WITH_FAKELIDAR')


@dataclass
class GtSampleBatch:
    """Device result of DataBaseSampler.sample_batch.  Scene b: points[point_off[b]:point_off[b+1]] (float32, C columns);
    boxes[box_off[b]:box_off[b] + box_cnt[b]] (float64 values, the scene's box dtype after `split`); box_src = the row
    of every output box within the scene's input rows (ground truths first, then the candidates), which names it."""
    points: torch.Tensor
    point_off: torch.Tensor
    boxes: torch.Tensor
    box_off: torch.Tensor
    box_cnt: torch.Tensor
    box_src: torch.Tensor
    accept: torch.Tensor
    status: torch.Tensor
    scenes: list = field(default_factory=list)      # host side of every scene (names, dtypes, the input dict)

    def split(self):
        """-> the scenes' data dicts, updated in place as the reference's __call__ does (points, gt_boxes, gt_names;
        gt_boxes_mask popped)."""
        s = int(self.status.item())
        if s:
            raise Dfu3dError("gt_sample: status %d (%s)" % (s, st.status_message(s) if s != st.ST_BOX_RANGE
                                                             else "a scene beyond the box or point cap"))
        pts = self.points.cpu().numpy()
        poff = self.point_off.cpu().numpy()
        boxes = self.boxes.cpu().numpy()
        src = self.box_src.cpu().numpy()
        cnt = self.box_cnt.cpu().numpy()
        boff = self.box_off.cpu().numpy()
        out = []
        for b, sc in enumerate(self.scenes):
            d = sc['dict']
            r0, k = int(boff[b]), int(cnt[b])
            rows = src[r0:r0 + k]
            ng = sc['n_gt']
            cand = rows[rows >= ng] - ng
            if len(cand):                     # else gt_boxes / gt_names stay as they came (mask not applied)
                d['gt_names'] = np.concatenate([d['gt_names'][rows[rows < ng]],
                                                np.array([sc['cand_names'][c] for c in cand])], axis=0)
                d['gt_boxes'] = boxes[r0:r0 + k].astype(sc['dtype'])
            d['points'] = pts[int(poff[b]):int(poff[b + 1])].copy()
            d.pop('gt_boxes_mask')
            out.append(d)
        return out


class DataBaseSampler(object):
    """Drop-in for pcdet.datasets.augmentor.database_sampler.DataBaseSampler (gt_sampling).  `__call__(data_dict)`: one
    scene, NumPy in and out, the reference's keys; `sample_batch(data_dicts)`: many scenes in one launch chain."""

    def __init__(self, root_path, sampler_cfg, class_names, logger=None, device="cuda:0", workers=8):
        for k in UNSUPPORTED:
            if sampler_cfg.get(k, None):
                raise Dfu3dError("gt_sampling: %s is not supported" % k)
        self.root_path = Path(root_path)
        self.class_names = class_names
        self.sampler_cfg = sampler_cfg
        self.logger = logger
        self.device = torch.device(device)
        self.use_shared_memory = sampler_cfg.get('USE_SHARED_MEMORY', False)     # accepted, ignored: always on device
        self.num_point_features = int(sampler_cfg['NUM_POINT_FEATURES'])
        self.remove_extra_width = sampler_cfg['REMOVE_EXTRA_WIDTH']
        self.db_infos = {c: [] for c in class_names}
        for db_info_path in sampler_cfg['DB_INFO_PATH']:
            with open(str(self.root_path.resolve() / db_info_path), 'rb') as f:
                infos = pickle.load(f)
                [self.db_infos[cur_class].extend(infos[cur_class]) for cur_class in class_names]
        for func_name, val in sampler_cfg['PREPARE'].items():
            if func_name not in ('filter_by_difficulty', 'filter_by_min_points'):
                raise Dfu3dError("gt_sampling: PREPARE step %r is not supported" % func_name)
            self.db_infos = getattr(self, func_name)(self.db_infos, val)

        self.sample_groups = {}
        self.sample_class_num = {}
        self.limit_whole_scene = sampler_cfg.get('LIMIT_WHOLE_SCENE', False)
        for x in sampler_cfg['SAMPLE_GROUPS']:
            class_name, sample_num = x.split(':')
            if class_name not in class_names:
                continue
            self.sample_class_num[class_name] = sample_num
            self.sample_groups[class_name] = {
                'sample_num': sample_num,
                'pointer': len(self.db_infos[class_name]),
                'indices': np.arange(len(self.db_infos[class_name]))
            }
        self._load_pool(workers)

    # ---- PREPARE (database_sampler.py:100-127) ----
    def filter_by_difficulty(self, db_infos, removed_difficulty):
        new_db_infos = {}
        for key, dinfos in db_infos.items():
            pre_len = len(dinfos)
            new_db_infos[key] = [info for info in dinfos if info['difficulty'] not in removed_difficulty]
            if self.logger is not None:
                self.logger.info('Database filter by difficulty %s: %d => %d' % (key, pre_len, len(new_db_infos[key])))
        return new_db_infos

    def filter_by_min_points(self, db_infos, min_gt_points_list):
        for name_num in min_gt_points_list:
            name, min_num = name_num.split(':')
            min_num = int(min_num)
            if min_num > 0 and name in db_infos.keys():
                filtered_infos = [info for info in db_infos[name] if info['num_points_in_gt'] >= min_num]
                if self.logger is not None:
                    self.logger.info('Database filter by min points %s: %d => %d' %
                                     (name, len(db_infos[name]), len(filtered_infos)))
                db_infos[name] = filtered_infos
        return db_infos

    # ---- the resident database ----
    def _load_pool(self, workers):
        C = self.num_point_features
        jobs = [(c, info) for c in self.class_names for info in self.db_infos[c]]

        def read(job):
            c, info = job
            path = str(self.root_path / info['path'])
            n = int(info['num_points_in_gt'])
            if os.path.getsize(path) != n * C * 4:
                raise Dfu3dError("gt_sampling: %s holds %d bytes, expected num_points_in_gt x NUM_POINT_FEATURES x 4 "
                                 "= %d" % (path, os.path.getsize(path), n * C * 4))
            return np.fromfile(path, dtype=np.float32).reshape(n, C)

        with ThreadPoolExecutor(workers) as ex:
            arrays = list(ex.map(read, jobs))
        sizes = np.array([a.shape[0] for a in arrays], np.int64)
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self._src, self._cnt, self._box, self._name = {}, {}, {}, {}
        k = 0
        for c in self.class_names:
            m = len(self.db_infos[c])
            self._src[c] = starts[k:k + m].copy()
            self._cnt[c] = sizes[k:k + m].astype(np.int32)
            bx = [np.asarray(info['box3d_lidar']) for info in self.db_infos[c]]
            if any(b.shape != (7,) for b in bx):
                raise Dfu3dError("gt_sampling: database boxes of class %s must have 7 values" % c)
            self._box[c] = np.stack(bx, 0).astype(np.float32) if m else np.zeros((0, 7), np.float32)
            self._name[c] = [info['name'] for info in self.db_infos[c]]
            k += m
        host = np.concatenate(arrays, 0) if arrays else np.zeros((0, C), np.float32)
        self.pool = torch.from_numpy(np.ascontiguousarray(host)).to(self.device)

    # ---- the host part: candidates in the reference's RNG order (database_sampler.py:129-146, 458-468) ----
    def sample_with_fixed_number(self, class_name, sample_group):
        """The indices into db_infos[class_name] that the reference's sample_with_fixed_number returns (same RNG calls)."""
        sample_num, pointer, indices = int(sample_group['sample_num']), sample_group['pointer'], sample_group['indices']
        if pointer >= len(self.db_infos[class_name]):
            indices = np.random.permutation(len(self.db_infos[class_name]))
            pointer = 0
        ids = np.asarray(indices[pointer: pointer + sample_num], np.int64)
        pointer += sample_num
        sample_group['pointer'] = pointer
        sample_group['indices'] = indices
        return ids

    def select(self, gt_names):
        """One scene's candidates: [(group rank, class name, indices into db_infos[class])] in SAMPLE_GROUPS order."""
        gt_names = np.asarray(gt_names).astype(str)
        out = []
        for g, (class_name, sample_group) in enumerate(self.sample_groups.items()):
            if self.limit_whole_scene:
                num_gt = np.sum(class_name == gt_names)
                sample_group['sample_num'] = str(int(self.sample_class_num[class_name]) - num_gt)
            if int(sample_group['sample_num']) > 0:
                ids = self.sample_with_fixed_number(class_name, sample_group)
                if len(ids) == 0:
                    raise Dfu3dError("gt_sampling: the database holds no %s objects to sample" % class_name)
                out.append((g, class_name, ids))
        return out

    def _prepare(self, d):
        gt_boxes = d['gt_boxes']
        if gt_boxes.ndim != 2 or gt_boxes.shape[1] != 7:
            raise Dfu3dError("gt_sampling: gt_boxes must be (N, 7), got %s" % (gt_boxes.shape,))
        if gt_boxes.dtype not in (np.float32, np.float64):
            raise Dfu3dError("gt_sampling: gt_boxes must be float32 or float64")
        pts = d['points']
        if isinstance(pts, torch.Tensor):                 # a scene already on the device (upload_batch concatenates there)
            if not pts.is_cuda or pts.dtype != torch.float32 or pts.dim() != 2:
                raise Dfu3dError("gt_sampling: points given as a tensor must be (n, C) float32 on the GPU")
        elif pts.dtype != np.float32 or pts.ndim != 2:
            raise Dfu3dError("gt_sampling: points must be (n, C) float32")
        if pts.shape[1] != self.num_point_features:
            raise Dfu3dError("gt_sampling: NUM_POINT_FEATURES %d != the scene's %d point columns"
                             % (self.num_point_features, pts.shape[1]))
        mask = np.asarray(d['gt_boxes_mask'])
        if mask.dtype != np.bool_ or mask.shape != (gt_boxes.shape[0],):
            raise Dfu3dError("gt_sampling: gt_boxes_mask must be a bool array of one entry per box")
        sel = self.select(d['gt_names'])
        # existed keeps gt_boxes' dtype (np.concatenate of float32 candidates onto it); enlarge_box3d casts the sampled
        # boxes to float32 first (common_utils.check_numpy_to_torch) and adds the float32 widths there
        dt = np.result_type(gt_boxes.dtype, np.float32)
        cand = [self._box[c][ids] for _, c, ids in sel]
        cand = np.concatenate(cand, 0) if cand else np.zeros((0, 7), np.float32)
        large = cand.copy()
        large[:, 3:6] += np.asarray(self.remove_extra_width, np.float64).astype(np.float32)[None, :]
        return {
            'dict': d, 'dtype': dt, 'n_gt': gt_boxes.shape[0], 'points': pts,
            'boxes': np.concatenate([gt_boxes.astype(np.float64), cand.astype(np.float64)], 0),
            'grp': np.concatenate([np.full(gt_boxes.shape[0], -1, np.int32)] +
                                  [np.full(len(ids), g, np.int32) for g, _, ids in sel]),
            'gt_mask': np.concatenate([(mask != 0).astype(np.int32), np.zeros(len(cand), np.int32)]),
            'large': np.concatenate([np.zeros((gt_boxes.shape[0], 7)), large.astype(np.float64)], 0),
            'obj_src': np.concatenate([np.zeros(gt_boxes.shape[0], np.int64)] + [self._src[c][ids] for _, c, ids in sel]),
            'obj_cnt': np.concatenate([np.zeros(gt_boxes.shape[0], np.int32)] + [self._cnt[c][ids] for _, c, ids in sel]),
            'cand_names': [self._name[c][i] for _, c, ids in sel for i in ids],
            'ids': sel,
        }

    # ---- the device part ----
    def sample_batch(self, data_dicts: List[dict]) -> GtSampleBatch:
        """B scenes (NumPy dicts with points, gt_boxes, gt_names, gt_boxes_mask) -> device tensors (GtSampleBatch);
        .split() turns them back into the scenes' dicts.  Candidates are drawn scene after scene, as B reference calls."""
        return self.launch_batch(self.upload_batch(data_dicts))

    def upload_batch(self, data_dicts: List[dict]) -> dict:
        """The host part of sample_batch: candidates drawn, the batch packed and copied to the device."""
        sc = [self._prepare(d) for d in data_dicts]
        B = len(sc)
        C = self.num_point_features
        npts = np.array([s['points'].shape[0] for s in sc], np.int64)
        nbox = np.array([s['boxes'].shape[0] for s in sc], np.int64)
        max_boxes = int(nbox.max()) if B else 0
        if max_boxes > st.GT_SAMPLE_MAX_BOXES:
            raise Dfu3dError("gt_sampling: a scene has %d boxes and candidates, at most %d"
                             % (max_boxes, st.GT_SAMPLE_MAX_BOXES))

        def cat(k, shape, dt):
            return np.concatenate([s[k] for s in sc], 0) if B else np.zeros(shape, dt)

        def h2d(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        # never an empty point tensor (a null pointer): one spare row when the batch has no points
        spare = np.zeros((0 if npts.sum() else 1, C), np.float32)
        if any(isinstance(s['points'], torch.Tensor) for s in sc):
            pts_d = torch.cat([s['points'].to(self.device) if isinstance(s['points'], torch.Tensor) else h2d(s['points'])
                               for s in sc] + [h2d(spare)], 0)
        else:
            pts_d = h2d(np.concatenate([s['points'] for s in sc] + [spare], 0))
        obj_cnt = cat('obj_cnt', (0,), np.int32)
        return {
            'scenes': sc, 'max_boxes': max_boxes, 'max_points': int(npts.max()) if B else 0,
            'cap': int(npts.sum()) + int(obj_cnt.astype(np.int64).sum()),      # no scene can outgrow its bound
            'points': pts_d, 'pt_off': h2d(np.concatenate([[0], np.cumsum(npts)]).astype(np.int64)),
            'box_off': h2d(np.concatenate([[0], np.cumsum(nbox)]).astype(np.int32)),
            'gt_cnt': h2d(np.array([s['n_gt'] for s in sc], np.int32)),
            'boxes': h2d(cat('boxes', (0, 7), np.float64)), 'grp': h2d(cat('grp', (0,), np.int32)),
            'gt_mask': h2d(cat('gt_mask', (0,), np.int32)), 'large': h2d(cat('large', (0, 7), np.float64)),
            'obj_src': h2d(cat('obj_src', (0,), np.int64)), 'obj_cnt': h2d(obj_cnt),
        }

    def launch_batch(self, u: dict) -> GtSampleBatch:
        """The device part of sample_batch: collision, then the paste, on the current stream; no host sync."""
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        accept, out_boxes, out_src, out_cnt = st.gt_sample_collide(u['boxes'], u['box_off'], u['gt_cnt'], u['grp'],
                                                                   u['gt_mask'], u['max_boxes'], status)
        out, out_off = st.gt_sample_paste(u['points'], u['pt_off'], u['max_points'], u['box_off'], u['gt_cnt'],
                                          u['boxes'], u['large'], accept, self.pool, u['obj_src'], u['obj_cnt'],
                                          u['cap'], status)
        return GtSampleBatch(out, out_off, out_boxes, u['box_off'], out_cnt, out_src, accept, status, u['scenes'])

    def __call__(self, data_dict):
        """One scene: database_sampler.py:444-501 (NumPy in, NumPy out; data_dict is updated and returned)."""
        return self.sample_batch([data_dict]).split()[0]
