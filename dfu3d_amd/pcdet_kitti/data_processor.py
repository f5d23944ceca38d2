"""Rows f-10, f-18 and f-19: OpenPCDet's DataProcessor for the dynamic-pillar CenterPoint configuration --
`mask_points_and_boxes_outside_range`, `shuffle_points`, `transform_points_to_voxels_placeholder` -- with the range
masks on the GPU (dfu3d_world_aug_collate, include/dfu3d_aug.h), PointRCNN's `sample_points` (NUM_POINTS per scene)
on the GPU (dfu3d_sample_points, csrc/dfu3d_smp.h), and the voxel models' `transform_points_to_voxels` (hard voxels)
on the GPU (dfu3d_hard_voxels, csrc/dfu3d_hvox.h).

Reference: pcdet/datasets/processor/data_processor.py (`__init__` :64-77, :79-115, :133-180, sample_points :182-214),
common_utils.mask_points_by_range, box_utils.mask_boxes_outside_range_numpy.

`forward(data_dict)` is the per-scene form, NumPy in and out; the batched form is data_augmentor.prepare_batch, which
asks this object for the range and for what to mask.  Divergences: every other entry raises
NotImplementedError at construction; USE_CENTER_TO_FILTER false raises; the batched form does not shuffle.
transform_points_to_voxels: the voxel generator is the rule of csrc/dfu3d_hvox.h in float32; it needs
MAX_POINTS_PER_VOXEL and MAX_NUMBER_OF_VOXELS (NotImplementedError without them, and for DOUBLE_FLIP).  sample_points
(DESIGN.md row f-18): the random words come from torch's generator of the device and not from NumPy's; equal words are
ordered by the row index; the rows a short scene repeats are drawn by a multiply-shift; a scene without points raises
Dfu3dError here and sets a status bit in the batched form; the entry needs NUM_POINTS and a range mask before it.
"""
from functools import partial

import numpy as np
import torch

from .. import hard_voxel_ops as hvox
from .. import point_sample_ops as smp
from .. import stages as st
from .._lib import Dfu3dError

SUPPORTED = ('mask_points_and_boxes_outside_range', 'shuffle_points', 'transform_points_to_voxels_placeholder',
             'sample_points', 'transform_points_to_voxels')


class DataProcessor(object):
    def __init__(self, processor_configs, point_cloud_range, training, num_point_features, device="cuda:0"):
        self.point_cloud_range = np.asarray(point_cloud_range)
        if self.point_cloud_range.shape != (6,):
            raise Dfu3dError("DataProcessor: point_cloud_range must have 6 values")
        self.training = training
        self.num_point_features = num_point_features
        self.mode = 'train' if training else 'test'
        self.grid_size = self.voxel_size = None
        self.device = torch.device(device)
        self.data_processor_queue = []
        self._mask_cfg = None
        self._sample_cfg = None
        self._voxel_cfg = None
        self._range = None
        for cur_cfg in processor_configs:
            name = cur_cfg['NAME']
            if name not in SUPPORTED:
                raise NotImplementedError("DataProcessor: the entry %r is not supported" % (name,))
            self.data_processor_queue.append(getattr(self, name)(config=cur_cfg))

    # ---- what the batched form asks ----
    def mask_mode(self):
        """The `mode` bits of dfu3d_world_aug_collate this processor's configuration stands for."""
        if self._mask_cfg is None:
            return 0
        boxes = self._mask_cfg.get('REMOVE_OUTSIDE_BOXES', False) and self.training
        return st.AUG_MASK_POINTS | (st.AUG_MASK_BOXES if boxes else 0)

    def sample_count(self):
        """The rows per scene `sample_points` makes in this mode; None without the entry or where it says -1."""
        if self._sample_cfg is None:
            return None
        k = int(self._sample_cfg['NUM_POINTS'][self.mode])
        return None if k == -1 else k

    def voxel_config(self):
        """What `transform_points_to_voxels` makes in this mode: {'voxel_size', 'grid_size', 'max_points', 'max_voxels'};
        None without the entry."""
        if self._voxel_cfg is None:
            return None
        return {'voxel_size': list(self.voxel_size), 'grid_size': [int(g) for g in self.grid_size],
                'max_points': int(self._voxel_cfg['MAX_POINTS_PER_VOXEL']),
                'max_voxels': int(self._voxel_cfg['MAX_NUMBER_OF_VOXELS'][self.mode])}

    def range_tensor(self):
        if self._range is None:
            self._range = torch.from_numpy(self.point_cloud_range.astype(np.float32)).to(self.device)
        return self._range

    # ---- the entries ----
    def mask_points_and_boxes_outside_range(self, data_dict=None, config=None):
        if data_dict is None:
            if not config.get('USE_CENTER_TO_FILTER', True):
                raise NotImplementedError("mask_points_and_boxes_outside_range: USE_CENTER_TO_FILTER false (the corner "
                                          "test) is not supported")
            self._mask_cfg = config
            return partial(self.mask_points_and_boxes_outside_range, config=config)
        points, boxes = data_dict.get('points', None), data_dict.get('gt_boxes', None)
        mask_boxes = boxes is not None and config['REMOVE_OUTSIDE_BOXES'] and self.training
        if points is None and not mask_boxes:
            return data_dict
        dev = self.device
        if points is None:
            points = np.zeros((0, 3), np.float32)
        if points.ndim != 2 or points.dtype != np.float32 or points.shape[1] < 3:
            raise Dfu3dError("mask_points_and_boxes_outside_range: points must be (n, C >= 3) float32")
        if mask_boxes:
            if boxes.ndim != 2 or boxes.shape[1] < 7 or boxes.dtype not in (np.float32, np.float64):
                raise Dfu3dError("mask_points_and_boxes_outside_range: gt_boxes must be (N, >= 7) float32 or float64")
            b7 = np.ascontiguousarray(boxes[:, 0:7])
        else:
            b7 = np.zeros((0, 7), np.float32)
        n, m = points.shape[0], b7.shape[0]

        def h2d(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        out, n_kept, _, _, _, _, keep = st.world_aug_collate(
            h2d(points), h2d(np.array([0, n], np.int64)), h2d(b7), h2d(np.array([0, m], np.int32)),
            h2d(np.array([m], np.int32)), torch.ones(m, dtype=torch.int32, device=dev),
            h2d(st.aug_params([{'flags': 0}])), self.range_tensor(),
            st.AUG_MASK_POINTS | (st.AUG_MASK_BOXES if mask_boxes else 0), m, status, want_keep=True)
        if data_dict.get('points', None) is not None:
            data_dict['points'] = out[:int(n_kept.item()), 1:].cpu().numpy()
        if mask_boxes:
            data_dict['gt_boxes'] = boxes[keep.cpu().numpy() != 0]
        return data_dict

    def shuffle_points(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.shuffle_points, config=config)
        if config['SHUFFLE_ENABLED'][self.mode]:
            points = data_dict['points']
            shuffle_idx = np.random.permutation(points.shape[0])
            data_dict['points'] = points[shuffle_idx]
        return data_dict

    def sample_points(self, data_dict=None, config=None):
        if data_dict is None:
            if 'NUM_POINTS' not in config:
                raise NotImplementedError("sample_points: NUM_POINTS is required")
            if self._mask_cfg is None:
                raise NotImplementedError("sample_points: the entry must come after mask_points_and_boxes_outside_range "
                                          "(the batched form samples what the range mask keeps)")
            k = int(config['NUM_POINTS'][self.mode])
            if k != -1 and not 1 <= k <= smp.MAX_OUT:
                raise Dfu3dError("sample_points: NUM_POINTS %d (-1, or 1 .. %d)" % (k, smp.MAX_OUT))
            self._sample_cfg = config
            return partial(self.sample_points, config=config)
        k = self.sample_count()
        if k is None:
            return data_dict
        points = data_dict['points']
        if points.ndim != 2 or points.dtype != np.float32 or points.shape[1] < 3:
            raise Dfu3dError("sample_points: points must be (n, C >= 3) float32")
        n = points.shape[0]
        if n == 0:
            raise Dfu3dError("sample_points: a scene without points")
        block = torch.from_numpy(np.concatenate([np.zeros((n, 1), np.float32), points], 1)).to(self.device)
        out, _ = smp.sample_points(block, torch.full((1,), n, dtype=torch.int32, device=self.device), k)
        data_dict['points'] = out[:, 1:].cpu().numpy()
        return data_dict

    def transform_points_to_voxels_placeholder(self, data_dict=None, config=None):
        if data_dict is None:
            grid_size = (self.point_cloud_range[3:6] - self.point_cloud_range[0:3]) / np.array(config['VOXEL_SIZE'])
            self.grid_size = np.round(grid_size).astype(np.int64)
            self.voxel_size = config['VOXEL_SIZE']
            return partial(self.transform_points_to_voxels_placeholder, config=config)
        return data_dict

    def transform_points_to_voxels(self, data_dict=None, config=None):
        if data_dict is None:
            if 'MAX_POINTS_PER_VOXEL' not in config or 'MAX_NUMBER_OF_VOXELS' not in config:
                raise NotImplementedError("transform_points_to_voxels: MAX_POINTS_PER_VOXEL and MAX_NUMBER_OF_VOXELS are "
                                          "required")
            if config.get('DOUBLE_FLIP', False):
                raise NotImplementedError("transform_points_to_voxels: DOUBLE_FLIP is not supported")
            grid_size = (self.point_cloud_range[3:6] - self.point_cloud_range[0:3]) / np.array(config['VOXEL_SIZE'])
            self.grid_size = np.round(grid_size).astype(np.int64)
            self.voxel_size = config['VOXEL_SIZE']
            t, v = int(config['MAX_POINTS_PER_VOXEL']), int(config['MAX_NUMBER_OF_VOXELS'][self.mode])
            if not 1 <= t <= hvox.MAX_POINTS or v < 1:
                raise Dfu3dError("transform_points_to_voxels: MAX_POINTS_PER_VOXEL %d (1 .. %d), MAX_NUMBER_OF_VOXELS %d "
                                 "(1 or more)" % (t, hvox.MAX_POINTS, v))
            self._voxel_cfg = config
            return partial(self.transform_points_to_voxels, config=config)
        points = data_dict['points']
        if points.ndim != 2 or points.dtype != np.float32 or points.shape[1] < 3:
            raise Dfu3dError("transform_points_to_voxels: points must be (n, C >= 3) float32")
        n, vc = points.shape[0], self.voxel_config()
        block = torch.from_numpy(np.concatenate([np.zeros((n, 1), np.float32), points], 1)).to(self.device)
        out = hvox.hard_voxels(block, torch.full((1,), n, dtype=torch.int32, device=self.device), self.point_cloud_range,
                               vc['voxel_size'], vc['grid_size'], vc['max_points'], vc['max_voxels'])
        host = torch.cat([out.n_voxels, out.status]).cpu().numpy()
        if host[1]:
            raise Dfu3dError("transform_points_to_voxels: status %d (%s)" % (host[1], hvox.status_message(int(host[1]))))
        nv = int(host[0])
        voxels = out.voxels[:nv].cpu().numpy()
        if not data_dict.get('use_lead_xyz', True):
            voxels = voxels[..., 3:]                                # remove xyz in voxels(N, 3)
        data_dict['voxels'] = voxels
        data_dict['voxel_coords'] = out.voxel_coords[:nv, 1:].cpu().numpy()
        data_dict['voxel_num_points'] = out.voxel_num_points[:nv].cpu().numpy()
        return data_dict

    def forward(self, data_dict):
        for cur_processor in self.data_processor_queue:
            data_dict = cur_processor(data_dict=data_dict)
        return data_dict
