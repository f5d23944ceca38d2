"""pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py: `VoxelSetAbstraction`, PV-RCNN's point feature encoder,
with the reference's state-dict keys (SA_layers.*, SA_rawpoints.*, vsa_point_feature_fusion.*).  Inference and training
forward alike; what differs from the reference is where the work runs (csrc/pointstack_stage.hip):

  keypoints        ONE stacked FPS launch for the batch, writing the (B * K, 4) [b, x, y, z] rows directly; a sample
                   shorter than NUM_KEYPOINTS repeats its picks, as the reference does;
  counts           batch_dict['point_cnt'] where the collate left it, else one counts call per source (three launches)
                   instead of B masked sums; the keypoints' counts are the constant K;
  bev              one bilinear launch on spatial_features in place;
  every source     one ball launch for both radii and one grouping launch per radius; coordinates that are columns of
                   `points` or of the keypoints are read in place.

The forward reads nothing from the device.  The status bits of all calls are collected in `self.status` (int32 (1) on
the device, fresh every forward); with `check = True` the forward reads it once at its end and raises on any bit.
POINT_SOURCE raw_points / voxel_centers, SAMPLE_METHOD FPS; SPC sampling and FILTER_NEIGHBOR_WITH_ROI (PV-RCNN++) raise
NotImplementedError naming the setting."""
import torch
import torch.nn as nn

from .. import point_stack_ops as ops
from .._lib import Dfu3dError
from . import pointnet2_stack_modules
from .common_utils import cfg_get, get_voxel_centers


class VoxelSetAbstraction(nn.Module):
    def __init__(self, model_cfg, voxel_size, point_cloud_range, num_bev_features=None, num_rawpoint_features=None,
                 **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.check = False
        self.status = None
        if cfg_get(model_cfg, 'SAMPLE_METHOD') != 'FPS':
            raise NotImplementedError("VoxelSetAbstraction: SAMPLE_METHOD = %r (only FPS is part of this package)"
                                      % (cfg_get(model_cfg, 'SAMPLE_METHOD'),))
        if cfg_get(model_cfg, 'POINT_SOURCE') not in ('raw_points', 'voxel_centers'):
            raise NotImplementedError("VoxelSetAbstraction: POINT_SOURCE = %r" % (cfg_get(model_cfg, 'POINT_SOURCE'),))
        sa_cfg = cfg_get(model_cfg, 'SA_LAYER')
        self.features_source = list(cfg_get(model_cfg, 'FEATURES_SOURCE'))
        self.num_keypoints = int(cfg_get(model_cfg, 'NUM_KEYPOINTS'))
        for src in self.features_source:
            if src != 'bev' and cfg_get(cfg_get(sa_cfg, src), 'FILTER_NEIGHBOR_WITH_ROI', False):
                raise NotImplementedError("VoxelSetAbstraction: SA_LAYER.%s.FILTER_NEIGHBOR_WITH_ROI is not part of this "
                                          "package" % src)
        self.SA_layers = nn.ModuleList()
        self.SA_layer_names = []
        self.downsample_times_map = {}
        c_in = 0
        for src in self.features_source:
            if src in ('bev', 'raw_points'):
                continue
            cfg = cfg_get(sa_cfg, src)
            self.downsample_times_map[src] = cfg_get(cfg, 'DOWNSAMPLE_FACTOR')
            input_channels = cfg_get(cfg, 'INPUT_CHANNELS', None)
            if input_channels is None:
                first = cfg_get(cfg, 'MLPS')[0]
                input_channels = first[0] if isinstance(first, (list, tuple)) else first
            layer, c_out = pointnet2_stack_modules.build_local_aggregation_module(input_channels=input_channels, config=cfg)
            self.SA_layers.append(layer)
            self.SA_layer_names.append(src)
            c_in += c_out
        if 'bev' in self.features_source:
            c_in += num_bev_features
        if 'raw_points' in self.features_source:
            self.SA_rawpoints, c_out = pointnet2_stack_modules.build_local_aggregation_module(
                input_channels=num_rawpoint_features - 3, config=cfg_get(sa_cfg, 'raw_points'))
            c_in += c_out
        out = cfg_get(model_cfg, 'NUM_OUTPUT_FEATURES')
        self.vsa_point_feature_fusion = nn.Sequential(nn.Linear(c_in, out, bias=False), nn.BatchNorm1d(out), nn.ReLU())
        self.num_point_features = out
        self.num_point_features_before_fusion = c_in
        self._keypoint_cnt = {}                           # device constants: the keypoints' counts, the geometry

    def interpolate_from_bev_features(self, keypoints, bev_features, batch_size, bev_stride):
        """keypoints (M, 4), bev_features (B, C, H, W) -> (M, C)."""
        return ops.bev_sample(keypoints, bev_features, self.point_cloud_range, self.voxel_size, bev_stride)

    @staticmethod
    def _counts_of(batch_column, batch_size):
        if batch_column.dtype not in (torch.float32, torch.int32):
            batch_column = batch_column.int()
        return ops.counts(batch_column, batch_size)[0]

    def _source_points(self, batch_dict):
        """-> xyz (N, 3) (a view where it can be), cnt int32 (B) of the set the keypoints are sampled from."""
        batch_size = batch_dict['batch_size']
        if cfg_get(self.model_cfg, 'POINT_SOURCE') == 'raw_points':
            points = batch_dict['points']
            cnt = batch_dict.get('point_cnt')
            return points[:, 1:4], cnt if cnt is not None else self._counts_of(points[:, 0], batch_size)
        coords = batch_dict['voxel_coords']
        return self._voxel_centers(coords[:, 1:4], 1), self._counts_of(coords[:, 0], batch_size)

    def get_sampled_points(self, batch_dict):
        """-> keypoints (B * NUM_KEYPOINTS, 4) [bs_idx, x, y, z]."""
        xyz, cnt = self._source_points(batch_dict)
        return ops.fps(xyz, ops.starts_of(cnt), self.num_keypoints)[1]

    def _voxel_centers(self, coords, downsample_times):
        """get_voxel_centers with the voxel size and the range kept on the device (copied once per device)."""
        key = ('geometry', coords.device)
        if key not in self._keypoint_cnt:
            self._keypoint_cnt[key] = (torch.tensor(self.voxel_size, device=coords.device),
                                       torch.tensor(self.point_cloud_range, device=coords.device))
        size, pc_range = self._keypoint_cnt[key]
        return get_voxel_centers(coords, downsample_times=downsample_times, voxel_size=size, point_cloud_range=pc_range)

    def _keypoint_counts(self, batch_size, device):
        key = (batch_size, device)
        if key not in self._keypoint_cnt:
            self._keypoint_cnt[key] = torch.full((batch_size,), self.num_keypoints, dtype=torch.int32, device=device)
        return self._keypoint_cnt[key]

    def forward(self, batch_dict):
        """batch_dict: batch_size, points (N, 1 + 3 + C) (optionally point_cnt int32 (B)), multi_scale_3d_features,
        spatial_features and spatial_features_stride as FEATURES_SOURCE asks -> point_features_before_fusion,
        point_features (B * K, NUM_OUTPUT_FEATURES), point_coords (B * K, 4)."""
        batch_size = batch_dict['batch_size']
        device = batch_dict['points'].device if 'points' in batch_dict else batch_dict['voxel_coords'].device
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        with ops.status_scope(self.status):
            src_xyz, src_cnt = self._source_points(batch_dict)
            keypoints = ops.fps(src_xyz, ops.starts_of(src_cnt), self.num_keypoints)[1]
            new_xyz, new_cnt = keypoints[:, 1:4], self._keypoint_counts(batch_size, device)
            parts = []
            if 'bev' in self.features_source:
                parts.append(self.interpolate_from_bev_features(keypoints, batch_dict['spatial_features'], batch_size,
                                                                bev_stride=batch_dict['spatial_features_stride']))
            if 'raw_points' in self.features_source:
                points = batch_dict['points']
                if cfg_get(self.model_cfg, 'POINT_SOURCE') == 'raw_points':
                    cnt = src_cnt
                else:
                    cnt = batch_dict.get('point_cnt')
                    cnt = cnt if cnt is not None else self._counts_of(points[:, 0], batch_size)
                feats = points[:, 4:].contiguous() if points.shape[1] > 4 else None
                parts.append(self.SA_rawpoints(xyz=points[:, 1:4], xyz_batch_cnt=cnt, new_xyz=new_xyz,
                                               new_xyz_batch_cnt=new_cnt, features=feats)[1])
            for layer, src in zip(self.SA_layers, self.SA_layer_names):
                level = batch_dict['multi_scale_3d_features'][src]
                coords = level.indices
                xyz = self._voxel_centers(coords[:, 1:4], self.downsample_times_map[src])
                parts.append(layer(xyz=xyz.contiguous(), xyz_batch_cnt=self._counts_of(coords[:, 0], batch_size),
                                   new_xyz=new_xyz, new_xyz_batch_cnt=new_cnt, features=level.features.contiguous())[1])
        point_features = torch.cat(parts, dim=-1)
        batch_dict['point_features_before_fusion'] = point_features.view(-1, point_features.shape[-1])
        batch_dict['point_features'] = self.vsa_point_feature_fusion(batch_dict['point_features_before_fusion'])
        batch_dict['point_coords'] = keypoints
        if self.check:
            bits = int(self.status.item())
            if bits:
                raise Dfu3dError("VoxelSetAbstraction: " + ops.status_message(bits))
        return batch_dict
