"""pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py without torch_scatter: PFNLayerV2, DynamicPillarVFE and
DynamicPillarVFESimple2D with the reference's constructor arguments, state-dict keys, `get_output_feature_dim()` and
`forward(batch_dict)`, on dfu3d_amd.pillar_ops (csrc/pillar_stage.hip).  Linear and BatchNorm1d stay torch's.

Divergences from the reference: the constructor creates no device tensor (the geometry is kept as Python numbers, so
the modules can be built without a GPU); points with a non-finite x or y or a batch index outside [0, batch_size) raise
Dfu3dError (the reference's result is undefined there); `voxel_coords` is int32 as in the reference, made on the device
by the grouping; every sum is taken in ascending point index, so two runs give the same bits.  `batch_dict` must hold
'batch_size' next to 'points' (pcdet's collate_batch puts it there)."""
import torch.nn as nn

from .. import pillar_ops


def _get(cfg, key, *default):
    if isinstance(cfg, dict):
        return cfg[key] if not default else cfg.get(key, default[0])
    return getattr(cfg, key) if not default else getattr(cfg, key, default[0])


class PFNLayerV2(nn.Module):
    def __init__(self, in_channels, out_channels, use_norm=True, last_layer=False):
        super().__init__()
        self.last_vfe = last_layer
        self.use_norm = use_norm
        if not self.last_vfe:
            out_channels = out_channels // 2
        if self.use_norm:
            self.linear = nn.Linear(in_channels, out_channels, bias=False)
            self.norm = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)
        else:
            self.linear = nn.Linear(in_channels, out_channels, bias=True)
        self.relu = nn.ReLU()

    def forward(self, inputs, group):
        """inputs (n_kept, in_channels), group: the PillarGroup of the points (the reference passes unq_inv here)."""
        x = self.linear(inputs)
        x = self.norm(x) if self.use_norm else x
        x = self.relu(x)
        if self.last_vfe:
            return pillar_ops.pillar_max(x, group)
        return pillar_ops.pillar_max_concat(x, group)


class _DynamicPillarBase(nn.Module):
    LAYOUT = None

    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.use_norm = _get(model_cfg, 'USE_NORM')
        self.with_distance = _get(model_cfg, 'WITH_DISTANCE')
        self.use_absolute_xyz = _get(model_cfg, 'USE_ABSLOTE_XYZ')
        self.num_raw_features = int(num_point_features)
        num_point_features = pillar_ops.feature_cols(self.num_raw_features + 1, self.LAYOUT, True, self.with_distance)
        if not self.use_absolute_xyz:
            num_point_features -= 3
        self.num_filters = list(_get(model_cfg, 'NUM_FILTERS'))
        assert len(self.num_filters) > 0
        num_filters = [num_point_features] + self.num_filters
        self.pfn_layers = nn.ModuleList(
            PFNLayerV2(num_filters[i], num_filters[i + 1], self.use_norm, last_layer=(i >= len(num_filters) - 2))
            for i in range(len(num_filters) - 1))
        self.voxel_size = [float(v) for v in voxel_size]
        self.grid_size = [int(v) for v in grid_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_x, self.voxel_y, self.voxel_z = self.voxel_size[:3]
        self.x_offset = self.voxel_x / 2 + self.point_cloud_range[0]
        self.y_offset = self.voxel_y / 2 + self.point_cloud_range[1]
        self.z_offset = self.voxel_z / 2 + self.point_cloud_range[2]
        self.scale_xy = self.grid_size[0] * self.grid_size[1]
        self.scale_y = self.grid_size[1]

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def _encode(self, batch_dict):
        group = pillar_ops.pillar_group(
            batch_dict['points'], batch_dict['batch_size'], self.point_cloud_range, self.voxel_size, self.grid_size,
            layout=self.LAYOUT, use_absolute_xyz=self.use_absolute_xyz, with_distance=self.with_distance,
            offsets=(self.x_offset, self.y_offset, self.z_offset))
        features = group.features
        for pfn in self.pfn_layers:
            features = pfn(features, group)
        return features, group


class DynamicPillarVFE(_DynamicPillarBase):
    LAYOUT = pillar_ops.LAYOUT_PILLAR

    def forward(self, batch_dict, **kwargs):
        features, group = self._encode(batch_dict)
        batch_dict['voxel_features'] = batch_dict['pillar_features'] = features
        batch_dict['voxel_coords'] = group.coords                         # int32 [b, 0, y, x]
        return batch_dict


class DynamicPillarVFESimple2D(_DynamicPillarBase):
    LAYOUT = pillar_ops.LAYOUT_SIMPLE2D

    def forward(self, batch_dict, **kwargs):
        features, group = self._encode(batch_dict)
        batch_dict['pillar_features'] = features
        batch_dict['pillar_coords'] = group.coords                        # int32 [b, y, x]
        return batch_dict
