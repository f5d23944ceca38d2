"""pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py on dfu3d_amd.bev_ops (csrc/bevscatter_stage.hip):
PointPillarScatter and PointPillarScatter3d with the reference's constructor arguments and batch_dict keys
('pillar_features', 'voxel_coords' -> 'spatial_features').

Divergences from the reference: the batch size is batch_dict['batch_size'] (the reference reads the maximum batch index
from the device, so a batch whose last samples are empty comes out shorter there); nothing is read from the device --
a pillar outside the canvas is dropped and two pillars on one cell keep the higher row, both recorded in `self.status`,
which `check_status()` reads and raises on at the caller's next natural synchronisation (the reference raises an index
error or writes into another sample's canvas); 'voxel_coords' of another integer type is converted to int32;
batch_dict['n_pillars'], when present, is the device count of a padded pillar list."""
import torch
import torch.nn as nn

from .. import bev_ops
from .._lib import Dfu3dError


def _get(cfg, key, *default):
    if isinstance(cfg, dict):
        return cfg[key] if not default else cfg.get(key, default[0])
    return getattr(cfg, key) if not default else getattr(cfg, key, default[0])


class _ScatterBase(nn.Module):
    def _scatter(self, batch_dict, check=False):
        coords = batch_dict['voxel_coords']
        if coords.dtype != torch.int32:
            coords = coords.to(torch.int32)
        info = bev_ops.ScatterInfo()
        batch_dict['spatial_features'] = bev_ops.pillar_scatter(
            batch_dict['pillar_features'], coords.contiguous(), batch_dict['batch_size'], (self.nx, self.ny, self.nz),
            n_pillars=batch_dict.get('n_pillars', None), check=check, info=info)
        self.status, self.cell_map = info.status, info.cell_map
        return batch_dict

    def check_status(self):
        """Raise if the last forward dropped a pillar or met two pillars on one cell (one host read)."""
        s = int(self.status.item()) if self.status is not None else 0
        if s:
            raise Dfu3dError("%s: status %d (%s)" % (type(self).__name__, s, bev_ops.status_message(s)))


class PointPillarScatter(_ScatterBase):
    def __init__(self, model_cfg, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = _get(model_cfg, 'NUM_BEV_FEATURES')
        self.nx, self.ny, self.nz = (int(v) for v in grid_size)
        assert self.nz == 1
        self.status = self.cell_map = None

    def forward(self, batch_dict, check=False, **kwargs):
        if batch_dict['pillar_features'].shape[1] != self.num_bev_features:
            raise Dfu3dError("PointPillarScatter: pillar_features of %d channels, NUM_BEV_FEATURES = %d"
                             % (batch_dict['pillar_features'].shape[1], self.num_bev_features))
        return self._scatter(batch_dict, check)


class PointPillarScatter3d(_ScatterBase):
    def __init__(self, model_cfg, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.nx, self.ny, self.nz = (int(v) for v in _get(model_cfg, 'INPUT_SHAPE'))
        self.num_bev_features = _get(model_cfg, 'NUM_BEV_FEATURES')
        self.num_bev_features_before_compression = self.num_bev_features // self.nz
        self.status = self.cell_map = None

    def forward(self, batch_dict, check=False, **kwargs):
        if batch_dict['pillar_features'].shape[1] != self.num_bev_features_before_compression:
            raise Dfu3dError("PointPillarScatter3d: pillar_features of %d channels, NUM_BEV_FEATURES // nz = %d"
                             % (batch_dict['pillar_features'].shape[1], self.num_bev_features_before_compression))
        return self._scatter(batch_dict, check)
