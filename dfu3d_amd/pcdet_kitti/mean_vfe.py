"""Row f-19: OpenPCDet's MeanVFE, the voxel feature encoder of the hard-voxel models -- the mean of every
voxel's stored rows.

Reference: pcdet/models/backbones_3d/vfe/mean_vfe.py.

The batched data path computes this mean inside the voxel stage (dfu3d_hard_voxels, csrc/dfu3d_hvox.h: `voxel_mean`,
prepare_batch(..., voxel_features_only=True)) without the (V, T, C) block ever being written; then the batch already
carries `voxel_features` and `forward` leaves it as it is.  With `voxels` in the batch `forward` applies the same rule
(THE MEAN of the header: +0.0, the slots added one by one in float32, one division by max(count, 1)), so both paths give
the same bits.  Divergence from the reference: its `sum(dim=1)` leaves the order of the additions
to the library; here it is the slot order.  No parameters and no backward: the inputs are data.
"""
import torch
import torch.nn as nn

from .. import hard_voxel_ops


class MeanVFE(nn.Module):
    def __init__(self, model_cfg, num_point_features, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_point_features = num_point_features

    def get_output_feature_dim(self):
        return self.num_point_features

    @torch.no_grad()
    def forward(self, batch_dict, **kwargs):
        """batch_dict: `voxels` (V, T, C) and `voxel_num_points` (V), or `voxel_features` (V, C) alone -> batch_dict with
        `voxel_features` (V, C)."""
        if 'voxels' in batch_dict:
            batch_dict['voxel_features'] = hard_voxel_ops.voxel_mean(batch_dict['voxels'], batch_dict['voxel_num_points'])
        elif 'voxel_features' not in batch_dict:
            raise hard_voxel_ops.Dfu3dError("MeanVFE: the batch has neither voxels nor voxel_features")
        return batch_dict
