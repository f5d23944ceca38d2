"""pcdet/models/roi_heads/pvrcnn_head.py with what it needs of roi_head_template.py: PV-RCNN's second stage, inference
half, with the reference's state-dict keys (roi_grid_pool_layer.*, shared_fc_layer.*, cls_layers.*, reg_layers.*).

  proposal_layer   PointRCNNHead's own (per-sample torch on the existing NMS: the dense head's 211 200 anchors are
                   beyond the batched proposal stage, as for SECOND); make_fc_layers, init_weights and
                   generate_predicted_boxes are PointRCNNHead's too -- shared, not copied;
  roi_grid_pool    B * R * GRID_SIZE^3 grid points as the centres of ONE StackSAModuleMSG call on the keypoints
                   (csrc/pointstack_stage.hip): the keypoint coordinates are read in place from point_coords, their
                   counts come from one counts call, the grid points' counts are a constant;
  get_dense_grid_points  the index grid by arange instead of `nonzero()` of a tensor of ones: the same rows in the same
                   order without a read from the device.

Forward in training mode raises NotImplementedError (target assignment and the losses of PV-RCNN are not part of this
package)."""
import torch
import torch.nn as nn

from .. import point_stack_ops as ops
from . import box_coder_utils, pointnet2_stack_modules
from .box_utils import rotate_points_along_z
from .common_utils import cfg_get
from .pointrcnn_head import PointRCNNHead, _as_dict


class PVRCNNHead(nn.Module):
    make_fc_layers = PointRCNNHead.make_fc_layers
    init_weights = PointRCNNHead.init_weights
    proposal_layer = PointRCNNHead.proposal_layer
    generate_predicted_boxes = PointRCNNHead.generate_predicted_boxes

    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__()
        self.model_cfg, self.num_class, self.forward_ret_dict = model_cfg, num_class, None
        target_cfg = cfg_get(model_cfg, 'TARGET_CONFIG')
        self.box_coder = getattr(box_coder_utils, cfg_get(target_cfg, 'BOX_CODER'))(
            **_as_dict(cfg_get(target_cfg, 'BOX_CODER_CONFIG', {})))
        pool_cfg = cfg_get(model_cfg, 'ROI_GRID_POOL')
        self.roi_grid_pool_layer, num_c_out = pointnet2_stack_modules.build_local_aggregation_module(
            input_channels=input_channels, config=pool_cfg)
        self.grid_size = int(cfg_get(pool_cfg, 'GRID_SIZE'))
        pre_channel = self.grid_size ** 3 * num_c_out
        shared, widths, drop = [], list(cfg_get(model_cfg, 'SHARED_FC')), cfg_get(model_cfg, 'DP_RATIO')
        for k, c in enumerate(widths):
            shared += [nn.Conv1d(pre_channel, c, kernel_size=1, bias=False), nn.BatchNorm1d(c), nn.ReLU()]
            pre_channel = c
            if k != len(widths) - 1 and drop > 0:
                shared.append(nn.Dropout(drop))
        self.shared_fc_layer = nn.Sequential(*shared)
        self.cls_layers = self.make_fc_layers(pre_channel, self.num_class, cfg_get(model_cfg, 'CLS_FC'))
        self.reg_layers = self.make_fc_layers(pre_channel, self.box_coder.code_size * self.num_class,
                                              cfg_get(model_cfg, 'REG_FC'))
        self.init_weights(weight_init='xavier')
        self._grid_cnt = {}

    @staticmethod
    def get_dense_grid_points(rois, batch_size_rcnn, grid_size):
        """rois (R, 7 + C) -> (R, grid_size^3, 3): the cell centres of every RoI's own box, x index slowest."""
        g = torch.arange(grid_size, device=rois.device, dtype=rois.dtype)
        dense_idx = torch.stack(torch.meshgrid(g, g, g, indexing='ij'), dim=-1).view(1, -1, 3)
        size = rois.view(batch_size_rcnn, -1)[:, 3:6].unsqueeze(dim=1)
        return (dense_idx + 0.5) / grid_size * size - (size / 2)

    def get_global_grid_points_of_roi(self, rois, grid_size):
        """-> global (R, grid_size^3, 3), local (R, grid_size^3, 3)."""
        rois = rois.view(-1, rois.shape[-1])
        local = self.get_dense_grid_points(rois, rois.shape[0], grid_size)
        glob = rotate_points_along_z(local.clone(), rois[:, 6]).squeeze(dim=1)
        return glob + rois[:, 0:3].unsqueeze(dim=1), local

    def _grid_counts(self, batch_size, per_sample, device):
        key = (batch_size, per_sample, device)
        if key not in self._grid_cnt:
            self._grid_cnt[key] = torch.full((batch_size,), per_sample, dtype=torch.int32, device=device)
        return self._grid_cnt[key]

    def roi_grid_pool(self, batch_dict):
        """rois (B, R, 7 + C), point_coords (N, 4), point_features (N, C), point_cls_scores (N) ->
        (B * R, GRID_SIZE^3, C_out)."""
        batch_size, rois, point_coords = batch_dict['batch_size'], batch_dict['rois'], batch_dict['point_coords']
        point_features = batch_dict['point_features'] * batch_dict['point_cls_scores'].view(-1, 1)
        global_grid, _ = self.get_global_grid_points_of_roi(rois, grid_size=self.grid_size)
        new_xyz = global_grid.reshape(-1, 3)
        xyz_batch_cnt, _ = ops.counts(point_coords[:, 0], batch_size)
        new_cnt = self._grid_counts(batch_size, new_xyz.shape[0] // batch_size, new_xyz.device)
        _, pooled = self.roi_grid_pool_layer(xyz=point_coords[:, 1:4], xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz,
                                             new_xyz_batch_cnt=new_cnt, features=point_features.contiguous())
        return pooled.view(-1, self.grid_size ** 3, pooled.shape[-1])

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError("PVRCNNHead.forward in training mode: target assignment and the losses of "
                                      "PV-RCNN are not part of this package")
        self.proposal_layer(batch_dict, nms_config=cfg_get(cfg_get(self.model_cfg, 'NMS_CONFIG'), 'TEST'))
        pooled = self.roi_grid_pool(batch_dict)                              # (B * R, G^3, C)
        rcnn = pooled.shape[0]
        shared = self.shared_fc_layer(pooled.permute(0, 2, 1).contiguous().view(rcnn, -1, 1))
        rcnn_cls = self.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        rcnn_reg = self.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        cls_preds, box_preds = self.generate_predicted_boxes(batch_dict['batch_size'], batch_dict['rois'], rcnn_cls,
                                                             rcnn_reg)
        batch_dict.update(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg, batch_cls_preds=cls_preds, batch_box_preds=box_preds,
                          cls_preds_normalized=False)
        self.forward_ret_dict = {'rcnn_cls': rcnn_cls, 'rcnn_reg': rcnn_reg}
        return batch_dict
