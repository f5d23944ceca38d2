"""PointRCNNHead, the second stage of PointRCNN (pcdet/models/roi_heads/pointrcnn_head.py with what it needs of
roi_head_template.py), with the reference's state-dict keys (xyz_up_layer.*, merge_down_layer.*, SA_modules.*,
cls_layers.*, reg_layers.*).  The inference half:

  proposal_layer   the first stage's stacked predictions viewed as (B, N, .) -- the backbone has checked on the device that
                   the samples have equal sizes, so no `batch_index == index` mask is built -- and the existing
                   class_agnostic_nms per sample (NMS_PRE_MAXSIZE = 9000 is beyond the segmented NMS's cap);
  roipool3d_gpu    ONE call of the fused RoI-point pooling (roipoint_ops.pool_fused: csrc/roipoint_stage.hip) instead of
                   the concatenation, the pooling op and the five torch ops around it;
  forward          in eval mode; generate_predicted_boxes; init_weights.

forward in training mode is the training row (not built) and raises NotImplementedError."""
import torch
import torch.nn as nn

from .. import roipoint_ops
from . import box_coder_utils, pointnet2_modules
from .base_bev_backbone import _get
from .box_utils import rotate_points_along_z
from .model_nms_utils import class_agnostic_nms
from .point_head_box import TRAINING_ROW


def _as_dict(cfg):
    return dict(cfg) if isinstance(cfg, dict) else dict(vars(cfg))


def _pointwise(channels, bias, norm, conv=nn.Conv2d):
    """1 x 1 convolutions channels[0] -> channels[1] -> ..., each followed by (a batch norm and) a ReLU."""
    layers = []
    for c_in, c_out in zip(channels[:-1], channels[1:]):
        layers.append(conv(c_in, c_out, kernel_size=1, bias=bias))
        if norm:
            layers.append(nn.BatchNorm2d(c_out))
        layers.append(nn.ReLU())
    return layers


class PointRCNNHead(nn.Module):
    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__()
        self.model_cfg, self.num_class, self.forward_ret_dict = model_cfg, num_class, None
        target_cfg = _get(model_cfg, 'TARGET_CONFIG')
        self.box_coder = getattr(box_coder_utils, _get(target_cfg, 'BOX_CODER'))(
            **_as_dict(_get(target_cfg, 'BOX_CODER_CONFIG', {})))
        use_bn = bool(_get(model_cfg, 'USE_BN'))
        self.num_prefix_channels = roipoint_ops.PREFIX_FUSED           # x', y', z', score, depth
        up = [self.num_prefix_channels] + list(_get(model_cfg, 'XYZ_UP_LAYER'))
        # registration order = state-dict order: SA_modules, xyz_up_layer, merge_down_layer, cls_layers, reg_layers
        self.SA_modules = nn.ModuleList()
        self.xyz_up_layer = nn.Sequential(*_pointwise(up, bias=not use_bn, norm=use_bn))
        self.merge_down_layer = nn.Sequential(*_pointwise([2 * up[-1], up[-1]], bias=not use_bn, norm=use_bn))
        sa, width = _get(model_cfg, 'SA_CONFIG'), input_channels
        for npoint, radius, nsample, mlp in zip(_get(sa, 'NPOINTS'), _get(sa, 'RADIUS'), _get(sa, 'NSAMPLE'), _get(sa, 'MLPS')):
            self.SA_modules.append(pointnet2_modules.PointnetSAModule(
                npoint=None if npoint == -1 else npoint, radius=radius, nsample=nsample, mlp=[width] + list(mlp),
                use_xyz=True, bn=use_bn))
            width = mlp[-1]
        self.cls_layers = self.make_fc_layers(width, self.num_class, _get(model_cfg, 'CLS_FC'))
        self.reg_layers = self.make_fc_layers(width, self.box_coder.code_size * self.num_class, _get(model_cfg, 'REG_FC'))
        self.init_weights(weight_init='xavier')

    def make_fc_layers(self, input_channels, output_channels, fc_list):
        """Conv1d / BatchNorm1d / ReLU per entry of fc_list, a Dropout behind the first (it has no parameters but takes
        an index of the Sequential, hence of the state-dict keys) when DP_RATIO >= 0, then the output Conv1d."""
        drop, layers, width = _get(self.model_cfg, 'DP_RATIO'), [], input_channels
        for k, c in enumerate(fc_list):
            layers += [nn.Conv1d(width, c, kernel_size=1, bias=False), nn.BatchNorm1d(c), nn.ReLU()]
            if k == 0 and drop >= 0:
                layers.append(nn.Dropout(drop))
            width = c
        return nn.Sequential(*layers, nn.Conv1d(width, output_channels, kernel_size=1, bias=True))

    def init_weights(self, weight_init='xavier'):
        """Every convolution's weight by the named rule, its bias zero; the last regression layer normal(0, 0.001)."""
        rules = {'kaiming': nn.init.kaiming_normal_, 'xavier': nn.init.xavier_normal_,
                 'normal': lambda w: nn.init.normal_(w, mean=0, std=0.001)}
        if weight_init not in rules:
            raise NotImplementedError(weight_init)
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.Conv2d)):
                rules[weight_init](m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    @torch.no_grad()
    def proposal_layer(self, batch_dict, nms_config):
        """batch_cls_preds (B * N, num_class) and batch_box_preds (B * N, 7 + C) stacked in sample order, or (B, N, .) ->
        rois (B, NMS_POST_MAXSIZE, 7 + C), roi_scores, roi_labels (1-based, int64); rows beyond a sample's survivors are
        zero (label 1).  batch_dict['roi_point_idx'] int64 (B, NMS_POST_MAXSIZE): the point of every RoI, -1 beyond."""
        if batch_dict.get('rois', None) is not None:
            return batch_dict
        if _get(nms_config, 'MULTI_CLASSES_NMS'):
            raise NotImplementedError("PointRCNNHead.proposal_layer: MULTI_CLASSES_NMS")
        batch_size = batch_dict['batch_size']
        box_preds, cls_preds = batch_dict['batch_box_preds'], batch_dict['batch_cls_preds']
        if box_preds.dim() == 2:
            if box_preds.shape[0] % batch_size:
                raise ValueError("proposal_layer: %d predictions are not %d samples of equal size"
                                 % (box_preds.shape[0], batch_size))
            box_preds = box_preds.view(batch_size, -1, box_preds.shape[-1])
            cls_preds = cls_preds.view(batch_size, -1, cls_preds.shape[-1])
        post = _get(nms_config, 'NMS_POST_MAXSIZE')
        rois = box_preds.new_zeros((batch_size, post, box_preds.shape[-1]))
        roi_scores = box_preds.new_zeros((batch_size, post))
        roi_labels = box_preds.new_zeros((batch_size, post), dtype=torch.long)
        roi_point_idx = box_preds.new_full((batch_size, post), -1, dtype=torch.long)
        all_scores, all_labels = torch.max(cls_preds, dim=2)
        for index in range(batch_size):
            selected, _ = class_agnostic_nms(box_scores=all_scores[index], box_preds=box_preds[index], nms_config=nms_config)
            n = len(selected)
            rois[index, :n] = box_preds[index][selected]
            roi_scores[index, :n] = all_scores[index][selected]
            roi_labels[index, :n] = all_labels[index][selected]
            roi_point_idx[index, :n] = selected
        batch_dict['rois'] = rois
        batch_dict['roi_scores'] = roi_scores
        batch_dict['roi_labels'] = roi_labels + 1
        batch_dict['roi_point_idx'] = roi_point_idx
        batch_dict['has_class_labels'] = cls_preds.shape[-1] > 1
        batch_dict.pop('batch_index', None)
        return batch_dict

    def roipool3d_gpu(self, batch_dict, return_idx=False):
        """point_coords (B * N, 4), point_features (B * N, C), point_cls_scores (B * N), rois (B, M, 7 + .) ->
        (B * M, S, 5 + C): per RoI its first S points, canonical coordinates, score, depth, features; empty RoIs zero."""
        cfg = _get(self.model_cfg, 'ROI_POINT_POOL')
        with torch.no_grad():
            return roipoint_ops.pool_fused(
                batch_dict['point_coords'].detach().contiguous(), batch_dict['point_cls_scores'].detach().contiguous(),
                batch_dict['point_features'].detach().contiguous(), batch_dict['rois'].detach(),
                _get(cfg, 'POOL_EXTRA_WIDTH'), _get(cfg, 'NUM_SAMPLED_POINTS'), _get(cfg, 'DEPTH_NORMALIZER'),
                return_idx=return_idx)

    def assign_targets(self, batch_dict):
        raise NotImplementedError("PointRCNNHead.assign_targets: " + TRAINING_ROW)

    def get_loss(self, tb_dict=None):
        raise NotImplementedError("PointRCNNHead.get_loss: " + TRAINING_ROW)

    def generate_predicted_boxes(self, batch_size, rois, cls_preds, box_preds):
        """rois (B, M, 7), cls_preds (B * M, num_class), box_preds (B * M, code_size) -> batch_cls_preds (B, M, .),
        batch_box_preds (B, M, code_size): decoded against the RoI at the origin, rotated by its heading, moved to it."""
        code_size = self.box_coder.code_size
        at_origin = rois.detach().clone()
        at_origin[..., 0:3] = 0
        local = self.box_coder.decode_torch(box_preds.view(batch_size, -1, code_size), at_origin)
        boxes = rotate_points_along_z(local.view(-1, 1, code_size), rois[..., 6].reshape(-1)).view(-1, code_size)
        boxes[:, 0:3] += rois[..., 0:3].reshape(-1, 3)
        return cls_preds.view(batch_size, -1, cls_preds.shape[-1]), boxes.view(batch_size, -1, code_size)

    def second_stage(self, pooled):
        """pooled (R, S, 5 + C) -> rcnn_cls (R, num_class), rcnn_reg (R, code_size * num_class): the prefix columns
        lifted to C channels and merged with the point features, the SA pyramid down to one feature per RoI, the two
        heads."""
        P = self.num_prefix_channels
        columns = pooled.transpose(1, 2).unsqueeze(3)                      # (R, 5 + C, S, 1)
        lifted = self.xyz_up_layer(columns[:, :P].contiguous())
        features = self.merge_down_layer(torch.cat((lifted, columns[:, P:]), dim=1)).squeeze(3).contiguous()
        xyz = pooled[..., 0:3].contiguous()
        for sa in self.SA_modules:
            xyz, features = sa(xyz, features)
        flat = lambda head: head(features).transpose(1, 2).contiguous().squeeze(1)   # noqa: E731    (R, 1, K) -> (R, K)
        return flat(self.cls_layers), flat(self.reg_layers)

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError("PointRCNNHead.forward in training mode: " + TRAINING_ROW)
        self.proposal_layer(batch_dict, nms_config=_get(_get(self.model_cfg, 'NMS_CONFIG'), 'TEST'))
        rcnn_cls, rcnn_reg = self.second_stage(self.roipool3d_gpu(batch_dict))
        cls_preds, box_preds = self.generate_predicted_boxes(batch_dict['batch_size'], batch_dict['rois'], rcnn_cls, rcnn_reg)
        batch_dict.update(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg, batch_cls_preds=cls_preds, batch_box_preds=box_preds,
                          cls_preds_normalized=False)
        return batch_dict
