"""pcdet/models/dense_heads/anchor_head_template.py and anchor_head_single.py under their names: the anchor head of
SECOND (and of PointPillars and PV-RCNN's first stage) -- three 1 x 1 convolutions over the BEV features, the target
assignment on the anchor target stage (axis_aligned_target_assigner -> csrc/anchor_stage.hip), the three losses and the
box decoding in plain torch on this package's loss classes and box coder.  Parameter names (`conv_cls`, `conv_box`,
`conv_dir_cls`) and initialisation are the reference's, so its checkpoints load.

Divergences from the reference: the anchors are no parameters and no buffers (as there), computed on the CPU and moved
with the module (`.to`, `.cuda`), never by a .cuda() of their own; `get_loss` reads its four scalars from the device in one
copy; USE_MULTIHEAD, the ATSS assigner and box coders other than ResidualCoder raise NotImplementedError."""
import numpy as np
import torch
import torch.nn as nn

from . import box_coder_utils, loss_utils
from .anchor_generator import AnchorGenerator
from .axis_aligned_target_assigner import AxisAlignedTargetAssigner
from .common_utils import cfg_get, limit_period


class AnchorHeadTemplate(nn.Module):
    def __init__(self, model_cfg, num_class, class_names, grid_size, point_cloud_range, predict_boxes_when_training):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.class_names = class_names
        self.predict_boxes_when_training = predict_boxes_when_training
        self.use_multihead = cfg_get(model_cfg, 'USE_MULTIHEAD', False)
        if self.use_multihead:
            raise NotImplementedError("AnchorHeadTemplate: USE_MULTIHEAD: True is not part of this package")
        target_cfg = cfg_get(model_cfg, 'TARGET_ASSIGNER_CONFIG')
        coder = cfg_get(target_cfg, 'BOX_CODER')
        if coder != 'ResidualCoder':
            raise NotImplementedError("AnchorHeadTemplate: BOX_CODER = %r is not part of this package (it has "
                                      "ResidualCoder)" % (coder,))
        self.box_coder = box_coder_utils.ResidualCoder(num_dir_bins=cfg_get(target_cfg, 'NUM_DIR_BINS', 6),
                                                       **dict(cfg_get(target_cfg, 'BOX_CODER_CONFIG', {})))
        anchors, self.num_anchors_per_location = self.generate_anchors(
            cfg_get(model_cfg, 'ANCHOR_GENERATOR_CONFIG'), grid_size=grid_size, point_cloud_range=point_cloud_range,
            anchor_ndim=self.box_coder.code_size)
        self.anchors = anchors                          # on the CPU until the module is moved (_apply)
        self.target_assigner = self.get_target_assigner(target_cfg)
        self.forward_ret_dict = {}
        self.build_losses(cfg_get(model_cfg, 'LOSS_CONFIG'))

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        first = next(self.parameters(), None)
        if first is not None:
            self.anchors = [a.to(first.device) for a in self.anchors]
        return out

    @staticmethod
    def generate_anchors(anchor_generator_cfg, grid_size, point_cloud_range, anchor_ndim=7):
        generator = AnchorGenerator(anchor_range=point_cloud_range, anchor_generator_config=anchor_generator_cfg)
        grid_size = np.asarray(grid_size)
        feature_map_size = [grid_size[:2] // cfg_get(c, 'feature_map_stride') for c in anchor_generator_cfg]
        anchors_list, per_location = generator.generate_anchors(feature_map_size)
        if anchor_ndim != 7:
            anchors_list = [torch.cat((a, a.new_zeros([*a.shape[0:-1], anchor_ndim - 7])), dim=-1) for a in anchors_list]
        return anchors_list, per_location

    def get_target_assigner(self, anchor_target_cfg):
        name = cfg_get(anchor_target_cfg, 'NAME')
        if name != 'AxisAlignedTargetAssigner':
            raise NotImplementedError("AnchorHeadTemplate: TARGET_ASSIGNER_CONFIG.NAME = %r is not part of this package "
                                      "(it has AxisAlignedTargetAssigner)" % (name,))
        return AxisAlignedTargetAssigner(model_cfg=self.model_cfg, class_names=self.class_names, box_coder=self.box_coder,
                                         match_height=cfg_get(anchor_target_cfg, 'MATCH_HEIGHT'))

    def build_losses(self, losses_cfg):
        self.add_module('cls_loss_func', loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0))
        reg_loss_name = cfg_get(losses_cfg, 'REG_LOSS_TYPE', None) or 'WeightedSmoothL1Loss'
        if reg_loss_name != 'WeightedSmoothL1Loss':
            raise NotImplementedError("AnchorHeadTemplate: REG_LOSS_TYPE = %r is not part of this package" % (reg_loss_name,))
        self.add_module('reg_loss_func', loss_utils.WeightedSmoothL1Loss(
            code_weights=cfg_get(losses_cfg, 'LOSS_WEIGHTS')['code_weights']))
        self.add_module('dir_loss_func', loss_utils.WeightedCrossEntropyLoss())

    def _loss_weight(self, key):
        return cfg_get(cfg_get(self.model_cfg, 'LOSS_CONFIG'), 'LOSS_WEIGHTS')[key]

    def assign_targets(self, gt_boxes):
        """gt_boxes (B, M, 8) -> the assigner's dict."""
        return self.target_assigner.assign_targets(self.anchors, gt_boxes)

    def flat_anchors(self):
        """(nz, ny, nx, all anchors of a location, 7): the classes one after another at every location."""
        return torch.cat(self.anchors, dim=-3) if isinstance(self.anchors, list) else self.anchors

    def get_cls_layer_loss(self, as_tensors=False):
        cls_preds = self.forward_ret_dict['cls_preds']
        box_cls_labels = self.forward_ret_dict['box_cls_labels']
        batch_size = int(cls_preds.shape[0])
        cared = box_cls_labels >= 0
        positives = box_cls_labels > 0
        negatives = box_cls_labels == 0
        cls_weights = (negatives * 1.0 + 1.0 * positives).float()
        if self.num_class == 1:
            box_cls_labels[positives] = 1                                   # class agnostic
        pos_normalizer = positives.sum(1, keepdim=True).float()
        cls_weights /= torch.clamp(pos_normalizer, min=1.0)
        cls_targets = box_cls_labels * cared.type_as(box_cls_labels)
        one_hot_targets = torch.zeros(*list(cls_targets.shape), self.num_class + 1, dtype=cls_preds.dtype,
                                      device=cls_targets.device)
        one_hot_targets.scatter_(-1, cls_targets.unsqueeze(dim=-1).long(), 1.0)
        cls_preds = cls_preds.view(batch_size, -1, self.num_class)
        cls_loss_src = self.cls_loss_func(cls_preds, one_hot_targets[..., 1:], weights=cls_weights)
        self.forward_ret_dict['cls_loss_src'] = cls_loss_src
        cls_loss = cls_loss_src.sum() / batch_size
        cls_loss = cls_loss * self._loss_weight('cls_weight')
        return cls_loss, {'rpn_loss_cls': cls_loss.detach() if as_tensors else cls_loss.item()}

    @staticmethod
    def add_sin_difference(boxes1, boxes2, dim=6):
        """sin(a - b) = sin a cos b - cos a sin b: the heading column of both becomes its half of the difference."""
        assert dim != -1
        rad_pred_encoding = torch.sin(boxes1[..., dim:dim + 1]) * torch.cos(boxes2[..., dim:dim + 1])
        rad_tg_encoding = torch.cos(boxes1[..., dim:dim + 1]) * torch.sin(boxes2[..., dim:dim + 1])
        boxes1 = torch.cat([boxes1[..., :dim], rad_pred_encoding, boxes1[..., dim + 1:]], dim=-1)
        boxes2 = torch.cat([boxes2[..., :dim], rad_tg_encoding, boxes2[..., dim + 1:]], dim=-1)
        return boxes1, boxes2

    @staticmethod
    def get_direction_target(anchors, reg_targets, one_hot=True, dir_offset=0, num_bins=2):
        batch_size = reg_targets.shape[0]
        anchors = anchors.view(batch_size, -1, anchors.shape[-1])
        rot_gt = reg_targets[..., 6] + anchors[..., 6]
        offset_rot = limit_period(rot_gt - dir_offset, 0, 2 * np.pi)
        dir_cls_targets = torch.floor(offset_rot / (2 * np.pi / num_bins)).long()
        dir_cls_targets = torch.clamp(dir_cls_targets, min=0, max=num_bins - 1)
        if one_hot:
            dir_targets = torch.zeros(*list(dir_cls_targets.shape), num_bins, dtype=anchors.dtype,
                                      device=dir_cls_targets.device)
            dir_targets.scatter_(-1, dir_cls_targets.unsqueeze(dim=-1).long(), 1.0)
            dir_cls_targets = dir_targets
        return dir_cls_targets

    def get_box_reg_layer_loss(self, as_tensors=False):
        box_preds = self.forward_ret_dict['box_preds']
        box_dir_cls_preds = self.forward_ret_dict.get('dir_cls_preds', None)
        box_reg_targets = self.forward_ret_dict['box_reg_targets']
        box_cls_labels = self.forward_ret_dict['box_cls_labels']
        batch_size = int(box_preds.shape[0])
        positives = box_cls_labels > 0
        reg_weights = positives.float()
        pos_normalizer = positives.sum(1, keepdim=True).float()
        reg_weights /= torch.clamp(pos_normalizer, min=1.0)
        anchors = self.flat_anchors()
        anchors = anchors.view(1, -1, anchors.shape[-1]).repeat(batch_size, 1, 1)
        box_preds = box_preds.view(batch_size, -1, box_preds.shape[-1] // self.num_anchors_per_location)
        box_preds_sin, reg_targets_sin = self.add_sin_difference(box_preds, box_reg_targets)
        loc_loss_src = self.reg_loss_func(box_preds_sin, reg_targets_sin, weights=reg_weights)
        self.forward_ret_dict['loc_loss_src'] = loc_loss_src
        loc_loss = loc_loss_src.sum() / batch_size
        loc_loss = loc_loss * self._loss_weight('loc_weight')
        box_loss = loc_loss
        tb_dict = {'rpn_loss_loc': loc_loss.detach() if as_tensors else loc_loss.item()}
        if box_dir_cls_preds is not None:
            num_bins = cfg_get(self.model_cfg, 'NUM_DIR_BINS')
            dir_targets = self.get_direction_target(anchors, box_reg_targets,
                                                    dir_offset=cfg_get(self.model_cfg, 'DIR_OFFSET'), num_bins=num_bins)
            dir_logits = box_dir_cls_preds.view(batch_size, -1, num_bins)
            weights = positives.type_as(dir_logits)
            weights /= torch.clamp(weights.sum(-1, keepdim=True), min=1.0)
            dir_loss_src = self.dir_loss_func(dir_logits, dir_targets, weights=weights)
            self.forward_ret_dict['dir_loss_src'] = dir_loss_src
            dir_loss = dir_loss_src.sum() / batch_size
            dir_loss = dir_loss * self._loss_weight('dir_weight')
            box_loss = box_loss + dir_loss
            tb_dict['rpn_loss_dir'] = dir_loss.detach() if as_tensors else dir_loss.item()
        return box_loss, tb_dict

    def get_loss(self):
        cls_loss, tb_dict = self.get_cls_layer_loss(as_tensors=True)
        box_loss, tb_dict_box = self.get_box_reg_layer_loss(as_tensors=True)
        tb_dict.update(tb_dict_box)
        rpn_loss = cls_loss + box_loss
        tb_dict['rpn_loss'] = rpn_loss.detach()
        keys = list(tb_dict)
        values = torch.stack([tb_dict[k].float() for k in keys]).tolist()      # the one read from the device
        return rpn_loss, dict(zip(keys, values))

    def generate_predicted_boxes(self, batch_size, cls_preds, box_preds, dir_cls_preds=None):
        """cls_preds (N, H, W, C1), box_preds (N, H, W, C2), dir_cls_preds (N, H, W, C3) -> batch_cls_preds
        (B, #anchors, #classes), batch_box_preds (B, #anchors, 7)."""
        anchors = self.flat_anchors()
        num_anchors = anchors.view(-1, anchors.shape[-1]).shape[0]
        batch_anchors = anchors.view(1, -1, anchors.shape[-1]).repeat(batch_size, 1, 1)
        batch_cls_preds = cls_preds.view(batch_size, num_anchors, -1).float()
        batch_box_preds = self.box_coder.decode_torch(box_preds.view(batch_size, num_anchors, -1), batch_anchors)
        if dir_cls_preds is not None:
            dir_offset = cfg_get(self.model_cfg, 'DIR_OFFSET')
            dir_limit_offset = cfg_get(self.model_cfg, 'DIR_LIMIT_OFFSET')
            dir_labels = torch.max(dir_cls_preds.view(batch_size, num_anchors, -1), dim=-1)[1]
            period = 2 * np.pi / cfg_get(self.model_cfg, 'NUM_DIR_BINS')
            dir_rot = limit_period(batch_box_preds[..., 6] - dir_offset, dir_limit_offset, period)
            batch_box_preds[..., 6] = dir_rot + dir_offset + period * dir_labels.to(batch_box_preds.dtype)
        return batch_cls_preds, batch_box_preds

    def forward(self, **kwargs):
        raise NotImplementedError


class AnchorHeadSingle(AnchorHeadTemplate):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range,
                 predict_boxes_when_training=True, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class, class_names=class_names, grid_size=grid_size,
                         point_cloud_range=point_cloud_range, predict_boxes_when_training=predict_boxes_when_training)
        self.num_anchors_per_location = sum(self.num_anchors_per_location)
        self.conv_cls = nn.Conv2d(input_channels, self.num_anchors_per_location * self.num_class, kernel_size=1)
        self.conv_box = nn.Conv2d(input_channels, self.num_anchors_per_location * self.box_coder.code_size, kernel_size=1)
        if cfg_get(model_cfg, 'USE_DIRECTION_CLASSIFIER', None) is not None:
            self.conv_dir_cls = nn.Conv2d(input_channels, self.num_anchors_per_location * cfg_get(model_cfg, 'NUM_DIR_BINS'),
                                          kernel_size=1)
        else:
            self.conv_dir_cls = None
        self.init_weights()

    def init_weights(self):
        pi = 0.01
        nn.init.constant_(self.conv_cls.bias, -np.log((1 - pi) / pi))
        nn.init.normal_(self.conv_box.weight, mean=0, std=0.001)

    def forward(self, data_dict):
        spatial_features_2d = data_dict['spatial_features_2d']
        cls_preds = self.conv_cls(spatial_features_2d).permute(0, 2, 3, 1).contiguous()      # (N, H, W, C)
        box_preds = self.conv_box(spatial_features_2d).permute(0, 2, 3, 1).contiguous()
        self.forward_ret_dict['cls_preds'] = cls_preds
        self.forward_ret_dict['box_preds'] = box_preds
        if self.conv_dir_cls is not None:
            dir_cls_preds = self.conv_dir_cls(spatial_features_2d).permute(0, 2, 3, 1).contiguous()
            self.forward_ret_dict['dir_cls_preds'] = dir_cls_preds
        else:
            dir_cls_preds = None
        if self.training:
            self.forward_ret_dict.update(self.assign_targets(gt_boxes=data_dict['gt_boxes']))
        if not self.training or self.predict_boxes_when_training:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
                batch_size=data_dict['batch_size'], cls_preds=cls_preds, box_preds=box_preds, dir_cls_preds=dir_cls_preds)
            data_dict['batch_cls_preds'] = batch_cls_preds
            data_dict['batch_box_preds'] = batch_box_preds
            data_dict['cls_preds_normalized'] = False
        return data_dict
