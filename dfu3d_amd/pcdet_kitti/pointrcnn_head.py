"""PointRCNNHead, the second stage of PointRCNN (pcdet/models/roi_heads/pointrcnn_head.py with what it needs of
roi_head_template.py), with the reference's state-dict keys (xyz_up_layer.*, merge_down_layer.*, SA_modules.*,
cls_layers.*, reg_layers.*).  The inference half:

  proposal_layer   the first stage's stacked predictions viewed as (B, N, .) -- the backbone has checked on the device that
                   the samples have equal sizes, so no `batch_index == index` mask is built -- and the existing
                   class_agnostic_nms per sample (NMS_PRE_MAXSIZE = 9000 is beyond the segmented NMS's cap);
  proposal_layer_batched  the same stage for the whole batch in proposal_ops.LAUNCHES launches and without a host read
                   (proposal_ops.proposals: csrc/proposal_stage.hip); taken by forward only with
                   batched_proposals=True.  Equal scores are ordered by point index there, by torch.topk here;
  roipool3d_gpu    ONE call of the fused RoI-point pooling (roipoint_ops.pool_fused: csrc/roipoint_stage.hip) instead of
                   the concatenation, the pooling op and the five torch ops around it;
  forward          in eval mode; generate_predicted_boxes; init_weights.

The training half is built only with trainable=True; without it forward in training mode,
assign_targets and get_loss raise NotImplementedError as before.  With it: the proposals with NMS_CONFIG.TRAIN, the
ProposalTargetLayer (two launches for the batch: proposal_target_layer.py), the canonical transform of the sampled
ground truth, the pooling and the second stage on the sampled RoIs, and the reference's two losses written as masked
sums over all ROI_PER_IMAGE rows (torch.where, not a product with zero) instead of `[fg_mask]` indexing and the
`fg_sum > 0` branch on the host: the same values and gradients without a host-sized shape.  The loss function and the
target layer have no parameters or buffers: the state dict is the same.  get_loss reads the device once for its tb_dict
(never with as_tensors=True); 'rcnn_loss_corner' is always present (0 without a foreground RoI, where the reference
leaves the key out)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import proposal_ops, roipoint_ops
from . import box_coder_utils, loss_utils, pointnet2_modules
from .base_bev_backbone import _get
from .box_utils import rotate_points_along_z
from .model_nms_utils import class_agnostic_nms
from .point_head_box import TRAINING_ROW, host_values
from .proposal_target_layer import ProposalTargetLayer


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
    def __init__(self, input_channels, model_cfg, num_class=1, trainable=False, batched_proposals=False, **kwargs):
        super().__init__()
        self.model_cfg, self.num_class, self.forward_ret_dict = model_cfg, num_class, None
        self.trainable = bool(trainable)
        self.batched_proposals = bool(batched_proposals)
        target_cfg = _get(model_cfg, 'TARGET_CONFIG')
        if self.trainable:
            self.proposal_target_layer = ProposalTargetLayer(roi_sampler_cfg=target_cfg)
            self.reg_loss_func = loss_utils.WeightedSmoothL1Loss(
                code_weights=_get(_get(model_cfg, 'LOSS_CONFIG'), 'LOSS_WEIGHTS')['code_weights'])
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

    @torch.no_grad()
    def proposal_layer_batched(self, batch_dict, nms_config):
        """proposal_layer for the whole batch at once: the same keys with the same meaning, plus 'num_rois' int32 (B), the
        survivors of every sample.  No host read.  Scores and labels are those of one torch.max(cls_preds, dim=2); among
        equal scores the lower point index comes first (proposal_layer leaves them to torch.topk)."""
        if batch_dict.get('rois', None) is not None:
            return batch_dict
        if _get(nms_config, 'MULTI_CLASSES_NMS'):
            raise NotImplementedError("PointRCNNHead.proposal_layer_batched: MULTI_CLASSES_NMS")
        if _get(nms_config, 'NMS_TYPE') != 'nms_gpu':
            raise NotImplementedError("PointRCNNHead.proposal_layer_batched: NMS_TYPE %r" % (_get(nms_config, 'NMS_TYPE'),))
        batch_size = batch_dict['batch_size']
        box_preds, cls_preds = batch_dict['batch_box_preds'], batch_dict['batch_cls_preds']
        if box_preds.dim() == 2:
            if box_preds.shape[0] % batch_size:
                raise ValueError("proposal_layer_batched: %d predictions are not %d samples of equal size"
                                 % (box_preds.shape[0], batch_size))
            box_preds = box_preds.view(batch_size, -1, box_preds.shape[-1])
            cls_preds = cls_preds.view(batch_size, -1, cls_preds.shape[-1])
        all_scores, all_labels = torch.max(cls_preds, dim=2)
        rois, roi_scores, roi_labels, roi_point_idx, num_rois = proposal_ops.proposals(
            all_scores.float().contiguous(), all_labels.contiguous(), box_preds.float().contiguous(),
            _get(nms_config, 'NMS_THRESH'), _get(nms_config, 'NMS_PRE_MAXSIZE'), _get(nms_config, 'NMS_POST_MAXSIZE'))
        batch_dict['rois'] = rois
        batch_dict['roi_scores'] = roi_scores
        batch_dict['roi_labels'] = roi_labels
        batch_dict['roi_point_idx'] = roi_point_idx
        batch_dict['num_rois'] = num_rois
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

    def assign_targets(self, batch_dict, sampled_inds=None):
        """rois, roi_scores, roi_labels, gt_boxes (B, G, 8) with G >= 1 (a batch without any box is padded to one all-zero
        row; G = 0 raises Dfu3dError) of the batch; sampled_inds (B, ROI_PER_IMAGE) given: no draw -> the target layer's dict with 'gt_of_rois_src' (the
        sampled ground truth as it is) and 'gt_of_rois' in the frame of its RoI: the centre moved to the RoI's, turned
        by -roi_ry, the heading difference folded into [-pi/2, pi/2] (a box facing the other way counts as aligned)."""
        if not self.trainable:
            raise NotImplementedError("PointRCNNHead.assign_targets: " + TRAINING_ROW)
        batch_size = batch_dict['batch_size']
        targets = self.proposal_target_layer(batch_dict, sampled_inds=sampled_inds)
        rois, gt = targets['rois'], targets['gt_of_rois']
        targets['gt_of_rois_src'] = gt.clone().detach()
        two_pi = 2 * math.pi
        roi_ry = rois[:, :, 6] % two_pi
        gt[:, :, 0:3] = gt[:, :, 0:3] - rois[:, :, 0:3]
        gt[:, :, 6] = gt[:, :, 6] - roi_ry
        gt = rotate_points_along_z(gt.view(-1, 1, gt.shape[-1]), -roi_ry.view(-1)).view(batch_size, -1, gt.shape[-1])
        heading = gt[:, :, 6] % two_pi                                     # 0 .. 2 pi
        opposite = (heading > math.pi * 0.5) & (heading < math.pi * 1.5)
        heading = torch.where(opposite, (heading + math.pi) % two_pi, heading)        # 0 .. pi/2 or 3 pi/2 .. 2 pi
        heading = torch.where(heading > math.pi, heading - math.pi * 2, heading)      # -pi/2 .. pi/2
        gt[:, :, 6] = torch.clamp(heading, min=-math.pi / 2, max=math.pi / 2)
        targets['gt_of_rois'] = gt
        return targets

    def _need_targets(self, what):
        if not self.trainable:
            raise NotImplementedError("PointRCNNHead.%s: %s" % (what, TRAINING_ROW))
        if not self.forward_ret_dict or 'rcnn_cls_labels' not in self.forward_ret_dict:
            raise RuntimeError("PointRCNNHead.%s: no targets -- run forward in training mode on a batch with gt_boxes first" % what)
        return self.forward_ret_dict

    def get_box_cls_layer_loss(self, forward_ret_dict):
        """The (binary) cross entropy of every sampled RoI whose label is not -1, their mean -> (loss, {'rcnn_loss_cls'})."""
        cfg = _get(self.model_cfg, 'LOSS_CONFIG')
        rcnn_cls, labels = forward_ret_dict['rcnn_cls'], forward_ret_dict['rcnn_cls_labels'].view(-1)
        kind = _get(cfg, 'CLS_LOSS')
        if kind == 'BinaryCrossEntropy':
            # an ignored RoI (-1) gets the target 0 and is masked below: binary_cross_entropy refuses targets outside [0, 1]
            each = F.binary_cross_entropy(torch.sigmoid(rcnn_cls.view(-1)), labels.clamp(min=0).float(), reduction='none')
        elif kind == 'CrossEntropy':
            each = F.cross_entropy(rcnn_cls, labels, reduction='none', ignore_index=-1)
        else:
            raise NotImplementedError("PointRCNNHead: CLS_LOSS %r" % (kind,))
        valid = labels >= 0
        loss = torch.where(valid, each, torch.zeros_like(each)).sum() / torch.clamp(valid.float().sum(), min=1.0)
        loss = loss * _get(cfg, 'LOSS_WEIGHTS')['rcnn_cls_weight']
        return loss, {'rcnn_loss_cls': loss.detach()}

    def get_box_reg_layer_loss(self, forward_ret_dict):
        """Over the RoIs with reg_valid_mask: the smooth L1 of the box code against the ResidualCoder code of the
        canonical ground truth (the RoI at the origin with heading 0 as the anchor), summed and divided by their number,
        plus the mean corner loss of the decoded boxes against the ground truth as it is -> (loss, {'rcnn_loss_reg' --
        without the corner term, as the reference records it --, 'rcnn_loss_corner'})."""
        cfg = _get(self.model_cfg, 'LOSS_CONFIG')
        weights = _get(cfg, 'LOSS_WEIGHTS')
        if _get(cfg, 'REG_LOSS') != 'smooth-l1':
            raise NotImplementedError("PointRCNNHead: REG_LOSS %r" % (_get(cfg, 'REG_LOSS'),))
        code_size = self.box_coder.code_size
        fg = forward_ret_dict['reg_valid_mask'].view(-1) > 0
        gt_ct = forward_ret_dict['gt_of_rois'][..., 0:code_size]
        gt_src = forward_ret_dict['gt_of_rois_src'][..., 0:code_size].reshape(-1, code_size)
        rois = forward_ret_dict['rois']
        rows = gt_ct.reshape(-1, code_size).shape[0]
        rcnn_reg = forward_ret_dict['rcnn_reg'].view(rows, -1)
        fg_sum = torch.clamp(fg.float().sum(), min=1.0)
        anchors = rois.clone().detach().view(-1, code_size)
        anchors[:, 0:3] = 0
        anchors[:, 6] = 0
        reg_targets = self.box_coder.encode_torch(gt_ct.reshape(rows, code_size), anchors)
        each = self.reg_loss_func(rcnn_reg.unsqueeze(dim=0), reg_targets.unsqueeze(dim=0)).view(rows, -1)
        loss_reg = torch.where(fg[:, None], each, torch.zeros_like(each)).sum() / fg_sum
        loss_reg = loss_reg * weights['rcnn_reg_weight']
        tb_dict = {'rcnn_loss_reg': loss_reg.detach()}
        corner = loss_reg.new_zeros(())
        if _get(cfg, 'CORNER_LOSS_REGULARIZATION'):
            # a row without a target decodes zeros (its own RoI): finite whatever the head predicts, and no gradient
            codes = torch.where(fg[:, None], rcnn_reg, torch.zeros_like(rcnn_reg))
            flat = rois.reshape(-1, code_size)
            at_origin = flat.clone().detach()
            at_origin[:, 0:3] = 0
            boxes = self.box_coder.decode_torch(codes.view(1, rows, code_size), at_origin.view(1, rows, code_size))
            boxes = rotate_points_along_z(boxes.view(-1, 1, code_size), flat[:, 6]).squeeze(dim=1)
            boxes = torch.cat((boxes[:, 0:3] + flat[:, 0:3], boxes[:, 3:]), dim=-1)
            each = loss_utils.get_corner_loss_lidar(boxes[:, 0:7], gt_src[:, 0:7])
            corner = torch.where(fg, each, torch.zeros_like(each)).sum() / fg_sum
            corner = corner * weights['rcnn_corner_weight']
        tb_dict['rcnn_loss_corner'] = corner.detach()
        return loss_reg + corner, tb_dict

    def get_loss(self, tb_dict=None, as_tensors=False):
        """-> (rcnn_loss, tb_dict): 'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss' as Python floats
        read with ONE copy, or with as_tensors=True as 0-dim device tensors without any synchronisation."""
        ret = self._need_targets('get_loss')
        tb_dict = {} if tb_dict is None else tb_dict
        loss_cls, own = self.get_box_cls_layer_loss(ret)
        loss_reg, more = self.get_box_reg_layer_loss(ret)
        loss = loss_cls + loss_reg
        own = dict(own, **more, rcnn_loss=loss.detach())
        tb_dict.update(own if as_tensors else host_values(own))
        return loss, tb_dict

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
        if self.training and not self.trainable:
            raise NotImplementedError("PointRCNNHead.forward in training mode: " + TRAINING_ROW)
        propose = self.proposal_layer_batched if self.batched_proposals else self.proposal_layer
        propose(batch_dict, nms_config=_get(_get(self.model_cfg, 'NMS_CONFIG'), 'TRAIN' if self.training else 'TEST'))
        if self.training:
            targets = self.assign_targets(batch_dict)
            batch_dict['rois'], batch_dict['roi_labels'] = targets['rois'], targets['roi_labels']
            rcnn_cls, rcnn_reg = self.second_stage(self.roipool3d_gpu(batch_dict))
            targets.update(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg)
            self.forward_ret_dict = targets
            return batch_dict
        rcnn_cls, rcnn_reg = self.second_stage(self.roipool3d_gpu(batch_dict))
        cls_preds, box_preds = self.generate_predicted_boxes(batch_dict['batch_size'], batch_dict['rois'], rcnn_cls, rcnn_reg)
        batch_dict.update(rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg, batch_cls_preds=cls_preds, batch_box_preds=box_preds,
                          cls_preds_normalized=False)
        return batch_dict
