"""PointHeadBox, the first stage of PointRCNN (pcdet/models/dense_heads/point_head_box.py over point_head_template.py):
per point a class score and a box against the point and the mean size of the predicted class, with the reference's
state-dict keys (cls_layers.*, box_layers.*).  The inference half: forward in eval mode, and in training mode without
targets when predict_boxes_when_training is set.

The training half is built only with trainable=True; without it target assignment and the losses
raise NotImplementedError as before.  assign_targets is ONE launch for the batch (rcnn_target_ops.point_targets:
csrc/rcnntarget_stage.hip) instead of the reference's per-sample masks, two point-in-box calls, scatters and encode; the
losses are the reference's formulas in torch without a host-sized shape; get_loss reads the device once for its tb_dict
(never with as_tensors=True).  The loss functions have no parameters or buffers: the state dict is the same.

Divergences from the reference: a point inside a box whose class column is < 1 (or beyond the mean
sizes) is background with a zero box label, where the reference encodes against mean_size[-1], takes the log of zero dims
and lets the NaN meet a zero weight; the dims are clamped to 1e-5 for the encode without writing to gt_boxes."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import rcnn_target_ops
from . import box_coder_utils, loss_utils
from .base_bev_backbone import _get

TRAINING_ROW = "the PointRCNN training row (assign_targets, ProposalTargetLayer, the heads' losses) is not built"


def host_values(tensors):
    """{name: 0-dim tensor} -> {name: Python float}, all of them in ONE copy to the host."""
    names = list(tensors)
    values = torch.stack([tensors[n].detach().float().reshape(()) for n in names]).tolist() if names else []
    return dict(zip(names, values))


class PointHeadBox(nn.Module):
    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, trainable=False, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.predict_boxes_when_training = predict_boxes_when_training
        self.trainable = bool(trainable)
        self.forward_ret_dict = None
        if self.trainable:
            self.build_losses(_get(model_cfg, 'LOSS_CONFIG'))
        self.cls_layers = self.make_fc_layers(fc_cfg=_get(model_cfg, 'CLS_FC'), input_channels=input_channels,
                                              output_channels=num_class)
        target_cfg = _get(model_cfg, 'TARGET_CONFIG')
        coder_cfg = _get(target_cfg, 'BOX_CODER_CONFIG', {})
        self.box_coder = getattr(box_coder_utils, _get(target_cfg, 'BOX_CODER'))(
            **(dict(coder_cfg) if isinstance(coder_cfg, dict) else dict(vars(coder_cfg))))
        self.box_layers = self.make_fc_layers(fc_cfg=_get(model_cfg, 'REG_FC'), input_channels=input_channels,
                                              output_channels=self.box_coder.code_size)

    @staticmethod
    def make_fc_layers(fc_cfg, input_channels, output_channels):
        layers, c_in = [], input_channels
        for c in fc_cfg:
            layers.extend([nn.Linear(c_in, c, bias=False), nn.BatchNorm1d(c), nn.ReLU()])
            c_in = c
        layers.append(nn.Linear(c_in, output_channels, bias=True))
        return nn.Sequential(*layers)

    def build_losses(self, losses_cfg):
        self.add_module('cls_loss_func', loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0))
        kind = _get(losses_cfg, 'LOSS_REG', None)
        if kind != 'WeightedSmoothL1Loss':
            raise NotImplementedError("PointHeadBox: LOSS_REG %r (this package has WeightedSmoothL1Loss)" % (kind,))
        self.reg_loss_func = loss_utils.WeightedSmoothL1Loss(
            code_weights=_get(_get(losses_cfg, 'LOSS_WEIGHTS'), 'code_weights', None))

    def assign_targets(self, input_dict):
        """input_dict: point_coords (B * N, 4) [bs_idx, x, y, z] stacked in sample order with equal sample sizes,
        gt_boxes (B, G, 8) with G >= 1 (a batch without any box is padded to one all-zero row; G = 0 raises Dfu3dError)
        -> {'point_cls_labels': int64 (B * N) -- the class of the first box that holds the point, -1
        inside an enlarged box only, 0 elsewhere --, 'point_box_labels': (B * N, 8), 'point_gt_idx': int32 (B * N)}."""
        if not self.trainable:
            raise NotImplementedError("PointHeadBox.assign_targets: " + TRAINING_ROW)
        coords, gt_boxes = input_dict['point_coords'], input_dict['gt_boxes']
        assert gt_boxes.dim() == 3 and coords.dim() == 2, (tuple(gt_boxes.shape), tuple(coords.shape))
        mean = None
        if getattr(self.box_coder, 'use_mean_size', False):
            if self.box_coder.mean_size.device != coords.device:
                self.box_coder.mean_size = self.box_coder.mean_size.to(coords.device)
            mean = self.box_coder.mean_size.contiguous()
        with torch.no_grad():
            cls, box, idx = rcnn_target_ops.point_targets(
                coords.detach().contiguous(), gt_boxes.detach().float().contiguous(),
                _get(_get(self.model_cfg, 'TARGET_CONFIG'), 'GT_EXTRA_WIDTH'), self.num_class, mean, return_idx=True)
        return {'point_cls_labels': cls, 'point_box_labels': box, 'point_gt_idx': idx, 'point_part_labels': None}

    def _need_targets(self, what):
        if not self.trainable:
            raise NotImplementedError("PointHeadBox.%s: %s" % (what, TRAINING_ROW))
        if not self.forward_ret_dict or 'point_cls_labels' not in self.forward_ret_dict:
            raise RuntimeError("PointHeadBox.%s: no targets -- run forward in training mode on a batch with gt_boxes first" % what)
        return self.forward_ret_dict

    def get_cls_layer_loss(self, tb_dict=None):
        """The focal loss of every point against its one-hot class, ignored points (-1) without weight, normalised by
        the number of positives -> (loss, tb_dict) with 0-dim tensors 'point_loss_cls' and 'point_pos_num'."""
        ret = self._need_targets('get_cls_layer_loss')
        labels = ret['point_cls_labels'].view(-1)
        preds = ret['point_cls_preds'].view(-1, self.num_class)
        n_pos = (labels > 0).sum().float()
        weights = (labels >= 0).float() / n_pos.clamp(min=1.0)             # 1 / n_pos for every point that is not ignored
        # column c - 1 is 1 for a point of class c; background and ignored points (clamped to 0) have an all-zero row
        one_hot = F.one_hot(labels.clamp(min=0), self.num_class + 1)[:, 1:].to(preds.dtype)
        loss = self.cls_loss_func(preds, one_hot, weights=weights).sum()
        loss = loss * _get(_get(self.model_cfg, 'LOSS_CONFIG'), 'LOSS_WEIGHTS')['point_cls_weight']
        tb_dict = {} if tb_dict is None else tb_dict
        tb_dict.update({'point_loss_cls': loss.detach(), 'point_pos_num': n_pos})
        return loss, tb_dict

    def get_box_layer_loss(self, tb_dict=None):
        """The code-weighted smooth L1 of the positives' box codes, normalised by their number -> (loss, tb_dict) with
        the 0-dim tensor 'point_loss_box'."""
        ret = self._need_targets('get_box_layer_loss')
        positive = ret['point_cls_labels'] > 0
        weights = positive.float() / positive.sum().float().clamp(min=1.0)
        loss = self.reg_loss_func(ret['point_box_preds'][None, ...], ret['point_box_labels'][None, ...],
                                  weights=weights[None, ...]).sum()
        loss = loss * _get(_get(self.model_cfg, 'LOSS_CONFIG'), 'LOSS_WEIGHTS')['point_box_weight']
        tb_dict = {} if tb_dict is None else tb_dict
        tb_dict.update({'point_loss_box': loss.detach()})
        return loss, tb_dict

    def get_loss(self, tb_dict=None, as_tensors=False):
        """-> (point_loss_cls + point_loss_box, tb_dict): 'point_loss_cls', 'point_pos_num', 'point_loss_box' as Python
        floats read with ONE copy, or with as_tensors=True as 0-dim device tensors without any synchronisation."""
        if not self.trainable:
            raise NotImplementedError("PointHeadBox.get_loss: " + TRAINING_ROW)
        tb_dict = {} if tb_dict is None else tb_dict
        loss_cls, own = self.get_cls_layer_loss()
        loss_box, own = self.get_box_layer_loss(own)
        tb_dict.update(own if as_tensors else host_values(own))
        return loss_cls + loss_box, tb_dict

    def generate_predicted_boxes(self, points, point_cls_preds, point_box_preds):
        """points (N, 3), point_cls_preds (N, num_class), point_box_preds (N, code_size) -> the scores as they are and
        the boxes (N, 7) decoded against the points and the mean size of the best class."""
        best = point_cls_preds.argmax(dim=-1) + 1                          # classes count from 1
        return point_cls_preds, self.box_coder.decode_torch(point_box_preds, points, best)

    def forward(self, batch_dict):
        """batch_dict: point_features (N1 + N2 + ..., C), point_coords (N1 + N2 + ..., 4) [bs_idx, x, y, z] ->
        point_cls_scores (N1 + N2 + ...), batch_cls_preds (., num_class), batch_box_preds (., 7), batch_index,
        cls_preds_normalized = False."""
        before_fusion = _get(self.model_cfg, 'USE_POINT_FEATURES_BEFORE_FUSION', False)
        features = batch_dict['point_features_before_fusion' if before_fusion else 'point_features']
        logits, codes = self.cls_layers(features), self.box_layers(features)
        self.forward_ret_dict = {'point_cls_preds': logits, 'point_box_preds': codes}
        batch_dict['point_cls_scores'] = logits.max(dim=-1)[0].sigmoid()
        if self.training and self.trainable:
            targets = self.assign_targets(batch_dict)
            self.forward_ret_dict.update(point_cls_labels=targets['point_cls_labels'],
                                         point_box_labels=targets['point_box_labels'])
        if self.training and not self.predict_boxes_when_training:
            if not self.trainable:
                self.assign_targets(batch_dict)                            # the training row is not built: raises
        else:
            coords = batch_dict['point_coords']
            _, boxes = self.generate_predicted_boxes(coords[:, 1:4], logits, codes)
            batch_dict.update(batch_cls_preds=logits, batch_box_preds=boxes, batch_index=coords[:, 0],
                              cls_preds_normalized=False)
        return batch_dict
