"""PointHeadBox, the first stage of PointRCNN (pcdet/models/dense_heads/point_head_box.py over point_head_template.py):
per point a class score and a box against the point and the mean size of the predicted class, with the reference's
state-dict keys (cls_layers.*, box_layers.*).  The inference half: forward in eval mode, and in training mode without
targets when predict_boxes_when_training is set.  Target assignment and the losses are the training row
(not built) and raise NotImplementedError."""
import torch
import torch.nn as nn

from . import box_coder_utils
from .base_bev_backbone import _get

TRAINING_ROW = "the PointRCNN training row (assign_targets, ProposalTargetLayer, the heads' losses) is not built"


class PointHeadBox(nn.Module):
    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.predict_boxes_when_training = predict_boxes_when_training
        self.forward_ret_dict = None
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

    def assign_targets(self, input_dict):
        raise NotImplementedError("PointHeadBox.assign_targets: " + TRAINING_ROW)

    def get_loss(self, tb_dict=None):
        raise NotImplementedError("PointHeadBox.get_loss: " + TRAINING_ROW)

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
        if self.training and not self.predict_boxes_when_training:
            self.assign_targets(batch_dict)                                # the training row: raises
        else:
            coords = batch_dict['point_coords']
            _, boxes = self.generate_predicted_boxes(coords[:, 1:4], logits, codes)
            batch_dict.update(batch_cls_preds=logits, batch_box_preds=boxes, batch_index=coords[:, 0],
                              cls_preds_normalized=False)
        return batch_dict
