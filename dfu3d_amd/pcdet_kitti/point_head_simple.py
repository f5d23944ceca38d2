"""pcdet/models/dense_heads/point_head_simple.py, the inference half: PV-RCNN's keypoint segmentation head with the
reference's state-dict keys (cls_layers.*).  `forward` writes `point_cls_scores` (the sigmoid's class maximum) and keeps
`point_cls_preds` in forward_ret_dict.  Target assignment and the loss are not part of this package: forward in training
mode raises NotImplementedError."""
import torch
import torch.nn as nn

from .common_utils import cfg_get


class PointHeadSimple(nn.Module):
    def __init__(self, num_class, input_channels, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg, self.num_class, self.forward_ret_dict = model_cfg, num_class, None
        self.cls_layers = self.make_fc_layers(fc_cfg=cfg_get(model_cfg, 'CLS_FC'), input_channels=input_channels,
                                              output_channels=num_class)

    @staticmethod
    def make_fc_layers(fc_cfg, input_channels, output_channels):
        layers, c_in = [], input_channels
        for c in fc_cfg:
            layers += [nn.Linear(c_in, c, bias=False), nn.BatchNorm1d(c), nn.ReLU()]
            c_in = c
        return nn.Sequential(*layers, nn.Linear(c_in, output_channels, bias=True))

    def forward(self, batch_dict):
        """point_features(_before_fusion) (N, C) -> batch_dict['point_cls_scores'] (N)."""
        if self.training:
            raise NotImplementedError("PointHeadSimple.forward in training mode: target assignment and the loss of "
                                      "PV-RCNN are not part of this package")
        before = cfg_get(self.model_cfg, 'USE_POINT_FEATURES_BEFORE_FUSION', False)
        point_cls_preds = self.cls_layers(batch_dict['point_features_before_fusion' if before else 'point_features'])
        batch_dict['point_cls_scores'], _ = torch.sigmoid(point_cls_preds).max(dim=-1)
        self.forward_ret_dict = {'point_cls_preds': point_cls_preds}
        return batch_dict
