"""The network half of pcdet/models/dense_heads/center_head.py: SeparateHead and CenterHeadModule (the reference's
CenterHead as an nn.Module) with its constructor arguments, state-dict keys (shared_conv.*, heads_list.i.<name>.*) and
initialisation -- the last 'hm' bias -2.19, Kaiming-normal weights and zero biases in the other branches, BN_EPS / BN_MOM,
USE_BIAS_BEFORE_NORM.  The geometry is the existing center_head.CenterHead, built on the input's device at the first
forward (the constructor creates no device tensor, so the module can be built without a GPU).

`forward(data_dict)`: the convolutions; in training `assign_targets` on data_dict['gt_boxes']; outside training, or with
predict_boxes_when_training, the boxes through `generate_predicted_boxes_batched` (`generate_predicted_boxes` for the
options the batched form rejects).  `get_loss()` is the fused loss on the RAW 'hm' logits: the reference's in-place
clamped sigmoid is part of the loss kernel, and forward_ret_dict['pred_dicts'] stays what the convolutions gave."""
import copy

import torch
import torch.nn as nn

from . import center_head


_get = center_head._get


class SeparateHead(nn.Module):
    def __init__(self, input_channels, sep_head_dict, init_bias=-2.19, use_bias=False, norm_func=None):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        norm_func = nn.BatchNorm2d if norm_func is None else norm_func
        for cur_name, cur in self.sep_head_dict.items():
            layers = [nn.Sequential(nn.Conv2d(input_channels, input_channels, 3, stride=1, padding=1, bias=use_bias),
                                    norm_func(input_channels), nn.ReLU())
                      for _ in range(_get(cur, 'num_conv') - 1)]
            layers.append(nn.Conv2d(input_channels, _get(cur, 'out_channels'), 3, stride=1, padding=1, bias=True))
            fc = nn.Sequential(*layers)
            if 'hm' in cur_name:
                fc[-1].bias.data.fill_(init_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, nn.Conv2d):
                        nn.init.kaiming_normal_(m.weight.data)
                        if m.bias is not None:
                            nn.init.constant_(m.bias, 0)
            setattr(self, cur_name, fc)

    def forward(self, x):
        return {cur_name: getattr(self, cur_name)(x) for cur_name in self.sep_head_dict}


class CenterHeadModule(nn.Module):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=True):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.grid_size = grid_size
        self.point_cloud_range = point_cloud_range
        self.voxel_size = voxel_size
        self.class_names = list(class_names)
        self.feature_map_stride = _get(_get(model_cfg, 'TARGET_ASSIGNER_CONFIG'), 'FEATURE_MAP_STRIDE', None)
        self.class_names_each_head = [[x for x in names if x in self.class_names]
                                      for names in _get(model_cfg, 'CLASS_NAMES_EACH_HEAD')]
        total = sum(len(x) for x in self.class_names_each_head)
        assert total == len(self.class_names), 'class_names_each_head=%s' % (self.class_names_each_head,)
        eps, mom = _get(model_cfg, 'BN_EPS', 1e-5), _get(model_cfg, 'BN_MOM', 0.1)
        use_bias = _get(model_cfg, 'USE_BIAS_BEFORE_NORM', False)

        def norm_func(channels):
            return nn.BatchNorm2d(channels, eps=eps, momentum=mom)
        shared = _get(model_cfg, 'SHARED_CONV_CHANNEL')
        self.shared_conv = nn.Sequential(nn.Conv2d(input_channels, shared, 3, stride=1, padding=1, bias=use_bias),
                                         norm_func(shared), nn.ReLU())
        self.heads_list = nn.ModuleList()
        self.separate_head_cfg = _get(model_cfg, 'SEPARATE_HEAD_CFG')
        branches = _get(self.separate_head_cfg, 'HEAD_DICT')
        branches = branches if isinstance(branches, dict) else vars(branches)
        for names in self.class_names_each_head:
            head_dict = {k: dict(out_channels=_get(v, 'out_channels'), num_conv=_get(v, 'num_conv'))
                         for k, v in copy.deepcopy(dict(branches)).items()}
            head_dict['hm'] = dict(out_channels=len(names), num_conv=_get(model_cfg, 'NUM_HM_CONV'))
            self.heads_list.append(SeparateHead(shared, head_dict, init_bias=-2.19, use_bias=use_bias, norm_func=norm_func))
        self.predict_boxes_when_training = predict_boxes_when_training
        self.forward_ret_dict = {}
        self._geometry = None

    def geometry(self, device):
        """The box geometry (center_head.CenterHead) on `device`; made at the first call and again if the device changes."""
        device = torch.device(device)
        if self._geometry is None or self._geometry.device != device:
            self._geometry = center_head.CenterHead(self.model_cfg, self.class_names, self.point_cloud_range,
                                                    self.voxel_size, device=device)
        return self._geometry

    @property
    def status(self):
        return None if self._geometry is None else self._geometry.status

    def check_status(self):
        if self._geometry is not None:
            self._geometry.check_status()

    def assign_targets(self, gt_boxes, feature_map_size=None, **kwargs):
        return self.geometry(gt_boxes.device).assign_targets(gt_boxes, feature_map_size=feature_map_size, **kwargs)

    def get_loss(self, as_tensors=False):
        pred_dicts = self.forward_ret_dict['pred_dicts']
        geom = self.geometry(pred_dicts[0]['hm'].device)
        return geom.get_loss(pred_dicts, self.forward_ret_dict['target_dicts'], as_tensors=as_tensors)

    def generate_predicted_boxes(self, batch_size, pred_dicts):
        geom = self.geometry(pred_dicts[0]['hm'].device)
        try:
            return geom.generate_predicted_boxes_batched(batch_size, pred_dicts)
        except NotImplementedError:                      # class_specific_nms, circle_nms, IoU rectification, an 'iou' head
            return geom.generate_predicted_boxes(batch_size, pred_dicts)

    @staticmethod
    def reorder_rois_for_refining(batch_size, pred_dicts):
        num_max_rois = max(1, max(len(d['pred_boxes']) for d in pred_dicts))     # one faked roi at least
        pred_boxes = pred_dicts[0]['pred_boxes']
        rois = pred_boxes.new_zeros((batch_size, num_max_rois, pred_boxes.shape[-1]))
        roi_scores = pred_boxes.new_zeros((batch_size, num_max_rois))
        roi_labels = pred_boxes.new_zeros((batch_size, num_max_rois)).long()
        for b, d in enumerate(pred_dicts):
            n = len(d['pred_boxes'])
            rois[b, :n] = d['pred_boxes']
            roi_scores[b, :n] = d['pred_scores']
            roi_labels[b, :n] = d['pred_labels']
        return rois, roi_scores, roi_labels

    def forward(self, data_dict):
        spatial_features_2d = data_dict['spatial_features_2d']
        x = self.shared_conv(spatial_features_2d)
        pred_dicts = [head(x) for head in self.heads_list]
        if self.training:
            self.forward_ret_dict['target_dicts'] = self.assign_targets(
                data_dict['gt_boxes'], feature_map_size=spatial_features_2d.size()[2:])
        self.forward_ret_dict['pred_dicts'] = pred_dicts
        if not self.training or self.predict_boxes_when_training:
            with torch.no_grad():
                boxes = self.generate_predicted_boxes(data_dict['batch_size'],
                                                      [{k: v.detach() for k, v in d.items()} for d in pred_dicts])
            data_dict['final_box_dicts'] = boxes
            if self.predict_boxes_when_training:         # a second stage reads these (the reference sets only these then)
                rois, roi_scores, roi_labels = self.reorder_rois_for_refining(data_dict['batch_size'], boxes)
                data_dict.update(rois=rois, roi_scores=roi_scores, roi_labels=roi_labels, has_class_labels=True)
        return data_dict
