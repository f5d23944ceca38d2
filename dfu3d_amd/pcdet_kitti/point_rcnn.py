"""pcdet/models/detectors/point_rcnn.py (over detector3d_template.py) assembled from this package's modules:
`backbone_3d` (PointNet2MSG) -> `point_head` (PointHeadBox) -> `roi_head` (PointRCNNHead), with the reference's submodule
names and its `global_step` buffer, so a reference checkpoint's 'model_state' loads with strict=True.

The inference path: `forward(batch_dict)` in eval mode returns (pred_dicts, recall_dict).  `post_processing` handles the
whole batch in one chain -- sigmoid, a descending sort of every sample's scores, the count at or above SCORE_THRESH (a
prefix after the sort), ONE segmented rotated NMS (iou3d_nms_utils.nms_gpu_segments), one gather -- and reads the B
survivor counts from the device once.

Training is opt-in: `PointRCNN(..., trainable=True)` passes the keyword to both heads, which then build their loss
functions and the proposal target layer (no parameters, no buffers: the state dict and its order do not change, and a
checkpoint moves between a trainable and a default model with strict=True).  In training mode `forward` then returns
({'loss': loss}, tb_dict, disp_dict) as train_utils' model_func expects, `get_training_loss` being the point head's loss
plus the RoI head's with ONE copy to the host for the whole tb_dict (none with as_tensors=True).  Without the keyword
training raises NotImplementedError as before."""
import torch
import torch.nn as nn

from . import iou3d_nms_utils
from .centerpoint import CenterPoint, _Dataset, _get
from .point_head_box import TRAINING_ROW, PointHeadBox, host_values
from .pointnet2_backbone import PointNet2MSG
from .pointrcnn_head import PointRCNNHead

MODULES = {'BACKBONE_3D': {'PointNet2MSG': PointNet2MSG}, 'POINT_HEAD': {'PointHeadBox': PointHeadBox},
           'ROI_HEAD': {'PointRCNNHead': PointRCNNHead}}
ABSENT = ('VFE', 'MAP_TO_BEV', 'PFE', 'BACKBONE_2D', 'DENSE_HEAD')


def _module_class(model_cfg, section):
    cfg = _get(model_cfg, section, None)
    if cfg is None:
        raise NotImplementedError("PointRCNN: the config has no %s" % section)
    name = _get(cfg, 'NAME')
    if name not in MODULES[section]:
        raise NotImplementedError("PointRCNN: %s.NAME = %r is not part of this package (it has %s)"
                                  % (section, name, ", ".join(sorted(MODULES[section]))))
    return cfg, MODULES[section][name]


class PointRCNN(nn.Module):
    def __init__(self, model_cfg, num_class, dataset=None, trainable=False, batched_proposals=False, **kwargs):
        """dataset: an object with class_names and point_feature_encoder.num_point_features -- or the same as keywords
        (num_point_features for the last).  trainable: build the training half of both heads.  batched_proposals: the
        RoI head's proposal stage for the whole batch at once (PointRCNNHead.proposal_layer_batched)."""
        super().__init__()
        self.trainable = bool(trainable)
        self.batched_proposals = bool(batched_proposals)
        if dataset is None:
            feats = kwargs.pop('num_point_features')
            dataset = _Dataset(point_feature_encoder=_Dataset(num_point_features=feats), **kwargs)
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.dataset = dataset
        self.class_names = list(dataset.class_names)
        self.register_buffer('global_step', torch.LongTensor(1).zero_())
        absent = [s for s in ABSENT if _get(model_cfg, s, None)]
        if absent:
            raise NotImplementedError("PointRCNN: the config's %s is not part of this model" % ", ".join(absent))
        cfg, cls = _module_class(model_cfg, 'BACKBONE_3D')
        self.backbone_3d = cls(model_cfg=cfg, input_channels=dataset.point_feature_encoder.num_point_features)
        num_point_features = self.backbone_3d.num_point_features
        cfg, cls = _module_class(model_cfg, 'POINT_HEAD')
        if _get(cfg, 'USE_POINT_FEATURES_BEFORE_FUSION', False):
            raise NotImplementedError("PointRCNN: POINT_HEAD.USE_POINT_FEATURES_BEFORE_FUSION (the backbone has none)")
        self.point_head = cls(model_cfg=cfg, input_channels=num_point_features,
                              num_class=num_class if not _get(cfg, 'CLASS_AGNOSTIC', False) else 1,
                              predict_boxes_when_training=bool(_get(model_cfg, 'ROI_HEAD', False)),
                              trainable=self.trainable)
        cfg, cls = _module_class(model_cfg, 'ROI_HEAD')
        self.roi_head = cls(model_cfg=cfg, input_channels=num_point_features,
                            num_class=num_class if not _get(cfg, 'CLASS_AGNOSTIC', False) else 1, trainable=self.trainable,
                            batched_proposals=self.batched_proposals)
        self.module_list = [self.backbone_3d, self.point_head, self.roi_head]

    @property
    def mode(self):
        return 'TRAIN' if self.training else 'TEST'

    def update_global_step(self):
        self.global_step += 1

    def forward(self, batch_dict):
        if self.training and not self.trainable:
            raise NotImplementedError("PointRCNN.forward in training mode: " + TRAINING_ROW)
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self, as_tensors=False):
        """-> (loss_point + loss_rcnn, tb_dict, disp_dict): the tb_dict of both heads -- 'point_loss_cls',
        'point_pos_num', 'point_loss_box', 'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss' -- as Python
        floats read with one copy, or 0-dim device tensors with as_tensors=True."""
        if not self.trainable:
            raise NotImplementedError("PointRCNN.get_training_loss: " + TRAINING_ROW)
        loss_point, tb_dict = self.point_head.get_loss(as_tensors=True)
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict, as_tensors=True)
        return loss_point + loss_rcnn, (tb_dict if as_tensors else host_values(tb_dict)), {}

    def select_predictions(self, batch_dict):
        """The detector's post-processing without the recall record, for the whole batch in one chain: batch_box_preds
        (B, M, 7 + C), batch_cls_preds (B, M, 1 or num_class) -> the list of {'pred_boxes', 'pred_scores',
        'pred_labels'} per sample, views of padded (B, M, .) tensors cut after ONE host read of the B counts.  Equal
        scores keep their order of arrival (a stable sort); the reference leaves them to torch.topk.  A box with a NaN
        score is never selected."""
        cfg = _get(self.model_cfg, 'POST_PROCESSING')
        nms_cfg = _get(cfg, 'NMS_CONFIG')
        if _get(nms_cfg, 'MULTI_CLASSES_NMS'):
            raise NotImplementedError("PointRCNN.post_processing: MULTI_CLASSES_NMS")
        if _get(nms_cfg, 'NMS_TYPE') != 'nms_gpu':
            raise NotImplementedError("PointRCNN.post_processing: NMS_TYPE %r" % (_get(nms_cfg, 'NMS_TYPE'),))
        box_preds, src_cls_preds = batch_dict['batch_box_preds'], batch_dict['batch_cls_preds']
        if box_preds.dim() != 3 or isinstance(src_cls_preds, list):
            raise NotImplementedError("PointRCNN.post_processing: stacked or multi-head predictions")
        assert src_cls_preds.shape[2] in [1, self.num_class]
        cls_preds = src_cls_preds if batch_dict['cls_preds_normalized'] else torch.sigmoid(src_cls_preds)
        scores, label_preds = torch.max(cls_preds, dim=-1)                              # (B, M)
        if batch_dict.get('has_class_labels', False):
            label_preds = batch_dict['roi_labels' if 'roi_labels' in batch_dict else 'batch_pred_labels']
            label_preds = label_preds.view(scores.shape)
        else:
            label_preds = label_preds + 1
        # a NaN score sorts in front of every number and fails `>= SCORE_THRESH`: as -inf it sorts last and stays out,
        # as the reference's mask leaves it out, and the boxes at or above the threshold are a prefix again
        sorted_scores, order = torch.sort(scores.nan_to_num(nan=float('-inf')), dim=1, descending=True, stable=True)
        counts = (sorted_scores >= _get(cfg, 'SCORE_THRESH')).sum(dim=1).int()          # a prefix of every sorted row
        sorted_boxes = box_preds.gather(1, order[..., None].expand(-1, -1, box_preds.shape[-1])).float().contiguous()
        keep, num_keep = iou3d_nms_utils.nms_gpu_segments(
            sorted_boxes, counts, _get(nms_cfg, 'NMS_THRESH'), pre_maxsize=_get(nms_cfg, 'NMS_PRE_MAXSIZE'),
            post_max_size=_get(nms_cfg, 'NMS_POST_MAXSIZE'))
        pos = keep.clamp(min=0).long()                                                  # (B, M): sorted positions, then 0
        selected = order.gather(1, pos)
        final_boxes = sorted_boxes.gather(1, pos[..., None].expand(-1, -1, sorted_boxes.shape[-1]))
        if _get(cfg, 'OUTPUT_RAW_SCORE', False):
            final_scores = torch.max(src_cls_preds, dim=-1)[0].gather(1, selected)
        else:
            final_scores = sorted_scores.gather(1, pos)
        final_labels = label_preds.gather(1, selected)
        return [{'pred_boxes': final_boxes[k, :n], 'pred_scores': final_scores[k, :n], 'pred_labels': final_labels[k, :n]}
                for k, n in enumerate(num_keep.tolist())]                               # tolist: the chain's one host read

    def post_processing(self, batch_dict):
        cfg = _get(self.model_cfg, 'POST_PROCESSING')
        pred_dicts = self.select_predictions(batch_dict)
        recall_dict = {}
        for index in range(batch_dict['batch_size']):
            box_preds = pred_dicts[index]['pred_boxes'] if 'rois' not in batch_dict else batch_dict['batch_box_preds'][index]
            recall_dict = self.generate_recall_record(box_preds, recall_dict, index, data_dict=batch_dict,
                                                      thresh_list=_get(cfg, 'RECALL_THRESH_LIST'))
        return pred_dicts, recall_dict

    generate_recall_record = staticmethod(CenterPoint.generate_recall_record)
    load_params_from_file = CenterPoint.load_params_from_file
