"""pcdet/models/detectors/second_net.py (over detector3d_template.py): the voxel assembly of
`CenterPoint(..., sparse_3d=True)` -- `vfe` (MeanVFE) -> `backbone_3d` (VoxelBackBone8x) -> `map_to_bev_module`
(HeightCompression) -> `backbone_2d` (BaseBEVBackbone) -> `dense_head` -- with AnchorHeadSingle as the dense head.  The
assembly, the checkpoint loading and the recall record are CenterPoint's own code; the submodule names and `global_step`
are the reference's, so a reference checkpoint's 'model_state' loads with strict=True after adapt_spconv_weights.

`forward(batch_dict)` in training returns ({'loss': loss}, tb_dict, disp_dict); in evaluation (pred_dicts, recall_dict)
through the template's post_processing of `batch_cls_preds` / `batch_box_preds`: sigmoid, the class maximum (or
MULTI_CLASSES_NMS), class_agnostic_nms with SCORE_THRESH, the recall record.  Evaluation is per-sample torch on the
existing NMS: NMS_PRE_MAXSIZE: 4096 over 211 200 anchors is beyond the batched proposal stage."""
import torch

from . import model_nms_utils
from .anchor_head_single import AnchorHeadSingle
from .centerpoint import CenterPoint, _get


class SECONDNet(CenterPoint):
    MORE_MODULES = {'DENSE_HEAD': {'AnchorHeadSingle': AnchorHeadSingle}}

    def __init__(self, model_cfg, num_class, dataset=None, **kwargs):
        kwargs.pop('sparse_3d', None)
        super().__init__(model_cfg, num_class, dataset=dataset, sparse_3d=True, **kwargs)

    def post_processing(self, batch_dict):
        cfg = _get(self.model_cfg, 'POST_PROCESSING')
        nms_cfg = _get(cfg, 'NMS_CONFIG')
        score_thresh = _get(cfg, 'SCORE_THRESH')
        recall_dict, pred_dicts = {}, []
        for index in range(batch_dict['batch_size']):
            assert batch_dict['batch_box_preds'].dim() == 3
            box_preds = batch_dict['batch_box_preds'][index]
            src_cls_preds = batch_dict['batch_cls_preds'][index]
            assert src_cls_preds.shape[1] in [1, self.num_class]
            cls_preds = src_cls_preds if batch_dict['cls_preds_normalized'] else torch.sigmoid(src_cls_preds)
            if _get(nms_cfg, 'MULTI_CLASSES_NMS'):
                mapping = torch.arange(1, self.num_class, device=cls_preds.device)
                assert cls_preds.shape[1] == len(mapping)
                final_scores, labels, final_boxes = model_nms_utils.multi_classes_nms(
                    cls_scores=cls_preds, box_preds=box_preds, nms_config=nms_cfg, score_thresh=score_thresh)
                final_labels = mapping[labels]
            else:
                cls_preds, label_preds = torch.max(cls_preds, dim=-1)
                label_preds = label_preds + 1
                selected, final_scores = model_nms_utils.class_agnostic_nms(
                    box_scores=cls_preds, box_preds=box_preds, nms_config=nms_cfg, score_thresh=score_thresh)
                if _get(cfg, 'OUTPUT_RAW_SCORE', False):
                    final_scores = torch.max(src_cls_preds, dim=-1)[0][selected]
                final_labels = label_preds[selected]
                final_boxes = box_preds[selected]
            recall_dict = self.generate_recall_record(final_boxes, recall_dict, index, data_dict=batch_dict,
                                                      thresh_list=_get(cfg, 'RECALL_THRESH_LIST'))
            pred_dicts.append({'pred_boxes': final_boxes, 'pred_scores': final_scores, 'pred_labels': final_labels})
        return pred_dicts, recall_dict
