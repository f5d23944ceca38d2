"""The box geometry of pcdet/models/dense_heads/center_head.py as a plain object (the network stays the reference's):
`assign_targets` and `generate_predicted_boxes` with the reference's arguments and returns, on
csrc/centerhead_stage.hip (dfu3d_center_assign / dfu3d_center_decode).

`assign_targets` launches one chain for all heads and samples and neither synchronises nor copies to the host.  More
than NUM_MAX_OBJS boxes of one head in one sample (where the reference raises) set a bit in `self.status`, a device
int32 the call resets: `assign_targets(..., check=True)` reads it and raises, otherwise `check_status()` does at the
caller's next natural synchronisation.

`generate_predicted_boxes_batched` is the inference end for a whole batch on csrc/postproc_stage.hip: the decode of
every head into one block, one segmented NMS and one gather, with one host read (none with as_padded=True).

`get_loss` is the reference's (center_head.py:229-295) on csrc/centerloss_stage.hip through
dfu3d_amd.center_loss_ops: all heads in three launches forward and two backward, no float atomics, and one
device-to-host copy for the tb_dict (none with as_tensors=True).

Divergences from the reference: `pred_dict['hm']` holds raw logits and `get_loss` does not overwrite it (the reference
replaces it by the clamped sigmoid); a masked-out slot contributes nothing to loss or gradient even where the
prediction at its cell is not finite (the reference multiplies by the mask and gives NaN), and the same holds for a NaN
target channel, which is skipped (the reference's `isnotnan` multiplies NaN by zero); the IoU branches raise
NotImplementedError; `gt_boxes` is not written (the reference leaves head-local class ids in its last column) and
boxes are assigned by the caller's original class ids."""
import numpy as np
import torch

from . import centernet_utils, model_nms_utils
from .. import center_loss_ops, stages
from .._lib import Dfu3dError


def _get(cfg, key, *default):
    if isinstance(cfg, dict):
        return cfg[key] if not default else cfg.get(key, default[0])
    return getattr(cfg, key) if not default else getattr(cfg, key, default[0])


class CenterHead:
    def __init__(self, model_cfg, class_names, point_cloud_range, voxel_size, device='cuda'):
        self.model_cfg = model_cfg
        self.class_names = list(class_names)
        self.point_cloud_range = point_cloud_range
        self.voxel_size = voxel_size
        self.device = torch.device(device)
        self.feature_map_stride = _get(_get(model_cfg, 'TARGET_ASSIGNER_CONFIG'), 'FEATURE_MAP_STRIDE', None)
        self.class_names_each_head = []
        self.class_id_mapping_each_head = []
        for cur_class_names in _get(model_cfg, 'CLASS_NAMES_EACH_HEAD'):
            names = [x for x in cur_class_names if x in self.class_names]
            self.class_names_each_head.append(names)
            self.class_id_mapping_each_head.append(
                torch.tensor([self.class_names.index(x) for x in names], dtype=torch.int64, device=self.device))
        total = sum(len(x) for x in self.class_names_each_head)
        assert total == len(self.class_names), 'class_names_each_head=%s' % (self.class_names_each_head,)
        tab = -np.ones((len(self.class_names) + 1, 2), np.int32)
        plane = [0]
        for h, names in enumerate(self.class_names_each_head):
            for j, n in enumerate(names):
                tab[self.class_names.index(n) + 1] = (h, j)
            plane.append(plane[-1] + len(names))
        self.head_plane = plane
        self._cls_tab = torch.from_numpy(tab).to(self.device)
        self._head_plane = torch.tensor(plane, dtype=torch.int32, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        # class id within a head -> 0-based id over class_names (generate_predicted_boxes_batched); unused slots 0
        post_map = np.zeros((len(self.class_names_each_head), max(1, max(len(x) for x in self.class_names_each_head))), np.int32)
        for h, names in enumerate(self.class_names_each_head):
            post_map[h, :len(names)] = [self.class_names.index(x) for x in names]
        self._post_cls_map = torch.from_numpy(post_map).to(self.device)
        self._post_limit = (None, None)
        head_cfg = _get(model_cfg, 'SEPARATE_HEAD_CFG', None)
        self.head_order = list(_get(head_cfg, 'HEAD_ORDER')) if head_cfg is not None else ['center', 'center_z', 'dim', 'rot']
        self.forward_ret_dict = {}

    def check_status(self):
        """Raise if the last assign_targets met more than NUM_MAX_OBJS boxes of one head in one sample (one host read)."""
        s = int(self.status.item())
        if s & stages.ST_CENTER_OVERFLOW:
            raise Dfu3dError("assign_targets: more than NUM_MAX_OBJS = %d boxes of one head in one sample"
                             % _get(_get(self.model_cfg, 'TARGET_ASSIGNER_CONFIG'), 'NUM_MAX_OBJS'))
        if s:
            raise Dfu3dError("assign_targets: status %d (%s)" % (s, stages.status_message(s)))

    def assign_targets(self, gt_boxes, feature_map_size=None, check=False, **kwargs):
        """gt_boxes (B, M, C) float32 on the device, feature_map_size [H, W] -> the reference's ret_dict: per head
        'heatmaps' (B, n_cls_head, H, W), 'target_boxes' (B, NUM_MAX_OBJS, C), 'inds', 'masks' (int64),
        'target_boxes_src'; 'heatmap_masks' stays an empty list."""
        cfg = _get(self.model_cfg, 'TARGET_ASSIGNER_CONFIG')
        H, W = int(feature_map_size[0]), int(feature_map_size[1])
        if gt_boxes.dtype != torch.float32:
            raise Dfu3dError("assign_targets: gt_boxes must be float32, got %s" % gt_boxes.dtype)
        gt_boxes = gt_boxes.contiguous()
        B = gt_boxes.shape[0]
        n_cls, n_heads = len(self.class_names), len(self.class_names_each_head)
        self.status.zero_()
        f = centernet_utils._f32
        heat, tgt, inds, masks, src = stages.center_assign(
            gt_boxes, self._cls_tab, self._head_plane, n_cls, n_heads, W, H,
            (f(self.point_cloud_range[0]), f(self.point_cloud_range[1])), (f(self.voxel_size[0]), f(self.voxel_size[1])),
            _get(cfg, 'FEATURE_MAP_STRIDE'), _get(cfg, 'NUM_MAX_OBJS'), _get(cfg, 'GAUSSIAN_OVERLAP'),
            _get(cfg, 'MIN_RADIUS'), self.status)
        ret_dict = {'heatmaps': [], 'target_boxes': [], 'inds': [], 'masks': [], 'heatmap_masks': [],
                    'target_boxes_src': []}
        hw = H * W
        for h in range(n_heads):
            p0, p1 = self.head_plane[h], self.head_plane[h + 1]
            ret_dict['heatmaps'].append(heat[B * p0 * hw:B * p1 * hw].view(B, p1 - p0, H, W))
            ret_dict['target_boxes'].append(tgt[h])
            ret_dict['inds'].append(inds[h])
            ret_dict['masks'].append(masks[h])
            ret_dict['target_boxes_src'].append(src[h])
        if check:
            self.check_status()
        return ret_dict

    def generate_predicted_boxes(self, batch_size, pred_dicts):
        """center_head.py:297-364: per head sigmoid / exp, the decode kernel, class mapping, optional IoU rectification,
        NMS; heads concatenated per sample, labels + 1."""
        post_process_cfg = _get(self.model_cfg, 'POST_PROCESSING')
        nms_cfg = _get(post_process_cfg, 'NMS_CONFIG')
        nms_type = _get(nms_cfg, 'NMS_TYPE')
        limit = torch.tensor(_get(post_process_cfg, 'POST_CENTER_LIMIT_RANGE'), dtype=torch.float32, device=self.device)
        ret_dict = [{'pred_boxes': [], 'pred_scores': [], 'pred_labels': []} for _ in range(batch_size)]
        for idx, pred_dict in enumerate(pred_dicts):
            final_pred_dicts = centernet_utils.decode_bbox_from_heatmap(
                heatmap=pred_dict['hm'].sigmoid(), rot_cos=pred_dict['rot'][:, 0].unsqueeze(dim=1),
                rot_sin=pred_dict['rot'][:, 1].unsqueeze(dim=1), center=pred_dict['center'],
                center_z=pred_dict['center_z'], dim=pred_dict['dim'].exp(),
                vel=pred_dict['vel'] if 'vel' in self.head_order else None,
                iou=(pred_dict['iou'] + 1) * 0.5 if 'iou' in pred_dict else None,
                point_cloud_range=self.point_cloud_range, voxel_size=self.voxel_size,
                feature_map_stride=self.feature_map_stride, K=_get(post_process_cfg, 'MAX_OBJ_PER_SAMPLE'),
                circle_nms=(nms_type == 'circle_nms'), score_thresh=_get(post_process_cfg, 'SCORE_THRESH'),
                post_center_limit_range=limit)
            for k, final_dict in enumerate(final_pred_dicts):
                final_dict['pred_labels'] = self.class_id_mapping_each_head[idx][final_dict['pred_labels'].long()]
                if _get(post_process_cfg, 'USE_IOU_TO_RECTIFY_SCORE', False) and 'pred_iou' in final_dict:
                    pred_iou = torch.clamp(final_dict['pred_iou'], min=0, max=1.0)
                    rect = final_dict['pred_scores'].new_tensor(_get(post_process_cfg, 'IOU_RECTIFIER'))
                    final_dict['pred_scores'] = torch.pow(final_dict['pred_scores'], 1 - rect[final_dict['pred_labels']]) \
                        * torch.pow(pred_iou, rect[final_dict['pred_labels']])
                if nms_type == 'class_specific_nms':
                    selected, selected_scores = model_nms_utils.class_specific_nms(
                        box_scores=final_dict['pred_scores'], box_preds=final_dict['pred_boxes'],
                        box_labels=final_dict['pred_labels'], nms_config=nms_cfg,
                        score_thresh=_get(nms_cfg, 'SCORE_THRESH', None))
                else:
                    selected, selected_scores = model_nms_utils.class_agnostic_nms(
                        box_scores=final_dict['pred_scores'], box_preds=final_dict['pred_boxes'], nms_config=nms_cfg,
                        score_thresh=None)
                ret_dict[k]['pred_boxes'].append(final_dict['pred_boxes'][selected])
                ret_dict[k]['pred_scores'].append(selected_scores)
                ret_dict[k]['pred_labels'].append(final_dict['pred_labels'][selected])
        for k in range(batch_size):
            ret_dict[k]['pred_boxes'] = torch.cat(ret_dict[k]['pred_boxes'], dim=0)
            ret_dict[k]['pred_scores'] = torch.cat(ret_dict[k]['pred_scores'], dim=0)
            ret_dict[k]['pred_labels'] = torch.cat(ret_dict[k]['pred_labels'], dim=0) + 1
        return ret_dict

    def generate_predicted_boxes_batched(self, batch_size, pred_dicts, as_padded=False):
        """`generate_predicted_boxes` for all heads and samples in one launch chain: per head the sigmoid / exp and the
        decode kernel writing into one (n_heads, B, K, C) block, then ONE segmented NMS over the n_heads * B row lists
        (stages.nms_bev_segments: the decode's rows are in descending score order already, nothing is sorted again) and
        ONE gather of the survivors (stages.center_collect).  Returns the list `generate_predicted_boxes` returns -- views
        of the padded tensors cut after one host read of the B row counts -- or, with as_padded=True, the dict
        {'pred_boxes' (B, out_cap, C), 'pred_scores', 'pred_labels' (B, out_cap), 'count' int32 (B)} without any
        synchronisation; rows at or beyond count[b] are 0.  Where scores tie, the decode's order (ascending flat index)
        decides; `generate_predicted_boxes` leaves ties to torch.topk / argsort.  class_specific_nms, circle_nms, IoU
        rectification and an 'iou' head raise NotImplementedError: `generate_predicted_boxes` is the path for them."""
        post_process_cfg = _get(self.model_cfg, 'POST_PROCESSING')
        nms_cfg = _get(post_process_cfg, 'NMS_CONFIG')
        nms_type = _get(nms_cfg, 'NMS_TYPE')
        if nms_type not in ('nms_gpu', 'nms_normal_gpu'):
            raise NotImplementedError("generate_predicted_boxes_batched: NMS_TYPE %r (use generate_predicted_boxes)" % (nms_type,))
        if _get(post_process_cfg, 'USE_IOU_TO_RECTIFY_SCORE', False):
            raise NotImplementedError("generate_predicted_boxes_batched: USE_IOU_TO_RECTIFY_SCORE reorders the scores "
                                      "after the decode (use generate_predicted_boxes)")
        if any('iou' in d for d in pred_dicts):
            raise NotImplementedError("generate_predicted_boxes_batched: an 'iou' head (use generate_predicted_boxes)")
        K = _get(post_process_cfg, 'MAX_OBJ_PER_SAMPLE')
        if isinstance(K, (list, tuple)):
            if len(set(int(k) for k in K)) != 1:
                raise NotImplementedError("generate_predicted_boxes_batched: heads with different MAX_OBJ_PER_SAMPLE %s "
                                          "(use generate_predicted_boxes)" % (list(K),))
            K = K[0]
        K = int(K)
        n_heads, B = len(pred_dicts), int(batch_size)
        if n_heads != len(self.class_names_each_head):
            raise Dfu3dError("generate_predicted_boxes_batched: %d pred_dicts for %d heads"
                             % (n_heads, len(self.class_names_each_head)))
        if any(int(d['hm'].shape[0]) != B for d in pred_dicts):
            raise Dfu3dError("generate_predicted_boxes_batched: a heat map's batch differs from batch_size = %d" % B)
        with_vel = 'vel' in self.head_order
        nb = 9 if with_vel else 7
        dev = pred_dicts[0]['hm'].device
        limit_key = (tuple(float(v) for v in _get(post_process_cfg, 'POST_CENTER_LIMIT_RANGE')), dev)
        if self._post_limit[0] != limit_key:                # a host-to-device copy synchronises: once per range, not per call
            self._post_limit = (limit_key, torch.tensor(limit_key[0], dtype=torch.float32, device=dev))
        limit = self._post_limit[1]
        boxes = torch.empty((n_heads, B, K, nb), dtype=torch.float32, device=dev)
        scores = torch.empty((n_heads, B, K), dtype=torch.float32, device=dev)
        labels = torch.empty((n_heads, B, K), dtype=torch.int32, device=dev)
        count = torch.empty((n_heads, B), dtype=torch.int32, device=dev)
        for idx, pred_dict in enumerate(pred_dicts):
            centernet_utils.decode_raw(
                heatmap=pred_dict['hm'].sigmoid(), rot_cos=pred_dict['rot'][:, 0].unsqueeze(dim=1),
                rot_sin=pred_dict['rot'][:, 1].unsqueeze(dim=1), center=pred_dict['center'],
                center_z=pred_dict['center_z'], dim=pred_dict['dim'].exp(), vel=pred_dict['vel'] if with_vel else None,
                point_cloud_range=self.point_cloud_range, voxel_size=self.voxel_size,
                feature_map_stride=self.feature_map_stride, K=K, score_thresh=_get(post_process_cfg, 'SCORE_THRESH'),
                post_center_limit_range=limit, out=(boxes[idx], scores[idx], labels[idx], None, count[idx]))
        post_max = int(_get(nms_cfg, 'NMS_POST_MAXSIZE'))
        keep, num_keep = stages.nms_bev_segments(
            boxes.view(n_heads * B, K, nb), count.view(-1), float(_get(nms_cfg, 'NMS_THRESH')),
            pre_max=int(_get(nms_cfg, 'NMS_PRE_MAXSIZE')), post_max=post_max, normal=(nms_type == 'nms_normal_gpu'))
        out_cap = n_heads * (min(K, post_max) if post_max > 0 else K)
        out_boxes, out_scores, out_labels, out_count = stages.center_collect(
            boxes, scores, labels, keep, num_keep, self._post_cls_map, out_cap)
        if as_padded:
            return {'pred_boxes': out_boxes, 'pred_scores': out_scores, 'pred_labels': out_labels, 'count': out_count}
        return [{'pred_boxes': out_boxes[k, :n], 'pred_scores': out_scores[k, :n], 'pred_labels': out_labels[k, :n]}
                for k, n in enumerate(out_count.tolist())]          # tolist: the call's one copy to the host

    def get_loss(self, pred_dicts=None, target_dicts=None, as_tensors=False):
        """center_head.py:229-295.  pred_dicts: per head {'hm': logits (B, n_cls, H, W), HEAD_ORDER's maps}; target_dicts:
        what assign_targets returns; both default to self.forward_ret_dict's.  Returns (loss, tb_dict): loss a
        differentiable 0-dim tensor, tb_dict with 'hm_loss_head_%d', 'loc_loss_head_%d' and 'rpn_loss' as Python floats
        read with one copy, or, with as_tensors=True, as 0-dim views of the device vector without any synchronisation."""
        pred_dicts = self.forward_ret_dict['pred_dicts'] if pred_dicts is None else pred_dicts
        target_dicts = self.forward_ret_dict['target_dicts'] if target_dicts is None else target_dicts
        if _get(self.model_cfg, 'IOU_REG_LOSS', False) or any('iou' in d for d in pred_dicts):
            raise NotImplementedError("CenterHead.get_loss: the IoU branches ('iou' head, IOU_REG_LOSS) are not supported")
        weights = _get(_get(self.model_cfg, 'LOSS_CONFIG'), 'LOSS_WEIGHTS')
        losses, _ = center_loss_ops.center_loss(
            [d['hm'] for d in pred_dicts], target_dicts['heatmaps'], [[d[name] for name in self.head_order] for d in pred_dicts],
            target_dicts['target_boxes'], target_dicts['inds'], target_dicts['masks'], cls_weight=weights['cls_weight'],
            loc_weight=weights['loc_weight'], code_weights=list(weights['code_weights']))
        values = losses.detach() if as_tensors else losses.tolist()          # tolist: the call's one copy to the host
        tb_dict = {}
        for idx in range(len(pred_dicts)):
            tb_dict['hm_loss_head_%d' % idx] = values[2 * idx]
            tb_dict['loc_loss_head_%d' % idx] = values[2 * idx + 1]
        tb_dict['rpn_loss'] = values[-1]
        return losses[-1], tb_dict
