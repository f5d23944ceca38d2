"""PointRCNN's target assignment on csrc/rcnntarget_stage.hip (C ABI: include/dfu3d_tgt.h), one launch per op for the
whole batch.

point_targets     PointHeadBox.assign_targets: stacked point_coords (B * N, 4) or points (B, N, 3), gt_boxes (B, G, 8) ->
                  point_cls_labels int64 (B * N), point_box_labels (B * N, 8) [, point_gt_idx int32 (B * N)].
roi_max_iou       get_max_iou_with_same_class / boxes_iou3d_gpu + max: rois (B, M, 7 + .), roi_labels (B, M), gt_boxes ->
                  max_overlaps (B, M), gt_assignment int32 (B, M).
roi_subsample     subsample_rois + sample_bg_inds from the caller's random numbers -> sampled_inds int32 (B, R).
proposal_targets  ProposalTargetLayer.forward: the two ops above, the draws on the device, the gathers and the labels.

float32 and contiguous, anything else raises Dfu3dError.  Every element of the outputs is written by the kernels
(torch.empty here).  Nothing in this module reads from the device: roi_subsample ORs into a status word the caller owns
and reads when it chooses (check_status)."""
import ctypes

import numpy as np
import torch

from . import _lib_tgt
from ._lib import Dfu3dError
from .roipoint_ops import _boxes7, _p, _stream, _want, extra_width

K = _lib_tgt.CONSTANTS
MAX_ROIS = K["DFU3D_TGT_MAX_ROIS"]
MAX_SAMPLED = K["DFU3D_TGT_MAX_SAMPLED"]
MAX_CLASSES = K["DFU3D_TGT_MAX_CLASSES"]
POINT_LAUNCHES = K["DFU3D_TGT_POINT_LAUNCHES"]
IOU_LAUNCHES = K["DFU3D_TGT_IOU_LAUNCHES"]
SAMPLE_LAUNCHES = K["DFU3D_TGT_SAMPLE_LAUNCHES"]
STATUS_NO_ROI = K["DFU3D_TGT_STATUS_NO_ROI"]


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


def _gt8(gt_boxes, what, B, dev):
    _want(gt_boxes, what, (B, None, 8), dev)
    if gt_boxes.shape[1] == 0:
        raise Dfu3dError("%s holds no row (pad the batch to one row at least)" % what)
    return gt_boxes


def point_targets(point_coords, gt_boxes, extra_width_xyz, num_class, mean_size=None, return_idx=False):
    """point_coords (B * N, 4) [sample, x, y, z] stacked in sample order with equal sample sizes (the sample column is not
    read) or points (B, N, 3); gt_boxes (B, G, 8), not written; mean_size (K, 3) float32 on the device or None
    (use_mean_size=False) -> point_cls_labels int64 (B * N), point_box_labels float32 (B * N, 8) [, point_gt_idx int32]."""
    if not isinstance(gt_boxes, torch.Tensor) or gt_boxes.dim() != 3:
        raise Dfu3dError("point_targets: gt_boxes must have the shape (B, G, 8)")
    B = int(gt_boxes.shape[0])
    if isinstance(point_coords, torch.Tensor) and point_coords.dim() == 2:
        _want(point_coords, "point_targets: point_coords", (None, 4))
        rows, stride, points = int(point_coords.shape[0]), 4, point_coords[:, 1:]      # a view: the address of x of row 0
    else:
        _want(point_coords, "point_targets: points", (B, None, 3))
        rows, stride, points = B * int(point_coords.shape[1]), 3, point_coords
    if B < 1 or rows == 0 or rows % B:
        raise Dfu3dError("point_targets: %d points for %d samples of equal size" % (rows, B))
    dev = point_coords.device
    _gt8(gt_boxes, "point_targets: gt_boxes", B, dev)
    n_mean = 0
    if mean_size is not None:
        _want(mean_size, "point_targets: mean_size", (None, 3), dev)
        n_mean = int(mean_size.shape[0])
        if not 1 <= n_mean <= MAX_CLASSES:
            raise Dfu3dError("point_targets: %d mean sizes (1 .. %d)" % (n_mean, MAX_CLASSES))
    extra = extra_width(extra_width_xyz)
    cls = torch.empty((rows,), dtype=torch.int64, device=dev)
    box = torch.empty((rows, 8), dtype=torch.float32, device=dev)
    idx = torch.empty((rows,), dtype=torch.int32, device=dev) if return_idx else None
    rc = _lib_tgt.lib().dfu3d_tgt_point_targets(_p(points), stride, _p(gt_boxes), _p(mean_size), B, rows // B,
                                                int(gt_boxes.shape[1]), n_mean, int(num_class), extra[0], extra[1],
                                                extra[2], _p(cls), _p(box), _p(idx), _stream())
    _lib_tgt.check(rc, "dfu3d_tgt_point_targets")
    return (cls, box, idx) if return_idx else (cls, box)


def roi_max_iou(rois, roi_labels, gt_boxes, by_class=True):
    """rois (B, M, 7 + .), roi_labels int64 (B, M), gt_boxes (B, G, 8) -> max_overlaps float32 (B, M), gt_assignment
    int32 (B, M): per RoI the best volume IoU with a row up to the sample's last non-zero one -- with by_class only
    rows of the RoI's class --, and that row; 0 and 0 when there is none."""
    B = int(rois.shape[0]) if isinstance(rois, torch.Tensor) and rois.dim() == 3 else 0
    if B < 1:
        raise Dfu3dError("roi_max_iou: rois must have the shape (B, M, 7 or more)")
    dev = rois.device
    boxes = _boxes7(rois, "roi_max_iou: rois", B, dev)
    M = int(boxes.shape[1])
    if (not isinstance(roi_labels, torch.Tensor) or roi_labels.dtype != torch.int64 or roi_labels.device != dev
            or tuple(roi_labels.shape) != (B, M) or not roi_labels.is_contiguous()):
        raise Dfu3dError("roi_max_iou: roi_labels must be contiguous torch.int64 (%d, %d) on the GPU of rois" % (B, M))
    _gt8(gt_boxes, "roi_max_iou: gt_boxes", B, dev)
    ov = torch.empty((B, M), dtype=torch.float32, device=dev)
    asg = torch.empty((B, M), dtype=torch.int32, device=dev)
    rc = _lib_tgt.lib().dfu3d_tgt_roi_max_iou(_p(boxes), _p(roi_labels), _p(gt_boxes), B, M, int(gt_boxes.shape[1]),
                                              1 if by_class else 0, _p(ov), _p(asg), _stream())
    _lib_tgt.check(rc, "dfu3d_tgt_roi_max_iou")
    return ov, asg


def sampler_numbers(cfg):
    """The host side of subsample_rois: (R, fg_per, fg_thresh, reg_fg_thresh, bg_thresh_lo, hard_ratio)."""
    R = int(_get(cfg, 'ROI_PER_IMAGE'))
    fg_per = int(np.round(_get(cfg, 'FG_RATIO') * R))
    return (R, fg_per, min(_get(cfg, 'REG_FG_THRESH'), _get(cfg, 'CLS_FG_THRESH')), _get(cfg, 'REG_FG_THRESH'),
            _get(cfg, 'CLS_BG_THRESH_LO'), float(_get(cfg, 'HARD_BG_RATIO')))


def new_status(device):
    """A zeroed status word for roi_subsample / proposal_targets: they only ever OR into it."""
    return torch.zeros((1,), dtype=torch.int32, device=device)


def check_status(status):
    """READS the word from the device: raises Dfu3dError if a sample had neither a foreground nor a background RoI (the
    reference raises NotImplementedError inside the step; here the step goes on with a row of zeros)."""
    word = int(status.item())
    if word & STATUS_NO_ROI:
        raise Dfu3dError("roi_subsample: a sample had neither a foreground nor a background RoI (every overlap NaN?)")
    return word


def roi_subsample(max_overlaps, cfg, rand_key, rand_u, status=None):
    """max_overlaps float32 (B, M), rand_key int32 (B, M), rand_u float32 (B, R) in [0, 1) -> sampled_inds int32 (B, R).
    status: the int32 word of new_status() to OR into (a fresh one when None; it is returned as the second value)."""
    _want(max_overlaps, "roi_subsample: max_overlaps", (None, None))
    B, M = (int(v) for v in max_overlaps.shape)
    dev = max_overlaps.device
    R, fg_per, fg_t, reg_t, lo_t, ratio = sampler_numbers(cfg)
    if B < 1 or not 1 <= M <= MAX_ROIS or not 1 <= R <= MAX_SAMPLED:
        raise Dfu3dError("roi_subsample: B = %d, M = %d (1 .. %d), ROI_PER_IMAGE = %d (1 .. %d)"
                         % (B, M, MAX_ROIS, R, MAX_SAMPLED))
    if (not isinstance(rand_key, torch.Tensor) or rand_key.dtype != torch.int32 or rand_key.device != dev
            or tuple(rand_key.shape) != (B, M) or not rand_key.is_contiguous()):
        raise Dfu3dError("roi_subsample: rand_key must be contiguous torch.int32 (%d, %d) on the GPU" % (B, M))
    _want(rand_u, "roi_subsample: rand_u", (B, R), dev)
    if status is None:
        status = new_status(dev)
    elif status.dtype != torch.int32 or status.numel() != 1 or status.device != dev:
        raise Dfu3dError("roi_subsample: status must be one torch.int32 word on the GPU")
    out = torch.empty((B, R), dtype=torch.int32, device=dev)
    rc = _lib_tgt.lib().dfu3d_tgt_roi_sample(_p(max_overlaps), _p(rand_key), _p(rand_u), B, M, R, fg_per, fg_t, reg_t, lo_t,
                                             ratio, _p(out), _p(status), _stream())
    _lib_tgt.check(rc, "dfu3d_tgt_roi_sample")
    return out, status


def cls_labels_of(ious, cfg):
    """rcnn_cls_labels of ProposalTargetLayer.forward for CLS_SCORE_TYPE 'cls' (int64: 1, 0, -1 ignored) and 'roi_iou'
    (float32 in [0, 1])."""
    kind, fg, bg = _get(cfg, 'CLS_SCORE_TYPE'), _get(cfg, 'CLS_FG_THRESH'), _get(cfg, 'CLS_BG_THRESH')
    if kind == 'cls':
        labels = (ious > fg).long()
        return torch.where((ious > bg) & (ious < fg), torch.full_like(labels, -1), labels)
    if kind == 'roi_iou':
        above, below = ious > fg, ious < bg
        return torch.where(~above & ~below, (ious - bg) / (fg - bg), above.float())
    raise NotImplementedError("CLS_SCORE_TYPE %r" % (kind,))


def proposal_targets(rois, roi_scores, roi_labels, gt_boxes, cfg, generator=None, sampled_inds=None, status=None):
    """ProposalTargetLayer.forward -> the reference's targets_dict (rois (B, R, 7 + C), gt_of_rois (B, R, 8 + C),
    gt_iou_of_rois, roi_scores, roi_labels, reg_valid_mask, rcnn_cls_labels) plus 'sampled_inds', 'max_overlaps',
    'gt_assignment' and 'status'.  generator: a torch.Generator of the RoIs' device for the draws; sampled_inds int32 or
    int64 (B, R) skips them."""
    by_class = bool(_get(cfg, 'SAMPLE_ROI_BY_EACH_CLASS', False))
    labels = roi_labels.contiguous()
    ov, asg = roi_max_iou(rois, labels, gt_boxes, by_class)
    B, M = (int(v) for v in ov.shape)
    dev = rois.device
    if sampled_inds is None:
        R = int(_get(cfg, 'ROI_PER_IMAGE'))
        key = torch.randint(0, 2 ** 31 - 1, (B, M), dtype=torch.int32, device=dev, generator=generator)
        u = torch.rand((B, R), dtype=torch.float32, device=dev, generator=generator)
        sampled_inds, status = roi_subsample(ov, cfg, key, u, status)
    inds = sampled_inds.long()
    wide = lambda t: inds[..., None].expand(-1, -1, t.shape[-1])       # noqa: E731
    ious = ov.gather(1, inds)
    gt_rows = asg.long().gather(1, inds)
    targets = {
        'rois': rois.gather(1, wide(rois)), 'gt_of_rois': gt_boxes.gather(1, gt_rows[..., None].expand(-1, -1, gt_boxes.shape[-1])),
        'gt_iou_of_rois': ious, 'roi_scores': roi_scores.gather(1, inds), 'roi_labels': labels.gather(1, inds),
        'reg_valid_mask': (ious > _get(cfg, 'REG_FG_THRESH')).long(), 'rcnn_cls_labels': cls_labels_of(ious, cfg),
        'sampled_inds': sampled_inds, 'max_overlaps': ov, 'gt_assignment': asg, 'status': status}
    return targets
