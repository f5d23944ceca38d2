"""PointRCNN's proposal stage on csrc/proposal_stage.hip (C ABI: csrc/dfu3d_prop.h): for a whole batch in LAUNCHES kernel
launches, the pre_max best points of every sample by score, their rotated NMS cut at post_max, and the padded RoI block.

proposals  scores (B, N), labels int64 (B, N), boxes (B, N, 7 + .) -> rois (B, post_max, 7 + .), roi_scores (B, post_max),
           roi_labels int64 (B, post_max) = label + 1, roi_point_idx int64 (B, post_max), num_rois int32 (B).

The order is the one total order of the header (the score's monotone key, -0.0 as +0.0, every NaN above +inf, equal keys
by ascending point index), so the result is a pure function of the input.  float32 and contiguous, anything else raises
Dfu3dError.  Every element of the outputs is written by the kernels (torch.empty here); one scratch tensor per call.
Nothing in this module reads from the device."""
import ctypes

import torch

from . import _lib_prop
from ._lib import Dfu3dError
from .stages import _chk, _stream

K = _lib_prop.CONSTANTS
LAUNCHES = K["DFU3D_PROP_LAUNCHES"]
MAX_POST = K["DFU3D_PROP_MAX_POST"]
MAX_POINTS = K["DFU3D_PROP_MAX_POINTS"]
MAX_BATCH = K["DFU3D_PROP_MAX_BATCH"]
MAX_ELEMS = K["DFU3D_PROP_MAX_ELEMS"]


def proposals(scores, labels, boxes, thresh, pre_max, post_max):
    """scores float32 (B, N); labels int64 (B, N), 0-based; boxes float32 (B, N, C >= 7) [x, y, z, dx, dy, dz, heading,
    ...]; thresh: the footprint IoU above which an earlier kept box suppresses a later one -> (rois (B, post_max, C),
    roi_scores (B, post_max), roi_labels int64 (B, post_max), roi_point_idx int64 (B, post_max), num_rois int32 (B)).
    Rows at or beyond num_rois[b] are zero, label 1, index -1."""
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 3 or boxes.shape[2] < 7:
        raise Dfu3dError("proposals: boxes must have the shape (B, N, 7 or more), got %s"
                         % (tuple(boxes.shape) if isinstance(boxes, torch.Tensor) else type(boxes).__name__,))
    B, N, C = (int(v) for v in boxes.shape)
    pre_max, post_max, thresh = int(pre_max), int(post_max), float(thresh)
    if pre_max < 1 or not 1 <= post_max <= MAX_POST:
        raise Dfu3dError("proposals: pre_max = %d (1 or more), post_max = %d (1 .. %d)" % (pre_max, post_max, MAX_POST))
    if N > MAX_POINTS or B > MAX_BATCH or max(B * N * C, B * post_max * C) > MAX_ELEMS:
        raise Dfu3dError("proposals: B = %d (at most %d), N = %d (at most %d), C = %d is out of range (DFU3D_ERANGE)"
                         % (B, MAX_BATCH, N, MAX_POINTS, C))
    b_p = _chk(boxes, "proposals: boxes", torch.float32)
    s_p = _chk(scores, "proposals: scores", torch.float32, numel=B * N)
    l_p = _chk(labels, "proposals: labels", torch.int64, numel=B * N)
    if tuple(scores.shape) != (B, N) or tuple(labels.shape) != (B, N):
        raise Dfu3dError("proposals: scores %s and labels %s must have the shape (%d, %d)"
                         % (tuple(scores.shape), tuple(labels.shape), B, N))
    dev = boxes.device
    if scores.device != dev or labels.device != dev:
        raise Dfu3dError("proposals: scores, labels and boxes must live on the same GPU")
    rois = torch.empty((B, post_max, C), dtype=torch.float32, device=dev)
    roi_scores = torch.empty((B, post_max), dtype=torch.float32, device=dev)
    roi_labels = torch.empty((B, post_max), dtype=torch.int64, device=dev)
    roi_point_idx = torch.empty((B, post_max), dtype=torch.int64, device=dev)
    num_rois = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return rois, roi_scores, roi_labels, roi_point_idx, num_rois
    if N == 0:
        return rois.zero_(), roi_scores.zero_(), roi_labels.fill_(1), roi_point_idx.fill_(-1), num_rois.zero_()
    L = _lib_prop.lib()
    nbytes = int(L.dfu3d_prop_scratch_bytes(B, N, pre_max))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = L.dfu3d_proposals(s_p, l_p, b_p, B, N, C, ctypes.c_float(thresh), pre_max, post_max,
                           _chk(scratch, "proposals: scratch", torch.uint8, min_numel=16), nbytes,
                           _chk(rois, "proposals: rois", torch.float32), _chk(roi_scores, "proposals: roi_scores", torch.float32),
                           _chk(roi_labels, "proposals: roi_labels", torch.int64),
                           _chk(roi_point_idx, "proposals: roi_point_idx", torch.int64),
                           _chk(num_rois, "proposals: num_rois", torch.int32, numel=B), _stream())
    _lib_prop.check(rc, "dfu3d_proposals")
    return rois, roi_scores, roi_labels, roi_point_idx, num_rois
