"""The anchor target assignment of AnchorHeadSingle on csrc/anchor_stage.hip (C ABI: csrc/dfu3d_anc.h): for a whole batch
in LAUNCHES kernel launches, what AxisAlignedTargetAssigner.assign_targets computes per sample and per anchor class.

assign_targets  anchors (A, 7), class_sets, gt_boxes (B, M, 8) -> box_cls_labels int32 (B, A), box_reg_targets (B, A, 7),
                reg_weights (B, A).

anchors is the head's flattened block: locations in y, x order, at each of them the class sets one after another.
class_sets: one (anchors_per_location, matched_threshold, unmatched_threshold, class_id) per set, class_id 1-based.  The
rule -- trailing zero rows, class 0 to the last set, nearest-BEV IoU, forced anchors, labels -- is the header's.  float32
and contiguous, anything else raises Dfu3dError.  Every element of the outputs is written by the kernels (torch.empty
here); one scratch tensor per call.  Nothing in this module reads from the device."""
import ctypes

import torch

from . import _lib_anc
from ._lib import Dfu3dError
from .stages import _chk, _stream

K = _lib_anc.CONSTANTS
LAUNCHES = K["DFU3D_ANC_LAUNCHES"]
MAX_SETS = K["DFU3D_ANC_MAX_SETS"]
MAX_BOXES = K["DFU3D_ANC_MAX_BOXES"]
MAX_BATCH = K["DFU3D_ANC_MAX_BATCH"]
MAX_ELEMS = K["DFU3D_ANC_MAX_ELEMS"]


def set_arrays(class_sets):
    """class_sets -> (per_loc, set_begin int32[S + 1], matched float[S], unmatched float[S], class_id int32[S]) as
    ctypes arrays the library reads on the host."""
    sets = [tuple(s) for s in class_sets]
    if not sets or any(len(s) != 4 for s in sets):
        raise Dfu3dError("assign_targets: class_sets must be a non-empty list of (anchors_per_location, "
                         "matched_threshold, unmatched_threshold, class_id)")
    if len(sets) > MAX_SETS:
        raise Dfu3dError("assign_targets: %d class sets, at most %d (DFU3D_ERANGE)" % (len(sets), MAX_SETS))
    begin = [0]
    for s in sets:
        begin.append(begin[-1] + int(s[0]))
    S = len(sets)
    return (begin[-1], (ctypes.c_int32 * (S + 1))(*begin), (ctypes.c_float * S)(*[float(s[1]) for s in sets]),
            (ctypes.c_float * S)(*[float(s[2]) for s in sets]), (ctypes.c_int32 * S)(*[int(s[3]) for s in sets]))


def assign_targets(anchors, class_sets, gt_boxes):
    """anchors float32 (A, 7); class_sets: see the module; gt_boxes float32 (B, M, 8) [x, y, z, dx, dy, dz, heading,
    class] -> (box_cls_labels int32 (B, A), box_reg_targets float32 (B, A, 7), reg_weights float32 (B, A))."""
    if not isinstance(anchors, torch.Tensor) or anchors.dim() != 2 or anchors.shape[1] != 7:
        raise Dfu3dError("assign_targets: anchors must have the shape (A, 7), got %s"
                         % (tuple(anchors.shape) if isinstance(anchors, torch.Tensor) else type(anchors).__name__,))
    if not isinstance(gt_boxes, torch.Tensor) or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 8:
        raise Dfu3dError("assign_targets: gt_boxes must have the shape (B, M, 8), got %s"
                         % (tuple(gt_boxes.shape) if isinstance(gt_boxes, torch.Tensor) else type(gt_boxes).__name__,))
    A = int(anchors.shape[0])
    B, M = int(gt_boxes.shape[0]), int(gt_boxes.shape[1])
    per_loc, begin, matched, unmatched, class_id = set_arrays(class_sets)
    if M > MAX_BOXES or B > MAX_BATCH or B * A * 7 > MAX_ELEMS:
        raise Dfu3dError("assign_targets: B = %d (at most %d), M = %d (at most %d), A = %d is out of range (DFU3D_ERANGE)"
                         % (B, MAX_BATCH, M, MAX_BOXES, A))
    a_p = _chk(anchors, "assign_targets: anchors", torch.float32)
    g_p = _chk(gt_boxes, "assign_targets: gt_boxes", torch.float32)
    dev = anchors.device
    if gt_boxes.device != dev:
        raise Dfu3dError("assign_targets: anchors and gt_boxes must live on the same GPU")
    labels = torch.empty((B, A), dtype=torch.int32, device=dev)
    targets = torch.empty((B, A, 7), dtype=torch.float32, device=dev)
    weights = torch.empty((B, A), dtype=torch.float32, device=dev)
    if B == 0 or A == 0:
        return labels, targets, weights
    L = _lib_anc.lib()
    nbytes = int(L.dfu3d_anc_scratch_bytes(B, A, M))
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    rc = L.dfu3d_anchor_targets(a_p, A, per_loc, begin, matched, unmatched, class_id, len(matched),
                                g_p if M > 0 and B > 0 else None, B, M,
                                _chk(scratch, "assign_targets: scratch", torch.uint8, min_numel=16), nbytes,
                                _chk(labels, "assign_targets: box_cls_labels", torch.int32),
                                _chk(targets, "assign_targets: box_reg_targets", torch.float32),
                                _chk(weights, "assign_targets: reg_weights", torch.float32), _stream())
    _lib_anc.check(rc, "dfu3d_anchor_targets")
    return labels, targets, weights
