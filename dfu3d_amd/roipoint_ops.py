"""RoI-point pooling on csrc/roipoint_stage.hip (C ABI: include/dfu3d_roi.h).

pool: the reference op's own form -- points (B, N, 3), point_features (B, N, C), boxes3d (B, M, 7) -> pooled
(B, M, S, 3 + C) with raw coordinates, the empty flags (B, M) and, on request, pooled_idx (B, M, S).
pool_fused: PointRCNNHead.roipool3d_gpu's -- the stacked point_coords (B * N, 4) or points (B, N, 3), point_scores
(B * N), point_features (B * N, C), rois (B, M, 7 + .) -> (B * M, S, 5 + C) rows [x', y', z', score, depth, features...],
the rows of empty RoIs zero; no concatenated feature tensor, no assignment matrix.

float32 and contiguous, indices and flags int32: anything else raises Dfu3dError.  Every element of the outputs is
written by the kernels (torch.empty here).  Nothing reads from the device."""
import ctypes

import torch

from . import _lib_roi
from ._lib import Dfu3dError

K = _lib_roi.CONSTANTS
MAX_ELEMS = K["DFU3D_ROI_MAX_ELEMS"]
MAX_PTS_STRIDE = K["DFU3D_ROI_MAX_PTS_STRIDE"]
LAUNCHES = K["DFU3D_ROI_LAUNCHES"]
PREFIX_PLAIN = K["DFU3D_ROI_PREFIX_PLAIN"]
PREFIX_FUSED = K["DFU3D_ROI_PREFIX_FUSED"]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def _want(t, what, shape, dev=None):
    """t: a contiguous float32 tensor on the GPU (on `dev` if given) whose shape matches `shape` (None: any size)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (dev is not None and t.device != dev):
        raise Dfu3dError("%s must be a tensor on the GPU%s" % (what, "" if dev is None else " of the other arguments"))
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise Dfu3dError("%s must be contiguous torch.float32, got %s%s"
                         % (what, t.dtype, "" if t.is_contiguous() else ", not contiguous"))
    if t.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(t.shape, shape)):
        raise Dfu3dError("%s must have the shape %s, got %s"
                         % (what, tuple("*" if s is None else s for s in shape), tuple(t.shape)))
    return t


def extra_width(w):
    """pool_extra_width as the three floats added to dx, dy, dz: a number or a sequence of three."""
    w = [float(v) for v in w] if isinstance(w, (list, tuple)) else [float(w)] * 3
    if len(w) != 3 or any(v != v for v in w):
        raise Dfu3dError("pool_extra_width must be a number or three numbers, got %r" % (w,))
    return w


def _launch(lib, what, points, stride, features, scores, boxes, B, N, M, C, S, extra, fused, normalizer):
    if S < 1:
        raise Dfu3dError("%s: num_sampled_points = %d" % (what, S))
    W = (PREFIX_FUSED if fused else PREFIX_PLAIN) + C
    if max(B * N * max(stride, C), B * M * S * W) >= MAX_ELEMS:
        raise Dfu3dError("%s: B = %d, N = %d, M = %d, S = %d, C = %d is beyond %d elements per tensor"
                         % (what, B, N, M, S, C, MAX_ELEMS))
    dev = points.device
    pooled = torch.empty((B * M, S, W) if fused else (B, M, S, W), dtype=torch.float32, device=dev)
    flag = torch.empty((B, M), dtype=torch.int32, device=dev)
    idx = torch.empty((B, M, S), dtype=torch.int32, device=dev)
    rc = lib.dfu3d_roi_pool(_p(points), stride, _p(features), _p(scores), _p(boxes), B, N, M, C, S, extra[0], extra[1],
                            extra[2], 1 if fused else 0, normalizer, _p(pooled), _p(flag), _p(idx), _stream())
    _lib_roi.check(rc, "dfu3d_roi_pool")
    return pooled, flag, idx


def _boxes7(boxes, what, B, dev):
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 3 or boxes.shape[-1] < 7:
        raise Dfu3dError("%s must have the shape (%d, *, 7 or more)" % (what, B))
    b7 = boxes[..., :7].contiguous()
    _want(b7, what, (B, None, 7), dev)
    if b7.shape[1] == 0:
        raise Dfu3dError("%s is empty" % what)
    return b7


def pool(points, point_features, boxes3d, pool_extra_width, num_sampled_points=512, return_idx=False):
    """RoIPointPool3dFunction.forward: -> pooled_features (B, M, S, 3 + C), pooled_empty_flag int32 (B, M)
    [, pooled_idx int32 (B, M, S)]."""
    _want(points, "pool: points", (None, None, 3))
    B, N = int(points.shape[0]), int(points.shape[1])
    _want(point_features, "pool: point_features", (B, N, None), points.device)
    C = int(point_features.shape[2])
    boxes = _boxes7(boxes3d, "pool: boxes3d", B, points.device)
    if B * N == 0:
        raise Dfu3dError("pool: points is empty")
    out = _launch(_lib_roi.lib(), "pool", points, 3, point_features, None, boxes, B, N, int(boxes.shape[1]), C,
                  int(num_sampled_points), extra_width(pool_extra_width), False, 1.0)
    return out if return_idx else out[:2]


def pool_fused(point_coords, point_scores, point_features, rois, pool_extra_width, num_sampled_points, depth_normalizer,
               return_idx=False):
    """PointRCNNHead.roipool3d_gpu: point_coords (B * N, 4) [sample, x, y, z] stacked in sample order with equal sample
    sizes (read in place at a stride of 4 floats) or points (B, N, 3); point_scores (B * N); point_features (B * N, C);
    rois (B, M, 7 + .) -> (B * M, S, 5 + C) [, pooled_empty_flag (B, M), pooled_idx (B, M, S)]."""
    B = int(rois.shape[0]) if isinstance(rois, torch.Tensor) and rois.dim() == 3 else 0
    if B < 1:
        raise Dfu3dError("pool_fused: rois must have the shape (B, M, 7 or more)")
    if isinstance(point_coords, torch.Tensor) and point_coords.dim() == 2:
        _want(point_coords, "pool_fused: point_coords", (None, 4))
        rows, stride, points = int(point_coords.shape[0]), 4, point_coords[:, 1:]     # a view: the address of x of row 0
    else:
        _want(point_coords, "pool_fused: points", (B, None, 3))
        rows, stride, points = B * int(point_coords.shape[1]), 3, point_coords
    if rows == 0 or rows % B:
        raise Dfu3dError("pool_fused: %d points for %d samples of equal size" % (rows, B))
    N, dev = rows // B, point_coords.device
    _want(point_scores, "pool_fused: point_scores", (rows,), dev)
    _want(point_features, "pool_fused: point_features", (rows, None), dev)
    C = int(point_features.shape[1])
    boxes = _boxes7(rois, "pool_fused: rois", B, dev)
    normalizer = float(depth_normalizer)
    if not normalizer > 0.0:
        raise Dfu3dError("pool_fused: depth_normalizer = %r" % (depth_normalizer,))
    out = _launch(_lib_roi.lib(), "pool_fused", points, stride, point_features, point_scores, boxes, B, N,
                  int(boxes.shape[1]), C, int(num_sampled_points), extra_width(pool_extra_width), True, normalizer)
    return out if return_idx else out[0]
