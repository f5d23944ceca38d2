"""The stacked set-abstraction ops on csrc/pointstack_stage.hip (C ABI: csrc/dfu3d_stk.h).

Plain functions over the entry points -- counts, starts, fps, ball_query, group, global_index, bev_sample -- and the
autograd function built on them: query_group (QueryAndGroup's output, already in the order the 1x1 convolution reads).
Stacked tensors: the rows of all samples one after the other; coordinates may be three columns of a wider float32
block (`points[:, 1:4]`): a view whose rows have one stride and whose columns are adjacent is read in place.  The rows
of a sample are given by `start` int32 (B + 1) on the device (counts() / starts() / starts_of()); nothing here reads
from the device.  The status bits of the calls are ORed into the word of the enclosing `status_scope`, or into a fresh
word nobody reads.

The grouping backward is pointnet2_ops' ordered gather over the inverse of the GLOBAL row of every entry
(global_index): empty balls are marked -1 there and pointnet2_ops.invert leaves them out; the BAD_INDEX bit invert
raises for them goes to a word of its own that is dropped, while a genuinely bad index has already been reported by
global_index in the caller's word."""
import contextlib
import ctypes

import torch

from . import _lib_stk
from . import pointnet2_ops as pn2
from ._lib import Dfu3dError

K = _lib_stk.CONSTANTS
ST_BAD_POINT = K["DFU3D_STK_ST_BAD_POINT"]
ST_BAD_INDEX = K["DFU3D_STK_ST_BAD_INDEX"]
ST_BAD_BATCH = K["DFU3D_STK_ST_BAD_BATCH"]
ST_UNSORTED = K["DFU3D_STK_ST_UNSORTED"]
ST_EMPTY = K["DFU3D_STK_ST_EMPTY"]
ST_BAD_COUNT = K["DFU3D_STK_ST_BAD_COUNT"]
MAX_SCALES = K["DFU3D_STK_MAX_SCALES"]
FPS_ONCHIP = K["DFU3D_STK_FPS_ONCHIP"]
MAX_ELEMS = K["DFU3D_STK_MAX_ELEMS"]

# kernel launches of one call (tools/bench_point_stack.py)
LAUNCHES = {"counts": 3, "starts": 1, "fps": 1, "ball_query": 1, "group": 1, "global_index": 1, "bev_sample": 1,
            "group_backward": 1 + 5 + 1}          # global_index, invert (fill + 4), gather_backward

STATUS_TEXT = {
    ST_BAD_POINT: "a non-finite coordinate in farthest point sampling (the picks are unspecified)",
    ST_BAD_INDEX: "a ball index outside its sample (row 0 of the sample was read, or the entry left out)",
    ST_BAD_BATCH: "a sample index outside [0, batch_size)",
    ST_UNSORTED: "the rows of a stacked tensor are not in ascending sample order",
    ST_EMPTY: "farthest point sampling of a sample without points (index 0 and a zero keypoint were written)",
    ST_BAD_COUNT: "per-sample counts that do not fit their tensor, or a sample beyond the given cap",
}

_SCOPE = []


def status_message(s):
    return "; ".join(t for b, t in STATUS_TEXT.items() if s & b)


@contextlib.contextmanager
def status_scope(status):
    """Every op called inside ORs its status bits into `status` (int32 (1) on the ops' device)."""
    _SCOPE.append(status)
    try:
        yield status
    finally:
        _SCOPE.pop()


def _status(dev):
    if _SCOPE and _SCOPE[-1].device == dev:
        return _SCOPE[-1]
    return torch.zeros(1, dtype=torch.int32, device=dev)


_stream, _p = pn2._stream, pn2._p


def _gpu(t, what, dtype, dev=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (dev is not None and t.device != dev):
        raise Dfu3dError("%s must be a tensor on the GPU%s" % (what, "" if dev is None else " of the other arguments"))
    if t.dtype != dtype:
        raise Dfu3dError("%s must be %s, got %s" % (what, dtype, t.dtype))
    return t


def _rows(t, what, dtype, cols, dev=None):
    """t: (rows, cols) of `dtype` on the GPU, read in place: adjacent columns, one row stride.  -> (rows, stride)."""
    _gpu(t, what, dtype, dev)
    if t.dim() != 2 or (cols is not None and int(t.shape[1]) != cols):
        raise Dfu3dError("%s must have the shape (*, %s), got %s" % (what, "*" if cols is None else cols, tuple(t.shape)))
    rows, width = int(t.shape[0]), int(t.shape[1])
    if rows == 0:
        return 0, max(width, 1)
    s0, s1 = t.stride()
    if (width > 1 and s1 != 1) or (rows > 1 and s0 < width):
        raise Dfu3dError("%s must have adjacent columns and one row stride, got the strides %s" % (what, (s0, s1)))
    return rows, (s0 if rows > 1 else max(width, 3))


def _vec(t, what, dtype, n, dev=None):
    _gpu(t, what, dtype, dev)
    if t.dim() != 1 or int(t.shape[0]) != n or not t.is_contiguous():
        raise Dfu3dError("%s must be contiguous of the shape (%d,), got %s" % (what, n, tuple(t.shape)))
    return t


def _check(rc, what):
    _lib_stk.check(rc, what)


def counts(column, batch_size):
    """column: column 0 of a stacked tensor, `points[:, 0]` (float32) or `indices[:, 0]` (int32), read in place ->
    cnt int32 (B), start int32 (B + 1).  Unsorted rows and sample indices outside [0, B) set their status bits."""
    if not isinstance(column, torch.Tensor) or column.dim() != 1 or column.dtype not in (torch.float32, torch.int32):
        raise Dfu3dError("counts: the batch column must be a float32 or int32 vector")
    _gpu(column, "counts: the batch column", column.dtype)
    B, rows = int(batch_size), int(column.shape[0])
    stride = int(column.stride(0)) if rows > 1 else 1
    if B < 1 or stride < 1:
        raise Dfu3dError("counts: batch_size = %d, stride %d" % (B, stride))
    cnt = torch.empty(B, dtype=torch.int32, device=column.device)
    start = torch.empty(B + 1, dtype=torch.int32, device=column.device)
    rc = _lib_stk.lib().dfu3d_stk_counts(_p(column), 1 if column.dtype == torch.int32 else 0, rows, stride, B, _p(cnt),
                                         _p(start), _p(_status(column.device)), _stream())
    _check(rc, "dfu3d_stk_counts")
    cnt._dfu3d_stk_start = (cnt._version, start)
    return cnt, start


def starts(cnt):
    """cnt int32 (B) -> start int32 (B + 1), the exclusive prefix."""
    _gpu(cnt, "starts: cnt", torch.int32)
    B = int(cnt.shape[0]) if cnt.dim() == 1 else 0
    _vec(cnt, "starts: cnt", torch.int32, B)
    if B < 1:
        raise Dfu3dError("starts: an empty batch")
    start = torch.empty(B + 1, dtype=torch.int32, device=cnt.device)
    rc = _lib_stk.lib().dfu3d_stk_starts(_p(cnt), B, _p(start), _p(_status(cnt.device)), _stream())
    _check(rc, "dfu3d_stk_starts")
    return start


def starts_of(cnt):
    """starts(cnt), built once per count tensor: kept on the tensor and reused while it has not been written to."""
    kept = getattr(cnt, "_dfu3d_stk_start", None)
    if kept is None or kept[0] != cnt._version:
        kept = (cnt._version, starts(cnt))
        cnt._dfu3d_stk_start = kept
    return kept[1]


def fps(xyz, start, npoint, cap=0):
    """xyz (N, 3) stacked, start (B + 1) -> idx int32 (B, npoint), sample-local, keypoints (B * npoint, 4) [b, x, y, z].
    A sample shorter than npoint repeats its picks.  cap: a bound on the rows of one sample, if the caller knows one."""
    N, stride = _rows(xyz, "fps: xyz", torch.float32, 3)
    _gpu(start, "fps: start", torch.int32, xyz.device)
    B, npoint, cap = int(start.numel()) - 1, int(npoint), int(cap)
    _vec(start, "fps: start", torch.int32, B + 1)
    if B < 1 or npoint < 1 or cap < 0:
        raise Dfu3dError("fps: batch of %d, npoint = %d, cap = %d" % (B, npoint, cap))
    L = _lib_stk.lib()
    nbytes = L.dfu3d_stk_fps_scratch_bytes(N, cap)
    if nbytes < 0:
        raise Dfu3dError("fps: xyz %s is out of range" % (tuple(xyz.shape),))
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=xyz.device) if nbytes else None
    idx = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
    kp = torch.empty((B * npoint, 4), dtype=torch.float32, device=xyz.device)
    rc = L.dfu3d_stk_fps(_p(xyz), stride, N, _p(start), B, npoint, cap, _p(idx), _p(kp), _p(scratch),
                         _p(_status(xyz.device)), _stream())
    _check(rc, "dfu3d_stk_fps")
    return idx, kp


def ball_query(xyz, start, centres, cstart, radii, nsamples):
    """xyz (N, 3) over start, centres (M, 3) over cstart, up to MAX_SCALES (radius, nsample) pairs ->
    [(idx int32 (M, nsample), empty uint8 (M))], all in one launch."""
    N, stride = _rows(xyz, "ball_query: xyz", torch.float32, 3)
    M, cstride = _rows(centres, "ball_query: centres", torch.float32, 3, xyz.device)
    B = int(start.numel()) - 1 if isinstance(start, torch.Tensor) else 0
    _vec(start, "ball_query: start", torch.int32, B + 1, xyz.device)
    _vec(cstart, "ball_query: cstart", torch.int32, B + 1, xyz.device)
    radii, nsamples = [float(r) for r in radii], [int(n) for n in nsamples]
    if len(radii) != len(nsamples) or not 1 <= len(radii) <= MAX_SCALES:
        raise Dfu3dError("ball_query: %d radii and %d sample counts, between 1 and %d pairs"
                         % (len(radii), len(nsamples), MAX_SCALES))
    if B < 1 or any(n < 1 for n in nsamples) or any(r != r for r in radii):
        raise Dfu3dError("ball_query: nsample must be positive and the radius a number, got %s %s" % (radii, nsamples))
    idx = [torch.empty((M, n), dtype=torch.int32, device=xyz.device) for n in nsamples]
    emp = [torch.empty(M, dtype=torch.uint8, device=xyz.device) for _ in nsamples]
    r, n = radii + [0.0], nsamples + [1]
    i, e = [ctypes.c_void_p(t.data_ptr()) for t in idx] + [None], [ctypes.c_void_p(t.data_ptr()) for t in emp] + [None]
    rc = _lib_stk.lib().dfu3d_stk_ball_query(_p(xyz), stride, N, _p(start), _p(centres), cstride, M, _p(cstart), B,
                                             len(radii), r[0], n[0], i[0], e[0], r[1], n[1], i[1], e[1],
                                             _p(_status(xyz.device)), _stream())
    _check(rc, "dfu3d_stk_ball_query")
    return list(zip(idx, emp))


def _group_args(xyz, start, centres, cstart, features, idx, empty, who):
    if xyz is None and (centres is not None or features is None):
        raise Dfu3dError("%s: without xyz there are no centres, and features are required" % who)
    _gpu(idx, who + ": idx", torch.int32)
    dev = idx.device
    if xyz is None:
        N, stride, M, cstride = int(features.shape[0]) if isinstance(features, torch.Tensor) else 0, 3, int(idx.shape[0]), 3
    else:
        N, stride = _rows(xyz, who + ": xyz", torch.float32, 3, dev)
        M, cstride = _rows(centres, who + ": centres", torch.float32, 3, dev)
    B = int(start.numel()) - 1 if isinstance(start, torch.Tensor) else 0
    _vec(start, who + ": start", torch.int32, B + 1, dev)
    _vec(cstart, who + ": cstart", torch.int32, B + 1, dev)
    if idx.dim() != 2 or int(idx.shape[0]) != M or int(idx.shape[1]) < 1 or not idx.is_contiguous():
        raise Dfu3dError("%s: idx must be contiguous (%d, nsample), got %s" % (who, M, tuple(idx.shape)))
    _vec(empty, who + ": empty", torch.uint8, M, dev)
    C = 0
    if features is not None:
        _gpu(features, who + ": features", torch.float32, dev)
        if features.dim() != 2 or int(features.shape[0]) != N or not features.is_contiguous():
            raise Dfu3dError("%s: features must be contiguous (%d, C), got %s" % (who, N, tuple(features.shape)))
        C = int(features.shape[1])
    if xyz is None and C < 1:
        raise Dfu3dError("%s: features %s without xyz" % (who, tuple(features.shape)))
    return N, stride, M, cstride, B, C, int(idx.shape[1])


def group(xyz, start, centres, cstart, features, idx, empty):
    """QueryAndGroup.forward behind the ball query: (3 + C, M, nsample), xyz - centre then the features; empty balls
    are zeros.  features (N, C) or None.  xyz and centres None: the plain grouping_operation, (C, M, nsample)."""
    N, stride, M, cstride, B, C, ns = _group_args(xyz, start, centres, cstart, features, idx, empty, "group")
    out = torch.empty(((0 if xyz is None else 3) + C, M, ns), dtype=torch.float32, device=idx.device)
    rc = _lib_stk.lib().dfu3d_stk_group(_p(xyz), stride, N, _p(start), _p(centres), cstride, M, _p(cstart), B,
                                        _p(features) if C else None, C, _p(idx), _p(empty), ns, _p(out),
                                        _p(_status(idx.device)), _stream())
    _check(rc, "dfu3d_stk_group")
    return out


def global_index(idx, empty, start, cstart, N):
    """idx (M, nsample), empty (M) -> int32 (1, M * nsample): the global row of every entry, -1 for what the backward
    leaves out (empty balls; an index outside its sample, which sets ST_BAD_INDEX)."""
    _gpu(idx, "global_index: idx", torch.int32)
    if idx.dim() != 2 or idx.numel() == 0 or not idx.is_contiguous():
        raise Dfu3dError("global_index: idx must be contiguous (M, nsample), got %s" % (tuple(idx.shape),))
    M, ns, B = int(idx.shape[0]), int(idx.shape[1]), int(start.numel()) - 1
    _vec(empty, "global_index: empty", torch.uint8, M, idx.device)
    _vec(start, "global_index: start", torch.int32, B + 1, idx.device)
    _vec(cstart, "global_index: cstart", torch.int32, B + 1, idx.device)
    gidx = torch.empty((1, M * ns), dtype=torch.int32, device=idx.device)
    rc = _lib_stk.lib().dfu3d_stk_global_index(_p(idx), _p(empty), M, ns, int(N), _p(start), _p(cstart), B, _p(gidx),
                                               _p(_status(idx.device)), _stream())
    _check(rc, "dfu3d_stk_global_index")
    return gidx


def group_backward(grad_out, idx, empty, start, cstart, N, skip=3):
    """grad_out (skip + C, M, nsample) -> grad_features (N, C): the entries of a source row summed in ascending entry
    number, float32, from +0.0f; the same bits on every run."""
    if not isinstance(grad_out, torch.Tensor) or grad_out.dim() != 3 or grad_out.dtype != torch.float32:
        raise Dfu3dError("group_backward: grad_out must be float32 (skip + C, M, nsample)")
    C = int(grad_out.shape[0]) - skip
    if C < 1 or tuple(grad_out.shape[1:]) != tuple(idx.shape):
        raise Dfu3dError("group_backward: grad_out %s for idx %s" % (tuple(grad_out.shape), tuple(idx.shape)))
    kept = getattr(idx, "_dfu3d_stk_inverse", None)
    if kept is None or kept[0] != (int(N), idx._version, empty._version):
        gidx = global_index(idx, empty, start, cstart, N)
        with pn2.status_scope(torch.zeros(1, dtype=torch.int32, device=idx.device)):   # the -1 marks are ours: dropped
            kept = ((int(N), idx._version, empty._version), pn2.invert(gidx, N))
        idx._dfu3d_stk_inverse = kept
    g = grad_out.contiguous()[skip:].unsqueeze(0)                     # (1, C, M, nsample): a view, contiguous
    return pn2.gather_backward(g, kept[1]).view(C, int(N)).t().contiguous()


class _QueryGroup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, xyz, start, centres, cstart, idx, empty):
        out = group(xyz, start, centres, cstart, features, idx, empty)
        ctx.saved = (idx, empty, start, cstart, int(features.shape[0]), 0 if xyz is None else 3)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return (group_backward(grad_out, *ctx.saved),) + (None,) * 6


def query_group(xyz, start, centres, cstart, features, idx, empty):
    """group() with the gradient of the features (xyz and the centres get none, as in the reference's use)."""
    if features is None or not features.requires_grad or int(features.shape[0]) == 0 or int(features.shape[1]) == 0:
        return group(xyz, start, centres, cstart, features, idx, empty)
    return _QueryGroup.apply(features, xyz, start, centres, cstart, idx, empty)


def bev_sample(keypoints, spatial_features, point_cloud_range, voxel_size, bev_stride):
    """keypoints (M, 4) [b, x, y, z], spatial_features (B, C, H, W) -> (M, C): interpolate_from_bev_features for the
    whole batch, the reference's float32 arithmetic operation by operation.  Forward only."""
    if getattr(keypoints, "requires_grad", False) or getattr(spatial_features, "requires_grad", False):
        raise NotImplementedError("bev_sample is forward only: an input requires grad")
    M, kstride = _rows(keypoints, "bev_sample: keypoints", torch.float32, None)
    if int(keypoints.shape[1]) < 3 or M < 1:
        raise Dfu3dError("bev_sample: keypoints %s" % (tuple(keypoints.shape),))
    _gpu(spatial_features, "bev_sample: spatial_features", torch.float32, keypoints.device)
    if spatial_features.dim() != 4 or not spatial_features.is_contiguous() or spatial_features.numel() == 0:
        raise Dfu3dError("bev_sample: spatial_features must be contiguous (B, C, H, W), got %s"
                         % (tuple(spatial_features.shape),))
    B, C, H, W = (int(v) for v in spatial_features.shape)
    out = torch.empty((M, C), dtype=torch.float32, device=keypoints.device)
    rc = _lib_stk.lib().dfu3d_stk_bev_sample(_p(keypoints), kstride, M, _p(spatial_features), B, C, H, W,
                                             float(point_cloud_range[0]), float(point_cloud_range[1]),
                                             float(voxel_size[0]), float(voxel_size[1]), float(bev_stride), _p(out),
                                             _p(_status(keypoints.device)), _stream())
    _check(rc, "dfu3d_stk_bev_sample")
    return out
