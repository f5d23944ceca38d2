"""Dynamic pillar grouping and per-pillar maximum on csrc/pillar_stage.hip (C ABI: include/dfu3d_vfe.h).

`pillar_group` turns a batch of points into pillars the way pcdet's DynamicPillarVFE does -- the mask, the cell key, the
pillar order of the sorted torch.unique, the feature matrix entering the first PFN layer -- with every float sum in
ascending point index, so the result is the same bits on every run.  It reads the device once: n_kept, P and the
status word arrive together (the reference's torch.unique synchronises too).

`pillar_max` / `pillar_max_concat` are autograd functions: the maximum over a pillar's rows, alone or fused into the
PFN layer's cat([x, x_max[unq_inv]], 1); the backward routes to the lowest row among equal maxima and sums without
float atomics.  x must be float32 and contiguous (mixed precision is out of scope).
"""
import ctypes

import numpy as np
import torch

from . import _lib_vfe
from ._lib import Dfu3dError

C = _lib_vfe.CONSTANTS
LAYOUT_PILLAR = C["DFU3D_VFE_LAYOUT_PILLAR"]
LAYOUT_SIMPLE2D = C["DFU3D_VFE_LAYOUT_SIMPLE2D"]
ST_BAD_POINT = C["DFU3D_VFE_ST_BAD_POINT"]
MAX_CELLS = C["DFU3D_VFE_MAX_CELLS"]
MAX_CHANNELS = C["DFU3D_VFE_MAX_CHANNELS"]

STATUS_TEXT = {
    ST_BAD_POINT: "a point has a non-finite x or y, or a batch index outside [0, batch_size)",
}


def _f32(v):
    return float(np.float32(v))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def feature_cols(point_cols, layout, use_absolute_xyz, with_distance):
    """Width of the feature matrix for points of `point_cols` columns (batch index included)."""
    raw = point_cols - 1 if use_absolute_xyz else point_cols - 4
    return raw + (6 if layout == LAYOUT_PILLAR else 3) + (1 if with_distance else 0)


class PillarGroup:
    """Result of pillar_group: kept_idx (n_kept) int32 indices of the kept points, unq_inv (n_kept) pillar of each,
    unq_cnt (P), coords (P, 4) [b, 0, y, x] or (P, 3) [b, y, x], the CSR offsets (P + 1) / plist (n_kept) of every
    pillar's rows in ascending order, features (n_kept, feat_cols), and the host integers n_kept, P, status."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def pillar_group(points, batch_size, point_cloud_range, voxel_size, grid_size, layout=LAYOUT_PILLAR,
                 use_absolute_xyz=True, with_distance=False, offsets=None, check=True):
    """points (N, 1 + F) float32 on the GPU, column 0 the batch index.  point_cloud_range / voxel_size / grid_size: the
    detector's sequences (their x and y entries, and z for the centre offset).  `offsets`: the (x, y, z) centre offsets
    as Python floats (default: voxel / 2 + range_min in Python floats, as the reference computes them).  Status bits
    raise Dfu3dError unless check=False (then they are in the result's `status`)."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise Dfu3dError("pillar_group: points must be a tensor on the GPU")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 4:
        raise Dfu3dError("pillar_group: points must be (N, 1 + F >= 4) float32, got %s %s" % (tuple(points.shape), points.dtype))
    points = points.contiguous()
    n, cols = int(points.shape[0]), int(points.shape[1])
    nx, ny, B = int(grid_size[0]), int(grid_size[1]), int(batch_size)
    if B < 1 or nx < 1 or ny < 1:
        raise Dfu3dError("pillar_group: batch_size and grid_size must be positive")
    cells = B * nx * ny
    if cells > MAX_CELLS:
        raise Dfu3dError("pillar_group: batch_size * nx * ny = %d cells, at most %d" % (cells, MAX_CELLS))
    if offsets is None:
        offsets = tuple(voxel_size[k] / 2 + point_cloud_range[k] for k in range(3))
    L = _lib_vfe.lib()
    dev = points.device
    fcols = feature_cols(cols, layout, use_absolute_xyz, with_distance)
    n1, p_cap = max(n, 1), max(min(n, cells), 1)                 # never a null pointer for an empty batch
    ints = torch.empty(3 * n1 + 2 * p_cap + 1 + p_cap * (4 if layout == LAYOUT_PILLAR else 3) + 4, dtype=torch.int32, device=dev)
    cut = np.cumsum([0, 4, n1, n1, n1, p_cap, p_cap + 1]).tolist()
    hdr, kept_idx, unq_inv, plist, unq_cnt, csr = (ints[cut[k]:cut[k + 1]] for k in range(6))
    coords = ints[cut[6]:]
    feats = torch.empty((n1, fcols), dtype=torch.float32, device=dev)
    nbytes = L.dfu3d_vfe_scratch_bytes(n, cells)
    if nbytes < 0:
        raise Dfu3dError("pillar_group: dfu3d_vfe_scratch_bytes(%d, %d) failed" % (n, cells))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rx, ry = _f32(point_cloud_range[0]), _f32(point_cloud_range[1])
    vx, vy = _f32(voxel_size[0]), _f32(voxel_size[1])
    status = ctypes.c_void_p(hdr.data_ptr() + 8)
    rc = L.dfu3d_pillar_group(_p(points), n, cols, B, rx, ry, vx, vy, nx, ny, layout, _p(kept_idx), _p(unq_inv),
                              _p(unq_cnt), _p(coords), _p(csr), _p(plist), _p(hdr), status, _p(scratch), nbytes, _stream())
    _lib_vfe.check(rc, "dfu3d_pillar_group")
    rc = L.dfu3d_pillar_features(_p(points), n, cols, rx, ry, vx, vy, _f32(offsets[0]), _f32(offsets[1]), _f32(offsets[2]),
                                 layout, int(bool(use_absolute_xyz)), int(bool(with_distance)), _p(kept_idx), _p(unq_inv),
                                 _p(csr), _p(plist), _p(hdr), _p(feats), fcols, _p(scratch), nbytes, _stream())
    _lib_vfe.check(rc, "dfu3d_pillar_features")
    n_kept, P, st = hdr[:3].tolist()                              # the call's one host read
    if st and check:
        raise Dfu3dError("pillar_group: status %d (%s)" % (st, "; ".join(t for b, t in STATUS_TEXT.items() if st & b)))
    ccols = 4 if layout == LAYOUT_PILLAR else 3
    return PillarGroup(n_kept=n_kept, P=P, status=st, sizes=hdr[:2], kept_idx=kept_idx[:n_kept], unq_inv=unq_inv[:n_kept],
                       unq_cnt=unq_cnt[:P], coords=coords[:P * ccols].view(P, ccols), offsets=csr[:P + 1],
                       plist=plist[:n_kept], features=feats[:n_kept])


def _check_x(x, group, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise Dfu3dError("%s: x must be a tensor on the GPU" % what)
    if x.dtype != torch.float32:
        raise Dfu3dError("%s: x must be float32, got %s" % (what, x.dtype))
    if x.dim() != 2 or not x.is_contiguous():
        raise Dfu3dError("%s: x must be a contiguous matrix" % what)
    if x.shape[0] != group.n_kept:
        raise Dfu3dError("%s: x has %d rows, the group %d points" % (what, x.shape[0], group.n_kept))
    if not 1 <= x.shape[1] <= MAX_CHANNELS:
        raise Dfu3dError("%s: %d channels, between 1 and %d" % (what, x.shape[1], MAX_CHANNELS))


def _forward(x, group, concat):
    n, ch, P = int(x.shape[0]), int(x.shape[1]), group.P
    x_max = torch.empty((P, ch), dtype=torch.float32, device=x.device)
    arg = torch.empty((P, ch), dtype=torch.int32, device=x.device)
    cat = torch.empty((n, 2 * ch), dtype=torch.float32, device=x.device) if concat else None
    if n:
        rc = _lib_vfe.lib().dfu3d_pillar_max(_p(x), n, ch, _p(group.offsets), _p(group.plist), P, _p(group.sizes), _p(x_max),
                                             _p(arg), _p(cat) if concat else None, _stream())
        _lib_vfe.check(rc, "dfu3d_pillar_max")
    return x_max, arg, cat


def _backward(group, arg, n, ch, grad_max=None, grad_cat=None):
    g = grad_max if grad_max is not None else grad_cat
    if g.dtype != torch.float32:
        raise Dfu3dError("pillar_max backward: the gradient must be float32, got %s" % g.dtype)
    g = g.contiguous()
    gx = torch.empty((n, ch), dtype=torch.float32, device=g.device)
    if n:
        rc = _lib_vfe.lib().dfu3d_pillar_max_backward(_p(g) if grad_max is not None else None,
                                                      _p(g) if grad_max is None else None, n, ch, _p(arg), _p(group.offsets),
                                                      _p(group.plist), group.P, _p(group.sizes), _p(gx), _stream())
        _lib_vfe.check(rc, "dfu3d_pillar_max_backward")
    return gx


class _PillarMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, group):
        _check_x(x, group, "pillar_max")
        x_max, arg, _ = _forward(x, group, False)
        ctx.group, ctx.arg, ctx.shape = group, arg, tuple(x.shape)
        ctx.mark_non_differentiable(arg)
        return x_max, arg

    @staticmethod
    def backward(ctx, grad_max, _grad_arg):
        return _backward(ctx.group, ctx.arg, ctx.shape[0], ctx.shape[1], grad_max=grad_max), None


class _PillarMaxConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, group):
        _check_x(x, group, "pillar_max_concat")
        _, arg, cat = _forward(x, group, True)
        ctx.group, ctx.arg, ctx.shape = group, arg, tuple(x.shape)
        return cat

    @staticmethod
    def backward(ctx, grad_cat):
        return _backward(ctx.group, ctx.arg, ctx.shape[0], ctx.shape[1], grad_cat=grad_cat), None


def pillar_max(x, group, return_arg=False):
    """x (n_kept, C) -> x_max (P, C): the maximum over every pillar's rows (torch_scatter.scatter_max(x, unq_inv, 0)[0]).
    return_arg: also the int32 (P, C) row of each maximum, the lowest among equals."""
    x_max, arg = _PillarMax.apply(x, group)
    return (x_max, arg) if return_arg else x_max


def pillar_max_concat(x, group):
    """x (n_kept, C) -> cat([x, x_max[unq_inv]], 1) of shape (n_kept, 2C), in one kernel."""
    return _PillarMaxConcat.apply(x, group)
