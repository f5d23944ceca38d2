"""Pillars into the dense BEV canvas on csrc/bevscatter_stage.hip (C ABI: include/dfu3d_bev.h).

`pillar_scatter` is an autograd function over dfu3d_pillar_scatter / dfu3d_pillar_scatter_backward: features (P, C) and
coords (P, 4) [b, z, y, x] (or (P, 3) [b, y, x]) -> the canvas (B, C * nz, ny, nx), every element written once, a pure
copy of the pillar's bits or +0.0.  Three launches forward, one backward, no host read unless check=True.  features must
be float32 and contiguous, coords int32 and contiguous (mixed precision is out of scope)."""
import ctypes

import torch

from . import _lib_bev
from ._lib import Dfu3dError

K = _lib_bev.CONSTANTS
ST_BAD_COORD = K["DFU3D_BEV_ST_BAD_COORD"]
ST_DUPLICATE = K["DFU3D_BEV_ST_DUPLICATE"]
MAX_CELLS = K["DFU3D_BEV_MAX_CELLS"]
MAX_CHANNELS = K["DFU3D_BEV_MAX_CHANNELS"]

STATUS_TEXT = {
    ST_BAD_COORD: "a pillar's batch index or cell lies outside the canvas (the row was dropped)",
    ST_DUPLICATE: "two or more pillars on one cell (the highest row index was kept)",
}


def status_message(s):
    return "; ".join(t for b, t in STATUS_TEXT.items() if s & b)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


class ScatterInfo:
    """What a pillar_scatter call leaves next to the canvas: cell_map int32 (B * nz * ny * nx), the row that owns a cell
    or -1, and status int32 (1), the DFU3D_BEV_ST_* bits of the call -- both on the device."""
    cell_map = None
    status = None


def _check_inputs(features, coords, batch_size, grid, n_pillars, out):
    if not isinstance(features, torch.Tensor) or not features.is_cuda:
        raise Dfu3dError("pillar_scatter: features must be a tensor on the GPU")
    if features.dtype != torch.float32 or features.dim() != 2 or not features.is_contiguous():
        raise Dfu3dError("pillar_scatter: features must be a contiguous float32 matrix, got %s %s"
                         % (tuple(features.shape), features.dtype))
    if not isinstance(coords, torch.Tensor) or coords.device != features.device:
        raise Dfu3dError("pillar_scatter: coords must be a tensor on the features' device")
    if coords.dtype != torch.int32 or coords.dim() != 2 or not coords.is_contiguous():
        raise Dfu3dError("pillar_scatter: coords must be a contiguous int32 matrix, got %s %s"
                         % (tuple(coords.shape), coords.dtype))
    nx, ny, nz = (int(v) for v in grid)
    B, P, C = int(batch_size), int(features.shape[0]), int(features.shape[1])
    if coords.shape[0] != P or coords.shape[1] not in (3, 4) or (coords.shape[1] == 3 and nz != 1):
        raise Dfu3dError("pillar_scatter: coords %s for %d pillars and nz = %d" % (tuple(coords.shape), P, nz))
    if B < 1 or nx < 1 or ny < 1 or nz < 1:
        raise Dfu3dError("pillar_scatter: batch_size and grid must be positive")
    if not 1 <= C <= MAX_CHANNELS:
        raise Dfu3dError("pillar_scatter: %d channels, between 1 and %d" % (C, MAX_CHANNELS))
    if B * nz * ny * nx > MAX_CELLS:
        raise Dfu3dError("pillar_scatter: %d cells, at most %d" % (B * nz * ny * nx, MAX_CELLS))
    if n_pillars is not None and (not isinstance(n_pillars, torch.Tensor) or n_pillars.device != features.device
                                  or n_pillars.dtype != torch.int32 or n_pillars.numel() < 1):
        raise Dfu3dError("pillar_scatter: n_pillars must be an int32 tensor on the features' device")
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.device != features.device or out.dtype != torch.float32
                or not out.is_contiguous() or out.numel() != B * C * nz * ny * nx):
            raise Dfu3dError("pillar_scatter: out must be a contiguous float32 tensor of %d elements on the features' device"
                             % (B * C * nz * ny * nx))
    return B, P, C, nx, ny, nz


class _PillarScatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, coords, geom, n_pillars, out, info):
        B, P, C, nx, ny, nz = geom
        dev = features.device
        canvas = out if out is not None else torch.empty((B, C * nz, ny, nx), dtype=torch.float32, device=dev)
        cell_map = torch.empty(B * nz * ny * nx, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = _lib_bev.lib().dfu3d_pillar_scatter(_p(features), _p(coords), int(coords.shape[1]), P, _p(n_pillars), C, B, nz,
                                                 ny, nx, _p(canvas), _p(cell_map), _p(status), _stream())
        _lib_bev.check(rc, "dfu3d_pillar_scatter")
        info.cell_map, info.status = cell_map, status
        ctx.geom, ctx.coords, ctx.n_pillars, ctx.cell_map = geom, coords, n_pillars, cell_map
        if out is not None:
            ctx.mark_dirty(out)
        return canvas

    @staticmethod
    def backward(ctx, grad_canvas):
        B, P, C, nx, ny, nz = ctx.geom
        if grad_canvas.dtype != torch.float32:
            raise Dfu3dError("pillar_scatter backward: the gradient must be float32, got %s" % grad_canvas.dtype)
        g = grad_canvas.contiguous()
        # rows at or beyond a device pillar count are not pillars: the stage leaves them alone, and their gradient is zero
        make = torch.zeros if ctx.n_pillars is not None else torch.empty
        gf = make((P, C), dtype=torch.float32, device=g.device)
        rc = _lib_bev.lib().dfu3d_pillar_scatter_backward(_p(g), _p(ctx.coords), int(ctx.coords.shape[1]), P,
                                                          _p(ctx.n_pillars), C, B, nz, ny, nx, _p(ctx.cell_map), _p(gf),
                                                          _stream())
        _lib_bev.check(rc, "dfu3d_pillar_scatter_backward")
        return gf, None, None, None, None, None


def pillar_scatter(features, coords, batch_size, grid, n_pillars=None, out=None, check=False, info=None):
    """features (P, C) float32, coords (P, 4) int32 [b, z, y, x] or (P, 3) [b, y, x] (nz = 1), grid (nx, ny, nz) -> the
    canvas (batch_size, C * nz, ny, nx): channel c of a pillar at depth z is canvas channel c * nz + z, as the reference's
    view of (B, C, nz, ny, nx) has it.

    n_pillars: an int32 device tensor; rows at or beyond n_pillars[0] are never read (the padded form of the chain).
    out: a contiguous float32 tensor of the canvas's size to write into (every element is written; it need not be
    cleared); the returned canvas is `out`.  info: a ScatterInfo that receives cell_map and status.
    check=True reads the status word (one host read) and raises Dfu3dError on any bit; otherwise nothing is read."""
    geom = _check_inputs(features, coords, batch_size, grid, n_pillars, out)
    B, P, C, nx, ny, nz = geom
    info = info if info is not None else ScatterInfo()
    if out is not None and tuple(out.shape) != (B, C * nz, ny, nx):
        out = out.view(B, C * nz, ny, nx)
    canvas = _PillarScatter.apply(features, coords, geom, n_pillars, out, info)
    if check:
        s = int(info.status.item())
        if s:
            raise Dfu3dError("pillar_scatter: status %d (%s)" % (s, status_message(s)))
    return canvas
