"""DataProcessor.transform_points_to_voxels and MeanVFE on csrc/hardvoxel_stage.hip (C ABI: csrc/dfu3d_hvox.h): for a whole
batch in LAUNCHES kernel launches, at most `max_voxels` voxels per scene in first-seen order with at most `max_points`
rows each, and the mean of every voxel's rows.

hard_voxels  points (R, 1 + C) by scene, point_cnt int32 (B) -> HardVoxels, the padded-form tensors of V_cap =
             min(B * max_voxels, R) rows; `n_voxels` (on the device) says how many of them are voxels.

The rule (which row goes to which voxel and slot) is stated in the header; the result is a pure function of the input.
float32 and contiguous, anything else raises Dfu3dError.  Every element of every output is written by the kernels
(torch.empty here); one scratch tensor per call, on the current stream.  Nothing in this module reads from the device."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib_hvox
from ._lib import Dfu3dError
from .stages import _chk, _stream

K = _lib_hvox.CONSTANTS
LAUNCHES = K["DFU3D_HVOX_LAUNCHES"]
MAX_POINTS = K["DFU3D_HVOX_MAX_POINTS"]
MAX_BATCH = K["DFU3D_HVOX_MAX_BATCH"]
MAX_ELEMS = K["DFU3D_HVOX_MAX_ELEMS"]
KEY_BITS = K["DFU3D_HVOX_KEY_BITS"]
BAD_POINT = K["DFU3D_HVOX_ST_BAD_POINT"]
BAD_COUNT = K["DFU3D_HVOX_ST_BAD_COUNT"]
STATUS_TEXT = {BAD_POINT: "a point with a non-finite x, y or z",
               BAD_COUNT: "point_cnt is negative or sums beyond the rows of points"}

HardVoxels = collections.namedtuple(
    "HardVoxels", "voxels voxel_mean voxel_coords voxel_num_points voxel_cnt n_voxels point_voxel status")


def status_message(word):
    return "; ".join(t for b, t in STATUS_TEXT.items() if word & b) or "ok"


def voxel_cap(B, R, max_voxels):
    """Rows of the padded outputs."""
    return min(B * int(max_voxels), R)


def hard_voxels(points, point_cnt, point_cloud_range, voxel_size, grid_size, max_points, max_voxels, out_cols=None,
                want_voxels=True, want_mean=False, status=None):
    """points float32 (R, 1 + C), C >= 3: scene b owns the point_cnt[b] rows behind those of the scenes before it (the
    output form of world_aug_collate / sample_points; rows at or beyond sum(point_cnt) are never read); point_cnt int32
    (B); point_cloud_range: 6 values, the first three are used (rounded to float32); voxel_size: 3 values (rounded to
    float32); grid_size: 3 ints (x, y, z); out_cols: feature columns to copy, 3 .. C (default C); status: int32 (1) the
    DFU3D_HVOX_ST_* bits are OR-ed into (default: a fresh zero word) -> HardVoxels; `voxels` is None without
    want_voxels, `voxel_mean` without want_mean."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] < 4:
        raise Dfu3dError("hard_voxels: points must have the shape (R, 1 + C) with C >= 3, got %s"
                         % (tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__,))
    if not isinstance(point_cnt, torch.Tensor) or point_cnt.dim() != 1:
        raise Dfu3dError("hard_voxels: point_cnt must be an int32 tensor (B)")
    if not (want_voxels or want_mean):
        raise Dfu3dError("hard_voxels: one of want_voxels / want_mean at least")
    R, C = int(points.shape[0]), int(points.shape[1]) - 1
    B, T, mv = int(point_cnt.shape[0]), int(max_points), int(max_voxels)
    out_cols = C if out_cols is None else int(out_cols)
    rmin = np.asarray(point_cloud_range, np.float64).reshape(-1)[:3].astype(np.float32)
    vs = np.asarray(voxel_size, np.float64).reshape(-1).astype(np.float32)
    grid = np.asarray(grid_size).reshape(-1)
    if rmin.shape != (3,) or vs.shape != (3,) or grid.shape != (3,):
        raise Dfu3dError("hard_voxels: point_cloud_range, voxel_size and grid_size must have 3 values for x, y, z")
    if T < 1 or mv < 1 or not 3 <= out_cols <= C or (grid < 1).any() or not (np.isfinite(vs).all() and (vs > 0).all()) \
            or not np.isfinite(rmin).all():
        raise Dfu3dError("hard_voxels: max_points = %d, max_voxels = %d (1 or more), out_cols = %d (3 .. %d), grid %s, "
                         "voxel size %s" % (T, mv, out_cols, C, grid.tolist(), vs.tolist()))
    cap = voxel_cap(B, R, mv)
    cells = max(B, 1) * int(grid[0]) * int(grid[1]) * int(grid[2])
    if T > MAX_POINTS or B > MAX_BATCH or cells >= 1 << KEY_BITS or (grid > 2 ** 31 - 1).any() \
            or max(R * (1 + C), cap * 4, cap * T * out_cols) > MAX_ELEMS:
        raise Dfu3dError("hard_voxels: max_points = %d (at most %d), B = %d (at most %d), grid %s, R = %d is out of range "
                         "(DFU3D_ERANGE)" % (T, MAX_POINTS, B, MAX_BATCH, grid.tolist(), R))
    dev = points.device
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)

    def empty(rows, *rest, dtype=torch.int32):
        # (a block of no rows still has an address the library may be given)
        return torch.empty((max(rows, 1),) + rest, dtype=dtype, device=dev)[:rows]
    out = HardVoxels(empty(cap, T, out_cols, dtype=torch.float32) if want_voxels else None,
                     empty(cap, out_cols, dtype=torch.float32) if want_mean else None,
                     empty(cap, 4), empty(cap), empty(B), empty(1), empty(R), status)
    if B == 0:
        out.n_voxels.zero_()
        return out
    if any(t.device != dev for t in (point_cnt, status)):
        raise Dfu3dError("hard_voxels: every operand must live on the GPU of points")
    L = _lib_hvox.lib()
    nbytes = int(L.dfu3d_hvox_scratch_bytes(B, R))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    c_rmin, c_vs = (ctypes.c_float * 3)(*rmin.tolist()), (ctypes.c_float * 3)(*vs.tolist())
    c_grid = (ctypes.c_int32 * 3)(*[int(g) for g in grid])

    def ptr(t, name, dtype):
        return None if t is None else _chk(t, "hard_voxels: " + name, dtype)
    rc = L.dfu3d_hard_voxels(
        ptr(points, "points", torch.float32) if R else None, ptr(point_cnt, "point_cnt", torch.int32), B, R, C,
        ctypes.cast(c_rmin, ctypes.c_void_p), ctypes.cast(c_vs, ctypes.c_void_p), ctypes.cast(c_grid, ctypes.c_void_p),
        T, mv, out_cols, _chk(scratch, "hard_voxels: scratch", torch.uint8, min_numel=16), nbytes,
        ptr(out.voxel_cnt, "voxel_cnt", torch.int32), ptr(out.n_voxels, "n_voxels", torch.int32),
        ptr(out.voxel_coords, "voxel_coords", torch.int32), ptr(out.voxel_num_points, "voxel_num_points", torch.int32),
        ptr(out.voxels, "voxels", torch.float32), ptr(out.voxel_mean, "voxel_mean", torch.float32),
        ptr(out.point_voxel, "point_voxel", torch.int32), _chk(status, "hard_voxels: status", torch.int32, numel=1),
        _stream())
    _lib_hvox.check(rc, "dfu3d_hard_voxels")
    return out


def voxel_mean(voxels, voxel_num_points):
    """THE MEAN of the header over a (V, T, C) block as hard_voxels makes it (empty slots +0.0): acc = +0.0, the slots
    added one by one in float32, divided by max(count, 1).  Sequential float32 additions in slot order are what the
    stage's voxel_mean holds, bit for bit: adding the +0.0 of an empty slot changes no bit of acc."""
    if voxels.dim() != 3 or voxel_num_points.shape != voxels.shape[:1]:
        raise Dfu3dError("voxel_mean: voxels (V, T, C) and voxel_num_points (V)")
    acc = torch.zeros(voxels.shape[0], voxels.shape[2], dtype=torch.float32, device=voxels.device)
    for s in range(voxels.shape[1]):
        acc = acc + voxels[:, s, :]
    return acc / torch.clamp_min(voxel_num_points, 1).to(torch.float32).unsqueeze(1)
