"""The batched FOV ingest on csrc/ingest_stage.hip (C ABI, keep rule and box rule: include/dfu3d_ingest.h).

`fov_ingest(points, point_off, calib, image_shape, ...)` takes the raw points of B frames, one after the other, with one
calibration record (`Calibration.record()`) and one image shape per frame, and returns -- all on the device, without a
host read -- the rows inside each frame's own camera image, compacted in frame order (DFU3D_ING_EMIT), and / or the number
of kept points inside every labelled box of a frame (DFU3D_ING_COUNT).  At most DFU3D_ING_LAUNCHES launches, whatever B.
Arguments are validated here, shapes and dtypes first, and anything else raises Dfu3dError."""
import ctypes
from collections import namedtuple

import torch

from . import _lib_ingest
from ._header import CONSTANTS as _ABI
from ._lib import Dfu3dError

K = _lib_ingest.CONSTANTS
EMIT, COUNT = K["DFU3D_ING_EMIT"], K["DFU3D_ING_COUNT"]
CHUNK = K["DFU3D_ING_CHUNK"]
LAUNCHES = K["DFU3D_ING_LAUNCHES"]
ST_OFFSETS, ST_SHAPE = K["DFU3D_ING_ST_OFFSETS"], K["DFU3D_ING_ST_SHAPE"]
MAX_ROWS, MAX_SCENES, MAX_COLS, MAX_BOXES = (K["DFU3D_ING_MAX_" + n] for n in ("ROWS", "SCENES", "POINT_COLS", "BOXES"))
CALIB_FLOATS = _ABI["DFU3D_CALIB_FLOATS"]

STATUS_TEXT = {ST_OFFSETS: "an offset table is not ascending from 0 to its array's length",
               ST_SHAPE: "an image side below 0 or beyond %d" % K["DFU3D_ING_MAX_SIDE"]}

FovIngest = namedtuple("FovIngest", "points out_off box_cnt status")
FovIngest.__doc__ = """points: float32 (n_rows, C), the kept rows first (None without EMIT); out_off: int64 (B + 1), the
kept rows of frame b are points[out_off[b]:out_off[b + 1]] (None without EMIT); box_cnt: int32 (n_boxes) (None without
COUNT); status: int32 (1), the DFU3D_ING_ST_* bits ORed in.  All on the device."""


def status_message(s):
    return "; ".join(t for b, t in STATUS_TEXT.items() if s & b)


def _check(t, what, dtype, shape):
    """shape: one entry per dimension, None for any length."""
    if not isinstance(t, torch.Tensor):
        raise Dfu3dError("fov_ingest: %s must be a tensor, got %s" % (what, type(t).__name__))
    if t.dtype != dtype:
        raise Dfu3dError("fov_ingest: %s must be %s, got %s" % (what, str(dtype).replace("torch.", ""), t.dtype))
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise Dfu3dError("fov_ingest: %s must be (%s), got %s"
                         % (what, ", ".join("n" if s is None else str(s) for s in shape), tuple(t.shape)))
    if not t.is_contiguous():
        raise Dfu3dError("fov_ingest: %s must be contiguous, strides %s" % (what, t.stride()))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def fov_ingest(points, point_off, calib, image_shape, boxes=None, box_off=None, mode=EMIT, status=None):
    """points float32 (sum n, C >= 3); point_off int64 (B + 1); calib float32 (B, DFU3D_CALIB_FLOATS); image_shape
    int32 (B, 2) rows (h, w); boxes float64 (sum m, 7) with box_off int32 (B + 1), both needed with DFU3D_ING_COUNT and
    not looked at without it; status: an int32 (1) tensor to OR into (a fresh zero one if None).  -> FovIngest."""
    if not isinstance(mode, int) or mode & ~(EMIT | COUNT) or not mode & (EMIT | COUNT):
        raise Dfu3dError("fov_ingest: mode must be DFU3D_ING_EMIT, DFU3D_ING_COUNT or both, got %r" % (mode,))
    _check(points, "points", torch.float32, (None, None))
    C = points.shape[1]
    if not 3 <= C <= MAX_COLS:
        raise Dfu3dError("fov_ingest: points must have 3 .. %d columns, got %d" % (MAX_COLS, C))
    _check(calib, "calib", torch.float32, (None, CALIB_FLOATS))
    B = calib.shape[0]
    if not 1 <= B <= MAX_SCENES:
        raise Dfu3dError("fov_ingest: %d frames, between 1 and %d" % (B, MAX_SCENES))
    _check(point_off, "point_off", torch.int64, (B + 1,))
    _check(image_shape, "image_shape", torch.int32, (B, 2))
    n_rows = points.shape[0]
    if n_rows > MAX_ROWS:
        raise Dfu3dError("fov_ingest: %d rows, at most %d" % (n_rows, MAX_ROWS))
    tensors = [("points", points), ("point_off", point_off), ("calib", calib), ("image_shape", image_shape)]
    n_boxes = 0
    if not mode & COUNT:
        boxes = box_off = None
    else:
        if boxes is None or box_off is None:
            raise Dfu3dError("fov_ingest: DFU3D_ING_COUNT needs boxes and box_off")
        _check(boxes, "boxes", torch.float64, (None, 7))
        _check(box_off, "box_off", torch.int32, (B + 1,))
        n_boxes = boxes.shape[0]
        if n_boxes > MAX_BOXES:
            raise Dfu3dError("fov_ingest: %d boxes, at most %d" % (n_boxes, MAX_BOXES))
        tensors += [("boxes", boxes), ("box_off", box_off)]
    if status is not None:
        _check(status, "status", torch.int32, (1,))
        tensors.append(("status", status))
    dev = points.device
    for what, t in tensors:
        if not t.is_cuda:
            raise Dfu3dError("fov_ingest: %s must be on the GPU, it is on %s" % (what, t.device))
        if t.device != dev:
            raise Dfu3dError("fov_ingest: %s is on %s, points on %s" % (what, t.device, dev))
    L = _lib_ingest.lib()
    with torch.cuda.device(dev):
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=dev)
        nbytes = L.dfu3d_fov_ingest_scratch_bytes(n_rows)
        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        out = torch.empty_like(points) if mode & EMIT else None
        out_off = torch.empty(B + 1, dtype=torch.int64, device=dev) if mode & EMIT else None
        box_cnt = torch.empty(n_boxes, dtype=torch.int32, device=dev) if mode & COUNT else None
        rc = L.dfu3d_fov_ingest(_ptr(points), n_rows, C, _ptr(point_off), B, _ptr(calib), _ptr(image_shape), _ptr(boxes),
                                n_boxes, _ptr(box_off), mode, _ptr(out), _ptr(out_off), _ptr(box_cnt), _ptr(scratch),
                                nbytes, _ptr(status), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib_ingest.check(rc, "dfu3d_fov_ingest")
    return FovIngest(out, out_off, box_cnt, status)
