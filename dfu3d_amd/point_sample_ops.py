"""DataProcessor.sample_points on csrc/pointsample_stage.hip (C ABI: csrc/dfu3d_smp.h): for a whole batch in LAUNCHES
kernel launches, a cloud of exactly `num_points` rows per scene -- the far rows kept while they fit, rows repeated where
the scene is short -- in a shuffled order.

sample_points  points (R, 1 + C) by scene, point_cnt int32 (B) -> (B * num_points, 1 + out_cols), column 0 the scene index.

The rule (which rows, in which order) is stated in the header; it is a pure function of the input and of three blocks of
random words: `sel` (R) ranks the rows of a scene, `ord` (B, K) orders the output slots, `rep` (B, K) draws the repeated
rows of a scene with fewer than K / 2 rows.  They are drawn here with torch.randint on the device unless given.  float32
and contiguous, anything else raises Dfu3dError.  Every element of the output is written by the kernels (torch.empty
here); one scratch tensor per call.  Nothing in this module reads from the device."""
import torch

from . import _lib_smp
from ._lib import Dfu3dError
from .stages import _chk, _stream

K = _lib_smp.CONSTANTS
LAUNCHES = K["DFU3D_SMP_LAUNCHES"]
MAX_OUT = K["DFU3D_SMP_MAX_OUT"]
MAX_BATCH = K["DFU3D_SMP_MAX_BATCH"]
MAX_ELEMS = K["DFU3D_SMP_MAX_ELEMS"]
EMPTY_SCENE = K["DFU3D_SMP_EMPTY_SCENE"]
BAD_COUNT = K["DFU3D_SMP_BAD_COUNT"]
STATUS_TEXT = {EMPTY_SCENE: "a scene without points", BAD_COUNT: "point_cnt is negative or sums beyond the rows of points"}


def status_message(word):
    return "; ".join(t for b, t in STATUS_TEXT.items() if word & b) or "ok"


def draw_words(R, B, num_points, device, generator=None):
    """The three blocks of random words of one call: sel int32 (R), ord and rep int32 (B, num_points), every bit drawn."""
    def draw(*shape):
        return torch.randint(-2 ** 31, 2 ** 31, shape, dtype=torch.int32, device=device, generator=generator)
    return draw(R), draw(B, num_points), draw(B, num_points)


def sample_points(points, point_cnt, num_points, out_cols=None, generator=None, words=None, status=None):
    """points float32 (R, 1 + C), C >= 3: scene b owns the point_cnt[b] rows behind those of the scenes before it (the
    output form of world_aug_collate; rows at or beyond sum(point_cnt) are never read); point_cnt int32 (B); num_points:
    rows per scene, 1 .. MAX_OUT; out_cols: feature columns to copy, 3 .. C (default C); generator: the torch.Generator
    of the draw; words: (sel, ord, rep) instead of a draw; status: int32 (1) the DFU3D_SMP_* bits are OR-ed into (default:
    a fresh zero word) -> (out float32 (B * num_points, 1 + out_cols), status)."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] < 4:
        raise Dfu3dError("sample_points: points must have the shape (R, 1 + C) with C >= 3, got %s"
                         % (tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__,))
    if not isinstance(point_cnt, torch.Tensor) or point_cnt.dim() != 1:
        raise Dfu3dError("sample_points: point_cnt must be an int32 tensor (B)")
    R, C = int(points.shape[0]), int(points.shape[1]) - 1
    B, k = int(point_cnt.shape[0]), int(num_points)
    out_cols = C if out_cols is None else int(out_cols)
    if k < 1 or not 3 <= out_cols <= C:
        raise Dfu3dError("sample_points: num_points = %d (1 or more), out_cols = %d (3 .. %d)" % (k, out_cols, C))
    if k > MAX_OUT or B > MAX_BATCH or max(R * (1 + C), B * k * (1 + out_cols)) > MAX_ELEMS:
        raise Dfu3dError("sample_points: num_points = %d (at most %d), B = %d (at most %d), R = %d is out of range "
                         "(DFU3D_ERANGE)" % (k, MAX_OUT, B, MAX_BATCH, R))
    dev = points.device
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty((B * k, 1 + out_cols), dtype=torch.float32, device=dev)
    if B == 0:
        return out, status
    if words is None:
        words = draw_words(R, B, k, dev, generator)
    sel, order, rep = words
    for name, w, shape in (("sel", sel, (R,)), ("ord", order, (B, k)), ("rep", rep, (B, k))):
        if not isinstance(w, torch.Tensor) or tuple(w.shape) != shape:
            raise Dfu3dError("sample_points: %s must be an int32 tensor %s" % (name, shape))
    if any(t.device != dev for t in (point_cnt, sel, order, rep, status)):
        raise Dfu3dError("sample_points: every operand must live on the GPU of points")
    L = _lib_smp.lib()
    nbytes = int(L.dfu3d_smp_scratch_bytes(B, R, k))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = L.dfu3d_sample_points(
        _chk(points, "sample_points: points", torch.float32) if R else None,
        _chk(point_cnt, "sample_points: point_cnt", torch.int32), B, R, C, k, out_cols,
        _chk(sel, "sample_points: sel", torch.int32) if R else None, _chk(order, "sample_points: ord", torch.int32),
        _chk(rep, "sample_points: rep", torch.int32), _chk(scratch, "sample_points: scratch", torch.uint8, min_numel=16),
        nbytes, _chk(out, "sample_points: out", torch.float32), _chk(status, "sample_points: status", torch.int32, numel=1),
        _stream())
    _lib_smp.check(rc, "dfu3d_sample_points")
    return out, status
