"""The PointNet++ set-abstraction ops on csrc/pointnet2_stage.hip (C ABI: include/dfu3d_pn2.h).

Plain functions over the entry points -- fps, ball_query, group, three_nn, three_interpolate, invert, gather_backward,
check_batch -- and the autograd functions built on them: query_group (QueryAndGroup's output in one launch),
grouping (the plain grouping_operation) and interpolate.  Coordinates (B, N, 3), features (B, C, N), float32 and
contiguous, indices int32: anything else raises Dfu3dError (mixed precision is out of scope).  Nothing here reads from
the device: the status bits of the calls are ORed into the word of the enclosing `status_scope`, which its owner reads
when it wants to (PointNet2MSG: once per forward), or into a fresh word nobody reads.

Both backwards are ONE ordered gather over the inverse of the index tensor (`inverse_of`): built on the first backward
that needs it, kept on the index tensor, reused by every backward that shares that tensor."""
import contextlib
import ctypes

import torch

from . import _lib_pn2
from ._lib import Dfu3dError

K = _lib_pn2.CONSTANTS
ST_BAD_POINT = K["DFU3D_PN2_ST_BAD_POINT"]
ST_BAD_INDEX = K["DFU3D_PN2_ST_BAD_INDEX"]
ST_BAD_BATCH = K["DFU3D_PN2_ST_BAD_BATCH"]
MAX_POINTS = K["DFU3D_PN2_MAX_POINTS"]
MAX_SCALES = K["DFU3D_PN2_MAX_SCALES"]
FPS_ONCHIP = K["DFU3D_PN2_FPS_ONCHIP"]

STATUS_TEXT = {
    ST_BAD_POINT: "a non-finite coordinate in farthest point sampling (the picks are unspecified)",
    ST_BAD_INDEX: "an index outside its point set (point 0 was read, or the entry left out)",
    ST_BAD_BATCH: "a row of the stacked points does not belong to sample row // points_per_sample",
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


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def _want(t, what, dtype, shape, dev=None):
    """t: a contiguous tensor of `dtype` on the GPU (on `dev` if given) whose shape matches `shape` (None: any size)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (dev is not None and t.device != dev):
        raise Dfu3dError("%s must be a tensor on the GPU%s" % (what, "" if dev is None else " of the other arguments"))
    if t.dtype != dtype or not t.is_contiguous():
        raise Dfu3dError("%s must be contiguous %s, got %s%s"
                         % (what, dtype, t.dtype, "" if t.is_contiguous() else ", not contiguous"))
    if t.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(t.shape, shape)):
        raise Dfu3dError("%s must have the shape %s, got %s"
                         % (what, tuple("*" if s is None else s for s in shape), tuple(t.shape)))
    if t.numel() == 0:
        raise Dfu3dError("%s is empty" % what)
    return t


def fps(xyz, npoint):
    """xyz (B, N, 3) -> idx int32 (B, npoint), new_xyz (B, npoint, 3) = xyz[idx]; the lowest index among equal maxima."""
    _want(xyz, "fps: xyz", torch.float32, (None, None, 3))
    B, N, npoint = int(xyz.shape[0]), int(xyz.shape[1]), int(npoint)
    if not 1 <= npoint <= N:
        raise Dfu3dError("fps: npoint = %d for %d points" % (npoint, N))
    if N > MAX_POINTS:
        raise Dfu3dError("fps: %d points, at most %d" % (N, MAX_POINTS))
    L = _lib_pn2.lib()
    nbytes = L.dfu3d_pn2_scratch_bytes(B, N, 0)
    if nbytes < 0:
        raise Dfu3dError("fps: xyz %s is out of range" % (tuple(xyz.shape),))
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=xyz.device) if nbytes else None
    idx = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
    new_xyz = torch.empty((B, npoint, 3), dtype=torch.float32, device=xyz.device)
    rc = L.dfu3d_pn2_fps(_p(xyz), B, N, npoint, _p(idx), _p(new_xyz), _p(scratch), _p(_status(xyz.device)), _stream())
    _lib_pn2.check(rc, "dfu3d_pn2_fps")
    return idx, new_xyz


def ball_query(xyz, centres, radii, nsamples):
    """xyz (B, N, 3), centres (B, M, 3), up to MAX_SCALES (radius, nsample) pairs -> [idx int32 (B, M, nsample)], all in
    one launch."""
    _want(xyz, "ball_query: xyz", torch.float32, (None, None, 3))
    B, N = int(xyz.shape[0]), int(xyz.shape[1])
    _want(centres, "ball_query: centres", torch.float32, (B, None, 3), xyz.device)
    M = int(centres.shape[1])
    radii, nsamples = [float(r) for r in radii], [int(n) for n in nsamples]
    if len(radii) != len(nsamples) or not 1 <= len(radii) <= MAX_SCALES:
        raise Dfu3dError("ball_query: %d radii and %d sample counts, between 1 and %d pairs"
                         % (len(radii), len(nsamples), MAX_SCALES))
    if any(n < 1 for n in nsamples) or any(r != r for r in radii):
        raise Dfu3dError("ball_query: nsample must be positive and the radius a number, got %s %s" % (radii, nsamples))
    out = [torch.empty((B, M, n), dtype=torch.int32, device=xyz.device) for n in nsamples]
    r, n, o = radii + [0.0], nsamples + [1], out + [None]
    rc = _lib_pn2.lib().dfu3d_pn2_ball_query(_p(xyz), _p(centres), B, N, M, len(radii), r[0], n[0], _p(o[0]), r[1], n[1],
                                             _p(o[1]), _stream())
    _lib_pn2.check(rc, "dfu3d_pn2_ball_query")
    return out


def _check_idx3(idx, what, B, dev):
    _want(idx, what, torch.int32, (B, None, None), dev)
    return int(idx.shape[1]), int(idx.shape[2])


def group(xyz, centres, features, idx, use_xyz=True):
    """The forward of QueryAndGroup for one scale: (B, (3 if use_xyz) + C, M, nsample); features may be None with use_xyz,
    xyz and centres may be None without."""
    if features is None and not use_xyz:
        raise Dfu3dError("group: no features and no xyz")
    lead = xyz if use_xyz else features
    B, dev = int(lead.shape[0]) if isinstance(lead, torch.Tensor) and lead.dim() == 3 else -1, getattr(lead, "device", None)
    C = 0
    if use_xyz:
        _want(xyz, "group: xyz", torch.float32, (None, None, 3))
        N = int(xyz.shape[1])
    if features is not None:
        _want(features, "group: features", torch.float32, (B, None, None) if use_xyz else (None, None, None), dev)
        C = int(features.shape[1])
        if use_xyz and int(features.shape[2]) != N:
            raise Dfu3dError("group: features %s for %d points" % (tuple(features.shape), N))
        N = int(features.shape[2])
    M, ns = _check_idx3(idx, "group: idx", B, dev)
    if use_xyz:
        _want(centres, "group: centres", torch.float32, (B, M, 3), dev)
    out = torch.empty((B, (3 if use_xyz else 0) + C, M, ns), dtype=torch.float32, device=dev)
    rc = _lib_pn2.lib().dfu3d_pn2_group(_p(xyz) if use_xyz else None, _p(centres) if use_xyz else None, _p(features),
                                        _p(idx), B, N, M, ns, C, 1 if use_xyz else 0, _p(out), _p(_status(dev)), _stream())
    _lib_pn2.check(rc, "dfu3d_pn2_group")
    return out


def three_nn(unknown, known):
    """unknown (B, n, 3), known (B, m, 3) -> dist (B, n, 3) (the distance, not its square), idx int32 (B, n, 3)."""
    _want(unknown, "three_nn: unknown", torch.float32, (None, None, 3))
    B, n = int(unknown.shape[0]), int(unknown.shape[1])
    _want(known, "three_nn: known", torch.float32, (B, None, 3), unknown.device)
    dist = torch.empty((B, n, 3), dtype=torch.float32, device=unknown.device)
    idx = torch.empty((B, n, 3), dtype=torch.int32, device=unknown.device)
    rc = _lib_pn2.lib().dfu3d_pn2_three_nn(_p(unknown), _p(known), B, n, int(known.shape[1]), _p(dist), _p(idx), _stream())
    _lib_pn2.check(rc, "dfu3d_pn2_three_nn")
    return dist, idx


def three_interpolate(features, idx, weight):
    """features (B, C, m), idx int32 (B, n, 3), weight (B, n, 3) -> (B, C, n); forward only."""
    _want(features, "three_interpolate: features", torch.float32, (None, None, None))
    B, C, m = (int(v) for v in features.shape)
    _want(idx, "three_interpolate: idx", torch.int32, (B, None, 3), features.device)
    n = int(idx.shape[1])
    _want(weight, "three_interpolate: weight", torch.float32, (B, n, 3), features.device)
    out = torch.empty((B, C, n), dtype=torch.float32, device=features.device)
    rc = _lib_pn2.lib().dfu3d_pn2_three_interpolate(_p(features), _p(idx), _p(weight), B, C, m, n, _p(out),
                                                    _p(_status(features.device)), _stream())
    _lib_pn2.check(rc, "dfu3d_pn2_three_interpolate")
    return out


class Inverse:
    """The inverse of idx (B, E) into N sources: csr int32 (B, N + 1), list int32 (B, E), the entries of a source in
    ascending entry number."""

    def __init__(self, csr, lst, N, E):
        self.csr, self.list, self.N, self.E = csr, lst, N, E


def invert(idx, N):
    """idx int32 (B, ...) with values in [0, N) -> Inverse over the flattened entries of a sample."""
    if not isinstance(idx, torch.Tensor) or idx.dim() < 2:
        raise Dfu3dError("invert: idx must be a tensor (B, ...)")
    B, N = int(idx.shape[0]), int(N)
    flat = idx.view(B, -1) if idx.is_contiguous() else idx
    _want(flat, "invert: idx", torch.int32, (B, None))
    E = int(flat.shape[1])
    L = _lib_pn2.lib()
    nbytes = L.dfu3d_pn2_scratch_bytes(B, N, E)
    if N < 1 or nbytes < 0:
        raise Dfu3dError("invert: idx %s into %d sources is out of range" % (tuple(idx.shape), N))
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=idx.device)
    csr = torch.empty((B, N + 1), dtype=torch.int32, device=idx.device)
    lst = torch.empty((B, E), dtype=torch.int32, device=idx.device)
    rc = L.dfu3d_pn2_invert(_p(flat), B, N, E, _p(csr), _p(lst), _p(scratch), _p(_status(idx.device)), _stream())
    _lib_pn2.check(rc, "dfu3d_pn2_invert")
    return Inverse(csr, lst, N, E)


def inverse_of(idx, N):
    """invert(idx, N), built once per index tensor: kept on the tensor and reused while it has not been written to."""
    kept = getattr(idx, "_dfu3d_pn2_inverse", None)
    if kept is None or kept[0] != (int(N), idx._version):
        kept = ((int(N), idx._version), invert(idx, N))
        idx._dfu3d_pn2_inverse = kept
    return kept[1]


def gather_backward(grad_out, inv, weight=None, k=1):
    """grad_out (B, C, E / k) (any trailing shape of that size), inv: Inverse, weight (B, E) or None -> (B, C, N): the
    entries of a source summed in ascending order, one float32 addition each."""
    if not isinstance(grad_out, torch.Tensor) or grad_out.dim() < 3:
        raise Dfu3dError("gather_backward: grad_out must be a tensor (B, C, ...)")
    if grad_out.dtype != torch.float32:
        raise Dfu3dError("gather_backward: the gradient must be float32, got %s" % grad_out.dtype)
    g = grad_out.contiguous()
    B, C = int(g.shape[0]), int(g.shape[1])
    _want(g, "gather_backward: grad_out", torch.float32, (B, C) + (None,) * (g.dim() - 2), inv.csr.device)
    if int(inv.csr.shape[0]) != B or g.numel() != B * C * (inv.E // k) or inv.E % k:
        raise Dfu3dError("gather_backward: grad_out %s for %d entries in groups of %d" % (tuple(g.shape), inv.E, k))
    if weight is not None:
        _want(weight, "gather_backward: weight", torch.float32, tuple(int(v) for v in weight.shape), g.device)
        if weight.numel() != B * inv.E:
            raise Dfu3dError("gather_backward: weight %s for %d entries" % (tuple(weight.shape), inv.E))
    gf = torch.empty((B, C, inv.N), dtype=torch.float32, device=g.device)
    rc = _lib_pn2.lib().dfu3d_pn2_gather_backward(_p(g), _p(weight), _p(inv.csr), _p(inv.list), B, C, inv.N, inv.E, k,
                                                  _p(gf), _stream())
    _lib_pn2.check(rc, "dfu3d_pn2_gather_backward")
    return gf


def check_batch(points, batch_size):
    """points (rows, cols >= 4): column 0 of row r must be r // (rows / batch_size); a mismatch sets ST_BAD_BATCH."""
    _want(points, "check_batch: points", torch.float32, (None, None))
    rows, cols = int(points.shape[0]), int(points.shape[1])
    if batch_size < 1 or rows % batch_size or cols < 4:
        raise Dfu3dError("check_batch: points %s for a batch of %d" % (tuple(points.shape), batch_size))
    rc = _lib_pn2.lib().dfu3d_pn2_check_batch(_p(points), rows, cols, rows // batch_size, _p(_status(points.device)),
                                              _stream())
    _lib_pn2.check(rc, "dfu3d_pn2_check_batch")


class _QueryGroup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, xyz, centres, idx, use_xyz):
        out = group(xyz, centres, features, idx, use_xyz)
        ctx.idx, ctx.N, ctx.skip = idx, int(features.shape[2]), 3 if use_xyz else 0
        return out

    @staticmethod
    def backward(ctx, grad_out):
        gf = gather_backward(grad_out[:, ctx.skip:], inverse_of(ctx.idx, ctx.N))
        return gf, None, None, None, None


def query_group(xyz, centres, features, idx, use_xyz=True):
    """group() with the gradient of the features (xyz and the centres get none, as in the reference's use)."""
    if features is None or not features.requires_grad:
        return group(xyz, centres, features, idx, use_xyz)
    return _QueryGroup.apply(features, xyz, centres, idx, use_xyz)


def grouping(features, idx):
    """The plain grouping_operation: features (B, C, N), idx (B, M, nsample) -> (B, C, M, nsample)."""
    return query_group(None, None, features, idx, use_xyz=False)


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        out = three_interpolate(features, idx, weight)
        ctx.idx, ctx.weight, ctx.m = idx, weight, int(features.shape[2])
        return out

    @staticmethod
    def backward(ctx, grad_out):
        gf = gather_backward(grad_out, inverse_of(ctx.idx, ctx.m), ctx.weight, 3)
        return gf, None, None


def interpolate(features, idx, weight):
    """three_interpolate() with the gradient of the features."""
    if not features.requires_grad:
        return three_interpolate(features, idx, weight)
    return _Interpolate.apply(features, idx, weight.detach())
