"""The stacked set-abstraction ops without a GPU: the agreement of csrc/dfu3d_stk.h with its binding, host-side argument
validation before any launch, and the Python layer's refusals."""
import ctypes
import os

import pytest

from dfu3d_amd import _build, _lib, _lib_stk

P16 = ctypes.c_void_p(16)            # a non-null, 16-byte aligned address no call may touch
P32 = ctypes.c_void_p(32)
SYMBOLS = ['dfu3d_stk_ball_query', 'dfu3d_stk_bev_sample', 'dfu3d_stk_counts', 'dfu3d_stk_fps',
           'dfu3d_stk_fps_scratch_bytes', 'dfu3d_stk_global_index', 'dfu3d_stk_group', 'dfu3d_stk_starts',
           'dfu3d_stk_version']


def test_header_and_binding_agree():
    assert _lib_stk.HEADER == os.path.join(_build.CSRC, "dfu3d_stk.h") and _lib_stk.HEADER in _build._deps()
    assert _lib_stk.header_symbols() == SYMBOLS
    L = _lib_stk.lib()
    assert all(hasattr(L, s) for s in SYMBOLS)
    assert L.dfu3d_stk_version() == _lib_stk.header_version() == 1
    K = _lib_stk.CONSTANTS
    assert all(k.startswith("DFU3D_STK_") for k in K)
    from dfu3d_amd import _lib_pn2
    assert K['DFU3D_STK_MAX_SCALES'] == _lib_pn2.CONSTANTS['DFU3D_PN2_MAX_SCALES']
    assert K['DFU3D_STK_FPS_ONCHIP'] == _lib_pn2.CONSTANTS['DFU3D_PN2_FPS_ONCHIP'] == 16384
    assert K['DFU3D_STK_MAX_ELEMS'] == 2 ** 31 - 1
    bits = [K['DFU3D_STK_ST_' + n] for n in ('BAD_POINT', 'BAD_INDEX', 'BAD_BATCH', 'UNSORTED', 'EMPTY', 'BAD_COUNT')]
    assert bits == [1, 2, 4, 8, 16, 32]
    nargs = {'dfu3d_stk_counts': 9, 'dfu3d_stk_starts': 5, 'dfu3d_stk_fps': 12, 'dfu3d_stk_ball_query': 20,
             'dfu3d_stk_group': 17, 'dfu3d_stk_global_index': 11, 'dfu3d_stk_bev_sample': 16}
    for name, n in nargs.items():
        res, args = _lib_stk.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == n and args[-1] is ctypes.c_void_p, name
    assert _lib_stk.SIGNATURES['dfu3d_stk_fps_scratch_bytes'] == (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32])
    assert not set(_lib_stk.SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib_pn2.SIGNATURES))
    from dfu3d_amd import point_stack_ops as ops
    from tests import point_stack_ref as R
    assert (ops.ST_BAD_POINT, ops.ST_BAD_INDEX, ops.ST_BAD_BATCH, ops.ST_UNSORTED, ops.ST_EMPTY, ops.ST_BAD_COUNT) == \
        (R.ST_BAD_POINT, R.ST_BAD_INDEX, R.ST_BAD_BATCH, R.ST_UNSORTED, R.ST_EMPTY, R.ST_BAD_COUNT)
    assert set(ops.LAUNCHES) >= {"counts", "fps", "ball_query", "group", "bev_sample", "group_backward"}
    assert all(ops.status_message(b) for b in bits)


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
    for s in SYMBOLS:
        if s not in ('dfu3d_stk_fps', 'dfu3d_stk_group'):
            setattr(Fake, s, object())
    with pytest.raises(_lib.Dfu3dError, match="dfu3d_stk_fps, dfu3d_stk_group"):
        _lib_stk.bind(Fake())


def _counts(L, col=P16, is_int=0, rows=64, stride=4, B=2, cnt=P16, start=P16, status=P16):
    return L.dfu3d_stk_counts(col, is_int, rows, stride, B, cnt, start, status, None)


def _starts(L, cnt=P16, B=2, start=P16, status=P16):
    return L.dfu3d_stk_starts(cnt, B, start, status, None)


def _fps(L, xyz=P16, stride=3, rows=64, start=P16, B=2, K=8, cap=0, idx=P16, kp=P16, scratch=None, status=P16):
    return L.dfu3d_stk_fps(xyz, stride, rows, start, B, K, cap, idx, kp, scratch, status, None)


def _ball(L, xyz=P16, stride=3, N=64, start=P16, ctr=P16, cstride=3, M=8, cstart=P16, B=2, S=2, r0=0.5, n0=4, i0=P16,
          e0=P16, r1=1.0, n1=8, i1=P32, e1=P32, status=P16):
    return L.dfu3d_stk_ball_query(xyz, stride, N, start, ctr, cstride, M, cstart, B, S, r0, n0, i0, e0, r1, n1, i1, e1,
                                  status, None)


def _group(L, xyz=P16, stride=3, N=64, start=P16, ctr=P16, cstride=3, M=8, cstart=P16, B=2, feat=P16, C=5, idx=P16,
           empty=P16, ns=4, out=P16, status=P16):
    return L.dfu3d_stk_group(xyz, stride, N, start, ctr, cstride, M, cstart, B, feat, C, idx, empty, ns, out, status, None)


def _gidx(L, idx=P16, empty=P16, M=8, ns=4, N=64, start=P16, cstart=P16, B=2, gidx=P16, status=P16):
    return L.dfu3d_stk_global_index(idx, empty, M, ns, N, start, cstart, B, gidx, status, None)


def _bev(L, kp=P16, kstride=4, M=8, sp=P16, B=2, C=3, H=5, W=7, out=P32, status=P16):
    return L.dfu3d_stk_bev_sample(kp, kstride, M, sp, B, C, H, W, 0.0, -1.0, 0.5, 0.5, 2.0, out, status, None)


def test_bad_arguments_return_before_any_launch():
    """Every call below passes pointers no kernel may touch: a launch would fault (or, without a GPU, fail with
    DFU3D_ELAUNCH); each must come back with the validation's own code."""
    L = _lib_stk.lib()
    EINVAL, ERANGE = _lib.CONSTANTS["DFU3D_EINVAL"], _lib.CONSTANTS["DFU3D_ERANGE"]
    MAXB, MAXE = _lib_stk.CONSTANTS['DFU3D_STK_MAX_BATCH'], _lib_stk.CONSTANTS['DFU3D_STK_MAX_ELEMS']
    for name in ('col', 'cnt', 'start', 'status'):
        assert _counts(L, **{name: None}) == EINVAL, name
    assert _counts(L, B=0) == EINVAL and _counts(L, stride=0) == EINVAL and _counts(L, rows=-1) == EINVAL
    assert _counts(L, B=MAXB + 1) == ERANGE and _counts(L, rows=2 ** 30, stride=4) == ERANGE
    for name in ('cnt', 'start', 'status'):
        assert _starts(L, **{name: None}) == EINVAL, name
    assert _starts(L, B=0) == EINVAL and _starts(L, B=MAXB + 1) == ERANGE
    for name in ('xyz', 'start', 'idx', 'kp', 'status'):
        assert _fps(L, **{name: None}) == EINVAL, name
    assert _fps(L, K=0) == EINVAL and _fps(L, B=0) == EINVAL and _fps(L, stride=2) == EINVAL and _fps(L, cap=-1) == EINVAL
    assert _fps(L, rows=-1) == EINVAL and _fps(L, rows=16385, scratch=None) == EINVAL
    assert _fps(L, rows=MAXE // 3 + 1) == ERANGE and _fps(L, B=MAXB + 1) == ERANGE and _fps(L, B=MAXB, K=2 ** 14) == ERANGE
    for name in ('xyz', 'start', 'ctr', 'cstart', 'i0', 'e0', 'i1', 'e1', 'status'):
        assert _ball(L, **{name: None}) == EINVAL, name
    assert _ball(L, n0=0) == EINVAL and _ball(L, n1=0) == EINVAL and _ball(L, S=0) == EINVAL and _ball(L, S=3) == EINVAL
    assert _ball(L, r0=float('nan')) == EINVAL and _ball(L, i1=P16) == EINVAL and _ball(L, e1=P16) == EINVAL
    assert _ball(L, stride=2) == EINVAL and _ball(L, cstride=2) == EINVAL and _ball(L, B=0) == EINVAL
    assert _ball(L, N=MAXE // 3 + 1) == ERANGE and _ball(L, M=2 ** 28, n1=8) == ERANGE
    for name in ('xyz', 'start', 'ctr', 'cstart', 'idx', 'empty', 'out', 'status'):
        assert _group(L, **{name: None}) == EINVAL, name
    assert _group(L, ns=0) == EINVAL and _group(L, C=-1) == EINVAL and _group(L, B=0) == EINVAL
    assert _group(L, M=2 ** 24, ns=64, C=5) == ERANGE and _group(L, N=2 ** 29, C=5) == ERANGE
    for name in ('idx', 'empty', 'start', 'cstart', 'gidx', 'status'):
        assert _gidx(L, **{name: None}) == EINVAL, name
    assert _gidx(L, M=0) == EINVAL and _gidx(L, ns=0) == EINVAL and _gidx(L, M=2 ** 29, ns=4) == ERANGE
    for name in ('kp', 'sp', 'out', 'status'):
        assert _bev(L, **{name: None}) == EINVAL, name
    assert _bev(L, M=0) == EINVAL and _bev(L, C=0) == EINVAL and _bev(L, H=0) == EINVAL and _bev(L, kstride=2) == EINVAL
    assert _bev(L, out=P16) == EINVAL and _bev(L, M=2 ** 30) == ERANGE and _bev(L, B=1024, C=1024, H=64, W=64) == ERANGE
    sb = L.dfu3d_stk_fps_scratch_bytes
    assert sb(-1, 0) == -1 and sb(64, -1) == -1 and sb(MAXE // 3 + 1, 0) == -1
    assert sb(0, 0) == 0 and sb(16384, 0) == 0 and sb(16385, 0) == 16385 * 4 and sb(40000, 16384) == 0
    assert sb(40000, 16385) == 40000 * 4


def test_ball_query_without_centres_needs_no_outputs():
    """M = 0: the outputs have no element, so the pointers torch gives for them are NULL; the call is a no-op, not
    DFU3D_EINVAL.  What does not depend on M is still checked."""
    L = _lib_stk.lib()
    OK, EINVAL = _lib.CONSTANTS["DFU3D_OK"], _lib.CONSTANTS["DFU3D_EINVAL"]
    none = dict(M=0, ctr=None, i0=None, e0=None, i1=None, e1=None)
    assert _ball(L, **none) == OK and _ball(L, S=1, **none) == OK
    assert _ball(L, n1=0, **none) == EINVAL and _ball(L, r0=float('nan'), **none) == EINVAL
    assert _ball(L, cstart=None, **none) == EINVAL and _ball(L, status=None, **none) == EINVAL


def test_ops_refuse_host_wrong_type_and_non_contiguous_tensors():
    import torch
    from dfu3d_amd import point_stack_ops as ops
    from dfu3d_amd._lib import Dfu3dError
    xyz, start = torch.zeros(16, 3), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(Dfu3dError, match="on the GPU"):
        ops.fps(xyz, start, 4)
    with pytest.raises(Dfu3dError, match="on the GPU"):
        ops.ball_query(xyz, start, xyz, start, [1.0], [4])
    with pytest.raises(Dfu3dError, match="on the GPU"):
        ops.counts(torch.zeros(5), 2)
    with pytest.raises(Dfu3dError, match="float32 or int32"):
        ops.counts(torch.zeros(5, dtype=torch.int64), 2)
    with pytest.raises(Dfu3dError, match="on the GPU"):
        ops.bev_sample(torch.zeros(4, 4), torch.zeros(1, 2, 3, 3), [0, 0, 0], [1, 1, 1], 1)
    with pytest.raises(NotImplementedError, match="forward only"):
        ops.bev_sample(torch.zeros(4, 4), torch.zeros(1, 2, 3, 3, requires_grad=True), [0, 0, 0], [1, 1, 1], 1)
    with pytest.raises(NotImplementedError, match="forward only"):
        ops.bev_sample(torch.zeros(4, 4, requires_grad=True), torch.zeros(1, 2, 3, 3), [0, 0, 0], [1, 1, 1], 1)

    class OnGpu(torch.Tensor):
        is_cuda = True
    meta = torch.zeros(16, 5, device='meta')
    assert ops._rows(meta[:, 1:4].as_subclass(OnGpu), "xyz", torch.float32, 3) == (16, 5)       # read in place
    assert ops._rows(torch.zeros(16, 3, device='meta').as_subclass(OnGpu), "xyz", torch.float32, 3) == (16, 3)
    for bad, what in ((meta[:, 1:4].double(), "float32"), (meta.t()[1:4].t()[:, ::2], "shape"),
                      (torch.zeros(3, 16, device='meta').t(), "adjacent columns"), (meta[:, :2], "shape")):
        with pytest.raises(Dfu3dError, match=what):
            ops._rows(bad.as_subclass(OnGpu), "xyz", torch.float32, 3)
