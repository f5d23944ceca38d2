"""The PointNet++ ops without a GPU: the agreement of include/dfu3d_pn2.h with its binding, host-side argument validation
before any launch, the Python layer's refusals, and the construction of the modules with the reference's keys."""
import ctypes
import os

import pytest

from dfu3d_amd import _build, _lib, _lib_pn2

P16 = ctypes.c_void_p(16)            # a non-null, 16-byte aligned address no call may touch
SYMBOLS = ['dfu3d_pn2_ball_query', 'dfu3d_pn2_check_batch', 'dfu3d_pn2_fps', 'dfu3d_pn2_gather_backward',
           'dfu3d_pn2_group', 'dfu3d_pn2_invert', 'dfu3d_pn2_scratch_bytes', 'dfu3d_pn2_three_interpolate',
           'dfu3d_pn2_three_nn', 'dfu3d_pn2_version']


def test_header_and_binding_agree():
    assert _lib_pn2.HEADER == os.path.join(_build.INCLUDE, "dfu3d_pn2.h") and _lib_pn2.HEADER in _build._deps()
    assert _lib_pn2.header_symbols() == SYMBOLS
    L = _lib_pn2.lib()
    assert all(hasattr(L, s) for s in SYMBOLS)
    assert L.dfu3d_pn2_version() == _lib_pn2.header_version() == 1
    K = _lib_pn2.CONSTANTS
    assert all(k.startswith("DFU3D_PN2_") for k in K)
    assert K['DFU3D_PN2_MAX_POINTS'] >= 65536 and K['DFU3D_PN2_MAX_SCALES'] >= 2
    assert (K['DFU3D_PN2_ST_BAD_POINT'], K['DFU3D_PN2_ST_BAD_INDEX'], K['DFU3D_PN2_ST_BAD_BATCH']) == (1, 2, 4)
    assert K['DFU3D_PN2_FPS_ONCHIP'] == 16384 and K['DFU3D_PN2_MAX_ELEMS'] == 2 ** 31 - 1
    nargs = {'dfu3d_pn2_fps': 9, 'dfu3d_pn2_ball_query': 13, 'dfu3d_pn2_group': 13, 'dfu3d_pn2_three_nn': 8,
             'dfu3d_pn2_three_interpolate': 10, 'dfu3d_pn2_invert': 9, 'dfu3d_pn2_gather_backward': 11,
             'dfu3d_pn2_check_batch': 6}
    for name, n in nargs.items():
        res, args = _lib_pn2.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == n and args[-1] is ctypes.c_void_p, name
    assert _lib_pn2.SIGNATURES['dfu3d_pn2_scratch_bytes'] == (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64])
    assert not set(_lib_pn2.SIGNATURES) & set(_lib.SIGNATURES)
    for other in ("dfu3d.h", "dfu3d_vfe.h", "dfu3d_head.h", "dfu3d_post.h", "dfu3d_aug.h", "dfu3d_bev.h", "dfu3d_opt.h",
                  "dfu3d_ingest.h"):
        assert "dfu3d_pn2" not in open(os.path.join(_build.INCLUDE, other)).read()
    from dfu3d_amd import pointnet2_ops as ops
    assert (ops.ST_BAD_POINT, ops.ST_BAD_INDEX, ops.ST_BAD_BATCH, ops.MAX_SCALES) == (1, 2, 4, K['DFU3D_PN2_MAX_SCALES'])


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
    for s in SYMBOLS:
        if s not in ('dfu3d_pn2_fps', 'dfu3d_pn2_invert'):
            setattr(Fake, s, object())
    with pytest.raises(_lib.Dfu3dError, match="dfu3d_pn2_fps, dfu3d_pn2_invert"):
        _lib_pn2.bind(Fake())


def _fps(L, xyz=P16, B=2, N=64, npoint=8, idx=P16, new_xyz=P16, scratch=None, status=P16):
    return L.dfu3d_pn2_fps(xyz, B, N, npoint, idx, new_xyz, scratch, status, None)


def _ball(L, xyz=P16, ctr=P16, B=2, N=64, M=8, S=2, r0=0.5, n0=4, i0=P16, r1=1.0, n1=8, i1=ctypes.c_void_p(32)):
    return L.dfu3d_pn2_ball_query(xyz, ctr, B, N, M, S, r0, n0, i0, r1, n1, i1, None)


def _group(L, xyz=P16, ctr=P16, feat=P16, idx=P16, B=2, N=64, M=8, ns=4, C=5, use_xyz=1, out=P16, status=P16):
    return L.dfu3d_pn2_group(xyz, ctr, feat, idx, B, N, M, ns, C, use_xyz, out, status, None)


def _nn(L, unk=P16, kn=P16, B=2, n=64, m=8, dist=P16, idx=P16):
    return L.dfu3d_pn2_three_nn(unk, kn, B, n, m, dist, idx, None)


def _interp(L, feat=P16, idx=P16, w=P16, B=2, C=4, m=8, n=64, out=ctypes.c_void_p(32), status=P16):
    return L.dfu3d_pn2_three_interpolate(feat, idx, w, B, C, m, n, out, status, None)


def _invert(L, idx=P16, B=2, N=64, E=32, csr=P16, lst=P16, scratch=P16, status=P16):
    return L.dfu3d_pn2_invert(idx, B, N, E, csr, lst, scratch, status, None)


def _bwd(L, go=P16, w=None, csr=P16, lst=P16, B=2, C=4, N=64, E=33, k=3, gf=ctypes.c_void_p(32)):
    return L.dfu3d_pn2_gather_backward(go, w, csr, lst, B, C, N, E, k, gf, None)


def _batch(L, pts=P16, rows=128, cols=5, per=64, status=P16):
    return L.dfu3d_pn2_check_batch(pts, rows, cols, per, status, None)


def test_bad_arguments_return_before_any_launch():
    """Every call below passes pointers no kernel may touch: a launch would fault (or, without a GPU, fail with
    DFU3D_ELAUNCH); each must come back with the validation's own code."""
    L = _lib_pn2.lib()
    EINVAL, ERANGE = _lib.CONSTANTS["DFU3D_EINVAL"], _lib.CONSTANTS["DFU3D_ERANGE"]
    K = _lib_pn2.CONSTANTS
    MAXP, MAXB = K['DFU3D_PN2_MAX_POINTS'], K['DFU3D_PN2_MAX_BATCH']
    for name in ('xyz', 'idx', 'new_xyz', 'status'):
        assert _fps(L, **{name: None}) == EINVAL, name
    assert _fps(L, npoint=65) == EINVAL                                   # npoint > N
    assert _fps(L, npoint=0) == EINVAL and _fps(L, N=0) == EINVAL and _fps(L, B=0) == EINVAL
    assert _fps(L, N=MAXP + 1) == ERANGE and _fps(L, B=MAXB + 1) == ERANGE
    assert _fps(L, B=4096, N=MAXP) == ERANGE                              # B * N * 3 elements
    assert _fps(L, N=K['DFU3D_PN2_FPS_ONCHIP'] + 1, scratch=None) == EINVAL
    for name in ('xyz', 'ctr', 'i0', 'i1'):
        assert _ball(L, **{name: None}) == EINVAL, name
    assert _ball(L, n0=0) == EINVAL and _ball(L, n1=0) == EINVAL and _ball(L, n1=-3) == EINVAL
    assert _ball(L, S=0) == EINVAL and _ball(L, S=K['DFU3D_PN2_MAX_SCALES'] + 1) == EINVAL
    assert _ball(L, r0=float('nan')) == EINVAL and _ball(L, i1=P16) == EINVAL
    assert _ball(L, N=MAXP + 1) == ERANGE and _ball(L, M=MAXP + 1) == ERANGE
    assert _ball(L, B=1024, M=MAXP, n1=64) == ERANGE
    for name in ('idx', 'out', 'status', 'xyz', 'ctr'):
        assert _group(L, **{name: None}) == EINVAL, name
    assert _group(L, feat=None, use_xyz=0) == EINVAL and _group(L, C=0, use_xyz=0) == EINVAL
    assert _group(L, ns=0) == EINVAL and _group(L, C=-1) == EINVAL and _group(L, M=0) == EINVAL
    assert _group(L, N=MAXP + 1) == ERANGE and _group(L, B=64, C=512, M=MAXP, ns=64) == ERANGE
    for name in ('unk', 'kn', 'dist', 'idx'):
        assert _nn(L, **{name: None}) == EINVAL, name
    assert _nn(L, m=0) == EINVAL and _nn(L, n=0) == EINVAL and _nn(L, m=MAXP + 1) == ERANGE
    for name in ('feat', 'idx', 'w', 'out', 'status'):
        assert _interp(L, **{name: None}) == EINVAL, name
    assert _interp(L, C=0) == EINVAL and _interp(L, out=P16) == EINVAL and _interp(L, n=MAXP + 1) == ERANGE
    for name in ('idx', 'csr', 'lst', 'scratch', 'status'):
        assert _invert(L, **{name: None}) == EINVAL, name
    assert _invert(L, E=0) == EINVAL and _invert(L, N=0) == EINVAL
    assert _invert(L, E=2 ** 31) == ERANGE and _invert(L, B=3, E=2 ** 30) == ERANGE and _invert(L, N=MAXP + 1) == ERANGE
    for name in ('go', 'csr', 'lst', 'gf'):
        assert _bwd(L, **{name: None}) == EINVAL, name
    assert _bwd(L, E=32) == EINVAL and _bwd(L, k=0) == EINVAL and _bwd(L, C=0) == EINVAL and _bwd(L, gf=P16) == EINVAL
    assert _bwd(L, E=2 ** 31 + 1) == ERANGE and _bwd(L, B=2, C=4096, N=MAXP) == ERANGE
    for name in ('pts', 'status'):
        assert _batch(L, **{name: None}) == EINVAL, name
    assert _batch(L, rows=100) == EINVAL and _batch(L, cols=3) == EINVAL and _batch(L, per=0) == EINVAL
    assert _batch(L, rows=2 ** 31, per=2 ** 30) == ERANGE
    sb = L.dfu3d_pn2_scratch_bytes
    assert sb(0, 64, 0) == -1 and sb(2, 0, 0) == -1 and sb(2, MAXP + 1, 0) == -1 and sb(2, 64, -1) == -1
    assert sb(3, 64, 2 ** 30) == -1
    assert sb(8, 16384, 0) == 0 and sb(2, 16385, 0) == 2 * 16385 * 4 and sb(2, 64, 32) == (2 * 64 + 2 * 32) * 4


def test_ops_refuse_host_wrong_type_and_non_contiguous_tensors():
    import torch
    from dfu3d_amd import pointnet2_ops as ops
    from dfu3d_amd._lib import Dfu3dError
    xyz = torch.zeros(2, 16, 3)
    with pytest.raises(Dfu3dError, match="on the GPU"):
        ops.fps(xyz, 4)
    with pytest.raises(Dfu3dError, match="on the GPU"):
        ops.three_nn(xyz, xyz)
    with pytest.raises(Dfu3dError, match="on the GPU"):
        ops.ball_query(xyz, xyz, [1.0], [4])
    with pytest.raises(Dfu3dError):
        ops.group(None, None, None, torch.zeros(2, 4, 4, dtype=torch.int32), use_xyz=False)
    # what the checks say about dtype, layout and shape, on tensors that only claim to be on a device
    meta = torch.zeros(2, 16, 3, device='meta')
    for bad, what in ((meta.double(), "float32"), (meta.transpose(0, 1), "contiguous"), (torch.zeros(2, 16, 2, device='meta'), "shape")):
        class OnGpu(torch.Tensor):
            is_cuda = True
        t = bad.as_subclass(OnGpu)
        with pytest.raises(Dfu3dError, match=what):
            ops._want(t, "xyz", torch.float32, (None, None, 3))


def test_modules_construct_with_the_reference_keys():
    from dfu3d_amd.pcdet_kitti.pointnet2_backbone import PointNet2MSG
    from dfu3d_amd.pcdet_kitti import pointnet2_modules as pm
    from tests import pointnet2_ref as R

    class Attr:
        def __init__(self, d):
            for k, v in d.items():
                setattr(self, k, Attr(v) if isinstance(v, dict) else v)
    for cfg in (R.G19_CFG, Attr(R.G19_CFG)):                               # dict and attribute access
        m = PointNet2MSG(cfg, 3 + R.G19_EXTRA)
        assert m.num_point_features == 16 and m.check is True
        keys = list(m.state_dict())
        assert keys[0] == 'SA_modules.0.mlps.0.0.weight' and 'FP_modules.1.mlp.4.running_var' in keys
        assert tuple(m.SA_modules[0].mlps[0][0].weight.shape) == (8, 4, 1, 1)
        assert tuple(m.FP_modules[0].mlp[0].weight.shape) == (16, 17, 1, 1)
        assert tuple(m.FP_modules[1].mlp[0].weight.shape) == (16, 96, 1, 1)
    assert R.G19_CFG['SA_CONFIG']['MLPS'][0][0] == [8, 16]                 # the configuration is not written to
    sa = pm.PointnetSAModule(mlp=[4, 8], npoint=None, use_xyz=True, pool_method='avg_pool')
    assert type(sa.groupers[0]).__name__ == 'GroupAll' and tuple(sa.mlps[0][0].weight.shape) == (8, 7, 1, 1)
    with pytest.raises(NotImplementedError):
        pm.PointnetSAModule(mlp=[4, 8], npoint=4, radius=1.0, nsample=4, pool_method='sum_pool')
    import torch
    from dfu3d_amd._lib import Dfu3dError
    with pytest.raises(Dfu3dError, match="equal size"):
        PointNet2MSG(R.G19_CFG, 4)(dict(batch_size=2, points=torch.zeros(5, 5)))
