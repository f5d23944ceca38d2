"""The pillar scatter without a GPU: the agreement of include/dfu3d_bev.h with its binding, host-side argument validation
before any launch, and the construction of the two modules."""
import ctypes
import os
import re

import pytest

from dfu3d_amd import _build, _lib, _lib_bev

P16 = ctypes.c_void_p(16)            # a non-null, 16-byte aligned address no call may touch


def test_header_and_binding_agree():
    assert _lib_bev.HEADER == os.path.join(_build.INCLUDE, "dfu3d_bev.h") and _lib_bev.HEADER in _build._deps()
    assert _lib_bev.header_symbols() == ['dfu3d_bev_scratch_bytes', 'dfu3d_bev_version', 'dfu3d_pillar_scatter',
                                         'dfu3d_pillar_scatter_backward']
    L = _lib_bev.lib()
    assert L.dfu3d_bev_version() == _lib_bev.header_version() == 1
    text = open(_lib_bev.HEADER).read()
    for name in ('dfu3d_pillar_scatter', 'dfu3d_pillar_scatter_backward'):
        proto = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        res, args = _lib_bev.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == len(proto.split(","))
    assert len(_lib_bev.SIGNATURES['dfu3d_pillar_scatter'][1]) == 14
    assert len(_lib_bev.SIGNATURES['dfu3d_pillar_scatter_backward'][1]) == 13
    assert _lib_bev.SIGNATURES['dfu3d_bev_scratch_bytes'] == (ctypes.c_int64, [ctypes.c_int64])
    K = _lib_bev.CONSTANTS
    assert all(k.startswith("DFU3D_BEV_") for k in K)
    assert K['DFU3D_BEV_MAX_CELLS'] == 1 << 24 == _lib_bev.CONSTANTS['DFU3D_BEV_MAX_CELLS']
    from dfu3d_amd import _lib_vfe
    assert K['DFU3D_BEV_MAX_CELLS'] == _lib_vfe.CONSTANTS['DFU3D_VFE_MAX_CELLS']
    assert (K['DFU3D_BEV_MAX_CHANNELS'], K['DFU3D_BEV_ST_BAD_COORD'], K['DFU3D_BEV_ST_DUPLICATE'], K['DFU3D_BEV_RUN']) \
        == (256, 1, 2, 64)
    assert not set(_lib_bev.SIGNATURES) & set(_lib.SIGNATURES)
    # the other headers do not know this one, and this one only adds to the library
    for other in ("dfu3d.h", "dfu3d_vfe.h", "dfu3d_head.h", "dfu3d_post.h", "dfu3d_aug.h"):
        assert "dfu3d_bev" not in open(os.path.join(_build.INCLUDE, other)).read()
    from dfu3d_amd import bev_ops
    assert (bev_ops.ST_BAD_COORD, bev_ops.ST_DUPLICATE, bev_ops.MAX_CELLS) == (1, 2, 1 << 24)


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
        dfu3d_bev_version = dfu3d_pillar_scatter = object()
    with pytest.raises(_lib.Dfu3dError, match="dfu3d_bev_scratch_bytes, dfu3d_pillar_scatter_backward"):
        _lib_bev.bind(Fake())


def _fwd(L, features=P16, coords=P16, cols=4, p_cap=8, n=None, C=64, B=1, nz=1, ny=4, nx=4, canvas=P16, cell_map=P16,
         status=P16):
    return L.dfu3d_pillar_scatter(features, coords, cols, p_cap, n, C, B, nz, ny, nx, canvas, cell_map, status, None)


def _bwd(L, grad=P16, coords=P16, cols=4, p_cap=8, n=None, C=64, B=1, nz=1, ny=4, nx=4, cell_map=P16, out=P16):
    return L.dfu3d_pillar_scatter_backward(grad, coords, cols, p_cap, n, C, B, nz, ny, nx, cell_map, out, None)


def test_bad_arguments_return_before_any_launch():
    L = _lib_bev.lib()
    EINVAL, ERANGE = _lib.CONSTANTS["DFU3D_EINVAL"], _lib.CONSTANTS["DFU3D_ERANGE"]
    MAX = _lib_bev.CONSTANTS["DFU3D_BEV_MAX_CELLS"]
    for f in (_fwd, _bwd):
        assert f(L, coords=None) == EINVAL
        assert f(L, cell_map=None) == EINVAL
        assert f(L, C=0) == EINVAL
        assert f(L, C=257) == EINVAL
        assert f(L, cols=3, nz=2) == EINVAL
        assert f(L, cols=5) == EINVAL
        assert f(L, p_cap=-1) == EINVAL
        assert f(L, B=0) == EINVAL
        assert f(L, nx=0) == EINVAL
        assert f(L, B=1, ny=1, nx=MAX + 1) == ERANGE
        assert f(L, B=4, nz=2, ny=2048, nx=2048) == ERANGE
        assert f(L, B=2047, nz=2047, ny=2047, nx=2047) == ERANGE                     # no overflow on the way
    assert _fwd(L, features=None) == EINVAL
    assert _fwd(L, canvas=None) == EINVAL
    assert _fwd(L, status=None) == EINVAL
    assert _bwd(L, grad=None) == EINVAL
    assert _bwd(L, out=None) == EINVAL
    assert L.dfu3d_bev_scratch_bytes(-1) == -1
    assert L.dfu3d_bev_scratch_bytes(MAX + 1) == -1
    assert L.dfu3d_bev_scratch_bytes(0) == 0 and L.dfu3d_bev_scratch_bytes(MAX) == 4 * MAX


def test_modules_construct_without_a_gpu():
    from dfu3d_amd.pcdet_kitti.pointpillar_scatter import PointPillarScatter, PointPillarScatter3d
    for cfg in ({'NUM_BEV_FEATURES': 64}, type('Cfg', (), {'NUM_BEV_FEATURES': 64})):     # dict and attribute access
        m = PointPillarScatter(cfg, grid_size=[256, 512, 1])
        assert (m.nx, m.ny, m.nz, m.num_bev_features) == (256, 512, 1, 64) and m.status is None
        assert len(m.state_dict()) == 0
        m.check_status()                                                                # nothing ran: nothing to raise
    with pytest.raises(AssertionError):
        PointPillarScatter({'NUM_BEV_FEATURES': 64}, grid_size=[256, 512, 2])
    m = PointPillarScatter3d({'NUM_BEV_FEATURES': 32, 'INPUT_SHAPE': [23, 19, 4]}, grid_size=[23, 19, 4])
    assert (m.nx, m.ny, m.nz, m.num_bev_features, m.num_bev_features_before_compression) == (23, 19, 4, 32, 8)


def test_op_refuses_host_tensors_and_wrong_types():
    import torch
    from dfu3d_amd import bev_ops
    from dfu3d_amd._lib import Dfu3dError
    with pytest.raises(Dfu3dError):
        bev_ops.pillar_scatter(torch.zeros(4, 8), torch.zeros(4, 4, dtype=torch.int32), 1, (4, 4, 1))
