"""The CenterHead loss without a GPU: the C ABI of include/dfu3d_head.h, the scratch size against the layout, and the
host-side argument validation (every refusal returns before any launch)."""
import ctypes

import pytest

from dfu3d_amd import _lib, _lib_head, _lib_vfe

P16 = ctypes.c_void_p(16)            # a non-null, 16-byte aligned address no call may touch
K = _lib_head.CONSTANTS


def test_library_exports_every_symbol_of_the_head_header():
    L = _lib_head.lib()
    assert _lib_head.header_symbols() == sorted([
        "dfu3d_head_version", "dfu3d_center_loss_scratch_bytes", "dfu3d_center_loss_fwd", "dfu3d_center_loss_bwd"])
    for name in _lib_head.header_symbols():
        assert getattr(L, name).argtypes is not None
    assert L.dfu3d_head_version() == _lib_head.header_version() == 100
    assert len(_lib.SIGNATURES) == 46                                                # dfu3d.h keeps its symbols
    assert not set(_lib_head.SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib_vfe.SIGNATURES))
    assert all(k.startswith("DFU3D_HEAD_") for k in K)


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
        dfu3d_head_version = dfu3d_center_loss_fwd = object()
    with pytest.raises(_lib.Dfu3dError, match="dfu3d_center_loss_bwd, dfu3d_center_loss_scratch_bytes"):
        _lib_head.bind(Fake())


def test_scratch_size_agrees_with_the_layout():
    L = _lib_head.lib()
    parts, code = K["DFU3D_HEAD_PARTS"], K["DFU3D_HEAD_MAX_CODE"]
    for n_heads, batch in ((1, 1), (6, 4), (8, 64), (2, 1000)):
        # {S_pos, S_neg, num_pos} doubles per partial, then {S_d, valid slots} doubles per (head, sample), 16 bytes of slack
        expect = n_heads * parts * 3 * 8 + n_heads * batch * (code + 1) * 8 + 16
        assert L.dfu3d_center_loss_scratch_bytes(n_heads, batch, 8) == expect
    assert L.dfu3d_center_loss_scratch_bytes(0, 1, 8) == -1
    assert L.dfu3d_center_loss_scratch_bytes(K["DFU3D_HEAD_MAX_HEADS"] + 1, 1, 8) == -1
    assert L.dfu3d_center_loss_scratch_bytes(1, 0, 8) == -1
    assert L.dfu3d_center_loss_scratch_bytes(1, 1, code + 1) == -1


def _fwd(L, n_heads=1, batch=2, hw=64, reg=(2, 1, 3, 2), n_max=8, maps="ok", losses=P16, scratch=P16, nbytes=1 << 20,
         n_cls=1):
    tab = (ctypes.c_uint64 * (max(n_heads, 1) * K["DFU3D_HEAD_FWD_PTRS"]))(*([16] * (max(n_heads, 1) * K["DFU3D_HEAD_FWD_PTRS"])))
    if maps == "no_heat":
        tab[1] = 0
    if maps == "no_ind":
        tab[3] = 0
    cls = (ctypes.c_int32 * max(n_heads, 1))(*([n_cls] * max(n_heads, 1)))
    ch = (ctypes.c_int32 * max(len(reg), 1))(*reg)
    w = (ctypes.c_double * (2 + K["DFU3D_HEAD_MAX_CODE"]))(*([1.0] * (2 + K["DFU3D_HEAD_MAX_CODE"])))
    return L.dfu3d_center_loss_fwd(None if maps is None else tab, cls, n_heads, batch, hw, ch, len(reg), n_max, w, losses,
                                   P16, P16, scratch, nbytes, None)


def test_bad_arguments_return_before_any_launch():
    L = _lib_head.lib()
    EINVAL, ERANGE = _lib.CONSTANTS["DFU3D_EINVAL"], _lib.CONSTANTS["DFU3D_ERANGE"]
    assert _fwd(L, maps=None) == EINVAL
    assert _fwd(L, losses=None) == EINVAL
    assert _fwd(L, scratch=None) == EINVAL
    assert _fwd(L, nbytes=64) == EINVAL                                               # scratch too small
    assert _fwd(L, scratch=ctypes.c_void_p(24)) == EINVAL                             # not 16-byte aligned
    assert _fwd(L, maps="no_heat") == EINVAL                                          # hm without its target heat map
    assert _fwd(L, maps="no_ind") == EINVAL
    assert _fwd(L, n_cls=0) == EINVAL
    assert _fwd(L, batch=0) == EINVAL
    assert _fwd(L, reg=(2, 0)) == EINVAL
    assert _fwd(L, n_heads=K["DFU3D_HEAD_MAX_HEADS"] + 1) == ERANGE                   # too many heads
    assert _fwd(L, n_max=K["DFU3D_HEAD_MAX_OBJS"] + 1) == ERANGE                      # NUM_MAX_OBJS > 1024
    assert _fwd(L, reg=(2, 1, 3, 2, 2, 2)) == ERANGE                                  # more maps than MAX_REG_MAPS
    assert _fwd(L, reg=(8, 8, 1)) == ERANGE                                           # more channels than MAX_CODE
    assert _fwd(L, batch=1 << 20, hw=1 << 20) == ERANGE
    tab = (ctypes.c_uint64 * K["DFU3D_HEAD_FWD_PTRS"])(*([16] * K["DFU3D_HEAD_FWD_PTRS"]))
    one = (ctypes.c_int32 * 1)(1)
    ch = (ctypes.c_int32 * 1)(2)
    w = (ctypes.c_double * 18)(*([1.0] * 18))
    assert L.dfu3d_center_loss_bwd(tab, None, one, 1, 1, 64, ch, 1, 8, w, P16, None, P16, None) == EINVAL
    assert L.dfu3d_center_loss_bwd(tab, tab, one, 1, 1, 64, ch, 1, 8, w, P16, None, None, None) == EINVAL
    assert L.dfu3d_center_loss_bwd(tab, tab, one, 9, 1, 64, ch, 1, 8, w, P16, None, P16, None) == ERANGE


def test_python_layer_refuses_without_a_gpu():
    """dtype and argument-form refusals happen on the host, before any tensor reaches the library."""
    import torch
    from dfu3d_amd import center_loss_ops
    from dfu3d_amd.pcdet_kitti import loss_utils
    x = torch.zeros(1, 1, 2, 2)
    with pytest.raises(_lib.Dfu3dError, match="on the GPU"):
        center_loss_ops.center_loss([x], [x], None, None, None, None)
    with pytest.raises(_lib.Dfu3dError, match="heads"):
        center_loss_ops.center_loss([x] * 9, [x] * 9, None, None, None, None)
    with pytest.raises(NotImplementedError, match="mask"):
        loss_utils.FocalLossCenterNet()(x, x, mask=x)
    with pytest.raises(NotImplementedError, match="ind=None"):
        loss_utils.RegLossCenterNet()(x, x)
