"""The CenterHead post-processing without a GPU: the C ABI of include/dfu3d_post.h, the scratch size, and the host-side
argument validation (every refusal returns before any launch)."""
import ctypes

import pytest

from dfu3d_amd import _lib, _lib_head, _lib_post, _lib_vfe

P16 = ctypes.c_void_p(16)            # a non-null, 16-byte aligned address no call may touch
K = _lib_post.CONSTANTS


def test_library_exports_every_symbol_of_the_post_header():
    L = _lib_post.lib()
    assert _lib_post.header_symbols() == sorted([
        "dfu3d_nms_segments_scratch_bytes", "dfu3d_nms_bev_segments", "dfu3d_center_collect"])
    for name in _lib_post.header_symbols():
        assert getattr(L, name).argtypes is not None
    assert _lib_post.header_version() == 1 and K["DFU3D_POST_MAX_CAP"] == 1024
    assert len(_lib.SIGNATURES) == 46                                                # dfu3d.h keeps its symbols
    assert _lib_head.header_symbols() == sorted([
        "dfu3d_head_version", "dfu3d_center_loss_scratch_bytes", "dfu3d_center_loss_fwd", "dfu3d_center_loss_bwd"])
    assert _lib_vfe.header_symbols() == sorted(_lib_vfe.SIGNATURES) and all("pillar" in n or "vfe" in n for n in _lib_vfe.SIGNATURES)
    assert not set(_lib_post.SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib_vfe.SIGNATURES) | set(_lib_head.SIGNATURES))
    assert all(k.startswith("DFU3D_POST_") for k in K)
    assert L.dfu3d_nms_segments_scratch_bytes.restype is ctypes.c_size_t


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
        dfu3d_center_collect = object()
    with pytest.raises(_lib.Dfu3dError, match="dfu3d_nms_bev_segments, dfu3d_nms_segments_scratch_bytes"):
        _lib_post.bind(Fake())


def test_scratch_size_is_monotone():
    L = _lib_post.lib()
    size = L.dfu3d_nms_segments_scratch_bytes
    for cap in (1, 64, 65, 500, 1024):
        sizes = [size(S, cap) for S in (0, 1, 6, 24, 384, 4096)]
        assert sizes == sorted(sizes) and sizes[1] > sizes[0], (cap, sizes)
    for S in (1, 24, 384):
        sizes = [size(S, cap) for cap in (0, 1, 63, 64, 65, 128, 500, 1000, 1024)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], (S, sizes)
    # the suppression masks: one 64-bit word per (row, block of 64 rows), 16 bytes of slack
    assert size(24, 500) == 24 * 500 * 8 * 8 + 16
    assert size(-1, 8) == 0 and size(1, -1) == 0 and size(1, K["DFU3D_POST_MAX_CAP"] + 1) == 0


def _nms(L, boxes=P16, S=2, cap=100, C=7, count=P16, scratch=P16, nbytes=1 << 30, keep=P16, num=P16):
    return L.dfu3d_nms_bev_segments(boxes, S, cap, C, count, 0.5, 0, 0, 0, scratch, nbytes, keep, num, None)


def _collect(L, n_heads=2, B=2, cap=8, C=7, max_cls=2, out_cap=16, **null):
    p = lambda k: None if null.get(k) else P16   # noqa: E731
    return L.dfu3d_center_collect(p("boxes"), p("scores"), p("labels"), p("keep"), p("num_keep"), n_heads, B, cap, C,
                                  p("cls_map"), max_cls, out_cap, p("out_boxes"), p("out_scores"), p("out_labels"),
                                  p("out_count"), None)


def test_bad_arguments_return_before_any_launch():
    L = _lib_post.lib()
    OK, EINVAL, ERANGE = (_lib.CONSTANTS["DFU3D_" + k] for k in ("OK", "EINVAL", "ERANGE"))
    for name in ("boxes", "count", "keep", "num", "scratch"):
        assert _nms(L, **{name: None}) == EINVAL, name
    assert _nms(L, C=6) == EINVAL
    assert _nms(L, S=-1) == EINVAL
    assert _nms(L, cap=-1) == EINVAL
    assert _nms(L, nbytes=L.dfu3d_nms_segments_scratch_bytes(2, 100) - 1) == EINVAL   # scratch too small
    assert _nms(L, scratch=ctypes.c_void_p(20)) == EINVAL                             # not 8-byte aligned
    assert _nms(L, cap=K["DFU3D_POST_MAX_CAP"] + 1) == ERANGE
    assert _nms(L, S=0) == OK and _nms(L, cap=0) == OK                                # nothing to do: no launch
    for name in ("boxes", "scores", "labels", "keep", "num_keep", "cls_map", "out_boxes", "out_scores", "out_labels",
                 "out_count"):
        assert _collect(L, **{name: True}) == EINVAL, name
    assert _collect(L, n_heads=0) == EINVAL
    assert _collect(L, B=-1) == EINVAL
    assert _collect(L, C=0) == EINVAL
    assert _collect(L, max_cls=0) == EINVAL
    assert _collect(L, out_cap=-1) == EINVAL
    assert _collect(L, n_heads=1 << 16) == ERANGE
    assert _collect(L, B=0) == OK


def test_python_layer_refuses_without_a_gpu():
    """Shape, dtype and configuration refusals happen on the host, before any tensor reaches the library."""
    import torch
    from dfu3d_amd import stages
    with pytest.raises(_lib.Dfu3dError, match="C >= 7"):
        stages.nms_bev_segments(torch.zeros(2, 8, 6), torch.zeros(2, dtype=torch.int32), 0.5)
    with pytest.raises(_lib.Dfu3dError, match="at most 1024"):
        stages.nms_bev_segments(torch.zeros(1, 1025, 7), torch.zeros(1, dtype=torch.int32), 0.5)
    with pytest.raises(_lib.Dfu3dError, match="on the GPU"):
        stages.nms_bev_segments(torch.zeros(2, 8, 7), torch.zeros(2, dtype=torch.int32), 0.5)
