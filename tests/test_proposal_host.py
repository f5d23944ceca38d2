"""The batched proposal stage without a GPU: the agreement of csrc/dfu3d_prop.h with its binding, host-side argument
validation before any launch, the order rule's restatement (tests/proposal_ref.py) on hand-written arrays, and the
constructor switch of PointRCNNHead."""
import ctypes
import glob
import importlib
import os

import numpy as np
import pytest

from dfu3d_amd import _build, _lib, _lib_prop
from tests import proposal_ref as P
from tests import roipoint_ref as R

P16 = ctypes.c_void_p(16)            # a non-null, 16-byte aligned address no call may touch
SYMBOLS = ['dfu3d_prop_scratch_bytes', 'dfu3d_prop_version', 'dfu3d_proposals']
POINTERS = ('scores', 'labels', 'boxes', 'scratch', 'rois', 'roi_scores', 'roi_labels', 'roi_idx', 'num')


def test_header_and_binding_agree():
    assert _lib_prop.HEADER == os.path.join(_build.CSRC, "dfu3d_prop.h") and _lib_prop.HEADER in _build._deps()
    assert "dfu3d_prop.h" not in os.listdir(_build.INCLUDE)
    assert _lib_prop.header_symbols() == SYMBOLS
    L = _lib_prop.lib()
    assert all(hasattr(L, s) for s in SYMBOLS)
    assert L.dfu3d_prop_version() == _lib_prop.header_version() == 1
    K = _lib_prop.CONSTANTS
    assert all(k.startswith("DFU3D_PROP_") for k in K)
    assert K == {'DFU3D_PROP_VERSION': 1, 'DFU3D_PROP_LAUNCHES': 2, 'DFU3D_PROP_MAX_POST': 1024,
                 'DFU3D_PROP_MAX_POINTS': 16384, 'DFU3D_PROP_MAX_BATCH': 65535, 'DFU3D_PROP_MAX_ELEMS': 2 ** 31 - 1,
                 'DFU3D_PROP_SORT_THREADS': 1024, 'DFU3D_PROP_BLOCK_ROWS': 64, 'DFU3D_PROP_QUEUE_PAIRS': 2936}
    assert 1 <= K['DFU3D_PROP_LAUNCHES'] <= 3 and K['DFU3D_PROP_MAX_POINTS'] >= 16384
    res, args = _lib_prop.SIGNATURES['dfu3d_proposals']
    assert res is ctypes.c_int32 and len(args) == 17 and args[-1] is ctypes.c_void_p
    assert [k for k, a in enumerate(args) if a is ctypes.c_float] == [6] and args[10] is ctypes.c_size_t
    assert args[3:6] == [ctypes.c_int32] * 3 and args[7:9] == [ctypes.c_int32] * 2
    assert _lib_prop.SIGNATURES['dfu3d_prop_scratch_bytes'] == (ctypes.c_size_t, [ctypes.c_int32] * 3)
    assert _lib_prop.SIGNATURES['dfu3d_prop_version'] == (ctypes.c_int32, [])
    others = [os.path.basename(p)[:-3] for p in glob.glob(os.path.join(os.path.dirname(_lib.__file__), "_lib*.py"))]
    assert "_lib_prop" in others and "_lib_tgt" in others and "_lib" in others
    for name in others:
        if name != "_lib_prop":
            mod = importlib.import_module("dfu3d_amd." + name)
            assert not set(_lib_prop.SIGNATURES) & set(mod.SIGNATURES), name
            assert not set(K) & set(mod.CONSTANTS), name
    own = open(_lib_prop.HEADER).read()
    for prefix in ('dfu3d_vfe', 'dfu3d_head', 'dfu3d_post', 'dfu3d_aug', 'dfu3d_bev', 'dfu3d_opt', 'dfu3d_ingest',
                   'dfu3d_pn2', 'dfu3d_roi', 'dfu3d_tgt'):
        assert prefix not in own and prefix.upper() not in own, prefix
    from dfu3d_amd import proposal_ops as ops
    assert (ops.LAUNCHES, ops.MAX_POST, ops.MAX_POINTS) == (2, 1024, 16384)


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
    Fake.dfu3d_prop_version = object()
    with pytest.raises(_lib.Dfu3dError, match="fake.so does not export dfu3d_prop_scratch_bytes, dfu3d_proposals"):
        _lib_prop.bind(Fake())


def _call(L, B=2, N=64, C=7, thresh=0.8, pre=50, post=12, nbytes=None, **ptr):
    p = {name: ctypes.c_void_p(16 * (k + 1)) for k, name in enumerate(POINTERS)}
    p.update(ptr)
    if nbytes is None:
        nbytes = L.dfu3d_prop_scratch_bytes(B, N, pre) or 16
    return L.dfu3d_proposals(p['scores'], p['labels'], p['boxes'], B, N, C, thresh, pre, post, p['scratch'], nbytes,
                             p['rois'], p['roi_scores'], p['roi_labels'], p['roi_idx'], p['num'], None)


def test_bad_arguments_return_before_any_launch():
    """Every call below passes pointers no kernel may touch: a launch would fault (or, without a GPU, fail with
    DFU3D_ELAUNCH); each must come back with the validation's own code."""
    L = _lib_prop.lib()
    OK, EINVAL, ERANGE = (_lib.CONSTANTS[k] for k in ("DFU3D_OK", "DFU3D_EINVAL", "DFU3D_ERANGE"))
    K = _lib_prop.CONSTANTS
    for name in POINTERS:
        assert _call(L, **{name: None}) == EINVAL, name
    assert _call(L, C=6) == EINVAL and _call(L, C=0) == EINVAL and _call(L, C=-1) == EINVAL
    assert _call(L, B=-1) == EINVAL and _call(L, N=-1) == EINVAL
    assert _call(L, pre=0) == EINVAL and _call(L, pre=-5) == EINVAL
    assert _call(L, scratch=ctypes.c_void_p(24)) == EINVAL                        # not on 16 bytes
    need = L.dfu3d_prop_scratch_bytes(2, 64, 50)
    assert need > 0 and _call(L, nbytes=need - 1) == EINVAL and _call(L, nbytes=0) == EINVAL
    # nothing to do: no launch, and the scratch is not looked at
    assert _call(L, B=0) == OK and _call(L, N=0) == OK and _call(L, B=0, N=0, nbytes=0) == OK
    assert _call(L, post=0) == ERANGE and _call(L, post=-1) == ERANGE
    assert _call(L, post=K['DFU3D_PROP_MAX_POST'] + 1) == ERANGE
    assert _call(L, N=K['DFU3D_PROP_MAX_POINTS'] + 1, nbytes=1 << 30) == ERANGE
    assert _call(L, B=K['DFU3D_PROP_MAX_BATCH'] + 1, N=1, nbytes=1 << 30) == ERANGE
    assert _call(L, B=65535, N=16384, C=7, nbytes=1 << 40) == ERANGE              # B * N * C
    assert _call(L, B=16, N=16384, C=8192, nbytes=1 << 40) == ERANGE
    assert _call(L, B=1, N=1, C=2 ** 22, post=1024, nbytes=1 << 30) == ERANGE     # B * post_max * C
    # an out-of-range size wins over what is empty
    assert _call(L, B=0, post=0) == ERANGE and _call(L, N=0, C=6) == EINVAL


def test_scratch_bytes():
    L = _lib_prop.lib()
    K = _lib_prop.CONSTANTS
    for bad in ((-1, 64, 50), (2, -1, 50), (2, 64, 0), (2, 64, -3), (2, K['DFU3D_PROP_MAX_POINTS'] + 1, 50),
                (K['DFU3D_PROP_MAX_BATCH'] + 1, 64, 50)):
        assert L.dfu3d_prop_scratch_bytes(*bad) == 0, bad
    sizes = [L.dfu3d_prop_scratch_bytes(B, 300, 200) for B in range(0, 12)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] == 0 and all(s % 16 == 0 for s in sizes)
    # two (key, index) buffers of N entries and the order of min(pre_max, N) per sample, rounded up to 16 and no more
    assert [sizes[B] for B in (1, 4, 5)] == [-(-B * (300 * 16 + 200 * 4) // 16) * 16 for B in (1, 4, 5)]
    assert L.dfu3d_prop_scratch_bytes(3, 300, 9000) == L.dfu3d_prop_scratch_bytes(3, 300, 300)
    big = L.dfu3d_prop_scratch_bytes(K['DFU3D_PROP_MAX_BATCH'], K['DFU3D_PROP_MAX_POINTS'], 9000)
    assert big >= 65535 * 16384 * 16                                              # no 32-bit wrap-around


def test_order_rule_on_hand_written_scores():
    nan, inf = float('nan'), float('inf')
    neg_nan = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
    s = np.array([0.5, -0.0, nan, 0.0, inf, 0.5, -inf, -1.0, neg_nan, 0.0, 1e-45, -1e-45], np.float32)
    key = P.sort_key(s)
    assert key[1] == key[3] == key[9] == 0x80000000                               # -0.0 is +0.0
    assert key[2] == key[8] == 0xFFFFFFFF and key[4] == 0xFF800000                # every NaN the one key above +inf
    assert key[6] == 0x007FFFFF and key[10] == 0x80000001 and key[11] == 0x7FFFFFFE
    full = [2, 8, 4, 0, 5, 10, 1, 3, 9, 11, 7, 6]                                 # equal keys by ascending index
    assert P.order_ref(s, 12).tolist() == full and P.order_ref(s, 100).tolist() == full     # pre_max > N
    assert P.order_ref(s, 5).tolist() == full[:5] and P.order_ref(s, 1).tolist() == [2]
    assert P.order_ref(np.zeros(0, np.float32), 4).size == 0
    # distinct finite scores: the descending sort
    rng = np.random.default_rng(0)
    d = P.distinct_scores(rng, 1, 500)[0]
    assert np.array_equal(P.order_ref(d, 123), np.argsort(-d.astype(np.float64), kind="stable")[:123])
    # the key is monotone over every finite float next to a boundary
    v = np.array([-inf, -3e38, -1.0, -1e-45, 0.0, 1e-45, 1.0, 3e38, inf], np.float32)
    assert (np.diff(P.sort_key(v).astype(np.int64)) > 0).all()


def test_pad_ref_pads_as_the_layer_does():
    rng = np.random.default_rng(1)
    scores, boxes = P.distinct_scores(rng, 2, 9), P.clustered_boxes(rng, 2, 9, C=9)
    labels = rng.integers(0, 3, (2, 9))
    kept = [np.array([4, 1, 7], np.int64), np.array([], np.int64)]
    rois, rs, rl, ri, num = P.pad_ref(kept, scores, labels, boxes, 2)
    assert num.tolist() == [2, 0] and ri.tolist() == [[4, 1], [-1, -1]] and rl[1].tolist() == [1, 1]
    assert np.array_equal(rois[0], boxes[0][[4, 1]]) and not rois[1].any() and rl[0].tolist() == (labels[0][[4, 1]] + 1).tolist()
    rois, rs, rl, ri, num = P.pad_ref(kept, scores, labels, boxes, 5)
    assert num.tolist() == [3, 0] and ri[0].tolist() == [4, 1, 7, -1, -1] and not rois[0, 3:].any() and not rs[0, 3:].any()


def test_the_switch_keeps_the_state_dict_and_is_off_by_default():
    from dfu3d_amd.pcdet_kitti.point_rcnn import PointRCNN
    from dfu3d_amd.pcdet_kitti.pointrcnn_head import PointRCNNHead
    plain = PointRCNN(R.g20_model_cfg(), 3, class_names=R.G20_CLASSES, num_point_features=4)
    model = PointRCNN(R.g20_model_cfg(), 3, class_names=R.G20_CLASSES, num_point_features=4, batched_proposals=True)
    assert not plain.batched_proposals and not plain.roi_head.batched_proposals
    assert model.batched_proposals and model.roi_head.batched_proposals and not model.trainable
    keys = [(k, tuple(v.shape)) for k, v in plain.state_dict().items()]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
    model.load_state_dict(plain.state_dict(), strict=True)
    cfg = R.g20_model_cfg()['ROI_HEAD']
    a = PointRCNNHead(16, cfg, num_class=1)
    b = PointRCNNHead(16, cfg, num_class=1, batched_proposals=True, trainable=True)
    assert not a.batched_proposals and b.batched_proposals and list(a.state_dict()) == list(b.state_dict())


def test_the_batched_layer_says_what_it_lacks():
    from dfu3d_amd.pcdet_kitti.pointrcnn_head import PointRCNNHead
    cfg = R.g20_model_cfg()['ROI_HEAD']
    head = PointRCNNHead(16, cfg, num_class=1, batched_proposals=True)
    nms = dict(cfg['NMS_CONFIG']['TEST'])
    with pytest.raises(NotImplementedError, match="MULTI_CLASSES_NMS"):
        head.proposal_layer_batched({'batch_size': 1}, dict(nms, MULTI_CLASSES_NMS=True))
    with pytest.raises(NotImplementedError, match="nms_normal_gpu"):
        head.proposal_layer_batched({'batch_size': 1}, dict(nms, NMS_TYPE='nms_normal_gpu'))
    done = {'batch_size': 1, 'rois': object()}
    assert head.proposal_layer_batched(done, nms) is done                          # as proposal_layer: RoIs given, nothing to do
